"""Numpy model of the --verifymixpct data pattern.

The specification the CPU loops and the HIP kernels are held to, bit for bit,
written from the definition and not from any loop:

* B is the block size, M = floor(B * pct / 100) rounded down to a multiple of 8;
* the u64 at 8-aligned file offset o holds mix(o + salt) if (o mod B) < M,
  else o + salt, little-endian, all arithmetic mod 2^64;
* mix(x) is one splitmix64 step from state x;
* a byte at an unaligned position p is byte p & 7 of the word at p & ~7.

The pattern depends on the file offset, B, M and the salt only.
"""

from __future__ import annotations

import numpy as np

from tests import kernel_model as km

MASK = km.MASK
U64_MAX = km.U64_MAX
_U = np.uint64


def mix_len(block_size: int, pct: int) -> int:
    assert 0 <= pct <= 100
    return block_size * pct // 100 // 8 * 8


def mix(x):
    """One splitmix64 step from state x (scalar or array), the output only."""
    shape = np.shape(x)
    z = np.atleast_1d(np.asarray(x, dtype=np.uint64)) + _U(km.GOLDEN)
    return km.splitmix_mix(z).reshape(shape)


def words(length: int, file_off: int, salt: int, block_size: int, m: int) -> np.ndarray:
    """The pattern's u64 words for the 8-aligned range [file_off, file_off + length)."""
    assert length % 8 == 0 and file_off % 8 == 0
    assert block_size % 8 == 0 and m % 8 == 0 and 0 <= m <= block_size
    o = _U(file_off & MASK) + np.arange(length // 8, dtype=np.uint64) * _U(8)
    plain = o + _U(salt & MASK)
    return np.where(o % _U(block_size) < _U(m), mix(plain), plain)


def pattern(length: int, file_off: int, salt: int, block_size: int, m: int) -> bytes:
    """Bytes of [file_off, file_off + length), any alignment."""
    lo = file_off // 8 * 8
    hi = (file_off + length + 7) // 8 * 8
    raw = words(hi - lo, lo, salt, block_size, m).astype("<u8").tobytes()
    return raw[file_off - lo:file_off - lo + length]


def verify(data: bytes, file_off: int, salt: int, block_size: int, m: int) -> tuple[int, int]:
    """(number of mismatching u64 words, lowest mismatching word's file offset
    or 2^64-1)."""
    assert len(data) % 8 == 0 and file_off % 8 == 0
    got = np.frombuffer(data, dtype="<u8")
    bad = np.flatnonzero(got != words(len(data), file_off, salt, block_size, m))
    if bad.size == 0:
        return 0, U64_MAX
    offs = _U(file_off & MASK) + bad.astype(np.uint64) * _U(8)
    return int(bad.size), int(offs.min())
