"""Numpy model of the --verifydiag classification.

The specification the CPU loop and the HIP kernels are held to, bit for bit,
written from the definition and not from any loop.

A launch is one buffer of len bytes at file offset file_off (both multiples of
8); its words are w = 0 .. len/8-1 at off(w) = file_off + 8w (mod 2^64).
exp(w) is the plain pattern off(w) + salt, or with block_size > 0 the
--verifymixpct pattern of tests/verify_mix_model.py. Word w is bad iff
v(w) != exp(w).

For a bad word the decoded value u(w) is v(w) at a plain position and
unmix64(v(w)) - GOLDEN at a hashed one, unmix64 being the inverse of the
splitmix64 finalizer; its delta is d(w) = u(w) - (off(w) + salt) mod 2^64, read
as int64. Words pair up as (2i, 2i+1); an odd final word has no partner.

Each bad word gets the first class that matches:
  ZERO     v(w) == 0
  PATTERN  the partner is bad too, neither is zero, d(w) == d(partner)
  BITFLIP  popcount(v(w) ^ exp(w)) <= 2
  OTHER
A run starts at bad word w iff w == 0 or word w-1 is good.

The record has eleven fields that accumulate over launches (combine()).

Only the CPU loop accepts other alignments (diagnose_bytes): a word that the
range holds in part is compared on the bytes it holds, and when bad it counts as
OTHER at the file offset of its first byte inside the range; pairs are counted
from the first whole word; runs go through partial and whole words alike.
"""

from __future__ import annotations

import numpy as np

from tests import kernel_model as km
from tests import verify_mix_model as vm

MASK = km.MASK
U64_MAX = km.U64_MAX
I64_MAX = (1 << 63) - 1
I64_MIN = -(1 << 63)
_U = np.uint64

FIELDS = ("nbad", "first", "last", "runs", "zero", "pattern", "bitflip", "other",
          "delta_min", "delta_max", "flip_or")


def empty() -> dict:
    return dict(nbad=0, first=U64_MAX, last=0, runs=0, zero=0, pattern=0, bitflip=0, other=0,
                delta_min=I64_MAX, delta_max=I64_MIN, flip_or=0)


def combine(a: dict, b: dict) -> dict:
    out = {k: a[k] + b[k] for k in ("nbad", "runs", "zero", "pattern", "bitflip", "other")}
    out["first"] = min(a["first"], b["first"])
    out["last"] = max(a["last"], b["last"])
    out["delta_min"] = min(a["delta_min"], b["delta_min"])
    out["delta_max"] = max(a["delta_max"], b["delta_max"])
    out["flip_or"] = a["flip_or"] | b["flip_or"]
    return out


def unmix64(z):
    """Inverse of km.splitmix_mix (the splitmix64 finalizer), scalar or array."""
    shape = np.shape(z)
    z = np.atleast_1d(np.asarray(z, dtype=np.uint64)).copy()
    z ^= (z >> _U(31)) ^ (z >> _U(62))
    z *= _U(0x319642B2D24D8EC3)
    z ^= (z >> _U(27)) ^ (z >> _U(54))
    z *= _U(0x96DE1B173F119089)
    z ^= (z >> _U(30)) ^ (z >> _U(60))
    return z.reshape(shape)


def popcount(x: np.ndarray) -> np.ndarray:
    b = np.ascontiguousarray(x.astype("<u8")).view(np.uint8).reshape(-1, 8)
    return np.unpackbits(b, axis=1).sum(axis=1)


def expected_words(length: int, file_off: int, salt: int, block_size: int = 0,
                   m: int = 0) -> np.ndarray:
    if block_size:
        return vm.words(length, file_off, salt, block_size, m)
    return km.checksum_words(length, file_off, salt)


def expected_bytes(length: int, file_off: int, salt: int, block_size: int = 0,
                   m: int = 0) -> bytes:
    """The pattern's bytes for [file_off, file_off + length), any alignment."""
    return vm.pattern(length, file_off, salt, block_size or 8, m)  # m == 0: the plain pattern


def diagnose(data: bytes, file_off: int, salt: int, block_size: int = 0, m: int = 0) -> dict:
    """The record of one launch."""
    assert len(data) % 8 == 0 and file_off % 8 == 0
    n = len(data) // 8
    rec = empty()
    if not n:
        return rec
    v = np.frombuffer(data, dtype="<u8").astype(np.uint64)
    exp = expected_words(len(data), file_off, salt, block_size, m)
    bad = v != exp
    if not bad.any():
        return rec

    off = _U(file_off & MASK) + np.arange(n, dtype=np.uint64) * _U(8)
    plain = off + _U(salt & MASK)
    hashed = (off % _U(block_size) < _U(m)) if block_size else np.zeros(n, dtype=bool)
    u = np.where(hashed, unmix64(v) - _U(km.GOLDEN), v)
    d = (u - plain).view(np.int64)

    partner = np.arange(n) ^ 1
    has_partner = partner < n
    partner = np.where(has_partner, partner, 0)
    nz = v != 0
    pattern = bad & has_partner & bad[partner] & nz & nz[partner] & (d == d[partner])
    zero = bad & ~nz
    diff = v ^ exp
    bitflip = bad & ~zero & ~pattern & (popcount(diff) <= 2)
    other = bad & ~zero & ~pattern & ~bitflip

    prev_bad = np.concatenate(([False], bad[:-1]))
    rec["nbad"] = int(bad.sum())
    rec["first"] = int(off[bad].min())
    rec["last"] = int(off[bad].max())
    rec["runs"] = int((bad & ~prev_bad).sum())
    rec["zero"] = int(zero.sum())
    rec["pattern"] = int(pattern.sum())
    rec["bitflip"] = int(bitflip.sum())
    rec["other"] = int(other.sum())
    if pattern.any():
        rec["delta_min"] = int(d[pattern].min())
        rec["delta_max"] = int(d[pattern].max())
    if bitflip.any():
        rec["flip_or"] = int(np.bitwise_or.reduce(diff[bitflip]))
    return rec


def diagnose_bytes(data: bytes, file_off: int, salt: int, block_size: int = 0,
                   m: int = 0) -> dict:
    """The CPU loop's record for a range of any alignment."""
    n = len(data)
    head = min((-file_off) % 8, n)
    tail = (n - head) % 8
    mid = diagnose(data[head:n - tail], file_off + head, salt, block_size, m)
    if not head and not tail:
        return mid

    want = expected_bytes(n, file_off, salt, block_size, m)
    words_bad = np.frombuffer(data[head:n - tail], dtype="<u8") != \
        np.frombuffer(want[head:n - tail], dtype="<u8")
    rec = mid
    head_bad = head and data[:head] != want[:head]
    tail_bad = tail and data[n - tail:] != want[n - tail:]
    if head_bad:
        part = dict(empty(), nbad=1, first=file_off & MASK, last=file_off & MASK, other=1, runs=1)
        rec = combine(rec, part)
        if words_bad.size and words_bad[0]:
            rec["runs"] -= 1  # the first whole word continues the head's run
    if tail_bad:
        o = (file_off + n - tail) & MASK
        part = dict(empty(), nbad=1, first=o, last=o, other=1, runs=1)
        if words_bad.size and words_bad[-1]:
            part["runs"] = 0  # continues the last whole word's run
        elif not words_bad.size and head_bad:
            part["runs"] = 0  # head and tail parts of two adjacent words
        rec = combine(rec, part)
    return rec


def message_suffix(rec: dict) -> str:
    """What a failed verify appends to its message under --verifydiag."""
    s = ("; diagnosis: last bad file offset: %d; runs: %d; zero: %d; pattern: %d; "
         "bitflip: %d; other: %d" % (rec["last"], rec["runs"], rec["zero"], rec["pattern"],
                                     rec["bitflip"], rec["other"]))
    if rec["pattern"]:
        s += "; pattern delta: %d" % rec["delta_min"]
        if rec["delta_min"] != rec["delta_max"]:
            s += "..%d" % rec["delta_max"]
    if rec["bitflip"]:
        s += "; flipped bits: 0x%x" % rec["flip_or"]
    return s
