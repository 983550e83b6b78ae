"""Numpy model of the --dedupepct / --compresspct data pattern.

The specification that fillReduceCPU and ebFillReduceKernel are held to, bit
for bit, written from the definition and not from any loop. With chunk size C
(a power of two), R random bytes per chunk (a multiple of 16, R <= C), dedupe
percentage d, pool size P and the two seeds, all arithmetic mod 2^64:

* mix(x) is one splitmix64 step from state x, GOLD = 0x9E3779B97F4A7C15;
* a worker numbers the chunks it generates in a phase n = 0, 1, 2, ...;
* dup(n) = ((n+1)*d) // 100 > (n*d) // 100, so exactly floor(N*d/100) of any
  first N chunks are duplicates;
* key(n) = mix(poolSeed + mix(uniqSeed ^ n) % P) if dup(n)
           else mix(uniqSeed ^ mix(n));
* the 8-byte word i of chunk n is mix(key(n) + i*GOLD) if 8*i < R, else 0,
  little-endian;
* a fill of `length` bytes starting at chunk `first_chunk` is the run of
  chunks first_chunk, first_chunk+1, ... cut at `length` bytes.

The engine's seeds for worker `rank` in the phase with sequence number s:
phaseSeed = benchSeed + GOLD*s, uniqSeed = mix(phaseSeed ^ (RANK_MULT *
(rank+1))), poolSeed = mix(benchSeed ^ POOL_XOR), P = 256.
"""

from __future__ import annotations

import numpy as np

MASK = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
RANK_MULT = 0xD1B54A32D192ED03
POOL_XOR = 0x5DED0C0DE5EED001
POOL = 256

_U = np.uint64


def mix(x):
    """One splitmix64 step from state x (scalar or array): the output only."""
    shape = np.shape(x)
    z = np.atleast_1d(np.asarray(x, dtype=np.uint64)) + _U(GOLD)  # arrays wrap silently
    z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
    return (z ^ (z >> _U(31))).reshape(shape)


def rand_bytes(chunk: int, compress_pct: int) -> int:
    """R of the engine: floor(C * (100 - c) / 100), down to a multiple of 16."""
    assert 0 <= compress_pct <= 100
    return chunk * (100 - compress_pct) // 100 // 16 * 16


def chunk_numbers(first_chunk: int, count: int) -> np.ndarray:
    return _U(first_chunk & MASK) + np.arange(count, dtype=np.uint64)


def is_dup(n: np.ndarray, d: int) -> np.ndarray:
    n = np.asarray(n, dtype=np.uint64)
    return ((n + _U(1)) * _U(d)) // _U(100) > (n * _U(d)) // _U(100)


def pool_member(n: np.ndarray, pool: int, uniq: int) -> np.ndarray:
    """Which of the `pool` contents a duplicate chunk n holds."""
    return mix(_U(uniq) ^ np.asarray(n, dtype=np.uint64)) % _U(pool)


def chunk_keys(n: np.ndarray, d: int, pool: int, uniq: int, pool_seed: int) -> np.ndarray:
    n = np.asarray(n, dtype=np.uint64)
    return np.where(is_dup(n, d),
                    mix(_U(pool_seed) + pool_member(n, pool, uniq)),
                    mix(_U(uniq) ^ mix(n)))


def model_fill(length: int, first_chunk: int, chunk: int, rand: int, d: int, pool: int,
               uniq: int, pool_seed: int) -> bytes:
    assert chunk >= 16 and chunk & (chunk - 1) == 0
    assert rand % 16 == 0 and 0 <= rand <= chunk
    assert 0 <= d <= 100 and pool >= 1
    count = -(-length // chunk)
    if not count:
        return b""
    keys = chunk_keys(chunk_numbers(first_chunk, count), d, pool, uniq, pool_seed)
    i = np.arange(chunk // 8, dtype=np.uint64)
    words = mix(keys[:, None] + i[None, :] * _U(GOLD))
    words[:, _U(8) * i >= _U(rand)] = 0
    return words.astype("<u8").tobytes()[:length]


def seeds(bench_seed: int, phase_seq: int, rank: int) -> tuple[int, int]:
    """(uniqSeed, poolSeed) of worker `rank` in phase number `phase_seq`."""
    phase_seed = (bench_seed + GOLD * phase_seq) & MASK
    uniq = int(mix(phase_seed ^ ((RANK_MULT * (rank + 1)) & MASK)))
    return uniq, int(mix(bench_seed ^ POOL_XOR))
