"""Plain numpy model of what the HIP fill/verify host wrappers must produce.

This is the specification the GPU kernels are held to, bit for bit. It is
written as whole-array uint64 arithmetic (numpy wraps mod 2^64), not as a
port of any kernel's loop structure: each function states which value lives
at which element and nothing more.

Conventions
-----------
* All lengths and offsets are in bytes; all values are little-endian u64.
* A "vec2 element" is 16 bytes (two u64: x then y) - the kernels' store unit.
* ``seq`` is the context's fill-call counter: 1 for the first fill_rand /
  blockvar call on a fresh context, 2 for the second, ...
* ``seed' = seed + seq * 0x9E3779B9`` is the seed handed to the device.
"""

from __future__ import annotations

import numpy as np

MASK = (1 << 64) - 1
U64_MAX = MASK
GOLDEN = 0x9E3779B97F4A7C15
SEQ_MULT = 0x9E3779B9
THREAD_MULT = 0xA24BAED4963EE407
STREAM_B_XOR = 0x9E6D62D06F6A9A9B

BLOCK = 256          # threads per workgroup
MAX_BLOCKS = 4096    # grid cap of every kernel
RAND_VEC_PER_STEP = 4  # vec2 elements a thread of the xoshiro kernels owns per pass

_U = np.uint64


def _arr(x) -> np.ndarray:
    return np.asarray(x, dtype=np.uint64)


# ---------------------------------------------------------------------------
# scalar / vector primitives
# ---------------------------------------------------------------------------

def splitmix_mix(z):
    """The splitmix64 output function (finalizer) of an already-advanced state."""
    shape = np.shape(z)
    z = np.atleast_1d(_arr(z))  # array ops wrap silently; numpy scalars warn
    z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
    return (z ^ (z >> _U(31))).reshape(shape)


def splitmix64(state: int) -> tuple[int, int]:
    """One splitmix64 step: returns (new_state, output)."""
    state = (state + GOLDEN) & MASK
    return state, int(splitmix_mix(state))


def _rotl(x, k: int):
    return (x << _U(k)) | (x >> _U(64 - k))


def xoshiro256pp_streams(seeds, n: int) -> np.ndarray:
    """n outputs of one xoshiro256++ stream per seed -> array [len(seeds), n].

    State words s0..s3 are the first four splitmix64 outputs from `seed`.
    """
    sm = _arr(seeds).reshape(-1).copy()
    s = []
    for _ in range(4):
        sm = sm + _U(GOLDEN)
        s.append(splitmix_mix(sm))
    s0, s1, s2, s3 = s
    out = np.empty((sm.size, n), dtype=np.uint64)
    for i in range(n):
        out[:, i] = _rotl(s0 + s3, 23) + s0
        t = s1 << _U(17)
        s2 = s2 ^ s0
        s3 = s3 ^ s1
        s1 = s1 ^ s2
        s0 = s0 ^ s3
        s2 = s2 ^ t
        s3 = _rotl(s3, 45)
    return out


# ---------------------------------------------------------------------------
# launch geometry (what decides which thread owns which element)
# ---------------------------------------------------------------------------

def _blocks(work_items: int) -> int:
    return min(max((work_items + BLOCK - 1) // BLOCK, 1), MAX_BLOCKS)


def threads_strided(nvec2: int) -> int:
    """Thread count of the one-element-per-thread kernels (checksum fill,
    fast fill, fast blockvar, verify)."""
    return BLOCK * _blocks(nvec2)


def threads_rand(nvec2: int) -> int:
    """Thread count T of the xoshiro kernels (rand fill, blockvar)."""
    return BLOCK * _blocks(nvec2 // RAND_VEC_PER_STEP)


def owner(family: str, idx: int, nvec2: int) -> tuple[int, int]:
    """(thread, grid-stride iteration) that owns vec2 element `idx`.

    family "rand": thread t owns elements t*4 + j*T*4 + {0..3};
    family "strided": thread t owns elements t + j*T.
    """
    if family == "rand":
        span = threads_rand(nvec2) * RAND_VEC_PER_STEP
        return (idx % span) // RAND_VEC_PER_STEP, idx // span
    if family == "strided":
        t = threads_strided(nvec2)
        return idx % t, idx // t
    raise ValueError(family)


# ---------------------------------------------------------------------------
# the five wrappers
# ---------------------------------------------------------------------------

def device_seed(seed: int, seq: int) -> int:
    return (seed + seq * SEQ_MULT) & MASK


def checksum_words(length: int, file_off: int, salt: int) -> np.ndarray:
    assert length % 8 == 0 and file_off % 8 == 0
    o = _U(file_off & MASK) + np.arange(length // 8, dtype=np.uint64) * _U(8)
    return o + _U(salt & MASK)


def checksum_pattern(length: int, file_off: int, salt: int) -> bytes:
    """Word at file offset o holds (o + salt) mod 2^64."""
    return checksum_words(length, file_off, salt).astype("<u8").tobytes()


def fast_words(n64: int, seed: int, seq: int) -> np.ndarray:
    k = np.arange(n64, dtype=np.uint64)
    return splitmix_mix(_U(device_seed(seed, seq)) + k * _U(GOLDEN))


def fill_fast(length: int, seed: int, seq: int = 1) -> bytes:
    """u64 k = splitmix-mix(seed' + k*GOLDEN)."""
    assert length % 16 == 0
    return fast_words(length // 8, seed, seq).astype("<u8").tobytes()


def rand_words(nvec2: int, seed: int, seq: int) -> np.ndarray:
    """The xoshiro fill as a flat u64 array of 2*nvec2 words.

    Thread t seeds stream A with seed' ^ (t*THREAD_MULT) and stream B with
    that ^ STREAM_B_XOR. Its m-th owned element (in increasing index order)
    holds (A's m-th output, B's m-th output).
    """
    if nvec2 == 0:
        return np.empty(0, dtype=np.uint64)
    T = threads_rand(nvec2)
    span = T * RAND_VEC_PER_STEP
    passes = (nvec2 + span - 1) // span
    n_thr = min(T, (nvec2 + RAND_VEC_PER_STEP - 1) // RAND_VEC_PER_STEP)
    per_thr = passes * RAND_VEC_PER_STEP

    t = np.arange(n_thr, dtype=np.uint64)
    seed_a = _U(device_seed(seed, seq)) ^ (t * _U(THREAD_MULT))
    a = xoshiro256pp_streams(seed_a, per_thr)
    b = xoshiro256pp_streams(seed_a ^ _U(STREAM_B_XOR), per_thr)

    # [thread, pass, v, (x|y)] -> element index = pass*span + thread*4 + v
    xy = np.stack([a, b], axis=-1).reshape(n_thr, passes, RAND_VEC_PER_STEP, 2)
    flat = xy.transpose(1, 0, 2, 3).reshape(-1)
    assert passes == 1 or n_thr == T
    return np.ascontiguousarray(flat[: 2 * nvec2])


def fill_rand(length: int, seed: int, seq: int = 1) -> bytes:
    assert length % 16 == 0
    return rand_words(length // 16, seed, seq).astype("<u8").tobytes()


def fill_const(seed: int, seq: int) -> int:
    """Host-side constant of the blockvar tail: first splitmix64 output from
    state seed + seq."""
    return splitmix64((seed + seq) & MASK)[1]


def blockvar_words(length: int, refill_len: int, seed: int, seq: int, fast: bool,
                   random_words: np.ndarray | None = None) -> np.ndarray:
    """`random_words` may pass in a precomputed rand_words/fast_words array for
    the same (length, seed, seq) so large cases are generated once."""
    assert length % 16 == 0
    nvec2 = length // 16
    refill_vec2 = min(refill_len // 16, nvec2)  # floors to a 16 B boundary
    if random_words is None:
        random_words = (fast_words(2 * nvec2, seed, seq) if fast
                        else rand_words(nvec2, seed, seq))
    out = np.full(2 * nvec2, fill_const(seed, seq), dtype=np.uint64)
    out[: 2 * refill_vec2] = random_words[: 2 * refill_vec2]
    return out


def blockvar(length: int, refill_len: int, seed: int, seq: int = 1,
             fast: bool = False) -> bytes:
    """First floor16(refill_len) bytes: the same data fill_rand / fill_fast
    would put there; the rest: fill_const repeated."""
    return blockvar_words(length, refill_len, seed, seq, fast).astype("<u8").tobytes()


def verify(data: bytes, file_off: int, salt: int) -> tuple[int, int]:
    """(number of mismatching u64 words, lowest mismatching word's file
    offset or 2^64-1)."""
    assert len(data) % 8 == 0 and file_off % 8 == 0
    got = np.frombuffer(data, dtype="<u8")
    bad = np.flatnonzero(got != checksum_words(len(data), file_off, salt))
    if bad.size == 0:
        return 0, U64_MAX
    offs = _U(file_off & MASK) + bad.astype(np.uint64) * _U(8)
    return int(bad.size), int(offs.min())
