"""Bit-exact tests of the gfx950 fill / verify kernels (real MI355X).

Every comparison is exact: the bytes a host wrapper produces must equal
tests/kernel_model.py (a plain numpy statement of the same operation, itself
checked on the CPU in test_kernel_model.py), and every verify result must
equal the model's (count, first offset) as integers. Fills run in a buffer
with a sentinel-filled guard region behind `len`; the guard must come back
untouched, because the engine's io-depth slots are contiguous.

Sizes are the smallest that reach each hazard: 1/63/64/65/255/256/257/1023/
1024/1025 vec2 (16 B) elements, counts not divisible by 4 on the xoshiro
path, and one large size per kernel family - the first at which a thread
runs a second grid-stride pass (16 MiB + 48 B for the one-element-per-thread
kernels, 64 MiB + 80 B for the four-elements-per-thread xoshiro kernels).
"""

import functools

import numpy as np
import pytest

from tests import kernel_model as km

pytestmark = pytest.mark.gpu

U64_MAX = 2**64 - 1
GUARD = 4096
SENTINEL = 0xA5

FILL_LENS = [16, 48, 64, 80, 1008, 1024, 1040, 4080, 4096, 4112, 16368, 16384, 16400]
WRAP_STRIDED = (16 << 20) + 48  # 4096*256 elements per pass, +3
WRAP_RAND = (64 << 20) + 80     # 4096*256*4 elements per pass, +5

SEED = 12345


@pytest.fixture(autouse=True)
def require_gpu(core):
    if core.gpu_device_count() < 1:
        pytest.fail("GPU test run but no HIP device available — the HIP path "
                    "must not silently fall back to CPU")


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------

def assert_fill_exact(got: bytes, expect_words: np.ndarray, ln: int, family: str):
    """got = len+GUARD bytes from gpu_fill_guarded. Bytes below ln must equal
    the model, guard bytes must still be the sentinel."""
    assert len(got) == ln + GUARD
    assert expect_words.size * 8 == ln
    words = np.frombuffer(got, dtype="<u8", count=ln // 8)
    if not np.array_equal(words, expect_words):
        w = int(np.flatnonzero(words != expect_words)[0])
        nvec2 = ln // 16
        idx = w // 2
        where = ("odd final u64 (thread 0)" if idx >= nvec2 else
                 "thread %d, iteration %d" % km.owner(family, idx, nvec2))
        n_diff = int(np.count_nonzero(words != expect_words))
        pytest.fail(f"len={ln}: first difference at vec2 element {idx} "
                    f"({'xy'[w & 1]} half, byte {w * 8}), owned by {where}: "
                    f"got {int(words[w]):#018x}, model {int(expect_words[w]):#018x}; "
                    f"{n_diff} of {words.size} u64 differ")
    guard = np.frombuffer(got, dtype=np.uint8, offset=ln)
    if not np.all(guard == SENTINEL):
        g = int(np.flatnonzero(guard != SENTINEL)[0])
        pytest.fail(f"len={ln}: kernel wrote past len: guard byte {g} (buffer byte "
                    f"{ln + g}) is {int(guard[g]):#04x}, sentinel {SENTINEL:#04x}; "
                    f"{int(np.count_nonzero(guard != SENTINEL))} guard bytes changed")


def guarded(core, op, ln, a=0, b=0, fast=False, calls=1):
    return core.gpu_fill_guarded(op, ln, GUARD, a, b, fast, SENTINEL, calls)


@functools.lru_cache(maxsize=None)
def rand_words_cached(nvec2: int, seed: int, seq: int) -> np.ndarray:
    w = km.rand_words(nvec2, seed, seq)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def clean_pattern(ln: int, off: int, salt: int) -> bytes:
    return km.checksum_pattern(ln, off, salt)


def corrupt(clean: bytes, words, mask=0x0100000000000001) -> bytes:
    """XOR `mask` into the given u64 word indices."""
    a = np.frombuffer(clean, dtype="<u8").copy()
    a[list(words)] ^= np.uint64(mask)
    return a.tobytes()


def assert_verify_exact(core, data: bytes, off: int, salt: int, lds: bool):
    got = tuple(core.gpu_verify_checksum(data, off, salt, 0, lds))
    want = km.verify(data, off, salt)
    if got != want:
        nvec2 = len(data) // 16
        bad = np.flatnonzero(np.frombuffer(data, dtype="<u8") !=
                             km.checksum_words(len(data), off, salt))
        owners = [(int(w) // 2,) + (km.owner("strided", int(w) // 2, nvec2)
                                    if int(w) // 2 < nvec2 else ("tail",))
                  for w in bad[:8]]
        pytest.fail(f"verify(lds={lds}) len={len(data)} off={off}: got (count, first)="
                    f"{got}, model {want}; corrupt (element, thread, iteration): {owners}")
    return got


# ---------------------------------------------------------------------------
# fills
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("ln", FILL_LENS + [n + 8 for n in FILL_LENS])
def test_fill_checksum_exact(core, ln):
    off, salt = 8192, 7
    got = guarded(core, "checksum", ln, off, salt)
    assert_fill_exact(got, km.checksum_words(ln, off, salt), ln, "strided")
    assert got[:ln] == core.fill_checksum(ln, off, salt)


@pytest.mark.parametrize("off,salt", [
    (0, 7), (8, 7), (1 << 30, 1), (2**63, 42), (2**64 - 4096, 2**64 - 1),
])
@pytest.mark.parametrize("ln", [1040, 4088, 8200])  # 8200 runs past 2^64 in the last case
def test_fill_checksum_offsets_and_salt(core, ln, off, salt):
    got = guarded(core, "checksum", ln, off, salt)
    assert_fill_exact(got, km.checksum_words(ln, off, salt), ln, "strided")
    assert got[:ln] == core.fill_checksum(ln, off, salt)
    assert core.gpu_fill_checksum(ln, off, salt) == got[:ln]


@pytest.mark.parametrize("ln", FILL_LENS)
def test_fill_fast_exact(core, ln):
    got = guarded(core, "rand", ln, SEED, fast=True)
    assert_fill_exact(got, km.fast_words(ln // 8, SEED, 1), ln, "strided")


@pytest.mark.parametrize("ln", FILL_LENS)
def test_fill_rand_exact(core, ln):
    got = guarded(core, "rand", ln, SEED)
    assert_fill_exact(got, km.rand_words(ln // 16, SEED, 1), ln, "rand")


@pytest.mark.parametrize("fast", [False, True], ids=["xoshiro", "fast"])
@pytest.mark.parametrize("ln", FILL_LENS)
def test_blockvar_exact(core, ln, fast):
    refill = ln * 37 // 100
    got = guarded(core, "blockvar", ln, SEED, refill, fast)
    assert_fill_exact(got, km.blockvar_words(ln, refill, SEED, 1, fast), ln,
                      "strided" if fast else "rand")


BV_LEN = 4112  # 257 elements: two blocks on the fast path, not a multiple of 4


@pytest.mark.parametrize("fast", [False, True], ids=["xoshiro", "fast"])
@pytest.mark.parametrize("refill", [0, 8, 16, 24, BV_LEN - 16, BV_LEN, BV_LEN + 4096,
                                    BV_LEN * 37 // 100])
def test_blockvar_refill_len(core, refill, fast):
    ln = BV_LEN
    got = guarded(core, "blockvar", ln, SEED, refill, fast)
    assert_fill_exact(got, km.blockvar_words(ln, refill, SEED, 1, fast), ln,
                      "strided" if fast else "rand")
    # stated separately: head is the model's random data, tail the host constant
    head_len = min(refill // 16 * 16, ln)
    rnd = km.fill_fast(ln, SEED, 1) if fast else km.fill_rand(ln, SEED, 1)
    assert got[:head_len] == rnd[:head_len]
    const = km.fill_const(SEED, 1).to_bytes(8, "little")
    assert got[head_len:ln] == const * ((ln - head_len) // 8)


def test_fill_call_counter(core):
    """The per-context fill counter enters the device seed: two consecutive
    calls on one context are the model at seq=1 then seq=2."""
    ln = 4112
    ops = core.GpuBufferOps(0, 1 << 20)
    first, second = ops.fill_rand(ln, SEED), ops.fill_rand(ln, SEED)
    assert first == km.fill_rand(ln, SEED, 1)
    assert second == km.fill_rand(ln, SEED, 2)
    assert first != second
    # the counter is shared by every fill kind: after two calls the buffer
    # holds the seq=2 result
    assert_fill_exact(guarded(core, "rand", ln, SEED, fast=True, calls=2),
                      km.fast_words(ln // 8, SEED, 2), ln, "strided")
    assert_fill_exact(guarded(core, "blockvar", ln, SEED, 1024, calls=2),
                      km.blockvar_words(ln, 1024, SEED, 2, False), ln, "rand")
    assert_fill_exact(guarded(core, "blockvar", ln, SEED, 1024, fast=True, calls=2),
                      km.blockvar_words(ln, 1024, SEED, 2, True), ln, "strided")


# --- grid-stride wrap: the only large cases ---

def test_wrap_fill_checksum(core):
    ln, off, salt = WRAP_STRIDED, 1 << 30, 7
    assert_fill_exact(guarded(core, "checksum", ln, off, salt),
                      km.checksum_words(ln, off, salt), ln, "strided")


def test_wrap_fill_fast(core):
    ln = WRAP_STRIDED
    assert_fill_exact(guarded(core, "rand", ln, SEED, fast=True),
                      km.fast_words(ln // 8, SEED, 1), ln, "strided")


def test_wrap_blockvar_fast(core):
    ln = WRAP_STRIDED
    refill = ln - 16  # second pass holds two random elements and one constant
    assert_fill_exact(guarded(core, "blockvar", ln, SEED, refill, fast=True),
                      km.blockvar_words(ln, refill, SEED, 1, True), ln, "strided")


def test_wrap_fill_rand(core):
    ln = WRAP_RAND
    assert_fill_exact(guarded(core, "rand", ln, SEED),
                      rand_words_cached(ln // 16, SEED, 1), ln, "rand")


def test_wrap_blockvar(core):
    ln = WRAP_RAND
    refill = ln - 32  # second pass holds three random elements and two constant
    want = km.blockvar_words(ln, refill, SEED, 1, False,
                             random_words=rand_words_cached(ln // 16, SEED, 1))
    assert_fill_exact(guarded(core, "blockvar", ln, SEED, refill), want, ln, "rand")


# --- argument contract ---

def test_wrappers_reject_misaligned_arguments(core):
    """Nothing is dropped silently: lengths and offsets the kernels cannot
    cover are refused before any launch."""
    for ln, off in [(20, 0), (4100, 0), (4096, 4), (16, 1)]:
        with pytest.raises(ValueError):
            core.gpu_fill_checksum(ln, off, 7)
        with pytest.raises(ValueError):
            core.gpu_verify_checksum(b"\0" * ln, off, 7)
        with pytest.raises(ValueError):
            core.gpu_verify_checksum(b"\0" * ln, off, 7, 0, True)
    ops = core.GpuBufferOps(0, 1 << 16)
    with pytest.raises(ValueError):
        ops.verify(b"\0" * 20, 0, 7)
    with pytest.raises(ValueError):
        ops.fill_checksum(20, 0, 7)
    for ln in (8, 24, 4104, 4100):
        for fast in (False, True):
            with pytest.raises(ValueError):
                core.gpu_fill_rand(ln, SEED, 0, fast)
            with pytest.raises(ValueError):
                core.gpu_blockvar_refill(ln, 16, SEED, 0, fast)
        with pytest.raises(ValueError):
            ops.fill_rand(ln, SEED)
    # a refused call did not advance the fill counter
    assert ops.fill_rand(64, SEED) == km.fill_rand(64, SEED, 1)


# ---------------------------------------------------------------------------
# verify (production kernel and the LDS-tiled A/B variant, same model)
# ---------------------------------------------------------------------------

VARIANTS = pytest.mark.parametrize("lds", [False, True], ids=["prod", "lds"])
V_LEN, V_OFF, V_SALT = 16400, 8192, 42  # 1025 elements: 5 blocks, 2 LDS tiles


@VARIANTS
@pytest.mark.parametrize("ln", [16, 4096, V_LEN])
def test_verify_clean(core, ln, lds):
    data = clean_pattern(ln, V_OFF, V_SALT)
    assert assert_verify_exact(core, data, V_OFF, V_SALT, lds) == (0, U64_MAX)


@VARIANTS
@pytest.mark.parametrize("word", [0, V_LEN // 8 - 1, 600, 601],
                         ids=["first", "last", "x-half", "y-half"])
def test_verify_single_word(core, word, lds):
    data = corrupt(clean_pattern(V_LEN, V_OFF, V_SALT), [word])
    got = assert_verify_exact(core, data, V_OFF, V_SALT, lds)
    assert got == (1, V_OFF + word * 8)


@VARIANTS
@pytest.mark.parametrize("elems", [(63,), (64,), (63, 64), (255,), (256,), (255, 256),
                                   (1023,), (1024,), (1023, 1024)],
                         ids=lambda e: "e" + "_".join(map(str, e)))
def test_verify_lane_block_tile_edges(core, elems, lds):
    # y half of the lower element, x half of the upper: adjacent words that
    # sit in different lanes / waves / blocks / LDS tiles
    words = [2 * e + (1 if e % 2 else 0) for e in elems]
    data = corrupt(clean_pattern(V_LEN, V_OFF, V_SALT), words)
    got = assert_verify_exact(core, data, V_OFF, V_SALT, lds)
    assert got == (len(words), V_OFF + min(words) * 8)


@VARIANTS
def test_verify_two_blocks_reports_lower_offset(core, lds):
    clean = clean_pattern(V_LEN, V_OFF, V_SALT)
    for words in ([2 * 900, 2 * 100 + 1], [2 * 1024, 2 * 3, 2 * 700 + 1]):
        got = assert_verify_exact(core, corrupt(clean, words), V_OFF, V_SALT, lds)
        assert got == (len(words), V_OFF + min(words) * 8)


@VARIANTS
def test_verify_every_word_corrupt(core, lds):
    ln = 1 << 20
    data = corrupt(clean_pattern(ln, V_OFF, V_SALT), range(ln // 8))
    got = assert_verify_exact(core, data, V_OFF, V_SALT, lds)
    assert got == (ln // 8, V_OFF)


@VARIANTS
def test_wrap_verify(core, lds):
    ln = WRAP_STRIDED
    clean = clean_pattern(ln, V_OFF, V_SALT)
    assert assert_verify_exact(core, clean, V_OFF, V_SALT, lds) == (0, U64_MAX)
    first_pass = 4096 * 256
    # only second-pass elements corrupt: y half of element T+1, x half of the last
    words = [2 * (first_pass + 1) + 1, 2 * (ln // 16 - 1)]
    got = assert_verify_exact(core, corrupt(clean, words), V_OFF, V_SALT, lds)
    assert got == (2, V_OFF + words[0] * 8)
    # a first-pass and a second-pass mismatch of the same thread
    words = [2 * (first_pass + 2), 2 * 2 + 1]
    got = assert_verify_exact(core, corrupt(clean, words), V_OFF, V_SALT, lds)
    assert got == (2, V_OFF + words[1] * 8)


@VARIANTS
def test_verify_counters_persist_until_fetch(core, lds):
    """Async launches accumulate into the context's device counters; one
    fetch returns the totals and resets them."""
    ln, salt = 4112, V_SALT
    offs = [1 << 20, 2 << 20, 3 << 20]
    a = clean_pattern(ln, offs[0], salt)
    b = corrupt(clean_pattern(ln, offs[1], salt), [301, 40])
    c = corrupt(clean_pattern(ln, offs[2], salt), [0, 1, 127, 128, 513])
    for data, off, n in ((a, offs[0], 0), (b, offs[1], 2), (c, offs[2], 5)):
        assert km.verify(data, off, salt)[0] == n
    later = clean_pattern(ln, offs[0], salt)
    res = core.gpu_verify_batch([(a, offs[0]), (b, offs[1]), (c, offs[2])], salt, lds,
                                (later, offs[0]))
    assert [tuple(r) for r in res] == [(7, offs[1] + 40 * 8), (0, U64_MAX), (0, U64_MAX)]
    # order of the launches does not matter for the minimum
    res = core.gpu_verify_batch([(c, offs[2]), (b, offs[1]), (a, offs[0])], salt, lds)
    assert [tuple(r) for r in res] == [(7, offs[1] + 40 * 8), (0, U64_MAX)]


@VARIANTS
@pytest.mark.parametrize("ln", [8, 24, 4104])
def test_verify_odd_final_word(core, ln, lds):
    """len % 16 == 8: the final u64 is checked like any other (the fill
    kernel writes it, so verify must read it)."""
    clean = clean_pattern(ln, V_OFF, V_SALT)
    assert assert_verify_exact(core, clean, V_OFF, V_SALT, lds) == (0, U64_MAX)
    data = corrupt(clean, [ln // 8 - 1])
    got = assert_verify_exact(core, data, V_OFF, V_SALT, lds)
    assert got == (1, V_OFF + ln - 8)
    if ln > 8:  # tail and body together: exact count, lowest offset
        data = corrupt(clean, [ln // 8 - 1, 1])
        got = assert_verify_exact(core, data, V_OFF, V_SALT, lds)
        assert got == (2, V_OFF + 8)


def test_buffer_ops_verify_odd_final_word(core):
    ops = core.GpuBufferOps(0, 1 << 16)
    ln = 4104
    clean = clean_pattern(ln, V_OFF, V_SALT)
    assert tuple(ops.verify(clean, V_OFF, V_SALT)) == (0, U64_MAX)
    bad = corrupt(clean, [ln // 8 - 1])
    assert tuple(ops.verify(bad, V_OFF, V_SALT)) == (1, V_OFF + ln - 8)
    assert tuple(ops.verify(clean, V_OFF, V_SALT)) == (0, U64_MAX)
