"""CPU checks of tests/kernel_model.py - the numpy specification the GPU
kernel tests compare against. The model must be trusted on its own, so it
is tied here to published constants and to the CPU implementations in
csrc/ (checksum fill/verify, xoshiro256++), without a GPU."""

import numpy as np
import pytest

from tests import kernel_model as km

U64_MAX = 2**64 - 1


def test_splitmix64_known_answers():
    # published splitmix64 test vector (state 0)
    state, first = km.splitmix64(0)
    assert first == 0xE220A8397B1DCDAF
    state, second = km.splitmix64(state)
    assert second == 0x6E789E6AA1B965F4
    # vector form agrees with the scalar form
    assert int(km.splitmix_mix(np.uint64(km.GOLDEN))) == first


@pytest.mark.parametrize("off,salt", [
    (0, 0), (8, 7), (4096, 123), (1 << 30, 1), (2**63, 42),
    (2**64 - 4096, 2**64 - 1),  # values wrap mod 2^64
])
@pytest.mark.parametrize("ln", [8, 16, 24, 4080, 4088])
def test_checksum_pattern_matches_cpu_fill(core, ln, off, salt):
    assert km.checksum_pattern(ln, off, salt) == core.fill_checksum(ln, off, salt)


def test_checksum_pattern_wraps_past_zero():
    # offsets themselves wrap: word i sits at (off + 8i) mod 2^64
    w = km.checksum_words(32, 2**64 - 16, 5)
    assert [int(x) for x in w] == [2**64 - 16 + 5, 2**64 - 8 + 5, 5, 13]


def test_verify_agrees_with_cpu_verify(core):
    ln, off, salt = 4096 + 8, 1 << 20, 99
    clean = km.checksum_pattern(ln, off, salt)
    assert km.verify(clean, off, salt) == (0, U64_MAX)
    assert core.verify_checksum(clean, off, salt) == U64_MAX

    for byte in (0, 7, 8, 1023, 2049, ln - 8, ln - 1):
        data = bytearray(clean)
        data[byte] ^= 0x40
        n_bad, first = km.verify(bytes(data), off, salt)
        cpu_first_byte = core.verify_checksum(bytes(data), off, salt)
        assert n_bad == 1
        # the model names the word, the CPU verify the byte inside it
        assert first == cpu_first_byte & ~7 == off + (byte & ~7)

    # several bad words: exact count, lowest offset
    data = bytearray(clean)
    for word in (500, 17, 300):
        data[word * 8 + 3] ^= 1
    assert km.verify(bytes(data), off, salt) == (3, off + 17 * 8)
    assert core.verify_checksum(bytes(data), off, salt) == off + 17 * 8 + 3


@pytest.mark.parametrize("seed", [0, 1, 0x243F6A88, 2**64 - 1,
                                  0xDEADBEEF ^ (3 * km.THREAD_MULT) % 2**64])
def test_xoshiro_stream_matches_cpu_implementation(core, seed):
    n = 257
    model = km.xoshiro256pp_streams([seed], n)[0]
    cpu = np.frombuffer(core.xoshiro256pp_stream(seed, n), dtype="<u8")
    assert np.array_equal(model, cpu)


def test_xoshiro_streams_vectorised_equals_one_by_one():
    seeds = [5, 6, 2**63, 2**64 - 2]
    both = km.xoshiro256pp_streams(seeds, 16)
    for i, s in enumerate(seeds):
        assert np.array_equal(both[i], km.xoshiro256pp_streams([s], 16)[0])


def test_rand_layout_small_by_hand():
    """rand_words against a direct per-element statement of the layout at a
    size with 5 threads' worth of elements and a partial last thread."""
    nvec2, seed, seq = 18, 77, 3
    words = km.rand_words(nvec2, seed, seq)
    assert words.size == 2 * nvec2
    sp = km.device_seed(seed, seq)
    assert sp == (77 + 3 * 0x9E3779B9) % 2**64
    for idx in range(nvec2):
        t, j = km.owner("rand", idx, nvec2)
        assert j == 0 and t == idx // 4
        sa = sp ^ ((t * km.THREAD_MULT) % 2**64)
        a = km.xoshiro256pp_streams([sa], 4)[0]
        b = km.xoshiro256pp_streams([sa ^ km.STREAM_B_XOR], 4)[0]
        assert words[2 * idx] == a[idx % 4]
        assert words[2 * idx + 1] == b[idx % 4]


def test_geometry():
    assert km.threads_rand(1) == 256
    assert km.threads_rand(4 * 256) == 256
    assert km.threads_rand(4 * 256 + 4) == 512
    assert km.threads_rand(1 << 40) == 256 * 4096
    assert km.threads_strided(257) == 512
    # first sizes at which a thread runs a second pass
    n16 = ((16 << 20) + 48) // 16
    assert km.owner("strided", n16 - 1, n16) == (2, 1)
    n64 = ((64 << 20) + 80) // 16
    assert km.owner("rand", n64 - 1, n64) == (1, 1)
    assert km.owner("rand", n64 - 2, n64) == (0, 1)


def test_blockvar_model_structure():
    ln, seed = 4096, 9
    for fast in (False, True):
        rnd = km.fill_fast(ln, seed, 1) if fast else km.fill_rand(ln, seed, 1)
        const = km.fill_const(seed, 1).to_bytes(8, "little")
        assert km.blockvar(ln, 0, seed, 1, fast) == const * (ln // 8)
        assert km.blockvar(ln, 15, seed, 1, fast) == const * (ln // 8)
        assert km.blockvar(ln, ln + 4096, seed, 1, fast) == rnd
        got = km.blockvar(ln, 24, seed, 1, fast)  # floors to 16
        assert got == rnd[:16] + const * ((ln - 16) // 8)
    assert km.fill_const(seed, 1) == km.splitmix64(seed + 1)[1]
