"""--dedupepct / --compresspct on a real MI355X: ebFillReduceKernel through
gpu_fill_reduce against the numpy model (tests/reduce_model.py) and the CPU
twin, and the engine cases of tests/reduce_cases.py with gpu_ids=[0], where
every block whose length is a multiple of 16 is generated in HBM. Expected
bytes are the ones the CPU run is held to.
"""

import pytest

from tests import kernel_model as km
from tests import reduce_cases as rc

pytestmark = pytest.mark.gpu

PAD = 64
SENTINEL = 0xA5


@pytest.fixture(autouse=True)
def require_gpu(core):
    if core.gpu_device_count() < 1:
        pytest.fail("GPU test run but no HIP device available — the HIP path "
                    "must not silently fall back to CPU")


def gpu_fill(core, length, first, c, r, d, p, pad=PAD):
    """The kernel's bytes; the sentinel behind them must be intact."""
    raw = core.gpu_fill_reduce(length, first, c, r, d, p, rc.UNIQ, rc.POOL_SEED, pad=pad,
                               sentinel=SENTINEL)
    assert len(raw) == length + pad
    assert raw[length:] == bytes([SENTINEL]) * pad, (
        f"write past len={length} (C={c} R={r} d={d} P={p} first={first})")
    return raw[:length]


@pytest.mark.parametrize("d", rc.PCTS)
@pytest.mark.parametrize("c", rc.CHUNKS)
def test_kernel_equals_model_and_cpu(core, c, d):
    for r, p, first, length in rc.grid(c, d, gpu=True):
        got = gpu_fill(core, length, first, c, r, d, p)
        what = (c, r, d, p, first, length)
        assert got == rc.model(length, first, c, r, d, p), what
        assert got == core.fill_reduce(length, first, c, r, d, p, rc.UNIQ, rc.POOL_SEED), what


def test_single_lane(core):
    for c in rc.CHUNKS:
        got = gpu_fill(core, 16, 5, c, 16, 50, 256)
        assert got == rc.model(16, 5, c, 16, 50, 256)
    assert core.gpu_fill_reduce(0, 0, 4096, 2048, 50, 256, 1, 2, pad=16) == bytes([SENTINEL]) * 16


# one workgroup step is 256 elements of 16 B; the grid is capped at
# kernel_model.MAX_BLOCKS workgroups, so from this length on a workgroup takes
# a second grid-stride step
FIRST_PASS = km.MAX_BLOCKS * km.BLOCK * 16


@pytest.mark.parametrize("c,r,d,first", [
    (16, 16, 50, 0),               # dense chunk boundaries, the per-lane key path
    (4096, 2048, 33, 2**40 + 7),   # the uniform key path across the wrap
])
def test_grid_stride_wrap(core, c, r, d, first):
    length = FIRST_PASS + 3 * 4096 + 48  # a partial last workgroup step in pass 2
    got = gpu_fill(core, length, first, c, r, d, 256)
    want = rc.model(length, first, c, r, d, 256)
    if got != want:
        raise AssertionError(rc.first_diff_report(got, want))


@pytest.mark.parametrize("c", [16, 64, 512, 4096, 8192, 65536])
def test_chunk_sizes_around_the_uniform_threshold(core, c):
    """Chunks below 4 KiB take the per-lane key, from 4 KiB on the workgroup-
    uniform one; 5 chunks and a cut one, R at both ends and inside."""
    length = 5 * c + 16
    for r in sorted({0, 16, c // 32 * 16, c - 16, c}):  # c // 32 * 16: half, in 16 B units
        for d in (0, 50, 100):
            got = gpu_fill(core, length, 98, c, r, d, 3)
            assert got == rc.model(length, 98, c, r, d, 3), (c, r, d)


def test_zero_and_full_random(core):
    c, n = 4096, 40
    assert gpu_fill(core, n * c, 0, c, 0, 50, 256) == bytes(n * c)
    full = gpu_fill(core, n * c, 0, c, c, 0, 256)
    assert full == rc.model(n * c, 0, c, c, 0, 256)
    assert all(ch[-16:] != bytes(16) for ch in rc.split_chunks(full, c)), "no zero tail"
    rc.check_properties(full, n, 0, c, c, 0, 256, "R=C")


@pytest.mark.parametrize("d", rc.PCTS)
def test_properties_of_kernel_output(core, d):
    c, n = 4096, 300
    for r in (16, 2048):
        for p in (3, 256):
            data = gpu_fill(core, n * c, 0, c, r, d, p)
            rc.check_properties(data, n, 0, c, r, d, p, f"gpu R={r} d={d} P={p}")


@pytest.mark.parametrize("chunk,rand,d,pool", rc.BAD_GEOMETRY)
def test_bad_geometry_raises(core, chunk, rand, d, pool):
    with pytest.raises(ValueError):
        core.gpu_fill_reduce(4096, 0, chunk, rand, d, pool, 1, 2)


def test_bad_length_and_first_chunk_raise(core):
    with pytest.raises(ValueError, match="multiple of 16"):
        core.gpu_fill_reduce(4104, 0, 4096, 2048, 50, 256, 1, 2)
    with pytest.raises(ValueError, match="2\\^56"):
        core.gpu_fill_reduce(4096, 1 << 56, 4096, 2048, 50, 256, 1, 2)


def test_does_not_touch_the_fill_counter(core):
    """A block-variance refill that follows fillReduceDev on the same context
    is that context's fill call 1: fillReduceDev takes no fill-call number."""
    got = core.gpu_fill_reduce(4096, 0, 4096, 2048, 50, 256, 1, 2, then_blockvar_seed=9)
    assert got == km.blockvar_words(4096, 2048, 9, 1, True).astype("<u8").tobytes()


# ---------------------------------------------------------------------------
# engine, gpu_ids=[0]
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(rc.ENGINE_CASES))
def test_engine_writes_the_model(core, tmp_path, name):
    rc.run_engine_case(core, tmp_path, [0], name)


def test_engine_second_phase(core, tmp_path):
    rc.run_two_phases(core, tmp_path, [0])
