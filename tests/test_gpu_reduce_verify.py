"""--dedupeverify on a real MI355X: ebVerifyReduceKernel through
gpu_verify_reduce against the expectations of tests/reduce_verify_cases.py and
the CPU twin, and the engine cases with gpu_ids=[0], where every block whose
length is a multiple of 16 is generated and checked in HBM.
"""

import pytest

from tests import kernel_model as km
from tests import reduce_cases as rc
from tests import reduce_verify_cases as rv

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def require_gpu(core):
    if core.gpu_device_count() < 1:
        pytest.fail("GPU test run but no HIP device available — the HIP path "
                    "must not silently fall back to CPU")


def gpu_verify(core):
    def verify(data, file_off, first, c, r, d, p, uniq=rv.UNIQ):
        got = core.gpu_verify_reduce(data, file_off, first, c, r, d, p, uniq, rv.POOL_SEED)
        assert got == core.verify_reduce(data, file_off, first, c, r, d, p, uniq,
                                         rv.POOL_SEED), "GPU and CPU verify disagree"
        return got
    return verify


@pytest.mark.parametrize("c", [16, 64, 512, 4096, 8192, 65536])
def test_kernel_agrees_with_cpu_and_expectation(core, c):
    """Chunks below 4 KiB take the per-lane key, from 4 KiB on the workgroup-
    uniform one; 5 chunks and a cut one, R at both ends and inside; clean and
    every corruption of reduce_verify_cases."""
    for r in sorted({0, 16, c // 32 * 16, c - 16, c}):
        for first, file_off in ((98, 98 * c), (2**40 + 7, 8 * 999)):
            rv.check_corruptions(gpu_verify(core), c, r, 5 * c + 16, first, file_off)


def test_single_element_and_zero_length(core):
    verify = gpu_verify(core)
    for c in (16, 4096):
        data = rc.model(16, 5, c, 16, 50, 256)
        assert verify(data, 5 * c, 5, c, 16, 50, 256) == rv.NONE
        assert verify(rv.flip(data, 9), 5 * c, 5, c, 16, 50, 256) == (1, 5 * c + 8)
    assert core.gpu_verify_reduce(b"", 4096, 1, 4096, 2048, 50, 256, 1, 2) == rv.NONE


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
    clean = rc.model(length, first, c, r, d, 256)
    file_off = first * c
    args = (file_off, first, c, r, d, 256, rv.UNIQ, rv.POOL_SEED)
    assert core.gpu_verify_reduce(clean, *args) == rv.NONE
    # one bad word each in pass 1, in pass 2 and in the partial last step
    offs = [5 * 4096 + 1032, FIRST_PASS + 4096 + 8, length - 8]
    assert core.gpu_verify_reduce(rv.flip(clean, *offs), *args) == (3, file_off + offs[0])
    assert core.gpu_verify_reduce(rv.flip(clean, *offs[1:]), *args) == (2, file_off + offs[1])
    assert core.gpu_verify_reduce(rv.flip(clean, offs[2]), *args) == (1, file_off + offs[2])


@pytest.mark.parametrize("c,length", [(64, 3 * 64 + 16), (4096, 4096 + 2048), (4096, 16)])
def test_nothing_past_len_is_read(core, c, length):
    """Bytes that match nothing lie directly behind len in the slot, up to
    the end of the last workgroup step and beyond: the result is that of the
    clean len bytes, and the first bad word before len is still reported."""
    r = c // 2
    clean = rc.model(length, 3, c, r, 50, 256)
    args = (800, 3, c, r, 50, 256, rv.UNIQ, rv.POOL_SEED)
    tail = bytes([0xA5]) * 8192
    assert core.gpu_verify_reduce(clean + tail, *args, verify_len=length) == rv.NONE
    assert core.gpu_verify_reduce(rv.flip(clean, length - 1) + tail, *args,
                                  verify_len=length) == (1, 800 + length - 8)


def test_counters_accumulate_until_fetched(core):
    c, r, d = 4096, 2048, 50
    a = rc.model(2 * c, 10, c, r, d, 256)
    b = rc.model(3 * c, 4, c, r, d, 256)
    items = [(rv.flip(a, 24, c + 8), 10 * c, 10), (rv.flip(b, 2 * c + 40), 4 * c, 4)]
    got = core.gpu_verify_reduce_batch(items, c, r, d, 256, rv.UNIQ, rv.POOL_SEED)
    assert got == [(3, 4 * c + 2 * c + 40), rv.NONE]
    clean = [(a, 10 * c, 10), (b, 4 * c, 4)]
    assert core.gpu_verify_reduce_batch(clean, c, r, d, 256, rv.UNIQ, rv.POOL_SEED) == [
        rv.NONE, rv.NONE]


@pytest.mark.parametrize("chunk,rand,d,pool", rc.BAD_GEOMETRY)
def test_bad_geometry_raises(core, chunk, rand, d, pool):
    with pytest.raises(ValueError):
        core.gpu_verify_reduce(bytes(4096), 0, 0, chunk, rand, d, pool, 1, 2)


def test_bad_length_offset_and_first_chunk_raise(core):
    with pytest.raises(ValueError, match="multiple of 16"):
        core.gpu_verify_reduce(bytes(4104), 0, 0, 4096, 2048, 50, 256, 1, 2)
    with pytest.raises(ValueError, match="multiple of 8"):
        core.gpu_verify_reduce(bytes(4096), 4, 0, 4096, 2048, 50, 256, 1, 2)
    with pytest.raises(ValueError, match="2\\^56"):
        core.gpu_verify_reduce(bytes(4096), 0, 1 << 56, 4096, 2048, 50, 256, 1, 2)


def test_bench_binding_runs(core):
    """The throughput binding at a toy size: it verifies its own clean buffer
    (and raises if that fails) and returns a positive rate."""
    for c, r in ((4096, 2048), (512, 512)):
        assert core.gpu_reduce_verify_bench_gbs(1 << 20, 2, 0, c, r, 50) > 0


# ---------------------------------------------------------------------------
# engine, gpu_ids=[0]
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(rv.ENGINE_CASES))
def test_engine_write_then_read(core, tmp_path, name):
    rv.run_engine_case(core, tmp_path, name, [0], [0])


@pytest.mark.parametrize("name", ["file2", "dir_chain"])
@pytest.mark.parametrize("write_gpu,read_gpu", [([0], []), ([], [0])])
def test_engine_gpu_and_cpu_sides_agree(core, tmp_path, name, write_gpu, read_gpu):
    rv.run_engine_case(core, tmp_path, name, write_gpu, read_gpu)
