"""Directory, custom-tree and mixed-mode cases of tests/engine_modes_cases.py
without a GPU (gpu_ids=[]): proves the expectations stated there - layouts,
slice and ownership rules, byte counts, error texts - on the CPU paths, which
share them with the GPU staging paths (tests/test_gpu_engine_modes.py)."""

import pytest

from tests import engine_modes_cases as c

GPU = []


@pytest.mark.parametrize("engine,bs,size,files", c.DIR_WRITE_CASES)
def test_dir_write_checksum(core, tmp_path, engine, bs, size, files):
    c.check_dir_write_checksum(core, tmp_path, GPU, engine, bs, size, files)


@pytest.mark.parametrize("case_name", list(c.DIR_VERIFY_CASES))
@pytest.mark.parametrize("engine", list(c.DIR_ENGINES))
def test_dir_verify_failure_then_clean(core, tmp_path, engine, case_name):
    c.check_dir_verify_failure(core, tmp_path, GPU, engine, case_name)


@pytest.mark.parametrize("engine", ["sync", "uring"])
def test_dir_read_inline(core, tmp_path, engine):
    c.check_dir_read_inline(core, tmp_path, GPU, engine)


@pytest.mark.parametrize("iodepth", [1, c.DEPTH])
def test_dir_dedicated_reader(core, tmp_path, iodepth):
    c.check_dir_dedicated_reader(core, tmp_path, GPU, iodepth)


@pytest.mark.parametrize("iodepth,round_robin,randomize", c.TREE_CASES)
def test_custom_tree(core, tmp_path, iodepth, round_robin, randomize):
    c.check_tree(core, tmp_path, GPU, iodepth, round_robin, randomize)


@pytest.mark.parametrize("path_name,tail,threads", c.TWO_PATH_CASES)
def test_two_paths(core, tmp_path, path_name, tail, threads):
    c.check_two_paths(core, tmp_path, GPU, path_name, tail, threads)


@pytest.mark.parametrize("order,path_name", c.ORDER_CASES)
def test_backward_and_strided(core, tmp_path, order, path_name):
    c.check_order(core, tmp_path, GPU, order, path_name)


@pytest.mark.parametrize("path_name", ["pipelined", "uring"])
def test_random_aligned_write_covers_file(core, tmp_path, path_name):
    c.check_random_aligned_write(core, tmp_path, GPU, path_name)


def test_unaligned_random_write(core, tmp_path):
    c.check_unaligned_random_write(core, tmp_path, GPU)


def test_unaligned_random_read(core, tmp_path):
    c.check_unaligned_random_read(core, tmp_path, GPU)


@pytest.mark.parametrize("fill", [("checksum", c.SALT), ("blockvar", 100, "fast")],
                         ids=["checksum", "bv100fast"])
@pytest.mark.parametrize("path_name", ["blockio", "uring"])
def test_verify_direct(core, tmp_path, path_name, fill):
    c.check_verify_direct(core, tmp_path, GPU, path_name, fill)


@pytest.mark.parametrize("dedicated", [False, True], ids=["pct30", "pct30_reader"])
def test_rwmix_file(core, tmp_path, dedicated):
    c.check_rwmix_file(core, tmp_path, GPU, dedicated)


@pytest.mark.parametrize("name", list(c.LAT_CASES))
def test_lat_one_sample_per_block(core, tmp_path, name):
    c.check_lat_file(core, tmp_path, GPU, name)


@pytest.mark.parametrize("name,tail", c.LAT_AFTER_FAILURE)
def test_lat_after_failed_read(core, tmp_path, name, tail):
    c.check_lat_after_failed_read(core, tmp_path, GPU, name, tail)


@pytest.mark.parametrize("engine,phase", c.LAT_DIR_CASES)
def test_lat_dir_mode(core, tmp_path, engine, phase):
    c.check_lat_dir(core, tmp_path, GPU, engine, phase)
