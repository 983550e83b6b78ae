"""--dataprofile on a real MI355X: ebDataProfileKernel against the numpy model
over the case table of tests/data_profile_cases.py (the slot poisoned past
len), accumulation over blocks and contexts, and the engine's GPU staging
paths, whose profile must equal the model over the file bytes bit for bit.
"""

import os

import pytest

from elbencho_amd.pathstore import CustomTree, write_treefile
from tests import data_profile_cases as dc
from tests import data_profile_model as dm

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def require_gpu(core):
    if core.gpu_device_count() < 1:
        pytest.fail("GPU test run but no HIP device available — the HIP path "
                    "must not silently fall back to CPU")


# ---------------------------------------------------------------------------
# kernel vs model
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", dc.CONTENTS)
@pytest.mark.parametrize("chunk", dc.CHUNKS)
def test_kernel_equals_model(core, chunk, kind):
    """512 and 4096 take the wave-per-chunk kernel, 65536 the workgroup-per-
    chunk one; the lengths cut the last 16 B element, word and chunk."""
    for length in dc.LENS:
        got = core.gpu_data_profile(dc.content(core, kind, length), chunk)
        dc.assert_same(got, dc.expected(core, kind, length, chunk), (chunk, length, kind))


def test_empty_block_and_bad_chunk(core):
    dc.assert_same(core.gpu_data_profile(b"", 4096), dm.empty(), "empty")
    for chunk in (256, 6144, 32 << 20):
        with pytest.raises(ValueError):
            core.gpu_data_profile(bytes(16), chunk)


def test_more_chunks_than_teams(core):
    """9 MiB of 512-byte chunks: 18432 chunks on a grid capped at 2048
    workgroups of 4 waves, so every wave strides over several chunks."""
    data = dc.content(core, "reduce", 1 << 20) * 9
    dc.assert_same(core.gpu_data_profile(data, 512), dm.profile(data, 512), "9 MiB / 512")


BATCH = [("random", 4096 + 520 + 3), ("reduce", 1 << 20), ("zeros", 513),
         ("verify", 3 * 4096), ("last_byte", 17)]


@pytest.mark.parametrize("chunk", [512, 65536])
def test_batch_accumulates(core, chunk):
    blocks = [dc.content(core, k, n) for k, n in BATCH]
    (got,) = core.gpu_data_profile_batch(blocks, chunk)
    dc.assert_same(got, dm.profile_blocks(blocks, chunk), ("batch", chunk))


def test_two_contexts_on_one_stream_keep_their_own(core):
    blocks = [dc.content(core, k, n) for k, n in BATCH]
    got = core.gpu_data_profile_batch(blocks, 4096, contexts=2)
    assert len(got) == 2
    dc.assert_same(got[0], dm.profile_blocks(blocks[0::2], 4096), "context 0")
    dc.assert_same(got[1], dm.profile_blocks(blocks[1::2], 4096), "context 1")


# ---------------------------------------------------------------------------
# engine with --gpuids 0
# ---------------------------------------------------------------------------

GPU = ["--gpuids", "0"]


@pytest.fixture(scope="module")
def reduce_file(tmp_path_factory):
    path, data = dc.write_reduce_file(tmp_path_factory.mktemp("dp_gpu_file"))
    return path, dm.profile(data, 4096)


@pytest.mark.parametrize("tag,argv", [
    ("pipelined", ["-t", "2", "-b", "1m"]),
    ("pipelined_64k", ["-t", "3", "-b", "64k"]),
    ("iodepth4", ["-t", "2", "-b", "256k", "--iodepth", "4"]),
    ("mmap", ["-t", "2", "-b", "128k", "--mmap"]),
])
def test_engine_file_paths(reduce_file, tmp_path, tag, argv):
    path, want = reduce_file
    (got,), _ = dc.read_profiles(tmp_path, argv + GPU + [path], tag)
    dc.assert_same(got, want, tag)


def test_engine_dir_mode_linked_chains(tmp_path):
    """Files of one block with --iodepth: the linked-chain small-file path,
    and 68 KiB files in blocks of 64 KiB + 4 KiB through the per-file path."""
    small = ["-t", "2", "-n", "2", "-N", "3", "-s", "64k", "-b", "64k"]
    root = os.path.join(str(tmp_path), "s")
    os.makedirs(root)
    assert dc.run_cli(["-d", "-w", *small, "--dedupepct", "50", "--compresspct", "50",
                       root]) == 0
    want = dc.model_over_tree(root, 4096)
    (got,), _ = dc.read_profiles(tmp_path, [*small, "--iodepth", "4", *GPU, root], "chains")
    dc.assert_same(got, want, "chains")

    root, want = dc.write_dir_files(tmp_path)
    (got,), _ = dc.read_profiles(tmp_path, [*dc.DIR_ARGS, "--iodepth", "4", *GPU, root],
                                 "dir_qd4")
    dc.assert_same(got, want, "dir_qd4")
    (got,), _ = dc.read_profiles(tmp_path, [*dc.DIR_ARGS, *GPU, root], "dir_sync")
    dc.assert_same(got, want, "dir_sync")


def test_engine_custom_tree(tmp_path):
    base = tmp_path / "tree"
    base.mkdir()
    tf = tmp_path / "tree.txt"
    tree = CustomTree(dirs=["d", "e"], files=[("d/a", 200000 + 13), ("d/b", 65536),
                                              ("e/c", 3 * 4096 + 520 + 3)])
    write_treefile(tree, str(tf))
    common = ["-t", "2", "-b", "64k", "--treefile", str(tf), str(base)]
    assert dc.run_cli(["-d", "-w"] + common) == 0
    want = dc.model_over_tree(str(base), 4096)
    assert want["bytes"] == 200013 + 65536 + 12811
    (got,), _ = dc.read_profiles(tmp_path, GPU + common, "tree")
    dc.assert_same(got, want, "tree")


def test_engine_with_verify(tmp_path):
    path = str(tmp_path / "v")
    size = 1024 * 1024 + 4096 + 520
    base = ["-s", str(size), "-b", "64k", "-t", "2", "--verify", "1", *GPU, path]
    assert dc.run_cli(["-w"] + base) == 0
    (got,), _ = dc.read_profiles(tmp_path, base, "verify")
    with open(path, "rb") as f:
        dc.assert_same(got, dm.profile(f.read(), 4096), "verify")


def test_two_read_phases_each_report_one_pass(reduce_file, tmp_path):
    path, want = reduce_file
    got, _ = dc.read_profiles(tmp_path, ["-t", "2", "-b", "256k", "-i", "2", *GPU, path],
                              "twice")
    assert len(got) == 2
    for i, g in enumerate(got):
        dc.assert_same(g, want, f"pass {i}")
