"""CPU side of tests/test_gpu_shared_streams.py (no GPU needed): the slice
oracle at 16 and 17 workers against what a CPU engine run reports, the refusals
of Engine.gpu_streams(), and the child runner without a device."""

import os
import subprocess
import sys

import pytest

from tests import shared_streams_cases as c
from tests.test_gpu_engine_exact import (B4K, SALT, assert_shares, fair_share, file_cfg,
                                         pattern_bytes, random_share, run_ok)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# the geometries of the GPU cases: 256 KiB x 5 blocks per worker (17 workers:
# + 8 bytes, a short block of its own for the last worker), 4 KiB x 513
@pytest.mark.parametrize("bs,blocks,threads,tail", [
    (c.BS256K, 5, 16, 0), (c.BS256K, 5, 17, 8), (4096, 2 * B4K + 1, 16, 0),
    (4096, 2 * B4K + 1, 17, 8), (4096, c.VERIFY_BLOCKS, 16, 0)],
    ids=["256k-w16", "256k-w17+8", "4k-w16", "4k-w17+8", "4k-verify-w16"])
def test_slice_rules_equal_cpu_engine(core, tmp_path, bs, blocks, threads, tail):
    size = threads * blocks * bs + tail
    what = f"bs={bs} blocks={blocks} threads={threads} tail={tail}"
    shares = fair_share(size, bs, threads)
    assert sum(s.nbytes for s in shares) == size
    assert [s.num_blocks for s in shares] == [blocks] * (threads - 1) + [blocks + bool(tail)]
    assert shares[-1].nbytes == blocks * bs + tail

    p = tmp_path / "f"
    eng = core.Engine(file_cfg(p, size, bs, threads, verify_salt=SALT))
    eng.prepare()
    assert_shares(run_ok(core, eng, "WRITE"), shares, what + " WRITE")
    assert p.read_bytes() == pattern_bytes(size, SALT)
    assert_shares(run_ok(core, eng, "READ"), shares, what + " READ")

    # random order: whole blocks only, the ragged tail belongs to nobody
    rshares = random_share(size, bs, threads)
    assert [(s.num_blocks, s.nbytes) for s in rshares] == [(blocks, blocks * bs)] * threads
    eng = core.Engine(file_cfg(p, size, bs, threads, random=True))
    eng.prepare()
    assert_shares(run_ok(core, eng, "READ"), rshares, what + " random READ")


def test_gpu_streams_needs_gpu_contexts_and_an_idle_engine(core, tmp_path):
    """Engine.gpu_streams (which HIP stream each worker is on, for the GPU
    tests) has the contract of gpu_slots: it raises for workers without a GPU
    context, as those of a CPU-only run, and raises instead of blocking while
    a phase runs."""
    p = str(tmp_path / "f")
    eng = core.Engine(dict(paths=[p], path_type="file", threads=2, num_dataset_threads=2,
                           file_size=2 << 20, block_size=1 << 20))
    eng.prepare()
    with pytest.raises(RuntimeError, match="no GPU context"):
        eng.gpu_streams()
    eng.start_phase(core.PHASES["WRITE"])
    with pytest.raises(RuntimeError, match="phase is running"):
        eng.gpu_streams()
    assert eng.wait_phase_done(30_000)
    with pytest.raises(RuntimeError, match="phase is running"):
        eng.gpu_streams()  # until finish_phase
    assert not [r["error"] for r in eng.finish_phase() if r["error"]]
    with pytest.raises(RuntimeError, match="worker 0 has no GPU context"):
        eng.gpu_streams()


def test_child_refuses_without_a_device():
    """tests.shared_streams_child with every device hidden: non-zero exit and
    a message that says why, no JSON line, no CPU run in its place."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", EB_GPU_SHARED_STREAMS="4")
    proc = subprocess.run([sys.executable, "-m", "tests.shared_streams_child"], env=env,
                          cwd=REPO, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 2, (proc.returncode, proc.stdout, proc.stderr)
    assert "no HIP device available" in proc.stderr, proc.stderr
    assert proc.stdout.strip() == "", proc.stdout
