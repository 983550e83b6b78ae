"""The exact GPU staging tests at the benchmark's concurrency: several workers
per HIP stream (real MI355X).

GpuCtx does not own a stream by default: contexts draw from a process-wide
pool (8 per device, EB_GPU_SHARED_STREAMS changes it), so with 16 workers two
host threads enqueue copies, fills, verifies, events and counter fetches into
every stream, and with 17 one stream carries three. The cases are those of
tests/test_gpu_engine_exact.py at that worker count (tests/shared_streams_cases.py);
every one asserts the stream layout it relies on from Engine.gpu_streams().

A. write - file bytes equal the model;
B. read, verify off - every worker's slots hold blocks of its own slice;
C. verify failures - reported by the worker whose slice is damaged, with its
   own slice's offset and word count, and gone on the next READ;
D. lat=True - one sample per block per worker;
E. pool sizes 4 (the benchmark's), 1 and 0 - a fresh child process each,
   because the pool size is read once per process.
"""

import collections
import json
import os
import subprocess
import sys

import pytest

from tests import shared_streams_cases as c
from tests.test_gpu_engine_exact import B4K, FILL_IDS, FILLS

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def require_gpu(core):
    if core.gpu_device_count() < 1:
        pytest.fail("GPU test run but no HIP device available — the HIP path "
                    "must not silently fall back to CPU")


def test_layout_rule_is_what_the_cases_claim():
    assert c.expected_histogram(16, 8) == [2] * 8          # every stream twice
    assert c.expected_histogram(17, 8) == [2] * 7 + [3]    # one stream three times
    assert c.expected_histogram(16, 4) == [4] * 4
    assert c.expected_histogram(16, 1) == [16]
    assert c.expected_histogram(16, 0) == [1] * 16


# ---------------------------------------------------------------------------
# A. write
# ---------------------------------------------------------------------------

A_FILLS = [FILLS[0], FILLS[4], FILLS[1], FILLS[5]]
A_FILL_IDS = [FILL_IDS[0], FILL_IDS[4], FILL_IDS[1], FILL_IDS[5]]
assert A_FILL_IDS == ["checksum", "bv37strong", "bv100fast", "bv0ring"]


# 256 KiB blocks run on a two-slot ring (io_uring: four slots): five blocks
# per worker wrap it twice. 17 workers: the file ends 8 bytes into a block of
# its own, which the last worker writes after its five whole ones.
@pytest.mark.parametrize("threads,tail", [(16, 0), (17, 8)], ids=["w16", "w17+8"])
@pytest.mark.parametrize("fill", A_FILLS, ids=A_FILL_IDS)
@pytest.mark.parametrize("path_name", ["pipelined", "uring", "mmap"])
def test_write_file_bytes_equal_model(core, tmp_path, capfd, monkeypatch, path_name, fill,
                                      threads, tail):
    c.check_write(core, tmp_path, capfd, monkeypatch, path_name, fill, c.BS256K, 5, threads,
                  tail)


@pytest.mark.parametrize("fill", [FILLS[0], FILLS[1]], ids=[FILL_IDS[0], FILL_IDS[1]])
def test_write_4k_blocks_wrap_the_ring(core, tmp_path, capfd, monkeypatch, fill):
    """512 slots of 4 KiB per worker: 2 * 256 + 1 blocks reuse slot 0."""
    c.check_write(core, tmp_path, capfd, monkeypatch, "pipelined", fill, 4096, 2 * B4K + 1,
                  c.WORKERS)


# ---------------------------------------------------------------------------
# B. read, verify off
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(c.READ_CASES))
def test_read_slots_hold_own_blocks(core, tmp_path, capfd, monkeypatch, name):
    c.check_read(core, tmp_path, capfd, monkeypatch, name)


# ---------------------------------------------------------------------------
# C. verify failures
# ---------------------------------------------------------------------------

C_PATHS = ["pipelined", "mmap", "blockio", "uring"]


@pytest.mark.parametrize("both", [False, True], ids=["one_slice", "both_of_a_stream"])
@pytest.mark.parametrize("path_name", C_PATHS)
def test_verify_failure_attributed_to_its_worker(core, tmp_path, capfd, monkeypatch, path_name,
                                                 both):
    c.check_verify(core, tmp_path, capfd, monkeypatch, path_name, both)


@pytest.mark.parametrize("path_name", ["pipelined", "blockio"], ids=["acc", "blk"])
def test_verify_diag_attributed_to_its_worker(core, tmp_path, capfd, monkeypatch, path_name):
    c.check_verify(core, tmp_path, capfd, monkeypatch, path_name, False, diag=True)


# ---------------------------------------------------------------------------
# D. lat=True
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(c.LAT_CASES))
def test_lat_one_sample_per_block(core, tmp_path, name):
    """Only the number of samples is asserted. A timed pair is three enqueues
    (start event, copy, end event) by one thread; on a shared stream a peer's
    copy can fall between them and is then part of the sample, so the values
    say how long the stream took, not how long this worker's copy did."""
    c.check_lat(core, tmp_path, name)


# ---------------------------------------------------------------------------
# E. other pool sizes, each in a fresh process
# ---------------------------------------------------------------------------

# Measured on an MI355X: the child's five cases take 0.5 s in this process
# (A pipelined checksum 0.28 s as the module's first case, bv37strong 0.04 s,
# B batched 4 KiB 0.08 s, mmap 0.08 s, C(i) pipelined 0.05 s), and a whole
# child 3.3 s, interpreter and HIP start-up included (10.0 s for the three).
# The limit is 18 times a child's run: it is there to end a hang, not to time
# the run.
CHILD_TIMEOUT_SEC = 60


def run_child(pool):
    env = dict(os.environ, EB_GPU_SHARED_STREAMS=str(pool))
    env.pop("EB_GPU_URING_BATCH", None)
    proc = subprocess.run([sys.executable, "-m", "tests.shared_streams_child"], env=env,
                          cwd=REPO, capture_output=True, text=True, timeout=CHILD_TIMEOUT_SEC)
    assert proc.returncode == 0, (
        f"pool {pool}: child ended with {proc.returncode}\n{proc.stdout}\n{proc.stderr}")
    return json.loads(proc.stdout.strip().splitlines()[-1])


def test_other_pool_sizes_in_child_processes():
    """One child after the other (with this process, two have the GPU open);
    the first that fails ends the test, the remaining sizes are not started."""
    for pool, want in [(4, [4] * 4), (1, [16]), (0, [1] * 16)]:
        out = run_child(pool)
        assert out["pool"] == str(pool)
        assert set(out["cases"]) == set(c_child_cases()), out
        for name, case in out["cases"].items():
            assert case["verdict"] == "ok", (pool, name, case)
            streams = case["streams"]
            assert len(streams) == c.WORKERS, (pool, name, streams)
            counts = sorted(collections.Counter(sid for sid, _ in streams).values())
            assert counts == want, (pool, name, counts)
            assert [shared for _, shared in streams] == [pool != 0] * c.WORKERS, (pool, name)


def c_child_cases():
    from tests.shared_streams_child import CASES
    return list(CASES)
