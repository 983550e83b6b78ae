"""bench.py command line: --dump-outputs and --full (single process)."""

import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FSIZE = 32 * 1024 * 1024
BLOCK = 1 << 20


def _run_bench(tmp_path, tag, *extra):
    out = tmp_path / f"out_{tag}"
    env = dict(os.environ, PYTHONPATH=REPO, EB_BENCH_DIR=str(tmp_path / tag),
               EB_BENCH_THREADS="4")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    res = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--steps", "3", "--warmup", "1", "--filesize", str(FSIZE),
         "--block", str(BLOCK), "--dump-outputs", str(out), *extra],
        env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), out


def test_bench_dump_outputs_reproducible_and_full(tmp_path, core):
    """Two runs with the same arguments (one of them --full) dump identical
    float arrays: the last timed pass moved every block of the dataset
    without error, and the sampled bytes are the verify pattern."""
    doc_a, out_a = _run_bench(tmp_path, "a")
    doc_b, out_b = _run_bench(tmp_path, "b", "--full")

    for doc in (doc_a, doc_b):
        for key in ("metric", "value", "unit", "higher_is_better", "dtype",
                    "ms_per_step", "steps", "warmup"):
            assert key in doc, key
        assert doc["steps"] == 3 and doc["warmup"] == 1
        assert doc["ms_per_step"] > 0
        # value and ms_per_step describe the same 3 timed passes
        gib = doc["value"] * doc["ms_per_step"] * 3 / 1000.0
        assert abs(gib * 1024 ** 3 - 3 * FSIZE) / (3 * FSIZE) < 0.01

    names = sorted(os.listdir(out_a))
    assert names == ["data_sample.npy", "pass_totals.npy",
                     "sample_offsets.npy"]
    assert sorted(os.listdir(out_b)) == names
    total = 0
    for name in names:
        a = np.load(out_a / name)
        b = np.load(out_b / name)
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        assert a.shape == b.shape and np.array_equal(a, b), name
        total += a.nbytes
    assert total <= 64 * 1000 * 1000

    totals = np.load(out_a / "pass_totals.npy")
    assert totals[1] == FSIZE            # bytes of one full pass
    assert totals[2] == FSIZE // BLOCK   # one I/O per block
    assert totals[3] == 0                # no worker reported an error

    offs = np.load(out_a / "sample_offsets.npy").astype(np.int64)
    sample = np.load(out_a / "data_sample.npy")
    assert offs[0] == 0 and offs[-1] == FSIZE - sample.shape[1]
    salt = doc_a["config"]["verify_salt"]
    assert salt is not None
    for i in (0, len(offs) // 2, len(offs) - 1):
        want = np.frombuffer(
            core.fill_checksum(sample.shape[1], int(offs[i]), salt),
            dtype=np.uint8)
        assert np.array_equal(sample[i], want.astype(np.float32)), i
