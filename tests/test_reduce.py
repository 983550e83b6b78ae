"""--dedupepct / --compresspct on the CPU: the fill against the numpy model
(tests/reduce_model.py), the pattern's properties, the configuration surface,
the engine with gpu_ids=[] and the elbencho-amd-datared tool. The cases live in
tests/reduce_cases.py and run again on the GPU in tests/test_gpu_reduce.py.
"""

import os
import re
import subprocess
import sys
import zlib

import pytest

from elbencho_amd import cli
from elbencho_amd.config import BenchConfig, ConfigError
from tests import reduce_cases as rc
from tests import reduce_model as rm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# the fill
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("d", rc.PCTS)
@pytest.mark.parametrize("c", rc.CHUNKS)
def test_fill_reduce_equals_model(core, c, d):
    for r, p, first, length in rc.grid(c, d):
        got = core.fill_reduce(length, first, c, r, d, p, rc.UNIQ, rc.POOL_SEED)
        assert got == rc.model(length, first, c, r, d, p), (c, r, d, p, first, length)


def test_seeds_equal_model(core):
    for seed in (0, rc.SEED, rm.MASK):
        for seq in (0, 1, 2, 77):
            for rank in (0, 1, 15, 4095):
                assert core.reduce_seeds(seed, seq, rank) == rm.seeds(seed, seq, rank)
    assert core.REDUCE_POOL_CHUNKS == rm.POOL == 256


# 300 chunks: more than the pool holds and three times the period of dup()
PROP_CHUNKS = 300


@pytest.mark.parametrize("source", ["model", "fill_reduce"])
@pytest.mark.parametrize("d", rc.PCTS)
@pytest.mark.parametrize("c", rc.CHUNKS)
def test_properties(core, c, d, source):
    for r in rc.rands(c):
        for p in rc.POOLS:
            for first in (0, 2**40 + 7):
                if source == "model":
                    data = rc.model(PROP_CHUNKS * c, first, c, r, d, p)
                else:
                    data = core.fill_reduce(PROP_CHUNKS * c, first, c, r, d, p, rc.UNIQ,
                                            rc.POOL_SEED)
                rc.check_properties(data, PROP_CHUNKS, first, c, r, d, p,
                                    f"{source} C={c} R={r} d={d} P={p} first={first}")


ZLIB_PCTS = (0, 25, 50, 75, 90, 100)
ZLIB_M = 0.0074
ZLIB_FRAMING = 0.0001


@pytest.mark.parametrize("source", ["model", "fill_reduce"])
@pytest.mark.parametrize("pct", ZLIB_PCTS)
def test_zlib_ratio(core, pct, source):
    """d = 0, C = 4096, 256 chunks (1 MiB), R = rand_bytes(C, pct): the zlib
    level-1 size over the input size lies in [R/C, R/C + m + framing].

    m = 0.0074: the largest excess over R/C that the *model's* bytes show for
    pct in ZLIB_PCTS (0.00031, 0.00518, 0.00648, 0.00721, 0.00738, 0.00438 in
    that order), rounded up. It is what deflate spends on block headers and on
    the matches that code each chunk's zero tail. framing = 0.0001 (105 bytes
    per MiB) is a fixed allowance for the zlib header and trailer (6 bytes) and
    for a deflate block more or less."""
    c, n = 4096, 256
    r = rm.rand_bytes(c, pct)
    if source == "model":
        data = rc.model(n * c, 0, c, r, 0, rm.POOL)
    else:
        data = core.fill_reduce(n * c, 0, c, r, 0, rm.POOL, rc.UNIQ, rc.POOL_SEED)
    ratio = len(zlib.compress(data, 1)) / len(data)
    print(f"pct={pct} R={r} ratio={ratio:.5f} excess={ratio - r / c:.5f}")
    assert r / c <= ratio <= r / c + ZLIB_M + ZLIB_FRAMING, (pct, ratio)


@pytest.mark.parametrize("chunk,rand,d,pool", rc.BAD_GEOMETRY)
def test_fill_reduce_rejects_bad_geometry(core, chunk, rand, d, pool):
    with pytest.raises(ValueError):
        core.fill_reduce(4096, 0, chunk, rand, d, pool, 1, 2)


# ---------------------------------------------------------------------------
# configuration surface
# ---------------------------------------------------------------------------

def parse(argv):
    return cli.args_to_config(cli.build_parser().parse_args(argv))


def test_cli_round_trips_into_wire_and_engine_dict(tmp_path):
    cfg = parse(["-w", "-s", "1m", "-b", "64k", "--dedupepct", "66", "--compresspct", "50",
                 "--dedupechunk", "8K", str(tmp_path / "f")])
    assert (cfg.dedupe_pct, cfg.compress_pct, cfg.dedupe_chunk) == (66, 50, 8192)
    wire = cfg.to_wire()
    assert (wire["dedupe_pct"], wire["compress_pct"], wire["dedupe_chunk"]) == (66, 50, 8192)
    back = BenchConfig.from_wire(wire)
    assert (back.dedupe_pct, back.compress_pct, back.dedupe_chunk) == (66, 50, 8192)
    d = back.engine_dict()
    assert (d["dedupe_pct"], d["compress_pct"], d["dedupe_chunk"]) == (66, 50, 8192)


def test_defaults_leave_the_feature_off(tmp_path):
    cfg = parse(["-w", "-s", "1m", "-b", "64k", str(tmp_path / "f")])
    d = cfg.engine_dict()
    assert (d["dedupe_pct"], d["compress_pct"], d["dedupe_chunk"]) == (0, 0, 4096)
    assert (BenchConfig().dedupe_pct, BenchConfig().compress_pct,
            BenchConfig().dedupe_chunk) == (0, 0, 4096)


def test_one_percentage_alone_is_accepted(tmp_path):
    for opt in ("--dedupepct", "--compresspct"):
        cfg = parse(["-w", "-s", "1m", "-b", "64k", opt, "100", str(tmp_path / "f")])
        assert cfg.dedupe_pct + cfg.compress_pct == 100
    # the chunk size is only looked at when the feature is on
    parse(["-w", "-s", "1m", "-b", "64k", "--dedupechunk", "100", str(tmp_path / "f")])


@pytest.mark.parametrize("extra,msg", [
    (["--dedupepct", "101"], "dedupepct must be in 0..100"),
    (["--dedupepct", "-1"], "dedupepct must be in 0..100"),
    (["--compresspct", "101"], "compresspct must be in 0..100"),
    (["--compresspct", "-1"], "compresspct must be in 0..100"),
    (["--dedupepct", "50", "--dedupechunk", "256"], "power of two in 512..16M"),
    (["--dedupepct", "50", "--dedupechunk", "32M"], "power of two in 512..16M"),
    (["--compresspct", "50", "--dedupechunk", "3K"], "power of two in 512..16M"),
    (["--dedupepct", "50", "--verify", "7"], "--verify"),
    (["--compresspct", "50", "--verify", "7"], "--verify"),
    (["--dedupepct", "50", "--blockvarpct", "50"], "--blockvarpct"),
    (["--compresspct", "50", "--blockvarpct", "0"], "--blockvarpct"),
])
def test_config_errors(tmp_path, extra, msg):
    argv = ["-w", "-s", "1m", "-b", "64k"] + extra + [str(tmp_path / "f")]
    with pytest.raises(ConfigError, match=re.escape(msg)):
        parse(argv)


@pytest.mark.parametrize("mode", ["s3", "hdfs", "netbench"])
def test_config_error_outside_file_bdev_dir(mode):
    cfg = BenchConfig()
    cfg.run_write = True
    cfg.compress_pct = 50
    cfg.block_size = 65536
    cfg.file_size = 1 << 20
    cfg.files = 1
    cfg.bench_mode = mode
    if mode == "s3":
        cfg.s3_endpoints = ["http://127.0.0.1:9"]
        cfg.paths = ["bucket"]
    elif mode == "hdfs":
        cfg.paths = ["hdfs://127.0.0.1:9/base"]
    else:
        cfg.hosts = ["127.0.0.1"]
        cfg.servers = ["127.0.0.1"]
    with pytest.raises(ConfigError, match="file, block device and directory paths only"):
        cfg.validate()
    cfg.compress_pct = 0
    cfg.validate()  # the same configuration is fine without the option


@pytest.mark.parametrize("cfg,msg", [
    (dict(dedupe_pct=101), "dedupe_pct"),
    (dict(dedupe_pct=-1), "dedupe_pct"),
    (dict(compress_pct=101), "compress_pct"),
    (dict(compress_pct=-1), "compress_pct"),
    (dict(dedupe_pct=50, dedupe_chunk=3000), "dedupe_chunk"),
    (dict(dedupe_pct=50, dedupe_chunk=8), "dedupe_chunk"),
    (dict(compress_pct=50, verify_salt=7), "verify_salt"),
])
def test_engine_rejects_bad_config(core, tmp_path, cfg, msg):
    full = rc.engine_cfg(tmp_path, "file", [], 0, 0, file_size=1 << 20, block_size=65536)
    full.update(cfg)
    with pytest.raises(ValueError, match=msg):
        core.Engine(full)


def test_docs_name_the_options():
    for rel in ("docs/help.md", "docs/help-all.md", "docs/help-multi.md", "docs/usage.md"):
        with open(os.path.join(REPO, rel)) as f:
            text = f.read()
        for opt in ("--dedupepct", "--compresspct", "--dedupechunk"):
            assert opt in text, (rel, opt)
    with open(os.path.join(REPO, "docs/service-protocol.md")) as f:
        text = f.read()
    for key in ("dedupe_pct", "compress_pct", "dedupe_chunk"):
        assert key in text, key
    for rel in ("docs/DESIGN.md", "COMPONENTS.md"):
        with open(os.path.join(REPO, rel)) as f:
            assert "ebFillReduceKernel" in f.read(), rel
    opts = re.search(r'local opts="([^"]*)"', cli.bash_completion()).group(1).split()
    assert {"--dedupepct", "--compresspct", "--dedupechunk"} <= set(opts)


# ---------------------------------------------------------------------------
# engine, gpu_ids=[]
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(rc.ENGINE_CASES))
def test_engine_writes_the_model(core, tmp_path, name):
    rc.run_engine_case(core, tmp_path, [], name)


def test_engine_second_phase(core, tmp_path):
    rc.run_two_phases(core, tmp_path, [])


def test_feature_off_launches_nothing_new(core, tmp_path):
    """With both percentages 0 the engine takes the block-variance path: the
    file is not the reduction pattern of any percentage pair the keys could
    have meant, and holds no zero chunk tail."""
    cfg = rc.engine_cfg(tmp_path, "file", [], 0, 0, file_size=1 << 20, block_size=65536)
    eng = core.Engine(cfg)
    eng.prepare()
    rc.run_ok(core, eng, "WRITE")
    data = (tmp_path / "f").read_bytes()
    on = dict(cfg, compress_pct=50)
    assert data != rc.expected_files(core, tmp_path, on, 1)[tmp_path / "f"]
    assert all(ch[2048:] != bytes(2048) for ch in rc.split_chunks(data, 4096))


# ---------------------------------------------------------------------------
# tools/elbencho-amd-datared
# ---------------------------------------------------------------------------

def run_tool(*args):
    res = subprocess.run([sys.executable, os.path.join(REPO, "tools", "elbencho-amd-datared"),
                          *args], capture_output=True, text=True)
    fields = dict(re.findall(r"^([a-z0-9 -]+): (.*)$", res.stdout, re.M))
    return res, fields


def test_datared_tool_reports_the_exact_counts(tmp_path):
    c, n, d, pct = 4096, 256, 50, 50
    r = rm.rand_bytes(c, pct)
    data = rc.model(n * c, 0, c, r, d, rm.POOL)
    p = tmp_path / "f"
    p.write_bytes(data)
    numbers = rm.chunk_numbers(0, n)
    dup = rm.is_dup(numbers, d)
    members = {int(m) for m in rm.pool_member(numbers[dup], rm.POOL, rc.UNIQ)}
    distinct = n - int(dup.sum()) + len(members)
    assert distinct == len(set(rc.split_chunks(data, c))) and int(dup.sum()) == n * d // 100

    res, f = run_tool(str(p))
    assert res.returncode == 0, res.stderr
    assert (int(f["bytes"]), int(f["chunk size"]), int(f["chunks"])) == (n * c, c, n)
    assert int(f["distinct chunks"]) == distinct
    assert f["dedupe ratio"] == f"{n / distinct:.3f}"
    packed = int(f["zlib-1 bytes"])
    assert r / c <= packed / len(data) <= r / c + ZLIB_M + ZLIB_FRAMING
    assert f["compress ratio"] == f"{len(data) / packed:.3f}"

    # a chunk size that is not the data's: every 1 KiB piece of the random
    # halves is distinct, the zero pieces are one
    res, f = run_tool(str(p), "--chunk", "1K")
    assert res.returncode == 0, res.stderr
    assert int(f["chunks"]) == 4 * n
    assert int(f["distinct chunks"]) == len(set(rc.split_chunks(data, 1024)))


def test_datared_tool_errors(tmp_path):
    res, _ = run_tool(str(tmp_path / "missing"))
    assert res.returncode == 1 and "ERROR" in res.stderr
    (tmp_path / "empty").write_bytes(b"")
    res, f = run_tool(str(tmp_path / "empty"))
    assert res.returncode == 0 and f["chunks"] == "0" and f["dedupe ratio"] == "n/a"
