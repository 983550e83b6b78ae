"""--dedupeverify on the CPU: verifyReduceCPU against the numpy model
(tests/reduce_model.py), the seeds, the configuration surface and the engine
with gpu_ids=[]. The cases live in tests/reduce_verify_cases.py and run again on
the GPU in tests/test_gpu_reduce_verify.py.
"""

import os
import re

import pytest

from elbencho_amd import cli
from elbencho_amd.config import BenchConfig, ConfigError
from tests import reduce_cases as rc
from tests import reduce_model as rm
from tests import reduce_verify_cases as rv

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cpu_verify(core):
    def verify(data, file_off, first, c, r, d, p, uniq=rv.UNIQ):
        return core.verify_reduce(data, file_off, first, c, r, d, p, uniq, rv.POOL_SEED)
    return verify


# ---------------------------------------------------------------------------
# the verify
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("d", rc.PCTS)
@pytest.mark.parametrize("c", rc.CHUNKS)
def test_clean_data_verifies(core, c, d):
    """The grid of test_reduce.py: cut last chunks, any length, and a file
    offset that is not 0 (it only moves the reported offset)."""
    verify = cpu_verify(core)
    for r, p, first, length in rc.grid(c, d):
        for file_off in (0, first * c & rm.MASK, 8 * 12345):
            what = (c, r, d, p, first, length, file_off)
            assert verify(rc.model(length, first, c, r, d, p), file_off, first, c, r, d,
                          p) == rv.NONE, what
        assert verify(core.fill_reduce(length, first, c, r, d, p, rv.UNIQ, rv.POOL_SEED), 0,
                      first, c, r, d, p) == rv.NONE, (c, r, d, p, first, length)


@pytest.mark.parametrize("c", [16, 64, 512, 4096, 8192])
def test_corruptions_are_counted_and_located(core, c):
    for r in sorted({0, 16, c // 32 * 16, c - 16, c}):
        for first, file_off in ((0, 0), (2**40 + 7, 8 * 999), (99, 99 * c)):
            rv.check_corruptions(cpu_verify(core), c, r, 3 * c + 16, first, file_off)


def test_cut_last_word(core):
    """A length that is no multiple of 8: the last word is compared over the
    bytes it has."""
    c, r, length = 64, 32, 64 + 21
    data = rc.model(length, 3, c, r, 50, 256)
    verify = cpu_verify(core)
    assert verify(data, 800, 3, c, r, 50, 256) == rv.NONE
    assert verify(rv.flip(data, length - 1), 800, 3, c, r, 50, 256) == (1, 800 + 64 + 16)
    assert verify(data[:-1], 800, 3, c, r, 50, 256) == rv.NONE


@pytest.mark.parametrize("chunk,rand,d,pool", rc.BAD_GEOMETRY)
def test_verify_reduce_rejects_bad_geometry(core, chunk, rand, d, pool):
    with pytest.raises(ValueError):
        core.verify_reduce(bytes(4096), 0, 0, chunk, rand, d, pool, 1, 2)


def test_seeds(core):
    for salt in (0, 7, rv.SALT, 2**63 - 1):
        for key in (0, 1, 2, 4095, rv.dir_file_key(1, 0, 2)):
            assert core.reduce_verify_seeds(salt, key) == rv.seeds(salt, key)
    uniq = {core.reduce_verify_seeds(s, k)[0] for s in (0, 7, 8) for k in range(64)}
    assert len(uniq) == 3 * 64, "the uniq seed differs per salt and per file key"
    for s in (0, 7, 8):
        pools = {core.reduce_verify_seeds(s, k)[1] for k in range(64)}
        assert len(pools) == 1, "the pool seed does not depend on the file key"
    assert core.reduce_verify_seeds(7, 0)[1] != core.reduce_verify_seeds(8, 0)[1]
    keys = {core.reduce_dir_file_key(r, d, f) for r in range(8) for d in range(8)
            for f in range(8)}
    assert len(keys) == 512
    for r, d, f in ((0, 0, 0), (1, 0, 2), (4095, 77, 2**32 + 5)):
        assert core.reduce_dir_file_key(r, d, f) == rv.dir_file_key(r, d, f)


# ---------------------------------------------------------------------------
# configuration surface
# ---------------------------------------------------------------------------

def parse(argv):
    return cli.args_to_config(cli.build_parser().parse_args(argv))


GOOD = ["-w", "-r", "-s", "1m", "-b", "64k", "--dedupepct", "50", "--compresspct", "50",
        "--dedupeverify", "5"]


def test_cli_round_trips_into_wire_and_engine_dict(tmp_path):
    cfg = parse(GOOD + [str(tmp_path / "f")])
    assert cfg.dedupe_verify == 5
    wire = cfg.to_wire()
    assert wire["dedupe_verify"] == 5
    back = BenchConfig.from_wire(wire)
    assert back.dedupe_verify == 5
    assert back.engine_dict()["reduce_verify_salt"] == 5
    for opt in ("--dedupepct", "--compresspct"):  # one percentage alone is enough
        parse(["-w", "-s", "1m", "-b", "64k", opt, "10", "--dedupeverify", "0",
               str(tmp_path / "f")])
    parse(GOOD + ["--rand", str(tmp_path / "f")])  # aligned random offsets are fine


def test_default_is_off(tmp_path):
    cfg = parse(["-w", "-s", "1m", "-b", "64k", "--dedupepct", "50", str(tmp_path / "f")])
    assert cfg.dedupe_verify == -1 and BenchConfig().dedupe_verify == -1
    assert cfg.engine_dict()["reduce_verify_salt"] == -1


@pytest.mark.parametrize("argv,msg", [
    (["-w", "-s", "1m", "-b", "64k", "--dedupeverify", "5"],
     "--dedupeverify requires a non-zero --dedupepct or --compresspct"),
    (GOOD + ["--verify", "7"], "--dedupeverify cannot be used together with --verify"),
    (GOOD + ["--verifymixpct", "50"],
     "--dedupeverify cannot be used together with --verifymixpct"),
    (GOOD + ["--verifydiag"], "--dedupeverify cannot be used together with --verifydiag"),
    (GOOD + ["--rand", "--norandalign"],
     "--dedupeverify cannot be used with unaligned random offsets"),
    (GOOD + ["-b", "6k"], "block size that is a multiple of --dedupechunk"),
    (GOOD + ["--dedupechunk", "128k"], "block size that is a multiple of --dedupechunk"),
    (GOOD[:-1] + ["-2"], "--dedupeverify needs a salt >= 0"),
])
def test_config_errors(tmp_path, argv, msg):
    with pytest.raises(ConfigError, match=re.escape(msg)):
        parse(argv + [str(tmp_path / "f")])


def test_verify_with_dedupepct_stays_rejected(tmp_path):
    with pytest.raises(ConfigError, match="--dedupepct/--compresspct cannot be used together "
                                          "with --verify"):
        parse(["-w", "-s", "1m", "-b", "64k", "--dedupepct", "50", "--verify", "7",
               str(tmp_path / "f")])


@pytest.mark.parametrize("mode", ["s3", "hdfs", "netbench"])
def test_config_error_outside_file_bdev_dir(mode):
    cfg = BenchConfig()
    cfg.run_write = True
    cfg.dedupe_verify = 5
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
    cfg.compress_pct = 50
    with pytest.raises(ConfigError, match="file, block device and directory paths only"):
        cfg.validate()
    cfg.compress_pct = 0
    with pytest.raises(ConfigError, match="--dedupeverify requires a non-zero"):
        cfg.validate()
    cfg.dedupe_verify = -1
    cfg.validate()


@pytest.mark.parametrize("cfg,msg", [
    (dict(dedupe_pct=0, compress_pct=0), "requires a non-zero dedupe_pct or compress_pct"),
    (dict(reduce_verify_salt=-2), "reduce_verify_salt must be >= 0"),
    (dict(verify_salt=7), "verify_salt"),
    (dict(verify_diag=True), "verify_diag"),
    (dict(random=True, rand_aligned=False), "unaligned random offsets"),
    (dict(block_size=6144), "multiple of dedupe_chunk"),
    (dict(dedupe_chunk=131072), "multiple of dedupe_chunk"),
])
def test_engine_rejects_bad_config(core, tmp_path, cfg, msg):
    full = rv.engine_cfg(tmp_path, "file1_tail16", [], "WRITE")
    core.Engine(full)  # the good case is accepted
    full.update(cfg)
    with pytest.raises(ValueError, match=msg):
        core.Engine(full)


def test_docs_name_the_option():
    for rel in ("docs/help.md", "docs/help-all.md", "docs/help-multi.md", "docs/usage.md"):
        with open(os.path.join(REPO, rel)) as f:
            assert "--dedupeverify" in f.read(), rel
    with open(os.path.join(REPO, "docs/service-protocol.md")) as f:
        assert "dedupe_verify" in f.read()
    with open(os.path.join(REPO, "COMPONENTS.md")) as f:
        assert "ebVerifyReduceKernel" in f.read()
    opts = re.search(r'local opts="([^"]*)"', cli.bash_completion()).group(1).split()
    # the packaged copy under dist/ is output of the generator and is not
    # regenerated with the source (tests/test_verify_mix.py states the rule)
    assert "--dedupeverify" in opts


# ---------------------------------------------------------------------------
# engine, gpu_ids=[]
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(rv.ENGINE_CASES))
def test_engine_write_then_read(core, tmp_path, name):
    rv.run_engine_case(core, tmp_path, name, [], [])


def test_cli_run_end_to_end(tmp_path):
    """The option through the command line: write, read, corrupt, read."""
    from elbencho_amd.__main__ import main
    path = tmp_path / "f"
    base = ["-s", "256k", "-b", "64k", "--dedupepct", "50", "--compresspct", "50",
            "--dedupeverify", "9", "--nolive", str(path)]
    assert main(["-w"] + base) == 0
    want = rm.model_fill(256 * 1024, 0, 4096, 2048, 50, rm.POOL, *rv.seeds(9, 0))
    assert path.read_bytes() == want
    assert main(["-r"] + base) == 0
    path.write_bytes(rv.flip(want, 70000))
    assert main(["-r"] + base) != 0


def test_without_the_option_nothing_changes(core, tmp_path):
    """reduce_verify_salt = -1 is the default: the engine case of
    tests/reduce_cases.py gives the per-worker sequence its model states, which
    is not the position-keyed content of any file key tried here, and a read
    of it checks nothing."""
    name = "two_threads"
    mode, kw, d, z = rc.ENGINE_CASES[name]
    cfg = rc.engine_cfg(tmp_path, mode, [], d, z, reduce_verify_salt=-1, **kw)
    eng = core.Engine(cfg)
    eng.prepare()
    rc.run_ok(core, eng, "WRITE")
    rc.assert_files(rc.expected_files(core, tmp_path, cfg, 1), name)
    rc.run_ok(core, eng, "READ")
    data = (tmp_path / "f").read_bytes()
    r = rm.rand_bytes(rc.C, z)
    for salt in (0, rc.SEED & (2**63 - 1)):
        nbad, _ = core.verify_reduce(data, 0, 0, rc.C, r, d, rm.POOL,
                                     *core.reduce_verify_seeds(salt, 0))
        assert nbad > len(data) // rc.C
