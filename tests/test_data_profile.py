"""--dataprofile without a GPU: the CPU twin against the numpy model
(tests/data_profile_model.py) over the case table of
tests/data_profile_cases.py, merging, the estimator, the configuration surface,
and the engine, the services and the ranks with CPU buffers. The kernel and
the GPU staging paths run the same cases in tests/test_gpu_data_profile.py.
"""

import json
import os
import re
import socket
import subprocess
import sys
import time
import urllib.request

import numpy as np
import pytest

from elbencho_amd import cli
from elbencho_amd.config import BenchConfig, ConfigError
from elbencho_amd.dataprofile import HLL_M, DataProfile, merge_profiles
from elbencho_amd.stats import CSV_COLUMNS
from tests import data_profile_cases as dc
from tests import data_profile_model as dm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# model vs native
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", dc.CONTENTS)
@pytest.mark.parametrize("chunk", dc.CHUNKS)
def test_cpu_twin_equals_model(core, chunk, kind):
    for length in dc.LENS:
        got = core.data_profile(dc.content(core, kind, length), chunk)
        dc.assert_same(got, dc.expected(core, kind, length, chunk), (chunk, length, kind))


def test_model_basics():
    """The model itself, on values worked out by hand from the definitions."""
    assert dm.mix(0) == 0xE220A8397B1DCDAF  # splitmix64's first output for state 0
    p = dm.profile(bytes(8), 512)
    fp = dm.mix(dm.mix(dm.GOLD) ^ 8)  # one zero word: S = mix(0 + GOLD*1)
    assert dm.fingerprint(bytes(8)) == fp
    regs = bytearray(dm.HLL_M)
    rest = (fp << 14) & dm.MASK
    regs[fp >> 50] = 64 - rest.bit_length() + 1 if rest else 51
    assert p == {"chunks": 1, "bytes": 8, "zero_chunks": 1,
                 "hist": [8] + [0] * 255, "regs": bytes(regs)}
    assert dm.profile(b"", 512) == dm.empty()
    assert list(dm.clz64(np.array([1, 2**63, 2**40 + 5], dtype=np.uint64))) == [63, 0, 23]
    # rest == 0 takes the cap
    assert dm.registers_of(np.array([5 << 50], dtype=np.uint64))[5] == 51


def test_empty_block_and_bad_chunk(core):
    dc.assert_same(core.data_profile(b"", 4096), dm.empty(), "empty")
    for chunk in (0, 256, 4097, 6144, 32 << 20):
        with pytest.raises(ValueError):
            core.data_profile(bytes(16), chunk)


def test_fingerprints_separate(core):
    """Word order and length both enter the fingerprint."""
    a = np.arange(1, 65, dtype="<u8")
    b = a.copy()
    b[[3, 40]] = b[[40, 3]]
    assert dm.fingerprint(a.tobytes()) != dm.fingerprint(b.tobytes())
    assert core.data_profile(a.tobytes(), 512)["regs"] != \
        core.data_profile(b.tobytes(), 512)["regs"]
    assert dm.fingerprint(bytes(8)) != dm.fingerprint(bytes(16))
    assert core.data_profile(bytes(8), 512)["regs"] != core.data_profile(bytes(16), 512)["regs"]


def test_merge(core):
    a = dc.content(core, "reduce", 3 * 4096)
    b = dc.content(core, "random", 4096 + 520 + 3)
    pa = DataProfile.from_engine(core.data_profile(a, 4096))
    pb = DataProfile.from_engine(core.data_profile(b, 4096))
    ab = DataProfile().merge(pa).merge(pb)
    ba = DataProfile().merge(pb).merge(pa)
    assert ab == ba, "merging is commutative"
    dc.assert_same(ab.to_engine(), dm.profile_blocks([a, b], 4096), "A then B")
    assert merge_profiles([None, pa, None, pb]) == ab
    assert merge_profiles([None, None]) is None
    assert DataProfile.from_wire(json.loads(json.dumps(ab.to_wire()))) == ab


# ---------------------------------------------------------------------------
# derived figures
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [100, 5000, 1_000_000])
def test_estimator(n):
    """Within 3 % of n = 3.7 standard errors (1.04 / sqrt(m) = 0.81 %). The n
    lie outside 2.5 m .. 5 m = 40960 .. 81920, where raw HyperLogLog is biased."""
    fps = dm.mix(np.arange(n, dtype=np.uint64))
    assert len(np.unique(fps)) == n
    p = DataProfile(chunks=n, bytes=n * 4096, regs=dm.registers_of(fps).tobytes())
    est = p.distinct_estimate()
    assert abs(est - n) <= 0.03 * n, (n, est)
    assert abs(p.dedupe_ratio() - 1.0) <= 0.031


def test_derived_figures():
    assert DataProfile().distinct_estimate() == 0.0
    assert DataProfile().suggest() == {"dedupepct": 0, "compresspct": 0}
    hist = [0] * 256
    hist[0], hist[255] = 512, 512
    # 1000 chunks that are 10 distinct ones; half the bytes zero, two values
    fps = dm.mix(np.arange(10, dtype=np.uint64))
    p = DataProfile(chunks=1000, bytes=1024, zero_chunks=0, hist=hist,
                    regs=dm.registers_of(fps).tobytes())
    assert abs(p.distinct_estimate() - 10) < 0.1  # linear counting: m ln(m / (m - 10))
    assert p.entropy_bits_per_byte() == 1.0 and p.compress_bound() == 8.0
    assert p.suggest() == {"dedupepct": 99, "compresspct": 50}
    const = DataProfile(chunks=1, bytes=8, zero_chunks=1, hist=[8] + [0] * 255)
    assert const.entropy_bits_per_byte() == 0.0 and const.compress_bound() == float("inf")
    doc = const.to_json(4096)
    assert doc["compressBound"] is None and doc["zeroBytes"] == 8 and doc["chunkSize"] == 4096
    json.dumps(doc)


# ---------------------------------------------------------------------------
# configuration surface
# ---------------------------------------------------------------------------

def parse(argv):
    return cli.args_to_config(cli.build_parser().parse_args(argv))


def test_cli_round_trips_into_wire_and_engine_dict(tmp_path):
    cfg = parse(["-r", "-s", "1m", "-b", "64k", "--dataprofile", str(tmp_path / "f")])
    assert cfg.data_profile is True
    back = BenchConfig.from_wire(cfg.to_wire())
    assert back.data_profile is True and back.engine_dict()["data_profile"] is True
    off = parse(["-r", "-s", "1m", "-b", "64k", str(tmp_path / "f")])
    assert off.data_profile is False and off.engine_dict()["data_profile"] is False


@pytest.mark.parametrize("argv,msg", [
    (["-w", "-s", "1m", "-b", "64k"], "--dataprofile requires a read phase (-r)"),
    (["-r", "-s", "1m", "-b", "64k", "--rand", "--norandalign"],
     "--dataprofile cannot be used with unaligned random offsets"),
    (["-r", "-s", "1m", "-b", "6k"], "block size that is a multiple of --dedupechunk"),
    (["-r", "-s", "1m", "-b", "64k", "--dedupechunk", "128k"],
     "block size that is a multiple of --dedupechunk"),
    (["-r", "-s", "1m", "-b", "64k", "--dedupechunk", "256"],
     "--dedupechunk must be a power of two in 512..16M"),
])
def test_config_errors(tmp_path, argv, msg):
    with pytest.raises(ConfigError, match=re.escape(msg)):
        parse(argv + ["--dataprofile", str(tmp_path / "f")])


@pytest.mark.parametrize("mode", ["s3", "hdfs", "netbench"])
def test_config_error_outside_file_bdev_dir(mode):
    cfg = BenchConfig()
    cfg.run_read = True
    cfg.data_profile = True
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
    with pytest.raises(ConfigError, match="--dataprofile supports file, block device and "
                                          "directory paths only"):
        cfg.validate()
    cfg.data_profile = False
    cfg.validate()


@pytest.mark.parametrize("bad,msg", [
    (dict(block_size=6144), "multiple of dedupe_chunk"),
    (dict(dedupe_chunk=256), "power of two in 512..16M"),
    (dict(random=True, rand_aligned=False), "unaligned random offsets"),
])
def test_engine_rejects_bad_config(core, tmp_path, bad, msg):
    full = dict(paths=[str(tmp_path / "f")], path_type="file", threads=1, file_size=1 << 20,
                block_size=65536, data_profile=True)
    core.Engine(full)
    full.update(bad)
    with pytest.raises(ValueError, match=msg):
        core.Engine(full)


def test_docs_name_the_option():
    for rel in ("docs/help.md", "docs/help-all.md", "docs/usage.md", "README.md"):
        with open(os.path.join(REPO, rel)) as f:
            assert "--dataprofile" in f.read(), rel
    with open(os.path.join(REPO, "COMPONENTS.md")) as f:
        assert "ebDataProfileKernel" in f.read()
    with open(os.path.join(REPO, "docs/service-protocol.md")) as f:
        assert "data_profile" in f.read()
    opts = re.search(r'local opts="([^"]*)"', cli.bash_completion()).group(1).split()
    assert "--dataprofile" in opts


# ---------------------------------------------------------------------------
# engine, no GPU
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def reduce_file(tmp_path_factory):
    path, data = dc.write_reduce_file(tmp_path_factory.mktemp("dp_file"))
    return path, dm.profile(data, 4096)


def test_engine_profile_is_independent_of_threads_blocks_and_depth(reduce_file, tmp_path):
    path, want = reduce_file
    assert want["chunks"] == 2048 + 2 and want["bytes"] == dc.FILE_SIZE
    shapes = {"t1_b1m": ["-t", "1", "-b", "1m"],
              "t3_b64k": ["-t", "3", "-b", "64k"],
              "t2_b256k_qd4": ["-t", "2", "-b", "256k", "--iodepth", "4"]}
    for tag, argv in shapes.items():
        (got,), _ = dc.read_profiles(tmp_path, argv + [path], tag)
        dc.assert_same(got, want, tag)


def test_engine_mmap(reduce_file, tmp_path):
    path, want = reduce_file
    (got,), _ = dc.read_profiles(tmp_path, ["-t", "2", "-b", "128k", "--mmap", path], "mmap")
    dc.assert_same(got, want, "mmap")


def test_engine_dir_mode(tmp_path):
    root, want = dc.write_dir_files(tmp_path)
    assert want["chunks"] == 2 * 2 * 3 * 17
    (got,), _ = dc.read_profiles(tmp_path, [*dc.DIR_ARGS, root], "dir")
    dc.assert_same(got, want, "dir")
    (got,), _ = dc.read_profiles(tmp_path, [*dc.DIR_ARGS, "--iodepth", "4", root], "dir_qd4")
    dc.assert_same(got, want, "dir_qd4")


def test_two_read_phases_each_report_one_pass(reduce_file, tmp_path):
    path, want = reduce_file
    got, _ = dc.read_profiles(tmp_path, ["-t", "2", "-b", "256k", "-i", "2", path], "twice")
    assert len(got) == 2
    for i, g in enumerate(got):
        dc.assert_same(g, want, f"pass {i}")


def test_with_verify(tmp_path):
    path = str(tmp_path / "v")
    size = 1024 * 1024 + 4096 + 520
    base = ["-s", str(size), "-b", "64k", "-t", "2", "--verify", "1", path]
    assert dc.run_cli(["-w"] + base) == 0
    (got,), _ = dc.read_profiles(tmp_path, base, "verify")
    with open(path, "rb") as f:
        data = f.read()
    dc.assert_same(got, dm.profile(data, 4096), "verify")
    # a verify failure still fails the run, with the --verify message
    with open(path, "r+b") as f:
        f.seek(70000)
        f.write(b"\xff")
    out = str(tmp_path / "bad.json")
    assert dc.run_cli(["-r", "--dataprofile", "--jsonfile", out] + base) != 0
    (doc,) = dc.json_docs(out)
    assert "dataProfile" not in doc
    assert any("Data verification failed" in e for e in doc["errors"])


def test_rwmix_reads_are_not_profiled(core, tmp_path):
    """Only READ phases profile: a write phase with rwmix reads reports none."""
    cfg = dict(paths=[str(tmp_path / "f")], path_type="file", threads=1, file_size=1 << 20,
               block_size=65536, data_profile=True)
    eng = core.Engine(cfg)
    eng.prepare()
    for phase, mix in (("WRITE", 0), ("READ", 0)):
        eng.start_phase(core.PHASES[phase])
        assert eng.wait_phase_done(60_000)
        res = eng.finish_phase()
        assert not any(r["error"] for r in res)
        assert ("data_profile" in res[0]) == (phase == "READ")
    eng2 = core.Engine(dict(cfg, rwmix_pct=50))
    eng2.prepare()
    eng2.start_phase(core.PHASES["WRITE"])
    assert eng2.wait_phase_done(60_000)
    res = eng2.finish_phase()
    assert res[0]["rm_bytes"] > 0 and "data_profile" not in res[0]


# ---------------------------------------------------------------------------
# command line output
# ---------------------------------------------------------------------------

def test_output_with_and_without_the_flag(reduce_file, tmp_path, capsys):
    path, want = reduce_file
    csv_on, csv_off = str(tmp_path / "on.csv"), str(tmp_path / "off.csv")
    capsys.readouterr()
    (got,), (doc,) = dc.read_profiles(tmp_path, ["-b", "1m", "--csvfile", csv_on, path], "on")
    text = capsys.readouterr().out
    assert "data profile" in text and "Replay with" in text
    p = doc["dataProfile"]
    assert p["chunkSize"] == 4096 and p["zeroChunks"] == 0 and p["chunks"] == 2050
    # half the chunks come from the pool of 256, so in a file this small the
    # distinct chunks are the unique half plus (nearly) the whole pool
    with open(path, "rb") as f:
        data = f.read()
    distinct = len({data[o:o + 4096] for o in range(0, len(data), 4096)})
    assert 1025 < distinct <= 1025 + 256
    assert abs(p["distinctEstimate"] - distinct) <= 0.03 * distinct
    assert abs(p["suggest"]["dedupepct"] - 100 * (1 - distinct / 2050)) <= 2
    assert p["suggest"]["compresspct"] == 50
    assert (f"--dedupepct {p['suggest']['dedupepct']} --compresspct 50 --dedupechunk 4096"
            in text)
    assert 4.9 < p["entropyBitsPerByte"] < 5.1  # half zeros, half uniform: 1 + 8 / 2

    out = str(tmp_path / "off.json")
    assert dc.run_cli(["-r", "-b", "1m", "--jsonfile", out, "--csvfile", csv_off, path]) == 0
    text = capsys.readouterr().out
    assert "data profile" not in text
    (doc,) = dc.json_docs(out)
    assert "dataProfile" not in doc
    with open(csv_on) as f_on, open(csv_off) as f_off:
        header_on, header_off = f_on.readline(), f_off.readline()
    assert header_on == header_off == ",".join(CSV_COLUMNS) + "\n"


# ---------------------------------------------------------------------------
# services and ranks
# ---------------------------------------------------------------------------

def free_port():
    s = socket.socket()
    s.bind(("", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture
def services():
    ports = [free_port(), free_port()]
    env = dict(os.environ, PYTHONPATH=REPO)
    procs = [subprocess.Popen([sys.executable, "-m", "elbencho_amd", "--service",
                               "--foreground", "--port", str(p)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for p in ports]
    deadline = time.monotonic() + 40
    for p in ports:
        while True:
            try:
                with urllib.request.urlopen(f"http://127.0.0.1:{p}/protocolversion",
                                            timeout=1) as r:
                    r.read()
                break
            except OSError:
                if time.monotonic() > deadline:
                    for pr in procs:
                        pr.kill()
                    raise RuntimeError("service did not become ready")
                time.sleep(0.1)
    yield ports
    for pr in procs:
        pr.terminate()
        try:
            pr.wait(5)
        except subprocess.TimeoutExpired:
            pr.kill()


def test_services_merge_to_the_single_process_profile(services, reduce_file, tmp_path):
    path, want = reduce_file
    hosts = ",".join(f"127.0.0.1:{p}" for p in services)
    out = str(tmp_path / "svc.json")
    res = subprocess.run([sys.executable, "-m", "elbencho_amd", "--nolive", "--hosts", hosts,
                          "-r", "--dataprofile", "-t", "2", "-b", "64k", "--jsonfile", out,
                          path], env=dict(os.environ, PYTHONPATH=REPO), capture_output=True,
                         text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "data profile" in res.stdout
    (doc,) = dc.json_docs(out)
    dc.assert_same(dc.profile_of_doc(doc), want, "two services")


def test_service_without_a_profile_gives_na(capsys):
    """A service that sends no profile: the master prints n/a, JSON has no key."""
    from elbencho_amd.stats import (PhaseResults, phase_results_json, print_phase_results)
    cfg = BenchConfig()
    cfg.data_profile = True
    r = PhaseResults(phase_name="READ", first_finish_usec=1, last_finish_usec=1, bytes=1)
    print_phase_results(cfg, r)
    assert re.search(r"data profile\s*:\s+n/a", capsys.readouterr().out)
    assert "dataProfile" not in phase_results_json(cfg, r)


RANK_WORKER = r"""
import json, os, sys
sys.path.insert(0, os.environ["EB_REPO"])
import torch.distributed as dist
from elbencho_amd import load_core, parallel
from elbencho_amd.stats import WorkerStats, aggregate_phase

core = load_core()
sync = parallel.init_from_env()
rank = sync.rank
path = os.path.join(os.environ["EB_TMP"], "rank%d" % rank)
cfg = dict(paths=[path], path_type="file", threads=2, file_size=(1 << 20) + 4096 * rank + 77,
           block_size=64 * 1024, dedupe_pct=50, compress_pct=50, data_profile=True,
           bench_seed=1000 + rank)
eng = core.Engine(cfg)
eng.prepare()
for phase in ("WRITE", "READ"):
    sync.barrier()
    eng.start_phase(core.PHASES[phase])
    eng.wait_phase_done(-1)
    workers = [WorkerStats.from_engine(d) for d in eng.finish_phase()]
    local = aggregate_phase(phase, "id", 0.0, workers)
    plain_len = len(local.io_lat.vec)
    total = sync.allreduce_results(local, with_profile=(phase == "READ"))
    if rank == 0:
        p = total.data_profile
        print(json.dumps({"phase": phase, "bytes": total.bytes,
                          "profile": p.to_wire() if p else None}), flush=True)
dist.destroy_process_group()
"""


def test_gloo_two_ranks(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(RANK_WORKER)
    env = dict(os.environ, EB_REPO=REPO, EB_TMP=str(tmp_path), PYTHONPATH=REPO,
               MASTER_ADDR="127.0.0.1", EB_DIST_BACKEND="gloo")
    res = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                          "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(free_port()), str(script)],
                         env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    docs = {d["phase"]: d for d in (json.loads(ln) for ln in res.stdout.splitlines()
                                    if ln.startswith("{"))}
    assert docs["WRITE"]["profile"] is None
    want = dm.empty()
    for rank in (0, 1):
        want = dm.merge(want, dm.profile((tmp_path / f"rank{rank}").read_bytes(), 4096))
    assert docs["READ"]["bytes"] == want["bytes"]
    dc.assert_same(DataProfile.from_wire(docs["READ"]["profile"]).to_engine(), want, "ranks")
    assert len(want["regs"]) == HLL_M
