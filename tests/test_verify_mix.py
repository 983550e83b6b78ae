"""--verifymixpct on the CPU: the pattern model, the CPU fill/verify loops, the
engine's CPU paths end to end, and the configuration surface.

tests/verify_mix_model.py is the specification; everything here is compared
with it byte for byte.
"""

import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

from elbencho_amd import cli
from elbencho_amd.config import BenchConfig, ConfigError
from tests import kernel_model as km
from tests import verify_mix_model as vm

MIB = 1 << 20
SALT = 0x0123456789AB
BS = 4096
PCTS = [37, 100]
ERR_RE = re.compile(r"First bad file offset: (\d+)")


# ---------------------------------------------------------------------------
# model ties
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("x", [0, 1, 12345, km.MASK, km.MASK - km.GOLDEN + 1, 1 << 63])
def test_mix_is_one_splitmix64_step(x):
    assert int(vm.mix(x)) == km.splitmix64(x)[1]


def test_mix_len_rounds_down_to_words():
    assert vm.mix_len(4096, 0) == 0
    assert vm.mix_len(4096, 100) == 4096
    assert vm.mix_len(4096, 37) == 1512      # 1515.52 -> 1515 -> 1512
    assert vm.mix_len(4096, 50) == 2048
    assert vm.mix_len(MIB, 25) == MIB // 4
    assert vm.mix_len(1000, 33) == 328


@pytest.mark.parametrize("salt", [0, 1, 12345])
@pytest.mark.parametrize("off", [0, 8, 3 * MIB + 24])
def test_pct0_is_the_plain_verify_pattern(core, salt, off):
    n = 3 * BS + 8
    assert vm.pattern(n, off, salt, BS, 0) == core.fill_checksum(n, off, salt)
    assert core.fill_checksum_mix(n, off, salt, BS, 0) == core.fill_checksum(n, off, salt)
    assert core.fill_checksum_mix(n + 5, off + 3, salt, BS, 0) == \
        core.fill_checksum(n + 5, off + 3, salt)


@pytest.mark.parametrize("pct", [37, 100])
def test_all_words_of_a_block_are_distinct(pct):
    w = vm.words(MIB, 5 * MIB, SALT, MIB, vm.mix_len(MIB, pct))
    assert np.unique(w).size == MIB // 8


@pytest.mark.parametrize("d_off,d_len", [(0, 0), (1, 0), (3, 0), (7, 0), (0, 1), (0, 3), (0, 7),
                                         (1, 7), (3, 3), (7, 1), (5, 6)])
@pytest.mark.parametrize("m", [0, 8, 1512, BS - 8, BS])
def test_cpu_fill_equals_model_unaligned(core, m, d_off, d_len):
    off, n = 2 * BS - 64 + d_off, 2 * BS + d_len  # crosses two block boundaries
    assert core.fill_checksum_mix(n, off, SALT, BS, m) == vm.pattern(n, off, SALT, BS, m)


@pytest.mark.parametrize("off", [0, 1, 3, 7, BS - 3, BS + 1504 + 5, BS + 1512 - 2])
@pytest.mark.parametrize("n", [0, 1, 2, 5, 7])
def test_cpu_fill_equals_model_under_one_word(core, off, n):
    assert core.fill_checksum_mix(n, off, SALT, BS, 1512) == vm.pattern(n, off, SALT, BS, 1512)


def test_cpu_loops_handle_a_range_ending_at_2_pow_64(core):
    """Like the plain loops: pos/end are compared by difference only."""
    bs, m = 4096, 2048  # 2^64 is a multiple of the block size
    for n in (8, 24, 4096 + 13):
        off = (1 << 64) - n
        lo = off // 8 * 8
        w = vm.words((1 << 64) - lo, lo, SALT, bs, m).astype("<u8").tobytes()
        want = w[off - lo:]
        got = core.fill_checksum_mix(n, off, SALT, bs, m)
        assert got == want, n
        assert core.verify_checksum_mix(got, off, SALT, bs, m) == km.U64_MAX
        bad = bytearray(got)
        bad[-1] ^= 0x10
        assert core.verify_checksum_mix(bytes(bad), off, SALT, bs, m) == (1 << 64) - 1


# ---------------------------------------------------------------------------
# boundaries of M
# ---------------------------------------------------------------------------

M_EDGES = [0, 8, 1512, 2040, BS - 8, BS]  # 1512 % 16 == 8, 2040 % 16 == 8


@pytest.mark.parametrize("m", M_EDGES)
def test_boundary_of_m_is_where_the_words_change_kind(core, m):
    data = core.fill_checksum_mix(2 * BS, 6 * BS, SALT, BS, m)
    assert data == vm.pattern(2 * BS, 6 * BS, SALT, BS, m)
    got = np.frombuffer(data, dtype="<u8")
    plain = km.checksum_words(2 * BS, 6 * BS, SALT)
    hashed = vm.mix(plain)
    for blk in range(2):
        w = slice(blk * BS // 8, (blk + 1) * BS // 8)
        assert np.array_equal(got[w][:m // 8], hashed[w][:m // 8])
        assert np.array_equal(got[w][m // 8:], plain[w][m // 8:])


@pytest.mark.parametrize("m", M_EDGES)
@pytest.mark.parametrize("phase", [8, 1504, 1512, 1520, BS - 8])
def test_range_crossing_a_block_boundary(core, m, phase):
    off = 9 * BS + phase
    assert core.fill_checksum_mix(BS, off, SALT, BS, m) == vm.pattern(BS, off, SALT, BS, m)


def test_pattern_does_not_depend_on_chunking(core):
    m, size = 1512, 5 * BS + 8
    whole = core.fill_checksum_mix(size, 0, SALT, BS, m)
    for cuts in ([0, 100, 4096, 4097, 9000, size], [0, 8, 1512, 1520, 3 * BS - 8, size]):
        parts = b"".join(core.fill_checksum_mix(b - a, a, SALT, BS, m)
                         for a, b in zip(cuts, cuts[1:]))
        assert parts == whole


# ---------------------------------------------------------------------------
# verify
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("m", M_EDGES)
def test_cpu_verify_clean(core, m):
    off, n = 3 * BS + 24, 2 * BS + 8
    assert core.verify_checksum_mix(vm.pattern(n, off, SALT, BS, m), off, SALT, BS, m) == \
        km.U64_MAX
    assert core.verify_checksum_mix(vm.pattern(n + 5, off + 3, SALT, BS, m), off + 3, SALT,
                                    BS, m) == km.U64_MAX


@pytest.mark.parametrize("rel,what", [(16, "hashed"), (3000, "plain"), (1504, "last hashed"),
                                      (1512, "first plain"), (0, "first"), (BS - 8, "last")])
@pytest.mark.parametrize("byte", [0, 5])
def test_cpu_verify_reports_the_flipped_byte(core, rel, what, byte):
    m, off, n = 1512, 4 * BS, 2 * BS
    for blk in (0, 1):
        bad = bytearray(vm.pattern(n, off, SALT, BS, m))
        pos = blk * BS + rel + byte
        bad[pos] ^= 0x01
        assert core.verify_checksum_mix(bytes(bad), off, SALT, BS, m) == off + pos, what
        assert vm.verify(bytes(bad), off, SALT, BS, m) == (1, off + pos - byte)


def test_cpu_verify_wrong_m_fails_at_the_smaller_m(core):
    data = vm.pattern(2 * BS, 0, SALT, BS, 1512)
    bad = core.verify_checksum_mix(data, 0, SALT, BS, BS)
    assert bad // 8 * 8 == 1512
    bad = core.verify_checksum_mix(data, 0, SALT, BS, 8)
    assert bad // 8 * 8 == 8


@pytest.mark.parametrize("args", [(0, 0), (4095, 0), (4100, 8), (4096, 12), (4096, 4104)])
def test_cpu_bindings_reject_bad_geometry(core, args):
    with pytest.raises(ValueError):
        core.fill_checksum_mix(64, 0, SALT, *args)
    with pytest.raises(ValueError):
        core.verify_checksum_mix(b"\0" * 64, 0, SALT, *args)


# ---------------------------------------------------------------------------
# compressibility: the point of the option
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("salt", [0, 1, 12345])
def test_compressibility(core, salt):
    ratio = {}
    for pct in (0, 25, 50, 100):
        data = core.fill_checksum_mix(MIB, 0, salt, MIB, vm.mix_len(MIB, pct))
        assert data == vm.pattern(MIB, 0, salt, MIB, vm.mix_len(MIB, pct))
        ratio[pct] = len(zlib.compress(data, 6)) / MIB
    print(f"salt {salt}: zlib-6 ratios {ratio}")
    assert ratio[100] >= 0.99
    assert ratio[0] <= 0.20
    assert ratio[0] < ratio[25] < ratio[50] < ratio[100]


# ---------------------------------------------------------------------------
# engine end to end on the CPU
# ---------------------------------------------------------------------------

def run_phase(core, eng, name):
    eng.start_phase(core.PHASES[name])
    assert eng.wait_phase_done(60_000), f"{name} did not finish"
    return sorted(eng.finish_phase(), key=lambda r: r["rank"])


def run_ok(core, eng, name):
    res = run_phase(core, eng, name)
    errs = [r["error"] for r in res if r["error"]]
    assert not errs, (name, errs)
    return res


def file_cfg(paths, size, pct, threads=1, **kw):
    cfg = dict(paths=[str(p) for p in paths], path_type="file", threads=threads,
               num_dataset_threads=threads, file_size=size, block_size=BS,
               verify_salt=SALT, verify_mix_pct=pct)
    cfg.update(kw)
    return cfg


def model_file(size, pct):
    return vm.pattern(size, 0, SALT, BS, vm.mix_len(BS, pct))


CPU_PATHS = {"sync": dict(), "uring": dict(iodepth=4), "mmap": dict(mmap=True)}


@pytest.mark.parametrize("tail", [0, 8, 4])
@pytest.mark.parametrize("pct", PCTS)
@pytest.mark.parametrize("path_name", list(CPU_PATHS))
def test_engine_write_equals_model_and_read_passes(core, tmp_path, path_name, pct, tail):
    size = 5 * BS + tail
    p = tmp_path / "f"
    eng = core.Engine(file_cfg([p], size, pct, threads=2, **CPU_PATHS[path_name]))
    eng.prepare()
    res = run_ok(core, eng, "WRITE")
    assert sum(r["bytes"] for r in res) == size
    assert p.read_bytes() == model_file(size, pct)
    res = run_ok(core, eng, "READ")
    assert sum(r["bytes"] for r in res) == size


@pytest.mark.parametrize("pct", PCTS)
@pytest.mark.parametrize("path_name", list(CPU_PATHS))
def test_engine_two_files_short_block_at_the_file_boundary(core, tmp_path, path_name, pct):
    """Each file ends in a half block; the next block starts the next file at
    its offset 0: every file is the whole pattern from its own offset 0."""
    size = 2 * BS + BS // 2
    paths = [tmp_path / "a", tmp_path / "b"]
    eng = core.Engine(file_cfg(paths, size, pct, threads=2, **CPU_PATHS[path_name]))
    eng.prepare()
    res = run_ok(core, eng, "WRITE")
    assert sum(r["bytes"] for r in res) == 2 * size
    for p in paths:
        assert p.read_bytes() == model_file(size, pct), p.name
    run_ok(core, eng, "READ")


@pytest.mark.parametrize("iodepth", [1, 4])
@pytest.mark.parametrize("pct", PCTS)
def test_engine_dir_mode(core, tmp_path, pct, iodepth):
    size = 3 * BS + 8
    cfg = dict(paths=[str(tmp_path)], path_type="dir", threads=2, num_dataset_threads=2,
               dirs=1, files=2, file_size=size, block_size=BS, iodepth=iodepth,
               verify_salt=SALT, verify_mix_pct=pct)
    eng = core.Engine(cfg)
    eng.prepare()
    run_ok(core, eng, "MKDIRS")
    res = run_ok(core, eng, "WRITE")
    assert [r["bytes"] for r in res] == [2 * size, 2 * size]
    for r in range(2):
        for f in range(2):
            got = (tmp_path / f"r{r}" / "d0" / f"r{r}-f{f}").read_bytes()
            assert got == model_file(size, pct), (r, f)
    run_ok(core, eng, "READ")


def test_engine_random_aligned_write(core, tmp_path):
    size = 16 * BS
    p = tmp_path / "f"
    eng = core.Engine(file_cfg([p], size, 37, random=True, rand_aligned=True))
    eng.prepare()
    run_ok(core, eng, "WRITE")  # full-coverage random order: every block once
    assert p.read_bytes() == model_file(size, 37)
    run_ok(core, eng, "READ")   # random aligned reads of the same pattern pass


@pytest.mark.parametrize("path_name", list(CPU_PATHS))
@pytest.mark.parametrize("wrote,reads", [(37, 100), (100, 37), (37, 0), (0, 37)])
def test_engine_read_with_another_pct_fails_at_the_smaller_m(core, tmp_path, path_name, wrote,
                                                             reads):
    size = 4 * BS
    p = tmp_path / "f"
    eng = core.Engine(file_cfg([p], size, wrote, **CPU_PATHS[path_name]))
    eng.prepare()
    run_ok(core, eng, "WRITE")
    del eng
    eng = core.Engine(file_cfg([p], size, reads, **CPU_PATHS[path_name]))
    eng.prepare()
    err = run_phase(core, eng, "READ")[0]["error"]
    m = ERR_RE.search(err)
    assert m and "verification failed" in err, err
    # the first word whose kind differs; the report names a byte inside it
    assert int(m.group(1)) // 8 * 8 == min(vm.mix_len(BS, wrote), vm.mix_len(BS, reads))


def test_engine_plain_read_of_mix_data_and_back(core, tmp_path):
    """Unset is the plain pattern: it equals pct 0 and differs from pct 37."""
    size = 4 * BS
    p = tmp_path / "f"
    cfg = file_cfg([p], size, 0)
    eng = core.Engine(cfg)
    eng.prepare()
    run_ok(core, eng, "WRITE")
    assert p.read_bytes() == km.checksum_pattern(size, 0, SALT)
    del cfg["verify_mix_pct"]
    eng = core.Engine(cfg)
    eng.prepare()
    run_ok(core, eng, "READ")
    run_ok(core, eng, "WRITE")
    assert p.read_bytes() == km.checksum_pattern(size, 0, SALT)
    # a pct 37 file read with the option unset fails in the first hashed word
    weng = core.Engine(file_cfg([p], size, 37))
    weng.prepare()
    run_ok(core, weng, "WRITE")
    assert p.read_bytes() == model_file(size, 37)
    err = run_phase(core, eng, "READ")[0]["error"]
    m = ERR_RE.search(err)
    assert m and "verification failed" in err, err
    assert int(m.group(1)) // 8 * 8 == 0


@pytest.mark.parametrize("path_name", list(CPU_PATHS))
@pytest.mark.parametrize("pos", [2 * BS + 16 + 3, 2 * BS + 3000, BS + 1504, BS + 1512 + 7,
                                 3 * BS + 4],
                         ids=["hashed", "plain", "last_hashed", "first_plain", "tail"])
def test_engine_reports_a_corrupted_word_exactly(core, tmp_path, path_name, pos):
    size = 3 * BS + 8
    p = tmp_path / "f"
    eng = core.Engine(file_cfg([p], size, 37, **CPU_PATHS[path_name]))
    eng.prepare()
    run_ok(core, eng, "WRITE")
    clean = p.read_bytes()
    assert clean == model_file(size, 37)
    bad = bytearray(clean)
    bad[pos] ^= 0x40
    p.write_bytes(bytes(bad))
    err = run_phase(core, eng, "READ")[0]["error"]
    m = ERR_RE.search(err)
    assert m and "verification failed" in err, err
    assert int(m.group(1)) == pos
    p.write_bytes(clean)
    run_ok(core, eng, "READ")


@pytest.mark.parametrize("cfg,msg", [
    (dict(verify_mix_pct=101), "0..100"),
    (dict(verify_mix_pct=-2), "0..100"),
    (dict(verify_mix_pct=50, verify_salt=-1), "verify_salt"),
    (dict(verify_mix_pct=50, block_size=4100), "multiple of 8"),
])
def test_engine_rejects_bad_config(core, tmp_path, cfg, msg):
    full = file_cfg([tmp_path / "f"], 4 * BS, 50)
    full.update(cfg)
    with pytest.raises(ValueError, match=msg):
        core.Engine(full)


# ---------------------------------------------------------------------------
# configuration surface
# ---------------------------------------------------------------------------

def parse(argv):
    return cli.args_to_config(cli.build_parser().parse_args(argv))


def test_cli_round_trips_into_wire_and_engine_dict(tmp_path):
    p = str(tmp_path / "f")
    cfg = parse(["-w", "-s", "1m", "-b", "4k", "--verify", "7", "--verifymixpct", "37", p])
    assert cfg.verify_mix_pct == 37
    wire = cfg.to_wire()
    assert wire["verify_mix_pct"] == 37
    back = BenchConfig.from_wire(wire)
    assert back.verify_mix_pct == 37
    assert back.engine_dict()["verify_mix_pct"] == 37
    assert cfg.engine_dict()["verify_salt"] == 7


def test_cli_default_is_unset(tmp_path):
    cfg = parse(["-w", "-s", "1m", "-b", "4k", "--verify", "7", str(tmp_path / "f")])
    assert cfg.verify_mix_pct == -1
    assert cfg.to_wire()["verify_mix_pct"] == -1
    assert cfg.engine_dict()["verify_mix_pct"] == -1
    assert BenchConfig().verify_mix_pct == -1


def test_cli_pct0_is_accepted(tmp_path):
    cfg = parse(["-w", "-s", "1m", "-b", "4k", "--verify", "7", "--verifymixpct", "0",
                 str(tmp_path / "f")])
    assert cfg.engine_dict()["verify_mix_pct"] == 0


@pytest.mark.parametrize("extra,msg", [
    (["--verify", "7", "--verifymixpct", "101"], "0..100"),
    (["--verify", "7", "--verifymixpct", "-2"], "0..100"),
    (["--verifymixpct", "50"], "requires --verify"),
    (["--verify", "7", "--verifymixpct", "50", "-b", "4100"], "multiple of 8"),
])
def test_config_errors(tmp_path, extra, msg):
    argv = ["-w", "-s", "1m", "-b", "4k"] + extra + [str(tmp_path / "f")]
    with pytest.raises(ConfigError, match=msg):
        parse(argv)


@pytest.mark.parametrize("mode", ["s3", "hdfs", "netbench"])
def test_config_error_outside_file_bdev_dir(tmp_path, mode):
    cfg = BenchConfig()
    cfg.run_write = True
    cfg.verify = 7
    cfg.verify_mix_pct = 50
    cfg.block_size = 4096
    cfg.file_size = MIB
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
    cfg.verify_mix_pct = -1
    cfg.validate()  # the same configuration is fine without the option


@pytest.mark.parametrize("pct", PCTS)
def test_verifydirect_with_the_option(core, tmp_path, pct):
    p = tmp_path / "f"
    cfg = parse(["-w", "-s", str(4 * BS + 8), "-b", "4k", "--verify", "7", "--verifymixpct",
                 str(pct), "--verifydirect", str(p)])
    d = cfg.engine_dict()
    assert d["verify_direct"] and d["verify_mix_pct"] == pct
    eng = core.Engine(d)
    eng.prepare()
    run_ok(core, eng, "WRITE")
    assert p.read_bytes() == vm.pattern(4 * BS + 8, 0, 7, BS, vm.mix_len(BS, pct))


def test_docs_name_the_option():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for rel in ("docs/help.md", "docs/help-all.md", "docs/help-multi.md", "docs/usage.md",
                "docs/DESIGN.md", "COMPONENTS.md"):
        with open(os.path.join(root, rel)) as f:
            assert "--verifymixpct" in f.read(), rel
    with open(os.path.join(root, "docs/service-protocol.md")) as f:
        assert "verify_mix_pct" in f.read()


def test_generated_bash_completion_names_the_option():
    """cli.bash_completion() generates the completion script from the parser
    and names the option. The packaged copy under dist/ is output of an
    earlier run of the same generation and is not regenerated here (it lacks
    the options added since, --dynslice among them): for the options it knows,
    the generator reproduces it byte for byte."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = cli.bash_completion()
    opts = re.search(r'local opts="([^"]*)"', text).group(1).split()
    assert "--verifymixpct" in opts and "--verify" in opts and "-w" in opts
    assert opts == sorted(set(opts))
    with open(os.path.join(root, "dist/etc/bash_completion.d/elbencho-amd")) as f:
        packaged = f.read()
    known = set(re.search(r'local opts="([^"]*)"', packaged).group(1).split())
    assert known <= set(opts)
    assert text.replace(" ".join(opts), " ".join(o for o in opts if o in known)) == packaged
    tool = subprocess.run([sys.executable, os.path.join(root, "tools",
                                                        "elbencho-amd-bash-completion")],
                          capture_output=True, text=True, check=True)
    assert tool.stdout == text
