"""--verifydiag on the CPU: the classification model, the CPU loop, the engine's
CPU paths end to end, and the configuration surface.

tests/verify_diag_model.py is the specification; every record here is compared
with it field for field.
"""

import os
import re

import numpy as np
import pytest

from elbencho_amd import cli
from elbencho_amd.config import BenchConfig, ConfigError
from tests import kernel_model as km
from tests import verify_diag_cases as dc
from tests import verify_diag_model as dm
from tests import verify_mix_model as vm

SALT = dc.SALT
MIB = 1 << 20


# ---------------------------------------------------------------------------
# the model itself
# ---------------------------------------------------------------------------

def test_unmix64_inverts_the_splitmix64_finalizer():
    rng = np.random.default_rng(1)
    z = rng.integers(0, 1 << 64, size=100_000, dtype=np.uint64)
    z[:4] = [0, 1, km.MASK, 1 << 63]
    assert np.array_equal(dm.unmix64(km.splitmix_mix(z.copy())), z)
    assert np.array_equal(km.splitmix_mix(dm.unmix64(z.copy())), z)
    assert int(dm.unmix64(vm.mix(12345))) - km.GOLDEN == 12345


@pytest.mark.parametrize("bs,m", [(0, 0), (8192, 8192)], ids=["plain", "hashed"])
def test_model_classifies_the_canonical_corruptions(bs, m):
    """What the model says about the failures the option is for, stated by hand."""
    n, off = 8192, 5 * 8192
    clean = dm.expected_words(n, off, SALT, bs, m)

    def rec(w):
        return dm.diagnose(w.astype("<u8").tobytes(), off, SALT, bs, m)

    assert rec(clean) == dm.empty()

    w = clean.copy()
    w[100:612] = 0  # a lost 4 KiB page
    assert rec(w) == dict(dm.empty(), nbad=512, first=off + 800, last=off + 611 * 8, runs=1,
                          zero=512)

    w = clean.copy()
    w[512:] = dm.expected_words(4096, off + 4096 - 4096, SALT, bs, m)  # landed 4096 too high
    assert rec(w) == dict(dm.empty(), nbad=512, first=off + 4096, last=off + 8184, runs=1,
                          pattern=512, delta_min=-4096, delta_max=-4096)

    r = rec(dm.expected_words(n, off, SALT + 5, bs, m))  # stale data of another salt
    assert (r["nbad"], r["pattern"], r["delta_min"], r["delta_max"], r["runs"]) == \
        (1024, 1024, 5, 5, 1)

    w = clean.copy()
    w[7] ^= np.uint64(1 << 44)
    assert rec(w) == dict(dm.empty(), nbad=1, first=off + 56, last=off + 56, runs=1, bitflip=1,
                          flip_or=1 << 44)
    w[7] ^= np.uint64((1 << 3) | (1 << 9))  # three bits now
    assert rec(w) == dict(dm.empty(), nbad=1, first=off + 56, last=off + 56, runs=1, other=1)


def test_model_same_flip_in_both_words_of_a_pair_counts_as_pattern():
    """The documented ambiguity (plain positions): delta +2^k gives it away."""
    off = 1 << 20
    w = dm.expected_words(64, off, SALT)
    w[2] ^= np.uint64(1 << 50)
    w[3] ^= np.uint64(1 << 50)
    r = dm.diagnose(w.astype("<u8").tobytes(), off, SALT)
    assert (r["pattern"], r["bitflip"], r["delta_min"], r["delta_max"]) == (2, 0, 1 << 50, 1 << 50)


def test_case_lists_cover_what_they_claim():
    geoms = dc.geometries()
    assert {g[0] for g in geoms} == set(dc.LENS)
    for length in dc.LENS:
        assert {g[1] for g in geoms if g[0] == length} >= ({0} if length < 4096 else set(dc.OFFS))
        assert len({g[2:] for g in geoms if g[0] == length}) == 6
    assert {g[1] for g in geoms} == set(dc.OFFS)
    # a launch that wraps its block boundary, with both kinds of words in it
    assert (4096, 8, 4096, 2048) in geoms
    names = {name for g in geoms for name, _ in dc.corrupted_buffers(g)}
    for want in ("zero_run", "block_from_above", "block_from_below", "other_salt",
                 "flip1_plain", "flip2_hashed", "flip3_plain", "flip8_partner_differs_hashed",
                 "same_flip_in_pair_plain", "bad_x_elem0", "bad_y_elem63", "bad_x_elem64",
                 "bad_x_elem256", "bad_tail", "bad_tail_and_predecessor", "run_127_129",
                 "run_511_513", "runs_at_wave_starts", "garbage"):
        assert want in names, want


# ---------------------------------------------------------------------------
# the CPU loop against the model
# ---------------------------------------------------------------------------

def plain_verify(data, off, bs, m):
    return vm.verify(data, off, SALT, bs, m) if bs else km.verify(data, off, SALT)


@pytest.mark.parametrize("geom", dc.geometries(), ids=dc.geom_id)
def test_cpu_diag_equals_model(core, geom):
    length, off, bs, m = geom
    clean = dc.clean_words(geom).astype("<u8").tobytes()
    assert core.verify_diag(clean, off, SALT, bs, m) == dm.empty()
    for name, data in dc.corrupted_buffers(geom):
        want = dm.diagnose(data, off, SALT, bs, m)
        assert (want["nbad"], want["first"]) == plain_verify(data, off, bs, m), name
        assert want["nbad"] > 0, name
        assert want["nbad"] == want["zero"] + want["pattern"] + want["bitflip"] + want["other"]
        got = core.verify_diag(data, off, SALT, bs, m)
        assert got == want, f"{name}: CPU {got}, model {want}"


@pytest.mark.parametrize("bs,m", [(0, 0), (32 * MIB, 8 * MIB + 8)], ids=["plain", "mix"])
def test_cpu_diag_large_buffer(core, bs, m):
    geom = (dc.BIG_LEN, (1 << 32) - 8, bs, m)
    w = dc.clean_words(geom)
    n = w.size
    wrap = 4096 * 256 * 2                            # first word of the second grid pass
    assert n == wrap + 6
    w[n - 1] ^= np.uint64(1)                         # the odd tail, predecessor bad
    w[n - 2] ^= np.uint64(0xF0F0)
    w[wrap - 2:wrap + 2] = 0                         # a run across the grid-stride wrap
    w[3:5] = dm.expected_words(16, geom[1] + 24 + 4096, SALT, bs, m)  # not one pair: 3 and 4
    w[10:12] = dm.expected_words(16, geom[1] + 80 + 4096, SALT, bs, m)
    data = w.astype("<u8").tobytes()
    want = dm.diagnose(data, geom[1], SALT, bs, m)
    assert want["pattern"] == 2 and want["runs"] == 4 and want["zero"] == 4
    assert core.verify_diag(data, geom[1], SALT, bs, m) == want


@pytest.mark.parametrize("bs,m", [(0, 0), (4096, 1512)], ids=["plain", "mix"])
@pytest.mark.parametrize("d_off,d_len", [(1, 0), (3, 5), (7, 1), (0, 3), (5, 6), (4, 4)])
def test_cpu_diag_unaligned_ranges(core, bs, m, d_off, d_len):
    """Only the CPU loop takes these: a word held in part counts as OTHER."""
    off, n = 3 * 4096 - 64 + d_off, 256 + d_len
    clean = dm.expected_bytes(n, off, SALT, bs, m)
    assert core.verify_diag(clean, off, SALT, bs, m) == dm.empty()
    for pos in ([0], [n - 1], [0, 8], [n - 1, n - 9], [0, n - 1], [40], list(range(n))):
        bad = bytearray(clean)
        for p in pos:
            bad[p] ^= 0x81
        want = dm.diagnose_bytes(bytes(bad), off, SALT, bs, m)
        assert want["nbad"] >= 1
        got = core.verify_diag(bytes(bad), off, SALT, bs, m)
        assert got == want, f"{pos}: CPU {got}, model {want}"


def test_cpu_diag_under_one_word(core):
    clean = dm.expected_bytes(5, 4099, SALT)
    assert core.verify_diag(clean, 4099, SALT) == dm.empty()
    bad = bytes([clean[0] ^ 1]) + clean[1:]
    assert core.verify_diag(bad, 4099, SALT) == dict(dm.empty(), nbad=1, first=4099, last=4099,
                                                     runs=1, other=1)
    assert core.verify_diag(b"", 0, SALT) == dm.empty()


def test_cpu_binding_rejects_bad_geometry(core):
    with pytest.raises(ValueError, match="multiple of 8"):
        core.verify_diag(bytes(64), 0, SALT, 4100, 0)
    with pytest.raises(ValueError, match="multiple of 8"):
        core.verify_diag(bytes(64), 0, SALT, 4096, 12)


def test_message_text_equals_model(core):
    recs = [dict(dm.empty(), nbad=3, first=8, last=4096, runs=2, zero=3),
            dict(dm.empty(), nbad=2, first=0, last=8, runs=1, pattern=2, delta_min=-4096,
                 delta_max=-4096),
            dict(dm.empty(), nbad=4, first=0, last=24, runs=1, pattern=4, delta_min=-8,
                 delta_max=1 << 50),
            dict(dm.empty(), nbad=1, first=0, last=0, runs=1, bitflip=1, flip_or=1 << 63),
            dict(dm.empty(), nbad=5, first=0, last=km.MASK - 7, runs=3, zero=1, pattern=2,
                 bitflip=1, other=1, delta_min=dm.I64_MIN, delta_max=dm.I64_MAX, flip_or=0xA0)]
    for r in recs:
        assert core.verify_diag_text(r) == dm.message_suffix(r)
    assert dm.message_suffix(recs[1]) == (
        "; diagnosis: last bad file offset: 8; runs: 1; zero: 0; pattern: 2; bitflip: 0; "
        "other: 0; pattern delta: -4096")
    assert dm.message_suffix(recs[3]).endswith("; other: 0; flipped bits: 0x8000000000000000")
    assert "; pattern delta: -8..1125899906842624" in dm.message_suffix(recs[2])


# ---------------------------------------------------------------------------
# engine end to end on the CPU (gpu_ids=[])
# ---------------------------------------------------------------------------

BS = 64 * 1024
SIZE = 5 * BS
BLK = 2  # the damaged block

CPU_PATHS = {"sync": dict(), "uring": dict(iodepth=4), "mmap": dict(mmap=True), "dir": None}


def run_phase(core, eng, name):
    eng.start_phase(core.PHASES[name])
    assert eng.wait_phase_done(60_000), f"{name} did not finish"
    return sorted(eng.finish_phase(), key=lambda r: r["rank"])


def run_ok(core, eng, name):
    res = run_phase(core, eng, name)
    errs = [r["error"] for r in res if r["error"]]
    assert not errs, (name, errs)
    return res


def engine_cfg(tmp_path, path_name, pct, diag):
    if path_name == "dir":
        p = tmp_path / "r0" / "d0" / "r0-f0"
        cfg = dict(paths=[str(tmp_path)], path_type="dir", threads=1, num_dataset_threads=1,
                   dirs=1, files=1, file_size=SIZE, block_size=BS, verify_salt=SALT)
    else:
        p = tmp_path / "f"
        cfg = dict(paths=[str(p)], path_type="file", threads=1, num_dataset_threads=1,
                   file_size=SIZE, block_size=BS, verify_salt=SALT, **CPU_PATHS[path_name])
    if pct is not None:
        cfg["verify_mix_pct"] = pct
    if diag:
        cfg["verify_diag"] = True
    return p, cfg


def geometry_of(pct):
    """(block_size, mix_len) as the model takes them."""
    return (0, 0) if pct is None else (BS, vm.mix_len(BS, pct))


def write_and_damage(core, tmp_path, path_name, pct):
    """Engine-written file (checked against the model), then block BLK damaged.
    Returns (path, clean bytes, damaged bytes)."""
    p, cfg = engine_cfg(tmp_path, path_name, pct, diag=True)
    eng = core.Engine(cfg)
    eng.prepare()
    if path_name == "dir":
        run_ok(core, eng, "MKDIRS")
    run_ok(core, eng, "WRITE")
    bs, m = geometry_of(pct)
    clean = p.read_bytes()
    assert clean == dm.expected_words(SIZE, 0, SALT, bs, m).astype("<u8").tobytes()
    run_ok(core, eng, "READ")  # a clean file passes with the flag set
    bad = dc.corrupt_block(clean, BLK, BS, m, mix=bs != 0)
    p.write_bytes(bad)
    return p, clean, bad


@pytest.mark.parametrize("pct", [None, 0, 50], ids=["plain", "pct0", "pct50"])
@pytest.mark.parametrize("path_name", list(CPU_PATHS))
def test_engine_cpu_message_equals_model(core, tmp_path, path_name, pct):
    p, clean, bad = write_and_damage(core, tmp_path, path_name, pct)
    bs, m = geometry_of(pct)
    lo = BLK * BS
    want = dm.diagnose(bad[lo:lo + BS], lo, SALT, bs, m)
    assert (want["zero"], want["pattern"], want["bitflip"], want["other"], want["runs"]) == \
        (512, 512, 1, 1, 4), "the test's damage is not what it claims"
    assert (want["delta_min"], want["delta_max"], want["flip_or"]) == (4096, 4096, 1 << 21)

    _, cfg = engine_cfg(tmp_path, path_name, pct, diag=True)
    eng = core.Engine(cfg)
    eng.prepare()
    err = run_phase(core, eng, "READ")[0]["error"]
    on_gpu, first, rec = dc.parse_message(err)
    assert not on_gpu
    assert rec == dc.without_first(want), err
    # the CPU path names the first bad byte, as it does without the flag
    assert first == dc.first_bad_byte(bad, clean) and first // 8 * 8 == want["first"]
    assert err == ("Data verification failed. First bad file offset: %d; mismatching 8-byte "
                   "words: %d" % (first, want["nbad"])) + dm.message_suffix(want)

    # without the flag: today's message, byte for byte, and the flagged one starts with it
    _, cfg = engine_cfg(tmp_path, path_name, pct, diag=False)
    plain_eng = core.Engine(cfg)
    plain_eng.prepare()
    plain_err = run_phase(core, plain_eng, "READ")[0]["error"]
    assert plain_err == f"Data verification failed. First bad file offset: {first}"
    assert err.startswith(plain_err + "; mismatching 8-byte words: ")

    # the repaired file passes on the engine that reported the failure
    p.write_bytes(clean)
    run_ok(core, eng, "READ")


@pytest.mark.parametrize("tail", [8, 4])
def test_engine_cpu_ragged_tail_block(core, tmp_path, tail):
    """A last block of 8 or 4 bytes: a whole word, and a word held in part."""
    size = 2 * BS + tail
    p = tmp_path / "f"
    cfg = dict(paths=[str(p)], path_type="file", threads=1, num_dataset_threads=1,
               file_size=size, block_size=BS, verify_salt=SALT, verify_diag=True)
    eng = core.Engine(cfg)
    eng.prepare()
    run_ok(core, eng, "WRITE")
    clean = p.read_bytes()
    bad = bytearray(clean)
    bad[2 * BS + 1] ^= 0x04
    p.write_bytes(bytes(bad))
    err = run_phase(core, eng, "READ")[0]["error"]
    _, first, rec = dc.parse_message(err)
    want = dm.diagnose_bytes(bytes(bad[2 * BS:]), 2 * BS, SALT)
    assert first == 2 * BS + 1 and rec == dc.without_first(want), err
    assert (want["bitflip"], want["other"]) == ((1, 0) if tail == 8 else (0, 1))
    p.write_bytes(clean)
    run_ok(core, eng, "READ")


# ---------------------------------------------------------------------------
# configuration surface
# ---------------------------------------------------------------------------

def parse(argv):
    return cli.args_to_config(cli.build_parser().parse_args(argv))


def test_cli_flag_round_trips_into_wire_and_engine_dict(tmp_path):
    base = ["-r", "-s", "1m", "-b", "4k", "--verify", "7", str(tmp_path / "f")]
    cfg = parse(base)
    assert cfg.verify_diag is False and BenchConfig().verify_diag is False
    assert cfg.to_wire()["verify_diag"] is False
    assert cfg.engine_dict()["verify_diag"] is False

    cfg = parse(["--verifydiag"] + base)
    assert cfg.verify_diag is True
    wire = cfg.to_wire()
    assert wire["verify_diag"] is True
    back = BenchConfig.from_wire(wire)
    assert back.verify_diag is True and back.to_wire() == wire
    assert back.engine_dict()["verify_diag"] is True

    cfg = parse(["--verifydiag", "--verifymixpct", "50"] + base)
    assert cfg.engine_dict()["verify_diag"] is True
    assert cfg.engine_dict()["verify_mix_pct"] == 50


def test_config_error_without_verify(tmp_path):
    with pytest.raises(ConfigError, match="--verifydiag requires --verify"):
        parse(["-r", "-s", "1m", "-b", "4k", "--verifydiag", str(tmp_path / "f")])


@pytest.mark.parametrize("mode", ["s3", "hdfs", "netbench"])
def test_config_error_outside_file_bdev_dir(mode):
    cfg = BenchConfig()
    cfg.run_read = True
    cfg.verify = 7
    cfg.verify_diag = True
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
    with pytest.raises(ConfigError,
                       match="--verifydiag supports file, block device and directory paths only"):
        cfg.validate()
    cfg.verify_diag = False
    cfg.validate()  # the same configuration is fine without the option


def test_docs_name_the_option():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for rel in ("docs/help.md", "docs/help-all.md", "docs/help-multi.md", "docs/usage.md",
                "docs/DESIGN.md", "COMPONENTS.md"):
        with open(os.path.join(root, rel)) as f:
            assert "--verifydiag" in f.read(), rel
    with open(os.path.join(root, "docs/service-protocol.md")) as f:
        assert "verify_diag" in f.read()
    with open(os.path.join(root, "docs/usage.md")) as f:
        usage = f.read()
    for cls in ("`zero`", "`pattern`", "`bitflip`", "`other`"):
        assert cls in usage, cls


def test_generated_bash_completion_names_the_option():
    opts = re.search(r'local opts="([^"]*)"', cli.bash_completion()).group(1).split()
    assert "--verifydiag" in opts
