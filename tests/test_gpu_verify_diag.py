"""--verifydiag on the GPU: ebVerifyDiagKernel / ebVerifyDiagMixKernel against
the numpy model (tests/verify_diag_model.py), against the plain verify kernels
and the CPU loop, and the engine's GPU read paths end to end.

Every record is compared with the model field for field. The shapes and
corruptions are those of tests/verify_diag_cases.py.
"""

import os

import numpy as np
import pytest

from tests import verify_diag_cases as dc
from tests import verify_diag_model as dm
from tests import verify_mix_model as vm

pytestmark = pytest.mark.gpu

SALT = dc.SALT
MIB = 1 << 20
VERIFY_FETCH_INTERVAL = 64  # GPU-checked blocks per fetch of the device record
URING_DEPTH = 4


@pytest.fixture(autouse=True)
def require_gpu(core):
    if core.gpu_device_count() < 1:
        pytest.fail("GPU test run but no HIP device available — the HIP path "
                    "must not silently fall back to CPU")


def as_bytes(w: np.ndarray) -> bytes:
    return w.astype("<u8").tobytes()


# ---------------------------------------------------------------------------
# kernels against the model
# ---------------------------------------------------------------------------

GEOMS = dc.geometries()


@pytest.mark.parametrize("gi", range(len(GEOMS)), ids=[dc.geom_id(g) for g in GEOMS])
def test_gpu_diag_equals_model(core, gi):
    """Every corruption of one geometry, each its own launch and fetch on one
    context; a clean launch first and last (it reports the initial record,
    also right after fetches that reported errors)."""
    geom = GEOMS[gi]
    length, off, bs, m = geom
    clean = as_bytes(dc.clean_words(geom))
    cases = list(dc.corrupted_buffers(geom))
    items = [(clean, off)] + [(data, off) for _, data in cases] + [(clean, off)]
    got = core.gpu_verify_diag_batch(items, SALT, 0, bs, m, fetch_each=True)
    assert len(got) == len(items)
    assert got[0] == dm.empty() and got[-1] == dm.empty()
    for (name, data), rec in zip(cases, got[1:-1]):
        want = dm.diagnose(data, off, SALT, bs, m)
        assert rec == want, f"{name}: GPU {rec}, model {want}"
        cpu = core.verify_diag(data, off, SALT, bs, m)
        assert rec == cpu, f"{name}: GPU {rec}, CPU {cpu}"

    # the plain verify kernels count the same words and find the same first one
    for k in (gi % len(cases), (gi * 7 + 3) % len(cases)):
        name, data = cases[k]
        plain = core.gpu_verify_checksum_mix(data, off, SALT, bs, m) if bs else \
            core.gpu_verify_checksum(data, off, SALT)
        assert (got[1 + k]["nbad"], got[1 + k]["first"]) == tuple(plain), name


@pytest.mark.parametrize("bs,m", [(0, 0), (4096, 2048)], ids=["plain", "mix"])
@pytest.mark.parametrize("length", [8, 24, 1040])
def test_gpu_diag_one_shot(core, length, bs, m):
    geom = (length, 8, bs, m)
    assert core.gpu_verify_diag(as_bytes(dc.clean_words(geom)), 8, SALT, 0, bs, m) == dm.empty()
    for name, data in dc.corrupted_buffers(geom):
        want = dm.diagnose(data, 8, SALT, bs, m)
        assert core.gpu_verify_diag(data, 8, SALT, 0, bs, m) == want, name


@pytest.mark.parametrize("bs,m", [(0, 0), (4096, 2048)], ids=["plain", "mix"])
def test_gpu_diag_batch_accumulates_and_resets(core, bs, m):
    """Several launches, one fetch: the record is the models' combination (runs
    do not join across launches). The second fetch and a clean launch after a
    fetch that reported errors give the initial record."""
    items, want = [], dm.empty()
    for i, off in enumerate([0, 4096, 3 * 4096, (1 << 40) + 2048 + 8]):  # the last: plain words
        geom = (4096 if i < 3 else 1040, off, bs, m)
        cases = dict(dc.corrupted_buffers(geom))
        name = ["zero_run", "block_from_above", "run_127_129", "flip1_plain"][i]
        items.append((cases[name], off))
        want = dm.combine(want, dm.diagnose(cases[name], off, SALT, bs, m))
    clean = as_bytes(dm.expected_words(4096, 7 * 4096, SALT, bs, m))
    got = core.gpu_verify_diag_batch(items, SALT, 0, bs, m, then=(clean, 7 * 4096))
    assert got[0] == want, f"GPU {got[0]}, model {want}"
    assert want["zero"] and want["pattern"] and want["bitflip"] and want["other"]
    assert got[1] == dm.empty()
    assert got[2] == dm.empty()

    # a bad launch after the reset is reported alone
    got = core.gpu_verify_diag_batch(items[:1], SALT, 0, bs, m, then=items[1])
    assert got[2] == dm.diagnose(items[1][0], items[1][1], SALT, bs, m)


def test_gpu_diag_runs_do_not_join_across_launches(core):
    w = dm.expected_words(8192, 0, SALT)
    w[500:524] = 0  # one run in one launch, two in two launches of 4096 bytes
    one = core.gpu_verify_diag(as_bytes(w), 0, SALT)
    two = core.gpu_verify_diag_batch([(as_bytes(w[:512]), 0), (as_bytes(w[512:]), 4096)], SALT)[0]
    assert one == dm.diagnose(as_bytes(w), 0, SALT) and one["runs"] == 1
    assert two == dict(one, runs=2)


@pytest.mark.parametrize("bs,m", [(0, 0), (32 * MIB, 8 * MIB + 8)], ids=["plain", "mix"])
def test_gpu_diag_grid_stride_wrap(core, bs, m):
    """16 MiB + 48: the grid is capped at 4096 workgroups, so elements from
    4096 * 256 on are a second pass of the first threads; the odd final word
    follows it."""
    off = (1 << 32) - 8
    geom = (dc.BIG_LEN, off, bs, m)
    w = dc.clean_words(geom)
    n = w.size
    wrap = 4096 * 256 * 2  # first word of the second grid pass
    assert n == wrap + 6
    w[n - 1] ^= np.uint64(1)          # the odd tail, its predecessor bad
    w[n - 2] ^= np.uint64(0xF0F0)
    w[wrap - 2:wrap + 2] = 0          # a run across the wrap: lane 0 loads its predecessor
    w[3:5] = dm.expected_words(16, off + 24 + 4096, SALT, bs, m)    # words of two pairs
    w[10:12] = dm.expected_words(16, off + 80 + 4096, SALT, bs, m)  # one pair
    w[wrap // 2 + 1] ^= np.uint64(1 << 62)
    data = as_bytes(w)
    want = dm.diagnose(data, off, SALT, bs, m)
    assert (want["pattern"], want["runs"], want["zero"]) == (2, 5, 4)
    got = core.gpu_verify_diag(data, off, SALT, 0, bs, m)
    assert got == want, f"GPU {got}, model {want}"
    assert got == core.verify_diag(data, off, SALT, bs, m)
    assert core.gpu_verify_diag(as_bytes(dc.clean_words(geom)), off, SALT, 0, bs, m) == dm.empty()


@pytest.mark.parametrize("args,msg", [
    ((bytes(20), 0, SALT, 0), "len 20 is not a multiple of 8"),
    ((bytes(16), 4, SALT, 0), "fileOff 4 is not a multiple of 8"),
    ((bytes(16), 0, SALT, 0, 4100, 0), "block size 4100"),
    ((bytes(16), 0, SALT, 0, 4096, 12), "mix length 12"),
    ((bytes(16), 0, SALT, 0, 4096, 4104), "exceeds the block size"),
    ((bytes(4104), 0, SALT, 0, 4096, 0), "len 4104 exceeds the block size"),
])
def test_gpu_diag_rejects_bad_arguments(core, args, msg):
    with pytest.raises(ValueError, match=msg):
        core.gpu_verify_diag(*args)


def test_gpu_diag_bench_runs(core):
    assert core.gpu_verify_diag_bench(1 << 20, 2, 0) > 0
    with pytest.raises(ValueError):
        core.gpu_verify_diag_bench(24, 2, 0)


# ---------------------------------------------------------------------------
# engine end to end, gpu_ids=[0]
# ---------------------------------------------------------------------------

CBS = 4096
W = CBS // 8
BLOCKS = 70  # more than one fetch window of the accumulating paths

# "acc": one diag launch per block into the device record, fetched after every
# 64 GPU-checked blocks and at the end of the phase: one report covers the
# fetch window. "blk": each block is checked as it completes: one report
# covers one block. (The half-ring batched read runs only with verify off.)
GPU_PATHS = {
    "pipelined": ("acc", dict(iodepth=1)),
    "mmap": ("acc", dict(mmap=True)),
    "blockio": ("blk", dict(flock_mode=1)),
    "uring": ("blk", dict(iodepth=URING_DEPTH)),
    "dir": ("blk", None),
}


def overwrite(p, data: bytes):
    """Rewrite in place (no truncation: the mmap path keeps the file mapped)."""
    with open(p, "r+b" if os.path.exists(p) else "wb") as f:
        f.write(data)


def run_phase(core, eng, name):
    eng.start_phase(core.PHASES[name])
    assert eng.wait_phase_done(60_000), f"{name} did not finish"
    return sorted(eng.finish_phase(), key=lambda r: r["rank"])


def run_ok(core, eng, name):
    res = run_phase(core, eng, name)
    errs = [r["error"] for r in res if r["error"]]
    assert not errs, (name, errs)
    return res


def gpu_engine_cfg(tmp_path, path_name, size, pct, diag=True):
    path_cfg = GPU_PATHS[path_name][1]
    if path_name == "dir":
        p = tmp_path / "r0" / "d0" / "r0-f0"
        os.makedirs(p.parent, exist_ok=True)
        cfg = dict(paths=[str(tmp_path)], path_type="dir", threads=1, num_dataset_threads=1,
                   dirs=1, files=1, file_size=size, block_size=CBS, iodepth=URING_DEPTH,
                   gpu_ids=[0], verify_salt=SALT)
    else:
        p = tmp_path / "f"
        cfg = dict(paths=[str(p)], path_type="file", threads=1, num_dataset_threads=1,
                   file_size=size, block_size=CBS, gpu_ids=[0], verify_salt=SALT, **path_cfg)
    if pct is not None:
        cfg["verify_mix_pct"] = pct
    if diag:
        cfg["verify_diag"] = True
    return p, cfg


def geometry_of(pct):
    return (0, 0) if pct is None else (CBS, vm.mix_len(CBS, pct))


def damaged_words(size, bs, m, window):
    """The clean file's words with damage in the first fetch window (blocks 3,
    20 and 40) and/or the second one (block 66)."""
    w = dm.expected_words(size // 8 * 8, 0, SALT, bs, m).copy()
    if "first" in window:
        w[3 * W + 10:3 * W + 201] = 0                       # zeros, not a whole page
        w[3 * W + 300] ^= np.uint64(1 << 7)                 # and a flipped bit (hashed or not)
        w[3 * W + 400] ^= np.uint64(1 << 9)
        w[20 * W + 511] ^= np.uint64(0x1001001)             # three bits, last word of a block
        w[40 * W:41 * W] = dm.expected_words(CBS, 41 * CBS, SALT, bs, m)  # block 41's data
    if "second" in window:
        w[66 * W + 3:66 * W + 5] = 0
    return w


def window_model(bad: bytes, blocks, bs, m):
    rec = dm.empty()
    for b in blocks:
        rec = dm.combine(rec, dm.diagnose(bad[b * CBS:(b + 1) * CBS], b * CBS, SALT, bs, m))
    return rec


@pytest.mark.parametrize("pct", [None, 50], ids=["plain", "pct50"])
@pytest.mark.parametrize("path_name", list(GPU_PATHS))
def test_engine_gpu_message_equals_model(core, tmp_path, path_name, pct):
    kind = GPU_PATHS[path_name][0]
    bs, m = geometry_of(pct)
    size = BLOCKS * CBS
    clean = as_bytes(dm.expected_words(size, 0, SALT, bs, m))
    bad = as_bytes(damaged_words(size, bs, m, ("first", "second")))
    blocks = range(VERIFY_FETCH_INTERVAL) if kind == "acc" else [3]
    want = window_model(bad, blocks, bs, m)
    if kind == "acc":
        assert (want["zero"], want["pattern"], want["bitflip"], want["other"], want["runs"]) == \
            (191, 512, 2, 1, 5), "the test's damage is not what it claims"
        assert (want["delta_min"], want["delta_max"]) == (4096, 4096)
        assert want["flip_or"] == (1 << 7) | (1 << 9)

    p, cfg = gpu_engine_cfg(tmp_path, path_name, size, pct)
    overwrite(p, bad)
    eng = core.Engine(cfg)
    eng.prepare()
    err = run_phase(core, eng, "READ")[0]["error"]
    on_gpu, first, rec = dc.parse_message(err)
    assert on_gpu and first == want["first"] and rec == dc.without_first(want), err
    assert err == ("Data verification failed (GPU). First bad file offset: %d; mismatching "
                   "8-byte words: %d" % (want["first"], want["nbad"])) + dm.message_suffix(want)

    # without the flag: today's message, byte for byte
    _, plain_cfg = gpu_engine_cfg(tmp_path, path_name, size, pct, diag=False)
    plain_eng = core.Engine(plain_cfg)
    plain_eng.prepare()
    plain_err = run_phase(core, plain_eng, "READ")[0]["error"]
    assert plain_err == ("Data verification failed (GPU). First bad file offset: %d; "
                         "mismatching 8-byte words: %d" % (want["first"], want["nbad"]))
    assert err.startswith(plain_err + "; diagnosis: ")

    # a failed diag READ, then a clean one on the same engine
    overwrite(p, clean)
    res = run_ok(core, eng, "READ")
    assert res[0]["bytes"] == size


@pytest.mark.parametrize("pct", [None, 50], ids=["plain", "pct50"])
@pytest.mark.parametrize("path_name", ["pipelined", "mmap"])
def test_engine_gpu_second_fetch_window(core, tmp_path, path_name, pct):
    """Damage in block 66 only: the fetch after 64 blocks is clean, the one at
    the end of the phase reports it."""
    bs, m = geometry_of(pct)
    size = BLOCKS * CBS
    bad = as_bytes(damaged_words(size, bs, m, ("second",)))
    want = window_model(bad, [66], bs, m)
    assert (want["nbad"], want["zero"], want["runs"]) == (2, 2, 1)
    p, cfg = gpu_engine_cfg(tmp_path, path_name, size, pct)
    overwrite(p, bad)
    eng = core.Engine(cfg)
    eng.prepare()
    err = run_phase(core, eng, "READ")[0]["error"]
    on_gpu, first, rec = dc.parse_message(err)
    assert on_gpu and first == want["first"] and rec == dc.without_first(want), err


@pytest.mark.parametrize("tail", [8, 4])
@pytest.mark.parametrize("path_name", ["pipelined", "mmap", "blockio"])
def test_engine_gpu_ragged_tail_and_stale_record(core, tmp_path, path_name, tail):
    """A last block of 8 or 4 bytes is checked on the CPU the moment it is
    reached. On the accumulating paths that is before the end-of-phase fetch,
    so the earlier block's record stays unfetched on the device when the phase
    fails; the next READ on the same engine must not report it."""
    kind = GPU_PATHS[path_name][0]
    blocks = 40
    size = blocks * CBS + tail
    clean = dm.expected_bytes(size, 0, SALT)
    bad = bytearray(clean)
    bad[blocks * CBS + 1] ^= 0x04
    early = (5 * W + 9) * 8
    bad[early:early + 8] = bytes(8)
    bad = bytes(bad)

    p, cfg = gpu_engine_cfg(tmp_path, path_name, size, None)
    overwrite(p, bad)
    eng = core.Engine(cfg)
    eng.prepare()
    err = run_phase(core, eng, "READ")[0]["error"]
    on_gpu, first, rec = dc.parse_message(err)
    if kind == "acc":
        want = dm.diagnose_bytes(bad[blocks * CBS:], blocks * CBS, SALT)
        assert not on_gpu and first == blocks * CBS + 1, err
        assert (want["bitflip"], want["other"]) == ((1, 0) if tail == 8 else (0, 1))
    else:
        want = dm.diagnose(bad[5 * CBS:6 * CBS], 5 * CBS, SALT)
        assert on_gpu and first == early and want["zero"] == 1, err
    assert rec == dc.without_first(want), err

    overwrite(p, clean)
    res = run_ok(core, eng, "READ")
    assert res[0]["bytes"] == size
