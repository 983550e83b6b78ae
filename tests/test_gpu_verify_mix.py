"""--verifymixpct on the GPU (real MI355X): ebFillChecksumMixKernel and
ebVerifyChecksumMixKernel through their host wrappers, and the engine's GPU
staging paths, all held to tests/verify_mix_model.py bit for bit.
"""

import os
import re

import numpy as np
import pytest

from tests import kernel_model as km
from tests import verify_mix_model as vm

pytestmark = pytest.mark.gpu

MIB = 1 << 20
SALT = 0x0123456789AB
SEED = 0x243F6A8885A308D3
SENTINEL = 0xA5
GUARD = 64
WG_BYTES = km.BLOCK * 16                          # one workgroup's worth of 16 B elements
GRID_WRAP = km.MAX_BLOCKS * km.BLOCK * 16 + 16    # first element of the second grid pass
URING_DEPTH = 4


@pytest.fixture(autouse=True)
def require_gpu(core):
    if core.gpu_device_count() < 1:
        pytest.fail("GPU test run but no HIP device available — the HIP path "
                    "must not silently fall back to CPU")


def m_edges(b):
    return [0, 8, b // 2 + 8, b - 8, b]  # b // 2 + 8 is 8 mod 16


def first_diff(got: bytes, want: bytes) -> str:
    g = np.frombuffer(got, dtype=np.uint8)
    w = np.frombuffer(want, dtype=np.uint8)
    diff = np.flatnonzero(g != w)
    word = int(diff[0]) // 8
    return (f"first difference at word {word}: got "
            f"{int.from_bytes(got[word * 8:word * 8 + 8], 'little'):#018x}, model "
            f"{int.from_bytes(want[word * 8:word * 8 + 8], 'little'):#018x}; "
            f"{diff.size} bytes differ")


def check_fill(core, n, file_off, b, m):
    out = core.gpu_fill_checksum_mix(n, GUARD, file_off, SALT, b, m, SENTINEL)
    what = f"len={n} file_off={file_off} B={b} M={m} phase={file_off % b}"
    assert len(out) == n + GUARD, what
    assert out[n:] == bytes([SENTINEL]) * GUARD, what + ": guard bytes behind len written"
    want = vm.pattern(n, file_off, SALT, b, m)
    if out[:n] != want:
        pytest.fail(what + ": " + first_diff(out[:n], want))


# ---------------------------------------------------------------------------
# fill, exact against the model
# ---------------------------------------------------------------------------

FILL_LENS = sorted({8, 16, 24, 4088, 4096, WG_BYTES - 16, WG_BYTES, WG_BYTES + 16})


# a launch never exceeds the block size (see the argument checks below)
@pytest.mark.parametrize("b,n", [(b, n) for b in (4096, MIB) for n in FILL_LENS if n <= b])
def test_fill_equals_model(core, b, n):
    for m in m_edges(b):
        phases = {0, 8}
        if n >= 16:  # phase + len > B: the wrap falls inside the range
            phases.add(b - n // 2 // 8 * 8)
            phases.add(b - 8)
        if 8 <= m < b:  # the boundary of M falls inside the range
            phases.add(m - 8)
        for phase in sorted(p for p in phases if 0 <= p < b):
            check_fill(core, n, 5 * b + phase, b, m)


def test_fill_large_file_offset(core):
    b = 4096
    for m in m_edges(b):
        check_fill(core, 4096, (1 << 45) + 3 * b + 2056, b, m)
        check_fill(core, 24, (1 << 64) - 24, b, m)  # the range ends at 2^64


def test_fill_pct0_equals_plain_kernel(core):
    n = WG_BYTES + 24
    assert core.gpu_fill_checksum_mix(n, 0, 4096, SALT, MIB, 0, SENTINEL) == \
        core.gpu_fill_checksum(n, 4096, SALT)


@pytest.fixture(scope="module")
def grid_wrap_model():
    b = GRID_WRAP
    m = b // 2
    assert m % 16 == 8 and b % 8 == 0
    return b, m, vm.pattern(GRID_WRAP, 0, SALT, b, m)


def test_fill_first_grid_stride_wrap(core, grid_wrap_model):
    b, m, want = grid_wrap_model
    out = core.gpu_fill_checksum_mix(GRID_WRAP, GUARD, 0, SALT, b, m, SENTINEL)
    assert out[GRID_WRAP:] == bytes([SENTINEL]) * GUARD
    if out[:GRID_WRAP] != want:
        pytest.fail("grid wrap: " + first_diff(out[:GRID_WRAP], want))


def test_verify_first_grid_stride_wrap(core, grid_wrap_model):
    b, m, want = grid_wrap_model
    assert core.gpu_verify_checksum_mix(want, 0, SALT, b, m) == (0, km.U64_MAX)
    bad = bytearray(want)
    for idx in (GRID_WRAP - 16, GRID_WRAP - 8):  # the element thread 0 takes on its 2nd pass
        bad[idx] ^= 0x01
    assert core.gpu_verify_checksum_mix(bytes(bad), 0, SALT, b, m) == (2, GRID_WRAP - 16)


# ---------------------------------------------------------------------------
# verify
# ---------------------------------------------------------------------------

VB = 16384
VM = 1032                    # 8 mod 16
VLEN = 2 * WG_BYTES + 8      # two workgroups and an odd tail word
VPHASE = VB - WG_BYTES - 8   # wrap at byte index 4104: inside one 16 B element
VOFF = 7 * VB + VPHASE


@pytest.mark.parametrize("b", [4096, MIB])
def test_verify_clean(core, b):
    for m in m_edges(b):
        for n, phase in ((8, 0), (24, 8), (4096, 0), (4096, b - 2056), (4088, 8)):
            off = 3 * b + phase
            data = vm.pattern(n, off, SALT, b, m)
            assert core.gpu_verify_checksum_mix(data, off, SALT, b, m) == (0, km.U64_MAX), \
                (b, m, n, phase)


FLIPS = {
    "word0": 0,
    "last_full_word": VLEN - 16,
    "odd_tail_word": VLEN - 8,
    "last_hashed_before_m": (VM - 8 - VPHASE) % VB,
    "first_plain_at_m": (VM - VPHASE) % VB,
    "last_word_before_wrap": VB - 8 - VPHASE,
    "first_word_after_wrap": VB - VPHASE,
    "lane63": 63 * 16,
    "lane64": 64 * 16 + 8,
    "workgroup_elem255": 255 * 16 + 8,
    "workgroup_elem256": 256 * 16,
}


@pytest.mark.parametrize("name", list(FLIPS))
def test_verify_single_flip(core, name):
    idx = FLIPS[name]
    assert idx % 8 == 0 and 0 <= idx < VLEN, "test states a position outside the buffer"
    clean = vm.pattern(VLEN, VOFF, SALT, VB, VM)
    assert core.gpu_verify_checksum_mix(clean, VOFF, SALT, VB, VM) == (0, km.U64_MAX)
    for bit in (0x01, 0x80):
        bad = bytearray(clean)
        bad[idx + (3 if bit == 0x80 else 0)] ^= bit
        assert vm.verify(bytes(bad), VOFF, SALT, VB, VM) == (1, VOFF + idx)
        assert core.gpu_verify_checksum_mix(bytes(bad), VOFF, SALT, VB, VM) == \
            (1, VOFF + idx), name


def test_verify_flip_either_side_of_m_without_wrap(core):
    off, n = 2 * VB, 4096
    clean = vm.pattern(n, off, SALT, VB, VM)
    for idx in (VM - 8, VM):
        bad = bytearray(clean)
        bad[idx + 7] ^= 0x10
        assert core.gpu_verify_checksum_mix(bytes(bad), off, SALT, VB, VM) == (1, off + idx)


def test_verify_wrong_m_fails_from_the_smaller_m(core):
    off, n = 2 * VB, 4096
    data = vm.pattern(n, off, SALT, VB, VM)
    want = vm.verify(data, off, SALT, VB, 2048)
    assert want[1] == off + VM and want[0] == (2048 - VM) // 8
    assert core.gpu_verify_checksum_mix(data, off, SALT, VB, 2048) == want


def test_verify_every_word_flipped(core):
    clean = vm.pattern(VLEN, VOFF, SALT, VB, VM)
    bad = bytes(x ^ 0xFF for x in clean)
    assert core.gpu_verify_checksum_mix(bad, VOFF, SALT, VB, VM) == (VLEN // 8, VOFF)


# ---------------------------------------------------------------------------
# batch and counters
# ---------------------------------------------------------------------------

def flipped(data: bytes, idxs) -> bytes:
    b = bytearray(data)
    for i in idxs:
        b[i] ^= 0x5A
    return bytes(b)


def batch_items():
    """(data, file_off, word indices flipped) with different phases; the
    lowest bad offset is in the fourth item, not the first."""
    out = []
    for k, (phase, n, flips) in enumerate([(0, 4096, []), (VB - 2056, 4096, [2048, 2056]),
                                           (8, 4088, [4080]), (VB - 8, 24, [0, 8, 16]),
                                           (1024, 4096, [])]):
        off = (9 - 2 * k) * VB + phase
        out.append((flipped(vm.pattern(n, off, SALT, VB, VM), flips), off, flips))
    return out


def test_batch_accumulates_without_fetch(core):
    items = batch_items()
    n_bad = sum(len(f) for _, _, f in items)
    first = min(off + min(f) for _, off, f in items if f)
    for data, off, f in items:  # the model agrees item by item
        assert vm.verify(data, off, SALT, VB, VM)[0] == len(f)
    res = core.gpu_verify_mix_batch([(d, o) for d, o, _ in items], SALT, VB, VM)
    assert res == [(n_bad, first), (0, km.U64_MAX)]


def test_batch_clean(core):
    items = [(vm.pattern(4096, k * VB + 8 * k, SALT, VB, VM), k * VB + 8 * k) for k in range(4)]
    assert core.gpu_verify_mix_batch(items, SALT, VB, VM) == [(0, km.U64_MAX)] * 2


def test_plain_launches_share_the_counters(core):
    items = batch_items()
    plain = [(flipped(km.checksum_pattern(4096, 64, SALT), [8, 4088]), 64),
             (km.checksum_pattern(4096, 3 * VB, SALT), 3 * VB),
             (flipped(km.checksum_pattern(24, 40, SALT), [16]), 40)]
    n_bad = sum(len(f) for _, _, f in items) + 3
    first = min(min(off + min(f) for _, off, f in items if f), 40 + 16)
    assert first == 56
    res = core.gpu_verify_mix_batch([(d, o) for d, o, _ in items], SALT, VB, VM, plain)
    assert res == [(n_bad, first), (0, km.U64_MAX)]
    # mix data is not plain data: the plain kernel counts the hashed words
    mixdata = vm.pattern(4096, 0, SALT, VB, VM)
    res = core.gpu_verify_mix_batch([(mixdata, 0)], SALT, VB, VM, [(mixdata, 0)])
    assert res == [(VM // 8, 0), (0, km.U64_MAX)]


# ---------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------

BAD_ARGS = {
    # (len, file_off, block_size, mix_len)
    "len_not_8": (20, 0, 4096, 8),
    "file_off_not_8": (16, 4, 4096, 8),
    "len_above_block": (4104, 0, 4096, 8),
    "block_not_8": (16, 0, 4100, 8),
    "block_zero": (16, 0, 0, 0),
    "mix_above_block": (16, 0, 4096, 4104),
    "mix_not_8": (16, 0, 4096, 12),
}


@pytest.mark.parametrize("name", list(BAD_ARGS))
def test_invalid_arguments(core, name):
    n, off, b, m = BAD_ARGS[name]
    with pytest.raises(ValueError):
        core.gpu_fill_checksum_mix(n, 0, off, SALT, b, m, SENTINEL)
    with pytest.raises(ValueError):
        core.gpu_verify_checksum_mix(b"\0" * n, off, SALT, b, m)
    with pytest.raises(ValueError):
        core.gpu_verify_mix_batch([(b"\0" * n, off)], SALT, b, m)


def test_bench_binding_runs(core):
    assert core.gpu_verify_mix_bench(MIB, 2, 0, MIB, MIB // 2) > 0
    with pytest.raises(ValueError):
        core.gpu_verify_mix_bench(MIB, 2, 0, MIB // 2, 0)  # len > block size


# ---------------------------------------------------------------------------
# engine on the GPU
# ---------------------------------------------------------------------------

BS = 4096
BLOCKS = 40
PCTS = [37, 100]
ERR_RE = re.compile(r"First bad file offset: (\d+)(?:; mismatching 8-byte words: (\d+))?")

ENGINE_PATHS = {
    "pipelined": dict(iodepth=1),
    "blockio": dict(flock_mode=1),
    "uring": dict(iodepth=URING_DEPTH),
    "mmap": dict(mmap=True),
}


def file_cfg(path, size, pct, threads=1, **kw):
    cfg = dict(paths=[str(path)], path_type="file", threads=threads,
               num_dataset_threads=threads, file_size=size, block_size=BS, bench_seed=SEED,
               verify_salt=SALT, verify_mix_pct=pct)
    cfg.update(kw)
    return cfg


def gpu_cfg(path, size, pct, threads=1, **kw):
    return file_cfg(path, size, pct, threads, gpu_ids=[0], **kw)


def dir_cfg(root, size, pct, threads, files, **kw):
    cfg = dict(paths=[str(root)], path_type="dir", threads=threads, num_dataset_threads=threads,
               dirs=1, files=files, file_size=size, block_size=BS, iodepth=URING_DEPTH,
               gpu_ids=[0], verify_salt=SALT, verify_mix_pct=pct, bench_seed=SEED)
    cfg.update(kw)
    return cfg


def run_phase(core, eng, name):
    eng.start_phase(core.PHASES[name])
    assert eng.wait_phase_done(60_000), f"{name} did not finish"
    return sorted(eng.finish_phase(), key=lambda r: r["rank"])


def run_ok(core, eng, name):
    res = run_phase(core, eng, name)
    errs = [r["error"] for r in res if r["error"]]
    assert not errs, (name, errs)
    return res


def model_file(size, pct):
    return vm.pattern(size, 0, SALT, BS, vm.mix_len(BS, pct))


def assert_file_is_model(data, size, pct, what):
    want = model_file(size, pct)
    assert len(data) == size, what
    if data != want:
        k = next(i for i in range(-(-size // BS))
                 if data[i * BS:(i + 1) * BS] != want[i * BS:(i + 1) * BS])
        pytest.fail(f"{what}: block {k}: "
                    + first_diff(data[k * BS:(k + 1) * BS], want[k * BS:(k + 1) * BS]))


@pytest.mark.parametrize("tail", [0, 8])
@pytest.mark.parametrize("pct", PCTS)
@pytest.mark.parametrize("path_name", list(ENGINE_PATHS))
def test_engine_write_equals_model_then_read_passes(core, tmp_path, path_name, pct, tail):
    size = BLOCKS * BS + tail
    p = tmp_path / "f"
    eng = core.Engine(gpu_cfg(p, size, pct, threads=2, **ENGINE_PATHS[path_name]))
    eng.prepare()
    res = run_ok(core, eng, "WRITE")
    assert sum(r["bytes"] for r in res) == size
    assert_file_is_model(p.read_bytes(), size, pct, f"{path_name} pct={pct} tail={tail}")
    res = run_ok(core, eng, "READ")
    assert sum(r["bytes"] for r in res) == size


@pytest.mark.parametrize("tail", [0, 8])
@pytest.mark.parametrize("pct", PCTS)
def test_engine_dir_mode_write_equals_model_then_read_passes(core, tmp_path, pct, tail):
    size = 10 * BS + tail
    eng = core.Engine(dir_cfg(tmp_path, size, pct, 2, 2))
    eng.prepare()
    run_ok(core, eng, "MKDIRS")
    res = run_ok(core, eng, "WRITE")
    assert [r["bytes"] for r in res] == [2 * size, 2 * size]
    for r in range(2):
        for f in range(2):
            got = (tmp_path / f"r{r}" / "d0" / f"r{r}-f{f}").read_bytes()
            assert_file_is_model(got, size, pct, f"dir pct={pct} tail={tail} worker {r} file {f}")
    res = run_ok(core, eng, "READ")
    assert [r["bytes"] for r in res] == [2 * size, 2 * size]


def test_engine_pct0_writes_the_plain_pattern(core, tmp_path):
    size = BLOCKS * BS + 8
    p = tmp_path / "f"
    eng = core.Engine(gpu_cfg(p, size, 0))
    eng.prepare()
    run_ok(core, eng, "WRITE")
    assert p.read_bytes() == km.checksum_pattern(size, 0, SALT)
    cfg = gpu_cfg(p, size, 0)
    del cfg["verify_mix_pct"]
    eng = core.Engine(cfg)
    eng.prepare()
    run_ok(core, eng, "READ")


M37 = vm.mix_len(BS, 37)
CORRUPT = {
    # byte offset of the corrupted word in a 40-block file written with pct 37
    "hashed": 17 * BS + 64,
    "plain": 23 * BS + M37 + 1024,
    "last_hashed": 5 * BS + M37 - 8,
    "first_plain": 31 * BS + M37,
}


@pytest.mark.parametrize("where", list(CORRUPT))
@pytest.mark.parametrize("path_name", list(ENGINE_PATHS) + ["dir"])
def test_engine_reports_a_corrupted_word_exactly(core, tmp_path, path_name, where):
    size = BLOCKS * BS
    pos = CORRUPT[where]
    assert (pos % BS < M37) == (where in ("hashed", "last_hashed"))
    if path_name == "dir":
        p = tmp_path / "r0" / "d0" / "r0-f0"
        os.makedirs(p.parent)
        cfg = dir_cfg(tmp_path, size, 37, 1, 1)
    else:
        p = tmp_path / "f"
        cfg = gpu_cfg(p, size, 37, **ENGINE_PATHS[path_name])
    weng = core.Engine(file_cfg(p, size, 37))  # written on the CPU path
    weng.prepare()
    run_ok(core, weng, "WRITE")
    del weng
    clean = p.read_bytes()
    assert clean == model_file(size, 37)
    bad = bytearray(clean)
    bad[pos + 2] ^= 0x04
    p.write_bytes(bytes(bad))
    assert vm.verify(bytes(bad), 0, SALT, BS, M37) == (1, pos)

    eng = core.Engine(cfg)
    eng.prepare()
    err = run_phase(core, eng, "READ")[0]["error"]
    m = ERR_RE.search(err)
    assert m and "verification failed" in err, err
    assert (int(m.group(1)), int(m.group(2)) if m.group(2) else None) == (pos, 1), err

    # same engine, repaired file: the reused context's counters were reset
    p.write_bytes(clean)
    res = run_ok(core, eng, "READ")
    assert res[0]["bytes"] == size


@pytest.mark.parametrize("path_name", list(ENGINE_PATHS))
def test_engine_read_with_another_pct_fails_from_the_smaller_m(core, tmp_path, path_name):
    size = BLOCKS * BS
    p = tmp_path / "f"
    weng = core.Engine(file_cfg(p, size, 100))
    weng.prepare()
    run_ok(core, weng, "WRITE")
    del weng
    eng = core.Engine(gpu_cfg(p, size, 37, **ENGINE_PATHS[path_name]))
    eng.prepare()
    err = run_phase(core, eng, "READ")[0]["error"]
    m = ERR_RE.search(err)
    assert m and "verification failed" in err, err
    assert int(m.group(1)) == M37, err  # block 0, the first word whose kind differs
