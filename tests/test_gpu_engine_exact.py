"""Exact end-to-end tests of the engine's GPU staging paths (real MI355X).

test_gpu_kernels.py holds the fill / verify kernels to tests/kernel_model.py
through their host wrappers. This module holds the engine's *use* of those
wrappers (slot rings, per-slot events, half-ring batched copies, the write
lookahead, mmap zero-copy, io_uring) to the same model, byte for byte:

A. write side - every byte a GPU-staged WRITE leaves in the file equals the
   model (checksum pattern, block-variance refill by fill counter, or the
   cycling pre-filled slot ring when nothing refills);
B. read side - after a verify-off READ (the configuration that selects the
   batched copies) every device slot, taken with Engine.gpu_slots(), holds one
   whole block of the worker's slice, and for sequential reads the resident
   blocks are exactly the last ones read;
C. verify failures - the offset and word count in the engine's error text
   equal what kernel_model.verify says about the bytes the check that fires
   first has seen, and the next READ on the same engine is clean again.

Path selection is by config only, plus EB_GPU_URING_BATCH (read at call time).
io_uring cases set EB_DEBUG_PATH and assert the path from stderr.
"""

import collections
import functools
import os
import re

import numpy as np
import pytest

from tests import kernel_model as km

pytestmark = pytest.mark.gpu

MASK = km.MASK
SEED = 0x243F6A8885A308D3
RANK_MULT = 0xD1B54A32D192ED03  # per-worker seed: bench_seed ^ (RANK_MULT * (rank + 1))
SALT = 0x0123456789AB
BATCH_BYTES = 1 << 20           # half-ring size of the batched read staging
PIPELINE_MIN_BS = 256 << 10     # from here on reads stage per block, not per half-ring
VERIFY_FETCH_INTERVAL = 64      # GPU-checked blocks per verify-counter fetch
URING_DEPTH = 4


@pytest.fixture(autouse=True)
def require_gpu(core):
    if core.gpu_device_count() < 1:
        pytest.fail("GPU test run but no HIP device available — the HIP path "
                    "must not silently fall back to CPU")


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------

Slice = collections.namedtuple("Slice", "first_block num_blocks start nbytes")


def fair_share(size: int, bs: int, threads: int) -> list:
    """The sequential fair-share rule, stated once: the file's ceil(size/bs)
    blocks are dealt out as floor(blocks/threads) contiguous blocks per
    worker, the last worker also takes the remainder (and so the short tail
    block)."""
    nblocks = -(-size // bs)
    per = nblocks // threads
    out = []
    for r in range(threads):
        first = r * per
        cnt = per if r < threads - 1 else nblocks - first
        end = min(size, (first + cnt) * bs)
        out.append(Slice(first, cnt, first * bs, max(end - first * bs, 0)))
    return out


def random_share(size: int, bs: int, threads: int) -> list:
    """Random-order rule: whole blocks only (floor), an equal contiguous range
    per worker, as many ops as the range has blocks."""
    per = (size // bs) // threads
    return [Slice(r * per, per, r * per * bs, per * bs) for r in range(threads)]


def file_cfg(path, size, bs, threads=1, **kw):
    cfg = dict(paths=[str(path)], path_type="file", threads=threads,
               num_dataset_threads=threads, file_size=size, block_size=bs,
               bench_seed=SEED)
    cfg.update(kw)
    return cfg


def gpu_cfg(path, size, bs, threads=1, **kw):
    return file_cfg(path, size, bs, threads, gpu_ids=[0], **kw)


def run_phase(core, eng, name):
    eng.start_phase(core.PHASES[name])
    assert eng.wait_phase_done(60_000), f"{name} did not finish"
    return sorted(eng.finish_phase(), key=lambda r: r["rank"])


def run_ok(core, eng, name):
    res = run_phase(core, eng, name)
    errs = [r["error"] for r in res if r["error"]]
    assert not errs, (name, errs)
    return res


def assert_shares(res, shares, what):
    """Cross-check the slice rule against what each worker reports."""
    assert len(res) == len(shares)
    for r, (got, want) in enumerate(zip(res, shares)):
        assert (got["bytes"], got["iops"]) == (want.nbytes, want.num_blocks), (
            f"{what}: worker {r} reports bytes={got['bytes']} iops={got['iops']}, "
            f"its slice is {want}")


@functools.lru_cache(maxsize=None)
def pattern_bytes(size: int, salt: int) -> bytes:
    """The checksum pattern of a whole file (a sub-word tail is the leading
    bytes of its word)."""
    return km.checksum_pattern((size + 7) // 8 * 8, 0, salt)[:size]


def write_pattern_file(core, path, size, salt=SALT):
    """Write `path` on the CPU path with verify_salt; the result is the model
    pattern, so every 8-byte word names its own file offset."""
    eng = core.Engine(file_cfg(path, size, 1 << 20, verify_salt=salt))
    eng.prepare()
    run_ok(core, eng, "WRITE")
    del eng
    with open(path, "rb") as f:
        assert f.read() == pattern_bytes(size, salt)


def uring_paths(capfd):
    """(gpu, batchedRead, batch, depth) of every '[eb] uring path' line on
    stderr since the last call."""
    err = capfd.readouterr().err
    return [tuple(int(x) for x in m) for m in re.findall(
        r"\[eb\] uring path: gpu=(\d+) batchedRead=(\d+) batch=(\d+) depth=(\d+)", err)]


def first_diff_report(got: bytes, want: bytes) -> str:
    n = min(len(got), len(want))
    g = np.frombuffer(got, dtype=np.uint8, count=n)
    w = np.frombuffer(want, dtype=np.uint8, count=n)
    diff = np.flatnonzero(g != w)
    b = int(diff[0])
    word = b // 8
    gw = int.from_bytes(got[word * 8:word * 8 + 8], "little")
    ww = int.from_bytes(want[word * 8:word * 8 + 8], "little")
    return (f"first difference at word {word} (block byte {b}): got {gw:#018x}, "
            f"model {ww:#018x}; {diff.size} of {n} bytes differ")


# ---------------------------------------------------------------------------
# A. write side: file bytes equal the model
# ---------------------------------------------------------------------------

# name -> (config that selects the path, slot that block k of a worker goes
# through, given (k, num_slots)); the slot is what a failure message names and
# what the pct-0 case compares against
WRITE_PATHS = {
    # iodepth 1: fill + D2H of block i+1 run while block i is pwritten
    "pipelined": (dict(iodepth=1), lambda k, n: k % n),
    # flock / ops log force the plain per-block path, which only uses slot 0
    "blockio_flock": (dict(flock_mode=1), lambda k, n: 0),
    "blockio_opslog": (dict(ops_log=True), lambda k, n: 0),
    # io_uring per slot: with in-order completions block k reuses slot k % depth
    "uring": (dict(iodepth=URING_DEPTH), lambda k, n: k % URING_DEPTH),
    # mmap zero-copy: D2H straight into the mapped file pages
    "mmap": (dict(mmap=True), lambda k, n: k % n),
}


def model_block(fill, rank, k, length):
    """Bytes of block k (0-based within the worker's slice) of worker `rank`,
    or None where the model does not state them (CPU refill of a block whose
    length is no multiple of 16)."""
    kind = fill[0]
    if kind == "blockvar":
        _, pct, algo = fill
        if length % 16:
            return None
        seed = SEED ^ ((RANK_MULT * (rank + 1)) & MASK)
        return km.blockvar_words(length, length * pct // 100, seed, k + 1,
                                 algo == "fast").astype("<u8").tobytes()
    raise AssertionError(fill)


def run_write_case(core, tmp_path, capfd, monkeypatch, path_name, fill, bs, size, threads):
    path_cfg, slot_of = WRITE_PATHS[path_name]
    path_cfg = dict(path_cfg)
    if path_cfg.get("ops_log"):
        path_cfg["ops_log"] = str(tmp_path / "ops.log")
    if fill[0] == "checksum":
        path_cfg["verify_salt"] = fill[1]
    elif fill[0] == "blockvar":
        path_cfg.update(blockvar_pct=fill[1], blockvar_algo=fill[2])
    else:  # "ring": nothing refills, verify off
        path_cfg.update(blockvar_pct=0)
    if path_name == "uring":
        monkeypatch.setenv("EB_DEBUG_PATH", "1")
        capfd.readouterr()

    p = tmp_path / "f"
    eng = core.Engine(gpu_cfg(p, size, bs, threads, **path_cfg))  # fresh: fill counter at 1
    eng.prepare()
    res = run_ok(core, eng, "WRITE")
    what = f"{path_name} {fill} bs={bs} size={size} threads={threads}"

    if path_name == "uring":
        seen = uring_paths(capfd)
        assert seen and all(s[0] == 1 and s[1] == 0 and s[3] == URING_DEPTH for s in seen), seen

    shares = fair_share(size, bs, threads)
    assert_shares(res, shares, what)
    data = p.read_bytes()
    assert len(data) == size, what

    if fill[0] == "checksum":
        want = pattern_bytes(size, fill[1])
        if data != want:  # every byte of the file, then name the place
            for r, sh in enumerate(shares):
                num_slots = eng.gpu_slots(r)[0]
                for k in range(sh.num_blocks):
                    o = sh.start + k * bs
                    if data[o:o + bs] != want[o:o + bs]:
                        pytest.fail(f"{what}: worker {r}, block {k} (file offset {o}, slot "
                                    f"{slot_of(k, num_slots)}): "
                                    + first_diff_report(data[o:o + bs], want[o:o + bs]))
        return eng

    for r, sh in enumerate(shares):
        num_slots, stride, raw = eng.gpu_slots(r)
        assert stride == (bs + 4095) // 4096 * 4096 and len(raw) == num_slots * stride
        for k in range(sh.num_blocks):
            o = sh.start + k * bs
            got = data[o:min(o + bs, size)]
            slot = slot_of(k, num_slots)
            if fill[0] == "ring":
                # the pre-filled slot ring cycles: block k is block k mod
                # num_slots again, and is what its device slot still holds
                prev = sh.start + (k % num_slots) * bs
                if got != data[prev:prev + len(got)]:
                    pytest.fail(f"{what}: worker {r}, block {k} (slot {slot}) differs from "
                                f"block {k % num_slots}: "
                                + first_diff_report(got, data[prev:prev + len(got)]))
                want = raw[slot * stride:slot * stride + len(got)]
            else:
                want = model_block(fill, r, k, len(got))
                if want is None:
                    continue
            if got != want:
                pytest.fail(f"{what}: worker {r}, block {k} (file offset {o}, slot {slot}, "
                            f"fill call {k + 1}): " + first_diff_report(got, want))
        if fill[0] == "ring":  # distinct slots were pre-filled with distinct data
            n = min(sh.num_blocks, num_slots if path_name in ("pipelined", "mmap") else
                    1 if path_name.startswith("blockio") else URING_DEPTH)
            heads = {data[sh.start + k * bs:sh.start + k * bs + 64] for k in range(n)}
            assert len(heads) == n, f"{what}: worker {r}: pre-filled slots repeat"
    return eng


FILE_WRITE_PATHS = ["pipelined", "blockio_flock", "uring", "mmap"]
FILLS = [("checksum", SALT), ("blockvar", 100, "fast"), ("blockvar", 100, "strong"),
         ("blockvar", 37, "fast"), ("blockvar", 37, "strong"), ("ring",)]
FILL_IDS = ["checksum", "bv100fast", "bv100strong", "bv37fast", "bv37strong", "bv0ring"]


# ~40 blocks per worker: more than any slot count at 64 KiB blocks, so every
# ring wraps; at 4 KiB the small-block ring has 512 slots and the depth-4 and
# one-slot paths still wrap
@pytest.mark.parametrize("bs,threads", [(4096, 1), (65536, 2)])
@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("path_name", FILE_WRITE_PATHS)
def test_write_file_bytes_equal_model(core, tmp_path, capfd, monkeypatch, path_name, fill,
                                      bs, threads):
    blocks = 41 if threads == 1 else 40
    run_write_case(core, tmp_path, capfd, monkeypatch, path_name, fill, bs,
                   blocks * bs * threads, threads)


@pytest.mark.parametrize("fill", [FILLS[0], FILLS[2], FILLS[5]],
                         ids=[FILL_IDS[0], FILL_IDS[2], FILL_IDS[5]])
def test_write_pipelined_1m_blocks(core, tmp_path, capfd, monkeypatch, fill):
    """1 MiB blocks run on a two-slot ring: five blocks wrap it twice."""
    run_write_case(core, tmp_path, capfd, monkeypatch, "pipelined", fill, 1 << 20, 5 << 20, 1)


@pytest.mark.parametrize("fill", [FILLS[0], FILLS[1]], ids=[FILL_IDS[0], FILL_IDS[1]])
def test_write_blockio_opslog(core, tmp_path, capfd, monkeypatch, fill):
    run_write_case(core, tmp_path, capfd, monkeypatch, "blockio_opslog", fill, 65536,
                   40 * 65536, 1)


# ragged files, two workers (the tail is the last block of worker 1, reached
# with the GPU pipeline in flight): +8 is a GPU checksum fill of a
# len % 16 == 8 block, +4 falls back to the CPU checksum fill, +16 is one
# full 16 B store; block-variance tails of +8 / +4 are refilled on the CPU
# (not modelled: only the blocks before them and the file size are checked)
@pytest.mark.parametrize("fill,tail", [
    (FILLS[0], 8), (FILLS[0], 4), (FILLS[0], 16), (FILLS[1], 16), (FILLS[4], 8), (FILLS[4], 4),
], ids=["checksum+8", "checksum+4", "checksum+16", "bv100fast+16", "bv37strong+8",
        "bv37strong+4"])
@pytest.mark.parametrize("path_name", FILE_WRITE_PATHS)
def test_write_ragged_tail(core, tmp_path, capfd, monkeypatch, path_name, fill, tail):
    bs = 65536
    run_write_case(core, tmp_path, capfd, monkeypatch, path_name, fill, bs, 79 * bs + tail, 2)


@pytest.mark.parametrize("tail", [0, 8, 4])
def test_write_dir_mode_iodepth_checksum(core, tmp_path, tail):
    """Directory mode with iodepth: every file of every worker is the whole
    checksum pattern."""
    bs, size = 65536, 10 * 65536 + tail
    cfg = dict(paths=[str(tmp_path)], path_type="dir", threads=2, num_dataset_threads=2,
               dirs=1, files=2, file_size=size, block_size=bs, iodepth=URING_DEPTH,
               gpu_ids=[0], verify_salt=SALT, bench_seed=SEED)
    eng = core.Engine(cfg)
    eng.prepare()
    run_ok(core, eng, "MKDIRS")
    res = run_ok(core, eng, "WRITE")
    assert [r["bytes"] for r in res] == [2 * size, 2 * size]
    want = pattern_bytes(size, SALT)
    for r in range(2):
        for f in range(2):
            got = (tmp_path / f"r{r}" / "d0" / f"r{r}-f{f}").read_bytes()
            assert len(got) == size
            if got != want:
                k = next(i for i in range(-(-size // bs))
                         if got[i * bs:(i + 1) * bs] != want[i * bs:(i + 1) * bs])
                pytest.fail(f"dir mode tail={tail}: worker {r}, file {f}, block {k}: "
                            + first_diff_report(got[k * bs:(k + 1) * bs],
                                                want[k * bs:(k + 1) * bs]))


# ---------------------------------------------------------------------------
# the snapshot hook itself
# ---------------------------------------------------------------------------

def test_gpu_slots_hook_contract(core, tmp_path):
    bs, size = 65536, 8 * 65536
    p = tmp_path / "f"
    eng = core.Engine(gpu_cfg(p, size, bs, 2, verify_salt=SALT))
    eng.prepare()
    eng.start_phase(core.PHASES["WRITE"])
    with pytest.raises(RuntimeError, match="phase is running"):
        eng.gpu_slots(0)  # refuses, does not block, even if the workers are done
    assert eng.wait_phase_done(60_000)
    with pytest.raises(RuntimeError, match="phase is running"):
        eng.gpu_slots(0)
    assert not [r["error"] for r in eng.finish_phase() if r["error"]]

    for r in range(2):
        num_slots, stride, raw = eng.gpu_slots(r)
        assert num_slots == 2 * (BATCH_BYTES // bs) and stride == bs
        assert len(raw) == num_slots * stride
        assert eng.gpu_slots(r) == (num_slots, stride, raw)  # read-only
        # worker r filled its four blocks into slots 0..3
        sh = fair_share(size, bs, 2)[r]
        for k in range(sh.num_blocks):
            assert raw[k * stride:k * stride + bs] == km.checksum_pattern(
                bs, sh.start + k * bs, SALT), (r, k)
    with pytest.raises(RuntimeError, match="no GPU context"):
        eng.gpu_slots(2)
    # the engine goes on undisturbed: the READ verifies what was written
    res = run_ok(core, eng, "READ")
    assert sum(r["bytes"] for r in res) == size


# ---------------------------------------------------------------------------
# B. read side: the slots hold the right blocks
# ---------------------------------------------------------------------------

def looks_like_pattern(words) -> bool:
    """Consecutive words that each name the next file offset."""
    w = words[:8].astype(np.uint64)
    return bool(np.all(w[1:] - w[:-1] == np.uint64(8)))


def check_read_slots(snapshot, what, rank, bs, share, file_size, in_use, sequential):
    """The device slots of one worker after a verify-off READ of a pattern
    file. The ring is not re-implemented: each slot's first word is decoded
    to the file offset it claims, and the slot must then hold that whole
    block."""
    num_slots, stride, raw = snapshot
    assert stride == (bs + 4095) // 4096 * 4096, what
    assert len(raw) == num_slots * stride, what
    assert in_use <= num_slots, what
    end = min(share.start + share.num_blocks * bs, file_size)
    live = min(share.num_blocks, in_use)  # slots that can have received a block
    resident = []
    for s in range(num_slots):
        words = np.frombuffer(raw, dtype="<u8", count=bs // 8, offset=s * stride)
        if s >= live:
            assert not looks_like_pattern(words), (
                f"{what}: worker {rank}: slot {s} lies beyond the {live} slots that can "
                f"have received a block but holds pattern data (first word names offset "
                f"{(int(words[0]) - SALT) & MASK})")
            continue
        off = (int(words[0]) - SALT) & MASK
        if off % bs or not share.start <= off < end:
            pytest.fail(f"{what}: worker {rank}: slot {s} starts with {int(words[0]):#x}, "
                        f"which names file offset {off}: not a block start inside the "
                        f"worker's slice [{share.start}, {end})")
        blen = min(bs, end - off)  # a short last block is checked to its own length
        want = km.checksum_words(blen, off, SALT)
        got = words[:blen // 8]
        if not np.array_equal(got, want):
            i = int(np.flatnonzero(got != want)[0])
            pytest.fail(f"{what}: worker {rank}: slot {s} holds block {off // bs} (file "
                        f"offset {off}, {blen} bytes) up to word {i}, where it has "
                        f"{int(got[i]):#018x} instead of {int(want[i]):#018x}; "
                        f"{int(np.count_nonzero(got != want))} of {got.size} words differ")
        resident.append(off // bs)
    if sequential:
        last = share.first_block + share.num_blocks
        assert sorted(resident) == list(range(last - live, last)), (
            f"{what}: worker {rank}: the {live} live slots must hold the last {live} blocks "
            f"of the slice [{last - live}, {last}), each once; they hold {sorted(resident)}")


def run_read_case(core, tmp_path, what, bs, size, threads, in_use, random=False, **path_cfg):
    """in_use(num_slots) -> number of slots the path under test cycles through."""
    p = tmp_path / "f"
    write_pattern_file(core, p, size)
    eng = core.Engine(gpu_cfg(p, size, bs, threads, random=random, **path_cfg))  # verify off
    eng.prepare()
    res = run_ok(core, eng, "READ")
    shares = (random_share if random else fair_share)(size, bs, threads)
    assert_shares(res, shares, what)
    for r, sh in enumerate(shares):
        snap = eng.gpu_slots(r)
        check_read_slots(snap, what, r, bs, sh, size, in_use(snap[0]), not random)
    return eng


def batch_of(bs):
    return BATCH_BYTES // bs


def sync_batched_in_use(bs):
    def in_use(num_slots):
        assert bs < PIPELINE_MIN_BS
        assert num_slots == 2 * batch_of(bs)  # ring = two half-ring batches
        return num_slots
    return in_use


B4K = batch_of(4096)
B6K = batch_of(6000)


# sync half-ring batched path (iodepth 1, verify off, small blocks): block
# counts per worker around one batch, one ring and past it, two workers
@pytest.mark.parametrize("blocks", [B4K - 1, B4K, B4K + 1, 2 * B4K, 2 * B4K + 1, 3 * B4K + 5])
def test_read_sync_batched_4k(core, tmp_path, blocks):
    bs = 4096
    run_read_case(core, tmp_path, f"sync batched bs={bs} blocks/worker={blocks}", bs,
                  2 * blocks * bs, 2, sync_batched_in_use(bs))


def test_read_sync_batched_4k_one_worker(core, tmp_path):
    bs, blocks = 4096, 3 * B4K + 5
    run_read_case(core, tmp_path, f"sync batched bs={bs} 1 worker", bs, blocks * bs, 1,
                  sync_batched_in_use(bs))


def test_read_sync_batched_stride_not_block_size(core, tmp_path):
    """block_size 6000: slots are 8192 apart, so a ranged copy also carries
    the padding between blocks."""
    bs, blocks = 6000, 3 * B6K + 5
    run_read_case(core, tmp_path, f"sync batched bs={bs}", bs, 2 * blocks * bs, 2,
                  sync_batched_in_use(bs))


def test_read_sync_batched_short_last_block(core, tmp_path):
    bs, blocks = 4096, 2 * B4K + 7
    run_read_case(core, tmp_path, "sync batched, short last block", bs,
                  2 * blocks * bs - bs + 2048, 2, sync_batched_in_use(bs))


def test_read_sync_batched_random(core, tmp_path):
    bs, blocks = 4096, 3 * B4K + 5
    run_read_case(core, tmp_path, "sync batched, random order", bs, 2 * blocks * bs, 2,
                  sync_batched_in_use(bs), random=True)


@pytest.mark.parametrize("size_blocks,tail", [(10, 0), (9, 8192)])
def test_read_pipelined_per_block(core, tmp_path, size_blocks, tail):
    """block_size >= 256 KiB: per-block copies on a two-slot ring."""
    bs = PIPELINE_MIN_BS

    def in_use(num_slots):
        assert num_slots == 2
        return num_slots
    run_read_case(core, tmp_path, f"per-block pipelined tail={tail}", bs,
                  size_blocks * bs + tail, 2, in_use)


@pytest.mark.parametrize("path_cfg", [dict(flock_mode=1), dict(ops_log=True)],
                         ids=["flock", "opslog"])
def test_read_plain_blockio(core, tmp_path, path_cfg):
    """Plain per-block path: every block goes through slot 0."""
    if path_cfg.get("ops_log"):
        path_cfg = dict(ops_log=str(tmp_path / "ops.log"))
    bs = 4096
    run_read_case(core, tmp_path, f"plain blockIO {path_cfg}", bs, 2 * 40 * bs + 2048, 2,
                  lambda num_slots: 1, **path_cfg)


@pytest.mark.parametrize("bs,tail", [(4096, 0), (4096, 2048), (PIPELINE_MIN_BS, 0)])
def test_read_uring_per_slot(core, tmp_path, capfd, monkeypatch, bs, tail):
    monkeypatch.setenv("EB_DEBUG_PATH", "1")
    monkeypatch.delenv("EB_GPU_URING_BATCH", raising=False)
    blocks = 40 if bs == 4096 else 6
    capfd.readouterr()
    run_read_case(core, tmp_path, f"io_uring per slot bs={bs} tail={tail}", bs,
                  2 * blocks * bs + tail, 2, lambda num_slots: URING_DEPTH,
                  iodepth=URING_DEPTH)
    seen = uring_paths(capfd)
    assert len(seen) == 2 and all(s[:2] == (1, 0) and s[3] == URING_DEPTH for s in seen), seen


def uring_batched_case(core, tmp_path, capfd, monkeypatch, depth, blocks, random=False):
    bs = 4096
    half = min(depth // 2, 64)
    monkeypatch.setenv("EB_DEBUG_PATH", "1")
    monkeypatch.setenv("EB_GPU_URING_BATCH", "1")
    capfd.readouterr()
    run_read_case(core, tmp_path,
                  f"io_uring half-ring batched depth={depth} blocks/worker={blocks}", bs,
                  2 * blocks * bs, 2, lambda num_slots: 2 * half, random=random,
                  iodepth=depth)
    seen = uring_paths(capfd)
    assert seen == [(1, 1, batch_of(bs), depth)] * 2, seen


# fewer blocks than one half, exactly two halves, two halves plus 3
@pytest.mark.parametrize("depth,blocks", [(8, 3), (8, 8), (8, 11), (16, 5), (16, 16), (16, 19),
                                          (16, 40)])
def test_read_uring_batched(core, tmp_path, capfd, monkeypatch, depth, blocks):
    uring_batched_case(core, tmp_path, capfd, monkeypatch, depth, blocks)


def test_read_uring_batched_random(core, tmp_path, capfd, monkeypatch):
    uring_batched_case(core, tmp_path, capfd, monkeypatch, 16, 40, random=True)


@pytest.mark.parametrize("tail", [0, 4096])
def test_read_mmap_zero_copy(core, tmp_path, tail):
    bs = 65536
    run_read_case(core, tmp_path, f"mmap zero-copy tail={tail}", bs, 2 * 40 * bs + tail, 2,
                  lambda num_slots: num_slots, mmap=True)


# ---------------------------------------------------------------------------
# C. verify failures are reported exactly
# ---------------------------------------------------------------------------

ERR_RE = re.compile(r"First bad file offset: (\d+)(?:; mismatching 8-byte words: (\d+))?")
CBS = 4096
W = CBS // 8  # words per block

# Which check sees what (from engine.cpp):
#  "acc" - the pipelined per-block read and the mmap read launch one verify
#          kernel per block into counters that are fetched after every 64
#          GPU-checked blocks and at the end of the phase: one report covers
#          the whole fetch window;
#  "blk" - plain blockIO, io_uring (file and directory mode) verify each block
#          synchronously as it completes: one report covers one block.
# A block whose length is no multiple of 16 is checked on the CPU the moment
# it is reached; that report carries the first bad byte offset and no count.
VERIFY_PATHS = {
    "pipelined": ("acc", dict(iodepth=1)),
    "mmap": ("acc", dict(mmap=True)),
    "blockio": ("blk", dict(flock_mode=1)),
    "uring": ("blk", dict(iodepth=URING_DEPTH)),
    "dir": ("blk", None),
}

Case = collections.namedtuple("Case", "blocks tail corrupt acc blk")
TAIL = 40 * CBS  # offset of the ragged tail block of a 40-block file
EARLY = (5 * W + 9) * 8
VERIFY_CASES = {
    # (byte offset, length) corrupted; want = (first bad offset, word count)
    "first_and_last_word": Case(40, 0, [(0, 8), (40 * CBS - 8, 8)], (0, 2), (0, 1)),
    "adjacent_across_block_boundary": Case(
        40, 0, [(4 * CBS - 8, 8), (4 * CBS, 8)], (4 * CBS - 8, 2), (4 * CBS - 8, 1)),
    # the higher block is listed (and corrupted) first: the lower offset wins
    "two_blocks": Case(40, 0, [((30 * W + 17) * 8, 8), ((7 * W + 5) * 8, 8)],
                       ((7 * W + 5) * 8, 2), ((7 * W + 5) * 8, 1)),
    # 70 blocks, the only bad word in block 66: found by the second fetch
    "second_fetch_window": Case(70, 0, [((66 * W + 3) * 8, 8)],
                                ((66 * W + 3) * 8, 1), ((66 * W + 3) * 8, 1)),
    # ragged tails are checked on the CPU
    "tail8": Case(40, 8, [(TAIL, 8)], (TAIL, None), (TAIL, None)),
    "tail4": Case(40, 4, [(TAIL, 4)], (TAIL, None), (TAIL, None)),
    # tail and an earlier GPU-checked block: with fewer than 64 blocks the
    # accumulating paths reach the tail's CPU check before their end-of-phase
    # fetch, so the tail is what they report; the per-block paths stop at the
    # earlier block
    "tail8_and_earlier": Case(40, 8, [(TAIL, 8), (EARLY, 8)], (TAIL, None), (EARLY, 1)),
    "tail4_and_earlier": Case(40, 4, [(TAIL, 4), (EARLY, 8)], (TAIL, None), (EARLY, 1)),
}


@pytest.mark.parametrize("case_name", list(VERIFY_CASES))
@pytest.mark.parametrize("path_name", list(VERIFY_PATHS))
def test_verify_failure_reported_exactly(core, tmp_path, capfd, monkeypatch, path_name,
                                         case_name):
    kind, path_cfg = VERIFY_PATHS[path_name]
    case = VERIFY_CASES[case_name]
    size = case.blocks * CBS + case.tail
    want = case.acc if kind == "acc" else case.blk

    if path_name == "dir":
        p = tmp_path / "r0" / "d0" / "r0-f0"
        os.makedirs(p.parent)
        cfg = dict(paths=[str(tmp_path)], path_type="dir", threads=1, num_dataset_threads=1,
                   dirs=1, files=1, file_size=size, block_size=CBS, iodepth=URING_DEPTH,
                   gpu_ids=[0], verify_salt=SALT, bench_seed=SEED)
    else:
        p = tmp_path / "f"
        cfg = gpu_cfg(p, size, CBS, 1, verify_salt=SALT, **path_cfg)
    write_pattern_file(core, p, size)
    clean = pattern_bytes(size, SALT)
    bad = bytearray(clean)
    for off, ln in case.corrupt:
        for i in range(off, off + ln):
            bad[i] ^= 0xA5
    with open(p, "r+b") as f:
        f.write(bad)

    # the oracle: kernel_model.verify over the bytes that the check which
    # fires first has seen
    first = min(off for off, _ in case.corrupt)
    if want[1] is not None:
        if kind == "acc":
            win = VERIFY_FETCH_INTERVAL * CBS
            lo, hi = first // win * win, min((first // win + 1) * win, case.blocks * CBS)
        else:
            lo, hi = first // CBS * CBS, first // CBS * CBS + CBS
        n_bad, first_bad = km.verify(bytes(bad[lo:hi]), lo, SALT)
        assert (first_bad, n_bad) == want, "test case states the wrong expectation"
        if kind == "acc" and case.blocks < VERIFY_FETCH_INTERVAL and not case.tail:
            assert km.verify(bytes(bad), 0, SALT) == (n_bad, first_bad)

    if path_name == "uring":
        monkeypatch.setenv("EB_DEBUG_PATH", "1")
        capfd.readouterr()
    eng = core.Engine(cfg)
    eng.prepare()
    res = run_phase(core, eng, "READ")
    if path_name == "uring":
        assert uring_paths(capfd) == [(1, 0, batch_of(CBS), URING_DEPTH)]
    err = res[0]["error"]
    m = ERR_RE.search(err)
    assert m and "verification failed" in err, err
    got = (int(m.group(1)), int(m.group(2)) if m.group(2) else None)
    assert got == want, (f"{path_name}/{case_name}: engine reports (first bad offset, "
                         f"mismatching words) = {got}, expected {want}: {err!r}")

    # same engine, repaired file: the reused context's counters were reset
    with open(p, "r+b") as f:
        f.write(clean)
    res = run_ok(core, eng, "READ")
    assert res[0]["bytes"] == size
