"""Cases of the exact GPU staging tests with 16 and 17 workers, so that several
GpuCtx enqueue into one HIP stream from several host threads. Written once and
run twice: tests/test_gpu_shared_streams.py runs them in process on the default
pool of 8 shared streams, tests/shared_streams_child.py runs a few of them in a
fresh process per EB_GPU_SHARED_STREAMS value (the variable is read once per
process).

The byte, slot and slice checks are those of tests/test_gpu_engine_exact.py,
the oracle is tests/kernel_model.py (tests/verify_diag_model.py for the
--verifydiag texts). What this module adds is the worker count and, for every
case, an assertion from Engine.gpu_streams() that the sharing the case claims
is real. A worker's context exists from its first data phase on, so the layout
is read right after that phase.
"""

import collections

import numpy as np

from tests import kernel_model as km
from tests import verify_diag_cases as dc
from tests import verify_diag_model as dm
from tests.engine_modes_cases import parse_err, samples
from tests.test_gpu_engine_exact import (B4K, CBS, PIPELINE_MIN_BS, SALT, URING_DEPTH,
                                         VERIFY_FETCH_INTERVAL, VERIFY_PATHS, W,
                                         assert_shares, batch_of, fair_share, gpu_cfg,
                                         pattern_bytes, run_ok, run_phase, run_read_case,
                                         run_write_case, sync_batched_in_use, uring_paths,
                                         write_pattern_file)

WORKERS = 16
DEFAULT_POOL = 8  # streams per device when EB_GPU_SHARED_STREAMS is not set
BS256K = PIPELINE_MIN_BS


# ---------------------------------------------------------------------------
# the stream layout
# ---------------------------------------------------------------------------

def expected_histogram(threads: int, pool: int) -> list:
    """How many workers enqueue into each stream, sorted. The pool hands its
    streams out round-robin in order of construction, and an engine's workers
    construct their contexts with nobody else in between: `threads`
    consecutive draws, wherever the round starts. pool 0: a private stream
    each."""
    if not pool:
        return [1] * threads
    return sorted(c for c in (threads // pool + (i < threads % pool) for i in range(pool)) if c)


def histogram(streams) -> list:
    return sorted(collections.Counter(sid for sid, _ in streams).values())


def assert_layout(eng, threads: int, pool: int, what: str) -> list:
    streams = eng.gpu_streams()
    assert len(streams) == threads, (what, streams)
    assert all(sid != 0 for sid, _ in streams), (what, streams)
    assert [shared for _, shared in streams] == [bool(pool)] * threads, (
        f"{what}: expected every stream to be {'shared' if pool else 'private'}: {streams}")
    assert histogram(streams) == expected_histogram(threads, pool), (
        f"{what}: {threads} workers on a pool of {pool} must use their streams "
        f"{expected_histogram(threads, pool)} times, they use them {histogram(streams)} times")
    return streams


def stream_pair(streams) -> tuple:
    """(first, second): the two lowest ranks of the first stream (in rank
    order) that more than one worker uses; without any sharing, ranks 0, 1."""
    by_stream = collections.OrderedDict()
    for rank, (sid, _) in enumerate(streams):
        by_stream.setdefault(sid, []).append(rank)
    for ranks in by_stream.values():
        if len(ranks) >= 2:
            return ranks[0], ranks[1]
    return 0, 1


# ---------------------------------------------------------------------------
# A. write: file bytes equal the model
# ---------------------------------------------------------------------------

def check_write(core, tmp_path, capfd, monkeypatch, path_name, fill, bs, blocks, threads,
                tail=0, pool=DEFAULT_POOL):
    """run_write_case at `blocks` blocks per worker; tail > 0 adds a short
    last block to the last worker's slice."""
    eng = run_write_case(core, tmp_path, capfd, monkeypatch, path_name, fill, bs,
                         threads * blocks * bs + tail, threads)
    return assert_layout(eng, threads, pool, f"write {path_name} {fill} threads={threads}")


# ---------------------------------------------------------------------------
# B. read, verify off: the slots hold the right blocks
# ---------------------------------------------------------------------------

MMAP_BS = 65536

# name -> (block size, blocks per worker, slots in use given num_slots, config)
READ_CASES = {
    # half-ring batched copies: two batches and one block, the ring wraps
    "sync_batched_4k": (4096, 2 * B4K + 1, sync_batched_in_use(4096), dict(iodepth=1)),
    "pipelined_256k": (BS256K, 5, lambda num_slots: num_slots, dict(iodepth=1)),
    "uring_per_slot": (4096, 40, lambda num_slots: URING_DEPTH, dict(iodepth=URING_DEPTH)),
    "uring_batched": (4096, 40, lambda num_slots: 16, dict(iodepth=16)),
    # 32 slots of 64 KiB per worker: 38 blocks wrap the ring
    "mmap": (MMAP_BS, 38, lambda num_slots: num_slots, dict(mmap=True)),
}


def check_read(core, tmp_path, capfd, monkeypatch, name, threads=WORKERS, pool=DEFAULT_POOL):
    bs, blocks, in_use, path_cfg = READ_CASES[name]
    what = f"read {name} threads={threads}"
    if name.startswith("uring"):
        monkeypatch.setenv("EB_DEBUG_PATH", "1")
        if name == "uring_batched":
            monkeypatch.setenv("EB_GPU_URING_BATCH", "1")
        else:
            monkeypatch.delenv("EB_GPU_URING_BATCH", raising=False)
        capfd.readouterr()
    eng = run_read_case(core, tmp_path, what, bs, threads * blocks * bs, threads, in_use,
                        **path_cfg)
    if name.startswith("uring"):
        batched = int(name == "uring_batched")
        assert uring_paths(capfd) == [(1, batched, batch_of(bs), path_cfg["iodepth"])] * threads
    return assert_layout(eng, threads, pool, what)


# ---------------------------------------------------------------------------
# C. verify failures are attributed to the right worker
# ---------------------------------------------------------------------------

VERIFY_BLOCKS = 40  # per worker: fewer than one fetch window of the "acc" paths
FLIP = np.uint64(0xA5A5A5A5A5A5A5A5)

# damaged words, as word indices within the worker's slice. "second" (the
# second worker of a stream): three words in two blocks, the higher block
# first. "first" (its peer, case (ii) only): two words in two blocks. So the
# two workers differ in what an "acc" report counts (3 and 2) and in what a
# "blk" report counts (2 and 1).
SECOND_WORDS = (30 * W + 17, 7 * W + 5, 7 * W + 100)
FIRST_WORDS = (20 * W + 9, 3 * W + 64)


def damage(words, share, role, diag):
    b = share.start // 8
    if role == "first":
        for i in FIRST_WORDS:
            words[b + i] ^= FLIP
    elif not diag:
        for i in SECOND_WORDS:
            words[b + i] ^= FLIP
    else:  # one of every class: block 7 zero x3 and a flipped bit, 12 pattern x2, 30 other
        words[b + 7 * W + 5:b + 7 * W + 8] = 0
        words[b + 7 * W + 100] ^= np.uint64(1 << 7)
        words[b + 12 * W:b + 12 * W + 2] = km.checksum_words(16, share.start + 12 * CBS + 4096,
                                                             SALT)
        words[b + 30 * W + 17] ^= FLIP


def seen_window(bad: bytes, clean: bytes, share, kind):
    """[lo, hi) of the bytes that the check which fires first has seen: "acc" -
    the worker's whole slice (one fetch at the end of a phase of fewer than 64
    blocks); "blk" - the lowest damaged block of the slice."""
    assert share.num_blocks < VERIFY_FETCH_INTERVAL and share.nbytes == share.num_blocks * CBS
    lo, hi = share.start, share.start + share.nbytes
    if kind == "blk":
        g = np.frombuffer(bad, dtype=np.uint8)[lo:hi]
        w = np.frombuffer(clean, dtype=np.uint8)[lo:hi]
        lo += int(np.flatnonzero(g != w)[0]) // CBS * CBS
        hi = lo + CBS
    return lo, hi


def plain_model(bad, clean, share, kind):
    lo, hi = seen_window(bad, clean, share, kind)
    n_bad, first_bad = km.verify(bad[lo:hi], lo, SALT)
    return first_bad, n_bad


def diag_model(bad, clean, share, kind):
    """One launch per block: the record is the blocks' combination."""
    lo, hi = seen_window(bad, clean, share, kind)
    rec = dm.empty()
    for o in range(lo, hi, CBS):
        rec = dm.combine(rec, dm.diagnose(bad[o:o + CBS], o, SALT))
    return rec


def check_verify(core, tmp_path, capfd, monkeypatch, path_name, both, diag=False,
                 threads=WORKERS, pool=DEFAULT_POOL):
    """both=False is case (i): only the second worker of a stream reads damaged
    data. both=True is case (ii): its peer on that stream does too."""
    kind, path_cfg = VERIFY_PATHS[path_name]
    what = f"verify {path_name} both={both} diag={diag} threads={threads}"
    size = threads * VERIFY_BLOCKS * CBS
    shares = fair_share(size, CBS, threads)
    p = tmp_path / "f"
    write_pattern_file(core, p, size)
    clean = pattern_bytes(size, SALT)

    if path_name == "uring":
        monkeypatch.setenv("EB_DEBUG_PATH", "1")
        capfd.readouterr()
    extra = dict(verify_diag=True) if diag else {}
    eng = core.Engine(gpu_cfg(p, size, CBS, threads, verify_salt=SALT, **path_cfg, **extra))
    eng.prepare()
    assert_shares(run_ok(core, eng, "READ"), shares, what + " clean READ")
    if path_name == "uring":
        assert uring_paths(capfd) == [(1, 0, batch_of(CBS), URING_DEPTH)] * threads
    streams = assert_layout(eng, threads, pool, what)
    first, second = stream_pair(streams)
    if pool:
        assert first < second and streams[first] == streams[second]

    words = np.frombuffer(clean, dtype="<u8").copy()
    roles = {second: "second"}
    if both:
        roles[first] = "first"
    for rank, role in roles.items():
        damage(words, shares[rank], role, diag)
    bad = words.tobytes()
    want = {rank: (diag_model if diag else plain_model)(bad, clean, shares[rank], kind)
            for rank in roles}
    if diag:  # the damage is what it claims
        w = want[second]
        assert (w["zero"], w["pattern"], w["bitflip"], w["other"], w["nbad"]) == (
            (3, 2, 1, 1, 7) if kind == "acc" else (3, 0, 1, 0, 4))
        assert w["first"] == shares[second].start + (7 * W + 5) * 8
    else:
        assert want[second] == (shares[second].start + (7 * W + 5) * 8, 3 if kind == "acc" else 2)
        if both:
            assert want[first] == (shares[first].start + (3 * W + 64) * 8,
                                   2 if kind == "acc" else 1)
    with open(p, "r+b") as f:  # in place: the mmap path sizes the file itself
        f.write(bad)

    res = run_phase(core, eng, "READ")
    reported = []
    for row in res:
        rank, err = row["rank"], row["error"]
        if "verification failed" not in err:
            assert err in ("", "interrupted"), (what, rank, err)
            continue
        assert rank in roles, (f"{what}: worker {rank} read clean data and reports {err!r}; "
                               f"damaged: {roles}, streams: {streams}")
        reported.append(rank)
        if diag:
            on_gpu, first_bad, rec = dc.parse_message(err)
            assert on_gpu and first_bad == want[rank]["first"] and \
                rec == dc.without_first(want[rank]), (
                    f"{what}: worker {rank} ({roles[rank]} of its stream) reports {err!r}, "
                    f"the model of its own slice is {want[rank]}")
        else:
            assert parse_err(err) == want[rank], (
                f"{what}: worker {rank} ({roles[rank]} of its stream) must report (first bad "
                f"offset, mismatching words) = {want[rank]} of its own slice: {err!r}; "
                f"all: {want}")
    if both:
        assert reported, (what, [r["error"] for r in res])
    else:
        assert reported == [second], (what, reported, [r["error"] for r in res])

    # same engine, same contexts, repaired file: every worker's counters are
    # its own and were reset
    assert eng.gpu_streams() == streams
    with open(p, "r+b") as f:
        f.write(clean)
    assert_shares(run_ok(core, eng, "READ"), shares, what + " re-READ")
    return streams


# ---------------------------------------------------------------------------
# D. lat=True: one sample per block per worker
# ---------------------------------------------------------------------------

# name -> (phase, block size, blocks per worker, config)
LAT_CASES = {
    "pipelined_read": ("READ", BS256K, 5, dict(iodepth=1)),
    # wraps the ring and ends on a short batch
    "batched_4k_read": ("READ", 4096, 2 * B4K + 41, dict(iodepth=1)),
    "mmap_read": ("READ", MMAP_BS, 38, dict(mmap=True, verify_salt=SALT)),
    "pipelined_write": ("WRITE", MMAP_BS, 38, dict(iodepth=1, verify_salt=SALT)),
}


def check_lat(core, tmp_path, name, threads=WORKERS, pool=DEFAULT_POOL):
    phase, bs, blocks, path_cfg = LAT_CASES[name]
    what = f"lat {name} threads={threads}"
    size = threads * blocks * bs
    p = tmp_path / "f"
    if phase == "READ":
        write_pattern_file(core, p, size)
    eng = core.Engine(gpu_cfg(p, size, bs, threads, lat=True, **path_cfg))
    eng.prepare()
    res = run_ok(core, eng, phase)
    streams = assert_layout(eng, threads, pool, what)
    assert_shares(res, fair_share(size, bs, threads), what)
    for r in res:
        assert r["iops"] == blocks and samples(r) == blocks, (
            f"{what}: worker {r['rank']} did {r['iops']} of {blocks} blocks and has "
            f"{samples(r)} latency samples")
    if phase == "WRITE":
        assert p.read_bytes() == pattern_bytes(size, SALT), what
    return streams
