"""Case tables and checks for the engine's directory, custom-tree and mixed
modes, written once and run twice: tests/test_engine_modes_exact.py runs them
with gpu_ids=[] (no GPU needed: it proves the layouts, slice rules and error
texts stated here), tests/test_gpu_engine_modes.py runs them with gpu_ids=[0],
where every block is staged through HBM, and adds the GPU-only checks
(block-variance bytes by fill counter, slot contents, word counts).

The oracle is tests/kernel_model.py. No expectation is taken from bytes the
engine produced, except the "pre-filled ring" idiom for blockvar_pct=0.

Rules of the engine that the checks rely on, each stated once:

* error texts - a block whose file offset is a multiple of 8 and whose length
  is a multiple of 16 is checked on the GPU when there is one; the report then
  carries the lowest bad word's offset and the number of bad words that the
  check has seen. Every other block (and every block without a GPU) is checked
  on the CPU, whose report names the first bad *byte* and carries no count.
  Offsets are relative to the file that holds the block.
* peers - the first worker that fails interrupts the others, so a worker
  whose own data is clean ends with error "" or "interrupted".
* directory mode - worker r owns r{r}/d0/r{r}-f{0..files-1} and goes through
  them in that order; its fill counter runs on across files.
* custom tree (tree_ownership) and several paths in file mode (virt_shares)
  are stated at those functions.
"""

import os

import numpy as np

from tests import kernel_model as km
from tests.test_gpu_engine_exact import (BATCH_BYTES, ERR_RE, PIPELINE_MIN_BS, SALT, SEED,
                                         URING_DEPTH, fair_share, first_diff_report,
                                         model_block, pattern_bytes, random_share, run_ok,
                                         run_phase, write_pattern_file)

BS = 65536
SBS = 4096
DEPTH = URING_DEPTH
SALT2 = SALT + (1 << 40)  # second file of a two-path READ: words name (file, offset)


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------

def parse_err(err):
    m = ERR_RE.search(err)
    if not (m and "verification failed" in err):
        return None
    return int(m.group(1)), int(m.group(2)) if m.group(2) else None


def gpu_checked(gpu_ids, off, length):
    return bool(gpu_ids) and off % 8 == 0 and length % 16 == 0


def flip(path, spans):
    with open(path, "r+b") as f:
        for off, ln in spans:
            f.seek(off)
            old = f.read(ln)
            f.seek(off)
            f.write(bytes(b ^ 0xA5 for b in old))


def assert_file(path, want, what):
    got = path.read_bytes()
    assert len(got) == len(want), f"{what}: {path.name} has {len(got)} bytes, not {len(want)}"
    if got != want:
        raise AssertionError(f"{what}: {path.name}: " + first_diff_report(got, want))


def assert_only_rank_reports(res, rank, want, what):
    """Worker `rank` reports exactly `want` = (offset, count or None); the
    others have nothing to report of their own."""
    for r in res:
        if r["rank"] == rank:
            assert parse_err(r["error"]) == want, (
                f"{what}: worker {rank} must report (first bad offset, mismatching words) = "
                f"{want}: {r['error']!r}")
        else:
            assert r["error"] in ("", "interrupted"), (what, r["rank"], r["error"])


def samples(res_row, key="io_lat"):
    """Number of samples in a latency histogram ([count, sum, min, max, buckets...])."""
    v = res_row[key]
    assert v[0] == sum(v[4:]), "histogram count and buckets disagree"
    return v[0]


# ---------------------------------------------------------------------------
# D. directory mode
# ---------------------------------------------------------------------------

# engine -> config that selects it (chains also need file_size <= block_size)
DIR_ENGINES = {"sync": dict(iodepth=1), "uring": dict(iodepth=DEPTH),
               "chains": dict(iodepth=DEPTH)}
CHAIN_FILES = 9


def dir_cfg(root, gpu_ids, bs, size, files, **kw):
    cfg = dict(paths=[str(root)], path_type="dir", threads=2, num_dataset_threads=2, dirs=1,
               files=files, file_size=size, block_size=bs, bench_seed=SEED,
               gpu_ids=list(gpu_ids))
    cfg.update(kw)
    return cfg


def dir_file(root, r, f):
    return root / f"r{r}" / "d0" / f"r{r}-f{f}"


def dir_engine(core, root, gpu_ids, engine, bs, size, files, **kw):
    if engine == "chains":
        assert size <= bs
    else:
        assert size > bs
    eng = core.Engine(dir_cfg(root, gpu_ids, bs, size, files, **DIR_ENGINES[engine], **kw))
    eng.prepare()
    return eng


def assert_dir_counts(res, files, size, bs, what, key="bytes"):
    iops = "iops" if key == "bytes" else "rm_iops"
    for r in res:
        assert (r[key], r[iops]) == (files * size, files * -(-size // bs)), (what, r["rank"], r)


def prewrite_dir(core, root, files, size, ranks=(0, 1)):
    for r in ranks:
        os.makedirs(root / f"r{r}" / "d0", exist_ok=True)
        for f in range(files):
            write_pattern_file(core, dir_file(root, r, f), size)


# (engine, block size, file size, files per worker)
DIR_WRITE_CASES = (
    [(e, BS, 10 * BS + tail, 2) for e in ("sync", "uring") for tail in (0, 8, 4)]
    + [("chains", BS, s, CHAIN_FILES) for s in (BS, BS - 8, BS - 4, 16, 8, 0)])


def check_dir_write_checksum(core, root, gpu_ids, engine, bs, size, files):
    what = f"dir {engine} size={size} gpu={gpu_ids}"
    eng = core.Engine(dir_cfg(root, gpu_ids, bs, size, files, verify_salt=SALT,
                              **DIR_ENGINES[engine]))
    eng.prepare()
    run_ok(core, eng, "MKDIRS")
    res = run_ok(core, eng, "WRITE")
    assert_dir_counts(res, files, size, bs, what)
    assert [r["entries"] for r in res] == [files, files], what
    for r in range(2):
        for f in range(files):
            assert_file(dir_file(root, r, f), pattern_bytes(size, SALT), what)
    # what was written verifies on the same engine
    res = run_ok(core, eng, "READ")
    assert_dir_counts(res, files, size, bs, what + " READ")


def dir_shape(engine):
    return (SBS, SBS, CHAIN_FILES) if engine == "chains" else (SBS, 10 * SBS, 2)


# name -> (corrupted worker, file, spans, tail bytes added to the file size)
DIR_VERIFY_CASES = {
    # the 4th block of worker 0's first file (chains: the 6th of 9 files, so
    # that other chains are in flight)
    "word": (0, {"chains": 5}, lambda size, bs: [(min(3 * bs, size - bs) + 72, 8)], 0),
    # a byte of the part that is checked on the CPU: the 4-byte tail block
    # (chains: the whole file, whose length is no multiple of 16)
    "tail_byte": (0, {"chains": 5}, lambda size, bs: [(size - 2, 1)], 4),
    # worker 0 is clean, worker 1's second file is not
    "worker1_file1": (1, {"sync": 1, "uring": 1, "chains": 1},
                      lambda size, bs: [(min(7 * bs, size - bs) + 8, 8)], 0),
}


def check_dir_verify_failure(core, root, gpu_ids, engine, case_name):
    rank, file_of, spans_of, tail = DIR_VERIFY_CASES[case_name]
    bs, size, files = dir_shape(engine)
    size = size - 12 + tail if engine == "chains" and tail else size + tail
    f = file_of.get(engine, 0)
    what = f"dir {engine} {case_name} gpu={gpu_ids}"
    prewrite_dir(core, root, files, size)
    spans = spans_of(size, bs)
    off, ln = spans[0]
    blk = off // bs * bs
    cnt = 1 if gpu_checked(gpu_ids, blk, min(bs, size - blk)) else None
    if ln == 8:  # the model agrees with the case table
        bad = bytearray(pattern_bytes(size, SALT))
        bad[off:off + 8] = bytes(b ^ 0xA5 for b in bad[off:off + 8])
        assert km.verify(bytes(bad[blk:blk + bs]), blk, SALT) == (1, off)
    else:
        assert cnt is None, "case must hit a CPU-checked block"
    flip(dir_file(root, rank, f), spans)

    eng = dir_engine(core, root, gpu_ids, engine, bs, size, files, verify_salt=SALT)
    res = run_phase(core, eng, "READ")
    assert_only_rank_reports(res, rank, (off, cnt), what)
    flip(dir_file(root, rank, f), spans)  # repair
    res = run_ok(core, eng, "READ")
    assert_dir_counts(res, files, size, bs, what + " re-READ")
    assert [r["entries"] for r in res] == [files, files]


def check_dir_read_inline(core, root, gpu_ids, engine):
    bs, size, files = BS, 10 * BS + 8, 2
    what = f"dir {engine} read_inline gpu={gpu_ids}"
    eng = dir_engine(core, root, gpu_ids, engine, bs, size, files, verify_salt=SALT,
                     read_inline=True)
    run_ok(core, eng, "MKDIRS")
    res = run_ok(core, eng, "WRITE")
    assert_dir_counts(res, files, size, bs, what)
    assert_dir_counts(res, files, size, bs, what + " inline reads", key="rm_bytes")
    for r in range(2):
        for f in range(files):
            assert_file(dir_file(root, r, f), pattern_bytes(size, SALT), what)


def check_dir_dedicated_reader(core, root, gpu_ids, iodepth):
    """rwmix_threads=1: worker 0 only reads (and verifies) its pre-written
    files inside the WRITE phase, worker 1 writes."""
    bs, size, files = SBS, 10 * SBS, 2
    what = f"dir dedicated reader iodepth={iodepth} gpu={gpu_ids}"
    prewrite_dir(core, root, files, size, ranks=(0,))
    os.makedirs(root / "r1" / "d0")
    eng = core.Engine(dir_cfg(root, gpu_ids, bs, size, files, verify_salt=SALT,
                              rwmix_threads=1, iodepth=iodepth))
    eng.prepare()
    res = run_ok(core, eng, "WRITE")
    assert (res[0]["bytes"], res[0]["rm_bytes"], res[0]["rm_iops"]) == (0, files * size,
                                                                        files * 10), what
    assert (res[1]["bytes"], res[1]["rm_bytes"], res[1]["iops"]) == (files * size, 0,
                                                                     files * 10), what
    for r in range(2):
        for f in range(files):
            assert_file(dir_file(root, r, f), pattern_bytes(size, SALT), what)

    off = 6 * bs + 40
    flip(dir_file(root, 0, 1), [(off, 8)])
    res = run_phase(core, eng, "WRITE")
    assert_only_rank_reports(res, 0, (off, 1 if gpu_ids else None), what)
    flip(dir_file(root, 0, 1), [(off, 8)])
    res = run_ok(core, eng, "WRITE")
    assert res[0]["rm_bytes"] == files * size, what


# --- GPU only ---------------------------------------------------------------

DIR_FILLS = [("blockvar", 100, "fast"), ("blockvar", 37, "strong"), ("ring",)]
DIR_FILL_IDS = ["bv100fast", "bv37strong", "bv0ring"]


def dir_bv_shape(engine):
    return (BS, BS, CHAIN_FILES) if engine == "chains" else (BS, 10 * BS, 2)


def check_dir_write_blockvar(core, root, engine, fill):
    """Block k of a worker's f-th file is fill call f*blocksPerFile + k + 1 of
    a fresh engine: prepSlot / startChain fill in generator and file order,
    whichever slot the block goes through. blockvar_pct=0 refills nothing:
    every block is the pre-filled content of one of the slots in use."""
    bs, size, files = dir_bv_shape(engine)
    bpf = size // bs
    what = f"dir {engine} {fill}"
    kw = dict(blockvar_pct=0) if fill[0] == "ring" else dict(blockvar_pct=fill[1],
                                                             blockvar_algo=fill[2])
    eng = dir_engine(core, root, [0], engine, bs, size, files, **kw)
    run_ok(core, eng, "MKDIRS")
    res = run_ok(core, eng, "WRITE")
    assert_dir_counts(res, files, size, bs, what)
    for r in range(2):
        num_slots, stride, raw = eng.gpu_slots(r)
        in_use = 1 if engine == "sync" else DEPTH
        ring = [raw[s * stride:s * stride + bs] for s in range(in_use)]
        assert len(set(ring)) == in_use, f"{what}: pre-filled slots repeat"
        seen = set()
        for f in range(files):
            data = dir_file(root, r, f).read_bytes()
            assert len(data) == size
            for k in range(bpf):
                got = data[k * bs:(k + 1) * bs]
                if fill[0] == "ring":
                    assert got in ring, f"{what}: worker {r} file {f} block {k} is no slot's data"
                    seen.add(got)
                    continue
                want = model_block(fill, r, f * bpf + k, bs)
                if got != want:
                    raise AssertionError(
                        f"{what}: worker {r}, file {f}, block {k} (fill call "
                        f"{f * bpf + k + 1}): " + first_diff_report(got, want))
        if fill[0] == "ring":
            assert len(seen) == in_use, f"{what}: worker {r} used {len(seen)} slots"


def check_dir_read_slots(core, root, engine):
    """After a verify-off READ every slot in use holds one whole block (chains:
    one whole file) of the worker; the blocks come from the model."""
    bs, size, files = dir_bv_shape(engine)
    bpf = size // bs
    fill = DIR_FILLS[0]
    what = f"dir {engine} READ slots"
    kw = dict(blockvar_pct=100, blockvar_algo="fast")
    eng = dir_engine(core, root, [0], engine, bs, size, files, **kw)
    run_ok(core, eng, "MKDIRS")
    run_ok(core, eng, "WRITE")
    del eng
    eng = dir_engine(core, root, [0], engine, bs, size, files, **kw)  # fresh slots
    res = run_ok(core, eng, "READ")
    assert_dir_counts(res, files, size, bs, what)
    for r in range(2):
        blocks = {model_block(fill, r, i, bs): i for i in range(files * bpf)}
        assert len(blocks) == files * bpf
        num_slots, stride, raw = eng.gpu_slots(r)
        held = [blocks.get(raw[s * stride:s * stride + bs]) for s in range(num_slots)]
        if engine == "sync":  # order is forced: slot 0 holds the last block read
            assert held[0] == files * bpf - 1, (what, r, held[:4])
            in_use = 1
        else:
            in_use = DEPTH
            assert None not in held[:in_use] and len(set(held[:in_use])) == in_use, (
                f"{what}: worker {r}: the {in_use} slots must hold {in_use} distinct whole "
                f"blocks of its files, they hold blocks {held[:in_use]}")
        assert set(held[in_use:]) == {None}, (what, r, "a slot beyond those in use was written")


# ---------------------------------------------------------------------------
# E. custom tree
# ---------------------------------------------------------------------------

TREE_FILES = [("a/zero", 0), ("a/w8", 8), ("b/m4100", 4100), ("b/one", BS),
              ("c/three", 3 * BS + 24), ("c/short", BS - 16), ("shared", 9 * BS + 8)]
TREE_SHARE = 4 * BS


def tree_ownership(files, bs, sharesize, ranks, round_robin):
    """customTreeFiles' rule: files below sharesize are dealt out whole, the
    k-th of them (in list order) to rank k % ranks. A file of at least
    sharesize is shared: each rank takes its fair_share slice, or with
    tree_round_robin the blocks b with b % ranks == rank (the short tail
    block belongs to the rank its index lands on). -> per rank (bytes, files
    touched, {name: [(offset, length)]})."""
    out = [[0, 0, {}] for _ in range(ranks)]
    k = 0
    for name, size in files:
        if not (sharesize and size >= sharesize):
            o = out[k % ranks]
            k += 1
            o[0] += size
            o[1] += 1
            o[2][name] = [(0, size)]
            continue
        for r, sh in enumerate(fair_share(size, bs, ranks)):
            if round_robin:
                spans = [(b * bs, min(bs, size - b * bs))
                         for b in range(r, -(-size // bs), ranks)]
            else:
                spans = [(sh.start, sh.nbytes)] if sh.nbytes else []
            if spans:
                out[r][0] += sum(ln for _, ln in spans)
                out[r][1] += 1
                out[r][2][name] = spans
    return out


TREE_CASES = [(iodepth, rr, rand) for iodepth in (1, DEPTH)
              for rr, rand in ((False, False), (True, False), (False, True))]


def check_tree(core, root, gpu_ids, iodepth, round_robin, randomize):
    what = f"tree iodepth={iodepth} rr={round_robin} rand={randomize} gpu={gpu_ids}"
    own = tree_ownership(TREE_FILES, BS, TREE_SHARE, 2, round_robin)
    assert sum(o[0] for o in own) == sum(s for _, s in TREE_FILES)
    cfg = dict(paths=[str(root)], path_type="dir", threads=2, num_dataset_threads=2,
               block_size=BS, tree_files=TREE_FILES, tree_dirs=[], sharesize=TREE_SHARE,
               tree_round_robin=round_robin, tree_rand=randomize, verify_salt=SALT,
               iodepth=iodepth, bench_seed=SEED, gpu_ids=list(gpu_ids))
    eng = core.Engine(cfg)
    eng.prepare()

    def assert_counts(res, phase):
        for r, o in zip(res, own):
            assert (r["bytes"], r["entries"]) == (o[0], o[1]), (what, phase, r["rank"], r, o[:2])

    assert_counts(run_ok(core, eng, "WRITE"), "WRITE")
    for name, size in TREE_FILES:
        assert_file(root / name, pattern_bytes(size, SALT), what)
    assert_counts(run_ok(core, eng, "READ"), "READ")

    # (a) a word of block 7 of the shared file: rank 1's in both cuttings
    off = 7 * BS + 192
    assert any(s <= off < s + n for s, n in own[1][2]["shared"])
    assert not any(s <= off < s + n for s, n in own[0][2]["shared"])
    flip(root / "shared", [(off, 8)])
    res = run_phase(core, eng, "READ")
    assert_only_rank_reports(res, 1, (off, 1 if gpu_ids else None), what + " (a)")
    flip(root / "shared", [(off, 8)])
    # (b) a byte of the last 4 bytes of the 4100-byte file: checked on the CPU
    assert "b/m4100" in own[0][2]
    flip(root / "b/m4100", [(4097, 1)])
    res = run_phase(core, eng, "READ")
    assert_only_rank_reports(res, 0, (4097, None), what + " (b)")
    flip(root / "b/m4100", [(4097, 1)])
    assert_counts(run_ok(core, eng, "READ"), "re-READ")


# ---------------------------------------------------------------------------
# F. file mode
# ---------------------------------------------------------------------------

# name -> (config, "acc": one report per fetch window / "blk": per block)
FILE_PATHS = {"pipelined": (dict(iodepth=1), "acc"), "blockio": (dict(flock_mode=1), "blk"),
              "uring": (dict(iodepth=DEPTH), "blk"), "mmap": (dict(mmap=True), "acc")}


def files_cfg(paths, gpu_ids, size, bs, threads, **kw):
    cfg = dict(paths=[str(p) for p in paths], path_type="file", threads=threads,
               num_dataset_threads=threads, file_size=size, block_size=bs, bench_seed=SEED,
               gpu_ids=list(gpu_ids))
    cfg.update(kw)
    return cfg


def virt_shares(size, bs, nfiles, threads):
    """fileModeBlocks with several paths: the files' ceil(size/bs) blocks are
    laid end to end, file after file, and that range is dealt out by the
    fair_share rule. -> per rank [(file, in-file offset, length)]."""
    bpf = -(-size // bs)
    out = []
    for sh in fair_share(bpf * nfiles * bs, bs, threads):
        blocks = []
        for v in range(sh.first_block, sh.first_block + sh.num_blocks):
            fi, k = divmod(v, bpf)
            blocks.append((fi, k * bs, min(bs, size - k * bs)))
        out.append(blocks)
    return out


def assert_virt_counts(res, shares, what):
    for r, blocks in zip(res, shares):
        assert (r["bytes"], r["iops"]) == (sum(b[2] for b in blocks), len(blocks)), (
            what, r["rank"], r["bytes"], r["iops"])


TWO_PATH_CASES = [(p, tail, threads) for p in FILE_PATHS for tail, threads in
                  ((0, 2), (8, 2), (4, 2), (8, 3))]  # 3 workers: one spans both files


def check_two_paths(core, root, gpu_ids, path_name, tail, threads):
    path_cfg, kind = FILE_PATHS[path_name]
    bs, size = BS, 40 * BS + tail
    what = f"two paths {path_name} tail={tail} threads={threads} gpu={gpu_ids}"
    paths = [root / "f0", root / "f1"]
    shares = virt_shares(size, bs, 2, threads)
    eng = core.Engine(files_cfg(paths, gpu_ids, size, bs, threads, verify_salt=SALT, **path_cfg))
    eng.prepare()
    assert_virt_counts(run_ok(core, eng, "WRITE"), shares, what)
    for p in paths:
        assert_file(p, pattern_bytes(size, SALT), what)
    assert_virt_counts(run_ok(core, eng, "READ"), shares, what + " READ")

    # two bad words in blocks 7 and 9 of the second file, both one worker's
    spans = [(9 * bs + 1024, 8), (7 * bs + 40, 8)]
    owners = {r for r, blocks in enumerate(shares) for fi, o, _ in blocks
              if fi == 1 and o in (7 * bs, 9 * bs)}
    assert len(owners) == 1 and len(shares[min(owners)]) <= 64
    bad = bytearray(pattern_bytes(size, SALT))
    for o, n in spans:
        bad[o:o + n] = bytes(b ^ 0xA5 for b in bad[o:o + n])
    assert km.verify(bytes(bad[:40 * bs]), 0, SALT) == (2, 7 * bs + 40)
    cnt = None if not gpu_ids else 2 if kind == "acc" else 1
    flip(paths[1], spans)
    res = run_phase(core, eng, "READ")
    assert_only_rank_reports(res, min(owners), (7 * bs + 40, cnt), what)
    flip(paths[1], spans)
    assert_virt_counts(run_ok(core, eng, "READ"), shares, what + " re-READ")


def check_two_paths_batched_read_slots(core, root, threads):
    """GPU only. Verify-off READ of small blocks = half-ring batched copies;
    a worker's blocks fit one batch, so slot k holds its k-th block, looked up
    in whichever file holds it (the files carry different salts)."""
    bs, size = SBS, 40 * SBS
    assert 40 * 2 // threads + 2 <= BATCH_BYTES // bs
    paths = [root / "f0", root / "f1"]
    salts = [SALT, SALT2]
    for p, s in zip(paths, salts):
        write_pattern_file(core, p, size, s)
    shares = virt_shares(size, bs, 2, threads)
    eng = core.Engine(files_cfg(paths, [0], size, bs, threads, iodepth=1))
    eng.prepare()
    assert_virt_counts(run_ok(core, eng, "READ"), shares, "two-path batched READ")
    for r, blocks in enumerate(shares):
        num_slots, stride, raw = eng.gpu_slots(r)
        for k, (fi, off, ln) in enumerate(blocks):
            got = raw[k * stride:k * stride + ln]
            want = km.checksum_pattern(ln, off, salts[fi])
            if got != want:
                raise AssertionError(f"two-path batched READ: worker {r} slot {k} must hold "
                                     f"file {fi} offset {off}: " + first_diff_report(got, want))


ORDER_CASES = [(o, p) for o in ("backward", "strided") for p in FILE_PATHS]


def check_order(core, root, gpu_ids, order, path_name):
    """backward: the fair_share slices, last block first, the file in full.
    strided: whole blocks only (floor(size/bs) blocks, block b to rank
    b % threads), so the 8-byte tail is never written: the file ends at the
    last whole block, except with mmap, which sizes the file first and so
    leaves a zero tail."""
    path_cfg, _ = FILE_PATHS[path_name]
    bs, size = BS, 40 * BS + 8
    what = f"{order} {path_name} gpu={gpu_ids}"
    p = root / "f"
    eng = core.Engine(files_cfg([p], gpu_ids, size, bs, 2, verify_salt=SALT,
                                **{order: True}, **path_cfg))
    eng.prepare()
    if order == "backward":
        want_counts = [(sh.nbytes, sh.num_blocks) for sh in fair_share(size, bs, 2)]
        want = pattern_bytes(size, SALT)
    else:
        want_counts = [(20 * bs, 20)] * 2
        want = pattern_bytes(40 * bs, SALT) + (bytes(8) if path_name == "mmap" else b"")
    for phase in ("WRITE", "READ"):
        res = run_ok(core, eng, phase)
        assert [(r["bytes"], r["iops"]) for r in res] == want_counts, (what, phase)
        assert_file(p, want, what)
    off = 33 * bs + 80  # rank 1 in both orders (block 33: odd, and in the upper half)
    flip(p, [(off, 8)])
    res = run_phase(core, eng, "READ")
    assert_only_rank_reports(res, 1, (off, 1 if gpu_ids else None), what)


def check_random_aligned_write(core, root, gpu_ids, path_name):
    """random + rand_aligned WRITE uses the full-coverage generator: every
    whole block of the worker's random_share range exactly once."""
    bs, size = BS, 80 * BS
    what = f"random aligned WRITE {path_name} gpu={gpu_ids}"
    p = root / "f"
    eng = core.Engine(files_cfg([p], gpu_ids, size, bs, 2, verify_salt=SALT, random=True,
                                **FILE_PATHS[path_name][0]))
    eng.prepare()
    res = run_ok(core, eng, "WRITE")
    assert [(r["bytes"], r["iops"]) for r in res] == [
        (sh.nbytes, sh.num_blocks) for sh in random_share(size, bs, 2)], what
    assert_file(p, pattern_bytes(size, SALT), what)


UNALIGNED_BS, UNALIGNED_SIZE = SBS, 64 * SBS
PREFILL = 0xEE


def unaligned_cfg(p, gpu_ids):
    return files_cfg([p], gpu_ids, UNALIGNED_SIZE, UNALIGNED_BS, 2, verify_salt=SALT,
                     random=True, rand_aligned=False, rand_amount=UNALIGNED_SIZE)


def check_unaligned_random_write(core, root, gpu_ids):
    """Unaligned random WRITE over a file of 0xEE bytes. The offsets come from
    the engine's generator and are not modelled; what the model does state:
    the pattern is a function of the file offset alone, so every byte is
    either untouched or the pattern byte of its offset, and every touched
    byte lies in a run of at least block_size pattern bytes (a byte whose
    pattern value is 0xEE counts for both)."""
    bs, size = UNALIGNED_BS, UNALIGNED_SIZE
    p = root / "f"
    p.write_bytes(bytes([PREFILL]) * size)
    eng = core.Engine(unaligned_cfg(p, gpu_ids))
    eng.prepare()
    res = run_ok(core, eng, "WRITE")
    assert [(r["bytes"], r["iops"]) for r in res] == [(size // 2, size // 2 // bs)] * 2
    got = np.frombuffer(p.read_bytes(), dtype=np.uint8)
    assert got.size == size
    pat = np.frombuffer(pattern_bytes(size, SALT), dtype=np.uint8)
    is_pat, is_pre = got == pat, got == PREFILL
    stray = np.flatnonzero(~(is_pat | is_pre))
    assert stray.size == 0, f"byte {int(stray[0])} is neither untouched nor the pattern"
    touched = is_pat & ~is_pre
    assert bs <= int(touched.sum()) <= size
    # run length of pattern bytes around every position
    edges = np.flatnonzero(np.diff(np.concatenate(([0], is_pat.view(np.int8), [0]))))
    run_len = np.zeros(size, dtype=np.int64)
    for a, b in zip(edges[::2], edges[1::2]):
        run_len[a:b] = b - a
    short = np.flatnonzero(touched & (run_len < bs))
    assert short.size == 0, (f"byte {int(short[0])} was written but its run of pattern bytes "
                             f"is only {int(run_len[short[0]])} long")
    # every worker stayed inside its own half
    for r in range(2):
        assert touched[r * size // 2:(r + 1) * size // 2].any()


def check_unaligned_random_read(core, root, gpu_ids):
    """verifyChecksumCPU names the first bad *byte*, also when the block
    starts inside a word. With one flipped byte at every multiple of bs/2,
    every bs-byte window holds two, so the first block a worker reads fails,
    at the lowest flipped byte at or after its start: a multiple of bs/2
    inside the worker's range. A block that happens to start on a word
    boundary is checked on the GPU instead and reports that same offset (the
    flipped byte is the first of its word) with an even word count."""
    bs, size = UNALIGNED_BS, UNALIGNED_SIZE
    p = root / "f"
    write_pattern_file(core, p, size)
    eng = core.Engine(unaligned_cfg(p, gpu_ids))
    eng.prepare()
    res = run_ok(core, eng, "READ")
    assert [(r["bytes"], r["iops"]) for r in res] == [(size // 2, size // 2 // bs)] * 2
    flip(p, [(o, 1) for o in range(0, size, bs // 2)])
    res = run_phase(core, eng, "READ")
    reports = 0
    for r in res:
        if r["error"] == "interrupted":
            continue
        got = parse_err(r["error"])
        assert got, r["error"]
        off, cnt = got
        lo = r["rank"] * size // 2
        assert off % (bs // 2) == 0 and lo <= off < lo + size // 2, (r["rank"], got)
        assert cnt is None or (gpu_ids and cnt % 2 == 0), (r["rank"], got)
        reports += 1
    assert reports >= 1
    flip(p, [(o, 1) for o in range(0, size, bs // 2)])
    res = run_ok(core, eng, "READ")
    assert [r["bytes"] for r in res] == [size // 2] * 2


def check_verify_direct(core, root, gpu_ids, path_name, fill):
    """verify_direct compares the file against the host buffer that holds the
    D2H copy of the block just written."""
    bs, size = BS, 40 * BS + 8
    what = f"verify_direct {path_name} {fill} gpu={gpu_ids}"
    kw = dict(verify_salt=SALT) if fill[0] == "checksum" else dict(blockvar_pct=fill[1],
                                                                  blockvar_algo=fill[2])
    p = root / "f"
    eng = core.Engine(files_cfg([p], gpu_ids, size, bs, 2, verify_direct=True, **kw,
                                **FILE_PATHS[path_name][0]))
    eng.prepare()
    res = run_ok(core, eng, "WRITE")
    shares = fair_share(size, bs, 2)
    assert [(r["bytes"], r["iops"]) for r in res] == [(s.nbytes, s.num_blocks) for s in shares]
    data = p.read_bytes()
    assert len(data) == size
    if fill[0] == "checksum":
        assert_file(p, pattern_bytes(size, SALT), what)
    elif gpu_ids:  # the CPU refill is not modelled
        for r, sh in enumerate(shares):
            for k in range(sh.num_blocks):
                o = sh.start + k * bs
                want = model_block(fill, r, k, len(data[o:o + bs]))
                if want is not None and data[o:o + bs] != want:
                    raise AssertionError(f"{what}: worker {r} block {k}: "
                                         + first_diff_report(data[o:o + bs], want))


def mix_reads(ops, pct):
    """rwmix_pct without reader threads: an op is a read while reads so far
    are below pct % of the ops so far."""
    reads = 0
    for n in range(ops):
        reads += reads * 100 < n * pct
    return reads


def check_rwmix_file(core, root, gpu_ids, dedicated):
    """rwmix on a pre-written pattern file with verify_salt: writes put the
    pattern back, so the file is unchanged; write bytes + mix-read bytes are
    the whole file. With rwmix_threads=1 worker 0 only reads its fair_share
    slice and verifies it block by block."""
    bs, size = SBS, 80 * SBS
    what = f"rwmix dedicated={dedicated} gpu={gpu_ids}"
    p = root / "f"
    write_pattern_file(core, p, size)
    kw = dict(rwmix_pct=30, rwmix_threads=1) if dedicated else dict(rwmix_pct=30)
    eng = core.Engine(files_cfg([p], gpu_ids, size, bs, 2, verify_salt=SALT, **kw))
    eng.prepare()
    res = run_ok(core, eng, "WRITE")
    assert sum(r["bytes"] + r["rm_bytes"] for r in res) == size, what
    shares = fair_share(size, bs, 2)
    if dedicated:
        assert [(r["bytes"], r["rm_bytes"]) for r in res] == [(0, shares[0].nbytes),
                                                              (shares[1].nbytes, 0)], what
    else:
        for r, sh in zip(res, shares):
            assert r["bytes"] + r["rm_bytes"] == sh.nbytes, what
            assert r["rm_iops"] == mix_reads(sh.num_blocks, 30), (what, r["rm_iops"])
    assert_file(p, pattern_bytes(size, SALT), what)
    if dedicated:
        off = 11 * bs + 16
        flip(p, [(off, 8)])
        res = run_phase(core, eng, "WRITE")
        assert_only_rank_reports(res, 0, (off, 1 if gpu_ids else None), what)
        flip(p, [(off, 8)])
        run_ok(core, eng, "WRITE")
        assert_file(p, pattern_bytes(size, SALT), what)


# ---------------------------------------------------------------------------
# G. lat=True: one latency sample per block, one per entry
# ---------------------------------------------------------------------------

# name -> (phase, block size, blocks per worker, threads, config)
LAT_CASES = {
    "pipelined_write": ("WRITE", BS, 40, 2, dict(iodepth=1, verify_salt=SALT)),
    "batched_read_short_final_batch": ("READ", SBS, 41, 1, dict(iodepth=1)),
    "batched_read_wraps_ring": ("READ", SBS, 2 * (BATCH_BYTES // SBS) + 41, 1, dict(iodepth=1)),
    "per_block_read_verify": ("READ", BS, 40, 2, dict(iodepth=1, verify_salt=SALT)),
    "per_block_read": ("READ", PIPELINE_MIN_BS, 5, 2, dict(iodepth=1)),
    "mmap_write": ("WRITE", BS, 40, 2, dict(mmap=True, verify_salt=SALT)),
    "mmap_read": ("READ", BS, 40, 2, dict(mmap=True, verify_salt=SALT)),
    "uring_read": ("READ", BS, 40, 2, dict(iodepth=DEPTH, verify_salt=SALT)),
}


def assert_one_sample_per_block(res, what):
    for r in res:
        assert r["iops"] > 0 and samples(r) == r["iops"], (
            f"{what}: worker {r['rank']} did {r['iops']} blocks and has {samples(r)} "
            f"latency samples")


def check_lat_file(core, root, gpu_ids, name):
    phase, bs, blocks, threads, kw = LAT_CASES[name]
    size = blocks * threads * bs
    p = root / "f"
    if phase == "READ":
        write_pattern_file(core, p, size)
    eng = core.Engine(files_cfg([p], gpu_ids, size, bs, threads, lat=True, **kw))
    eng.prepare()
    res = run_ok(core, eng, phase)
    assert [r["iops"] for r in res] == [blocks] * threads
    assert_one_sample_per_block(res, f"lat {name} gpu={gpu_ids}")


# (case, tail): tail 0 - a bad word late in every worker's slice, found by a
# GPU check (the accumulating paths find it in their end-of-phase fetch);
# tail 8 - a bad 8-byte tail block, which the last worker's CPU check throws
# on in the middle of its loop
LAT_AFTER_FAILURE = [(n, t) for n in ("per_block_read_verify", "mmap_read", "uring_read")
                     for t in (0, 8)]


def check_lat_after_failed_read(core, root, gpu_ids, name, tail):
    """A READ that fails leaves timed pairs behind that nobody collected; the
    next READ on the same engine must not count them as its own samples."""
    phase, bs, blocks, threads, kw = LAT_CASES[name]
    size = blocks * threads * bs + tail
    want_iops = [blocks] * (threads - 1) + [blocks + (1 if tail else 0)]
    p = root / "f"
    write_pattern_file(core, p, size)
    eng = core.Engine(files_cfg([p], gpu_ids, size, bs, threads, lat=True, **kw))
    eng.prepare()
    if tail:
        spans = [(size - tail, tail)]
    else:
        spans = [((r * blocks + blocks - 3) * bs + 8, 8) for r in range(threads)]
    flip(p, spans)
    res = run_phase(core, eng, "READ")
    assert any(parse_err(r["error"]) for r in res), [r["error"] for r in res]
    flip(p, spans)
    res = run_ok(core, eng, "READ")
    assert [r["iops"] for r in res] == want_iops
    assert_one_sample_per_block(res, f"lat {name} tail={tail} after a failed READ "
                                     f"gpu={gpu_ids}")


LAT_DIR_CASES = [(e, phase) for e in DIR_ENGINES for phase in ("WRITE", "READ")]


def check_lat_dir(core, root, gpu_ids, engine, phase):
    bs, size, files = dir_shape(engine)
    what = f"lat dir {engine} {phase} gpu={gpu_ids}"
    if phase == "READ":
        prewrite_dir(core, root, files, size)
    eng = dir_engine(core, root, gpu_ids, engine, bs, size, files, verify_salt=SALT, lat=True)
    if phase == "WRITE":
        run_ok(core, eng, "MKDIRS")
    res = run_ok(core, eng, phase)
    assert_dir_counts(res, files, size, bs, what)
    assert_one_sample_per_block(res, what)
    for r in res:
        assert r["entries"] == files and samples(r, "entry_lat") == files, (what, r["rank"])
