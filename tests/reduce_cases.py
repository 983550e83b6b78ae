"""Case tables and checks for --dedupepct / --compresspct, written once and run
twice: tests/test_reduce.py runs them on the CPU (bindings and engine with
gpu_ids=[]), tests/test_gpu_reduce.py on the GPU (ebFillReduceKernel through
gpu_fill_reduce and the engine with gpu_ids=[0]).

The oracle is tests/reduce_model.py. No expectation is taken from bytes the
code under test produced.

Rules of the engine that the expected files rely on, each stated once:

* a worker numbers its chunks 0, 1, 2, ... from the start of a phase; every
  block it fills takes the next ceil(len / C) numbers, in the order in which
  it issues the blocks, whatever file or offset a block goes to; a block whose
  length is no multiple of C ends with a cut chunk;
* sequential file mode deals blocks out by fair_share; --backward issues a
  slice's blocks last first, the short tail block (if any) before the others;
* directory mode: worker r owns r{r}/d0/r{r}-f{0..files-1}, in that order;
* the seeds are reduce_seeds(bench_seed, phase_seq, rank), with phase_seq read
  from the engine (MKDIRS counts as a phase).
"""

import itertools

import numpy as np

from tests import reduce_model as rm
from tests.test_gpu_engine_exact import SEED, fair_share, first_diff_report, run_ok

UNIQ, POOL_SEED = 0x0123456789ABCDEF, 0xFEDCBA9876543210

# ---------------------------------------------------------------------------
# the fill itself: (C, R, d, P, first_chunk, len)
# ---------------------------------------------------------------------------

CHUNKS = (16, 64, 4096)
PCTS = (0, 1, 33, 50, 99, 100)
POOLS = (1, 3, 256)
FIRST_CHUNKS = (0, 99, 2**32 - 1, 2**40 + 7)  # the last two: a 64-bit product in dup()


def rands(c):
    return sorted({0, 16, c - 16, c})


def lens(c):
    return sorted({0, 1, 7, 16, c - 8, c, c + 16, 3 * c + 5})


def grid(c, d, gpu=False):
    """Every (R, P, first_chunk, len) of the grid for one (C, d); gpu=True
    keeps the lengths the kernel takes (multiples of 16)."""
    ls = [n for n in lens(c) if not gpu or n % 16 == 0]
    return itertools.product(rands(c), POOLS, FIRST_CHUNKS, ls)


def model(length, first, c, r, d, p):
    return rm.model_fill(length, first, c, r, d, p, UNIQ, POOL_SEED)


def split_chunks(data, c):
    return [data[o:o + c] for o in range(0, len(data), c)]


def pool_contents(c, r, p, pool_seed):
    """The p chunk contents of the pool, each from its key alone."""
    keys = rm.mix(np.uint64(pool_seed) + np.arange(p, dtype=np.uint64))
    i = np.arange(c // 8, dtype=np.uint64)
    words = rm.mix(keys[:, None] + i[None, :] * np.uint64(rm.GOLD))
    words[:, i * np.uint64(8) >= np.uint64(r)] = 0
    return [row.astype("<u8").tobytes() for row in words]


def check_properties(data, n_chunks, first, c, r, d, p, what):
    """Properties of n_chunks whole chunks starting at chunk `first`."""
    assert len(data) == n_chunks * c, what
    chunks = split_chunks(data, c)
    n = rm.chunk_numbers(first, n_chunks)
    dup = rm.is_dup(n, d)
    if first == 0:  # exactly floor(N*d/100) of the first N chunks, for every N
        want = np.arange(1, n_chunks + 1) * d // 100
        assert np.array_equal(np.cumsum(dup), want), what
    pool = pool_contents(c, r, p, POOL_SEED)
    members = rm.pool_member(n, p, UNIQ)
    uniq = []
    for k, ch in enumerate(chunks):
        assert ch[r:] == bytes(c - r), f"{what}: chunk {k} is not zero from byte {r} on"
        if dup[k]:  # the pool content that its number selects
            assert ch == pool[int(members[k])], f"{what}: chunk {k} is not its pool chunk"
        else:
            uniq.append(ch)
    assert len(uniq) == n_chunks - int(dup.sum()), what
    if r:  # with R = 0 every chunk is all zeros
        assert len(set(uniq)) == len(uniq), f"{what}: unique chunks repeat"
        assert not set(uniq) & set(pool), f"{what}: a unique chunk equals a pool chunk"


# geometry that fill_reduce and gpu_fill_reduce must refuse:
# (chunk, rand_bytes, dedupe_pct, pool)
BAD_GEOMETRY = [
    (0, 0, 50, 256), (8, 0, 50, 256), (48, 16, 50, 256), (4095, 16, 50, 256),  # C
    (4096, 4112, 50, 256), (4096, 8, 50, 256), (4096, 4088, 50, 256),          # R
    (4096, 2048, -1, 256), (4096, 2048, 101, 256),                            # d
    (4096, 2048, 50, 0),                                                      # P
]


# ---------------------------------------------------------------------------
# engine cases
# ---------------------------------------------------------------------------

BS = 65536
MIB = 1 << 20
C = 4096

# name -> (mode, engine config, dedupe_pct, compress_pct)
ENGINE_CASES = {
    # short last block: len % 16 == 0 but len % C != 0
    "seq_tail16": ("file", dict(file_size=MIB + 4112, block_size=BS), 50, 50),
    # len % 16 != 0: the tail block is filled on the CPU also when there is a GPU
    "seq_tail4": ("file", dict(file_size=MIB + 4100, block_size=BS), 50, 50),
    "two_threads": ("file", dict(file_size=MIB + 4112, block_size=BS, threads=2), 33, 25),
    "backward": ("file", dict(file_size=MIB + 4112, block_size=BS, backward=True), 50, 50),
    "iodepth4": ("file", dict(file_size=MIB + 4112, block_size=BS, iodepth=4), 75, 0),
    "mmap": ("file", dict(file_size=MIB + 4112, block_size=BS, mmap=True), 0, 75),
    # 3 files of 8K per thread: one block each; with iodepth the small-file chain
    "dir_sync": ("dir", dict(file_size=8192, block_size=8192, files=3, threads=2), 50, 50),
    "dir_chain": ("dir", dict(file_size=8192, block_size=8192, files=3, threads=2,
                              iodepth=4), 50, 50),
    # blocks smaller than a chunk: every block is one cut chunk
    "bs_1k": ("file", dict(file_size=64 * 1024 + 16, block_size=1024), 50, 50),
}


def engine_cfg(root, mode, gpu_ids, d, c, **kw):
    threads = kw.pop("threads", 1)
    cfg = dict(path_type=mode, threads=threads, num_dataset_threads=threads, bench_seed=SEED,
               gpu_ids=list(gpu_ids), dedupe_pct=d, compress_pct=c, dedupe_chunk=C)
    if mode == "dir":
        cfg.update(paths=[str(root)], dirs=1)
    else:
        cfg.update(paths=[str(root / "f")])
    cfg.update(kw)
    return cfg


def worker_ops(root, cfg):
    """Per worker, the (path, offset, length) of the blocks it fills, in order."""
    size, bs, threads = cfg["file_size"], cfg["block_size"], cfg["threads"]
    if cfg["path_type"] == "dir":
        return [[(root / f"r{r}" / "d0" / f"r{r}-f{f}", o, min(bs, size - o))
                 for f in range(cfg["files"]) for o in range(0, size, bs)]
                for r in range(threads)]
    out = []
    for sh in fair_share(size, bs, threads):
        ops = [(root / "f", sh.start + k * bs, min(bs, sh.start + sh.nbytes - (sh.start + k * bs)))
               for k in range(sh.num_blocks)]
        out.append(ops[::-1] if cfg.get("backward") else ops)
    return out


def expected_files(core, root, cfg, phase_seq):
    """path -> bytes, from the model alone."""
    r_bytes = rm.rand_bytes(cfg["dedupe_chunk"], cfg["compress_pct"])
    files = {}
    for rank, ops in enumerate(worker_ops(root, cfg)):
        uniq, pool = core.reduce_seeds(cfg["bench_seed"], phase_seq, rank)
        assert (uniq, pool) == rm.seeds(cfg["bench_seed"], phase_seq, rank)
        n = 0
        for path, off, length in ops:
            buf = files.setdefault(path, bytearray(cfg["file_size"]))
            buf[off:off + length] = rm.model_fill(length, n, cfg["dedupe_chunk"], r_bytes,
                                                  cfg["dedupe_pct"], rm.POOL, uniq, pool)
            n += -(-length // cfg["dedupe_chunk"])
    return {p: bytes(b) for p, b in files.items()}


def assert_files(want, what):
    for path, data in want.items():
        got = path.read_bytes()
        assert len(got) == len(data), f"{what}: {path.name} has {len(got)} bytes"
        if got != data:
            raise AssertionError(f"{what}: {path.name}: " + first_diff_report(got, data))


def run_engine_case(core, root, gpu_ids, name):
    mode, kw, d, c = ENGINE_CASES[name]
    cfg = engine_cfg(root, mode, gpu_ids, d, c, **kw)
    eng = core.Engine(cfg)
    eng.prepare()
    assert eng.phase_seq == 0
    if mode == "dir":
        run_ok(core, eng, "MKDIRS")
    res = run_ok(core, eng, "WRITE")
    ops = worker_ops(root, cfg)
    assert [(r["bytes"], r["iops"]) for r in res] == [
        (sum(o[2] for o in w), len(w)) for w in ops], name
    assert eng.phase_seq == (2 if mode == "dir" else 1)
    assert_files(expected_files(core, root, cfg, eng.phase_seq), f"{name} gpu={gpu_ids}")


def run_two_phases(core, root, gpu_ids):
    """Two WRITE phases on one Engine: each file image equals the model with
    that phase's seeds; unique chunks all differ between the phases, pool
    chunks come from the same 256 contents."""
    size, d, c = 256 * 1024, 50, 50
    cfg = engine_cfg(root, "file", gpu_ids, d, c, file_size=size, block_size=BS)
    eng = core.Engine(cfg)
    eng.prepare()
    images = []
    for seq in (1, 2):
        run_ok(core, eng, "WRITE")
        assert eng.phase_seq == seq
        want = expected_files(core, root, cfg, seq)
        assert_files(want, f"phase {seq} gpu={gpu_ids}")
        images.append(want[root / "f"])
    assert core.reduce_seeds(SEED, 1, 0)[1] == core.reduce_seeds(SEED, 2, 0)[1]
    assert core.reduce_seeds(SEED, 1, 0)[0] != core.reduce_seeds(SEED, 2, 0)[0]
    r_bytes = rm.rand_bytes(C, c)
    pool_seed = core.reduce_seeds(SEED, 1, 0)[1]
    pool = set(pool_contents(C, r_bytes, rm.POOL, pool_seed))
    assert len(pool) == rm.POOL
    dup = rm.is_dup(rm.chunk_numbers(0, size // C), d)
    uniq = []
    for img in images:
        chunks = split_chunks(img, C)
        assert all(ch in pool for ch, is_d in zip(chunks, dup) if is_d)
        uniq.append({ch for ch, is_d in zip(chunks, dup) if not is_d})
        assert len(uniq[-1]) == int((~dup).sum()) and not uniq[-1] & pool
    assert not uniq[0] & uniq[1], "unique chunks of the two phases must differ"
