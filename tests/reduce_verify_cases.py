"""Case tables and checks for --dedupeverify, written once and run twice:
tests/test_reduce_verify.py runs them on the CPU (bindings and engine with
gpu_ids=[]), tests/test_gpu_reduce_verify.py on the GPU (ebVerifyReduceKernel
through gpu_verify_reduce and the engine with gpu_ids=[0]).

The oracle is tests/reduce_model.py plus the three rules below, written here
from their definition. No expectation is taken from bytes or results that the
code under test produced.

* seeds of a file: poolSeed = mix(salt ^ POOL_XOR),
  uniqSeed = mix(mix(salt ^ UNIQ_XOR) + fileKey * GOLD);
* file key: the path's index in file mode, the file's index in the tree file
  list in custom-tree mode, mix(mix(mix(rank + 1) ^ dir) ^ file) in directory
  mode (r{rank}/d{dir}/r{rank}-f{file});
* a file holds chunks 0, 1, 2, ... of the reduce pattern with those seeds, cut
  at its size: the block at offset o starts with chunk o / C, and every block
  size the option accepts is a multiple of C.
"""

import re

import numpy as np

from tests import reduce_cases as rc
from tests import reduce_model as rm
from tests.test_gpu_engine_exact import SEED, first_diff_report, run_ok, run_phase

MASK = rm.MASK
NONE = (0, MASK)  # the empty verify result
POOL_XOR = 0xA0761D6478BD642F
UNIQ_XOR = 0xE7037ED1A0B428DB
UNIQ, POOL_SEED = rc.UNIQ, rc.POOL_SEED


def seeds(salt: int, file_key: int) -> tuple[int, int]:
    base = int(rm.mix(salt ^ UNIQ_XOR))
    return (int(rm.mix((base + file_key * rm.GOLD) & MASK)), int(rm.mix(salt ^ POOL_XOR)))


def dir_file_key(rank: int, d: int, f: int) -> int:
    return int(rm.mix(int(rm.mix(int(rm.mix(rank + 1)) ^ d)) ^ f))


def flip(data: bytes, *offsets: int, bit: int = 0) -> bytes:
    b = bytearray(data)
    for o in offsets:
        b[o] ^= 1 << bit
    return bytes(b)


# ---------------------------------------------------------------------------
# corruptions of one buffer
# ---------------------------------------------------------------------------

def corruption_cases(c: int, r: int, length: int):
    """(name, byte offsets to flip) in a buffer of `length` >= 3*c + 16 bytes
    with r random bytes per chunk. Whatever a word should hold, one flipped
    bit makes it a bad word, so the expected result follows from the offsets."""
    cases = [
        ("first_word", [0]),
        ("last_word", [length - 3]),
        ("both_words_of_an_element", [2 * c + 16, 2 * c + 24 + 7]),
        ("two_far_apart", [2 * c + 8, c + 8 + 1]),
    ]
    if r:
        cases.append(("last_random_word", [c + r - 1]))
    if r < c:
        cases += [("first_zero_word", [c + r]), ("last_zero_word", [2 * c - 1])]
    return cases


def expected(offsets, file_off):
    words = {o // 8 for o in offsets}
    return (len(words), file_off + 8 * min(words))


def check_corruptions(verify, c, r, length, first, file_off, d=50, p=256):
    """verify(data, file_off, first_chunk, c, r, d, p, uniq=UNIQ) -> (nbad, first)."""
    clean = rc.model(length, first, c, r, d, p)
    assert verify(clean, file_off, first, c, r, d, p) == NONE, (c, r, "clean")
    for name, offs in corruption_cases(c, r, length):
        got = verify(flip(clean, *offs, bit=5), file_off, first, c, r, d, p)
        assert got == expected(offs, file_off), (c, r, name, got)
    if r:
        # the neighbouring chunk sequence: detected, from the first word on
        nbad, at = verify(clean, file_off, first + 1, c, r, d, p)
        assert nbad > 0 and at == file_off, (c, r, "first_chunk + 1", nbad, at)
        # another uniq seed with d = 0: every random word is bad, no zero word is
        clean0 = rc.model(length, first, c, r, 0, p)
        assert verify(clean0, file_off, first, c, r, 0, p) == NONE
        whole, cut = divmod(length, c)
        want = whole * (r // 8) + min(cut, r) // 8
        got = verify(clean0, file_off, first, c, r, 0, p, uniq=UNIQ ^ 1)
        assert got == (want, file_off), (c, r, "other uniq seed", got, want)


# ---------------------------------------------------------------------------
# engine cases
# ---------------------------------------------------------------------------

BS = 65536
MIB = 1 << 20
C = 4096
SALT = 77
D, Z = 50, 50  # dedupe_pct, compress_pct
R = rm.rand_bytes(C, Z)

# name -> (mode, engine config; threads = (write, read))
ENGINE_CASES = {
    # short last block with len % 16 == 0: checked in HBM when there is a GPU
    "file1_tail16": ("file", dict(file_size=MIB + 4112, block_size=BS, threads=(1, 3))),
    # len % 16 != 0: the last block is filled and checked on the CPU
    "file1_tail4": ("file", dict(file_size=MIB + 4100, block_size=BS, threads=(1, 3))),
    "file2": ("file", dict(file_size=MIB + 4112, block_size=BS, threads=(1, 3), paths=2)),
    "file2_random": ("file", dict(file_size=MIB, block_size=BS, threads=(1, 3), paths=2,
                                  random=True)),
    "file2_iodepth4": ("file", dict(file_size=MIB + 4112, block_size=BS, threads=(3, 1), paths=2,
                                    iodepth=4)),
    "file2_mmap": ("file", dict(file_size=MIB + 4112, block_size=BS, threads=(1, 3), paths=2,
                                mmap=True)),
    # more blocks per worker than one verify fetch interval (64)
    "file1_4k_blocks": ("file", dict(file_size=100 * C + 16, block_size=C, threads=(2, 1))),
    "dir_sync": ("dir", dict(file_size=2 * BS + 4112, block_size=BS, files=3, threads=(2, 2))),
    "dir_iodepth4": ("dir", dict(file_size=5 * BS + 4112, block_size=BS, files=2, threads=(2, 2),
                                 iodepth=4)),
    # one block per file and iodepth: the linked small-file chain, files in flight
    "dir_chain": ("dir", dict(file_size=8192, block_size=8192, files=5, threads=(2, 2),
                              iodepth=4)),
    "tree": ("tree", dict(block_size=BS, threads=(2, 2), sharesize=4 * BS)),
    "tree_iodepth4": ("tree", dict(block_size=BS, threads=(2, 2), sharesize=4 * BS, iodepth=4)),
}

TREE_FILES = [("d1/a", BS), ("d1/odd", 3 * BS + 4100), ("big", 9 * BS + 4112), ("b", 2 * BS)]


def engine_cfg(root, name, gpu_ids, phase, salt=SALT, threads=None, **over):
    mode, kw = ENGINE_CASES[name]
    kw = dict(kw)
    tw, tr = kw.pop("threads")
    t = threads or (tw if phase == "WRITE" else tr)
    npaths = kw.pop("paths", 1)
    cfg = dict(threads=t, num_dataset_threads=t, bench_seed=SEED, gpu_ids=list(gpu_ids),
               dedupe_pct=D, compress_pct=Z, dedupe_chunk=C, reduce_verify_salt=salt)
    if mode == "file":
        cfg.update(path_type="file", paths=[str(root / f"f{i}") for i in range(npaths)])
    elif mode == "dir":
        cfg.update(path_type="dir", paths=[str(root)], dirs=1)
    else:
        cfg.update(path_type="dir", paths=[str(root)], tree_dirs=["d1"], tree_files=TREE_FILES)
    cfg.update(kw)
    cfg.update(over)
    return cfg


def expected_files(root, name, salt=SALT):
    """path -> bytes, from the model alone."""
    mode, kw = ENGINE_CASES[name]
    if mode == "file":
        keyed = [(root / f"f{i}", i, kw["file_size"]) for i in range(kw.get("paths", 1))]
    elif mode == "dir":
        keyed = [(root / f"r{r}" / "d0" / f"r{r}-f{f}", dir_file_key(r, 0, f), kw["file_size"])
                 for r in range(kw["threads"][0]) for f in range(kw["files"])]
    else:
        keyed = [(root / rel, i, size) for i, (rel, size) in enumerate(TREE_FILES)]
    return {path: rm.model_fill(size, 0, C, R, D, rm.POOL, *seeds(salt, key))
            for path, key, size in keyed}


def phase(core, cfg, name, ok=True):
    eng = core.Engine(cfg)
    eng.prepare()
    if name == "WRITE" and cfg["path_type"] == "dir":
        run_ok(core, eng, "MKDIRS")
    return run_ok(core, eng, name) if ok else run_phase(core, eng, name)


ERR_RE = re.compile(r"^Data verification failed( \(GPU\))?\. First bad file offset: (\d+); "
                    r"mismatching 8-byte words: (\d+)$")


def verify_errors(res):
    """(on the GPU, offset, count) of every worker that reports a mismatch;
    any other error fails."""
    out = []
    for r in res:
        if not r["error"] or "interrupted" in r["error"].lower():
            continue
        m = ERR_RE.match(r["error"])
        assert m, r["error"]
        out.append((bool(m.group(1)), int(m.group(2)), int(m.group(3))))
    return out


def assert_files(want, what):
    for path, data in want.items():
        got = path.read_bytes()
        assert len(got) == len(data), f"{what}: {path.name} has {len(got)} bytes"
        if got != data:
            raise AssertionError(f"{what}: {path.name}: " + first_diff_report(got, data))


def assert_sharing(want):
    """Files share pool chunks but no unique chunk."""
    files = list(want.values())
    if len(files) < 2:
        return
    dup = rm.is_dup(rm.chunk_numbers(0, max(len(f) for f in files) // C), D)
    pool = set(rc.pool_contents(C, R, rm.POOL, int(rm.mix(SALT ^ POOL_XOR))))
    seen = set()
    for data in files:
        chunks = rc.split_chunks(data[:len(data) // C * C], C)
        assert all(ch in pool for ch, is_d in zip(chunks, dup) if is_d)
        uniq = {ch for ch, is_d in zip(chunks, dup) if not is_d}
        assert not uniq & pool and not uniq & seen, "a unique chunk occurs in two files"
        seen |= uniq


def run_engine_case(core, root, name, write_gpu, read_gpu):
    """Write, compare with the model, read clean (other thread count), read
    with another salt, rewrite with another thread count where the file names
    do not depend on it, then flip one word of the last file and read."""
    mode, kw = ENGINE_CASES[name]
    want = expected_files(root, name)
    what = f"{name} write_gpu={write_gpu} read_gpu={read_gpu}"

    phase(core, engine_cfg(root, name, write_gpu, "WRITE"), "WRITE")
    assert_files(want, what)
    assert_sharing(want)

    res = phase(core, engine_cfg(root, name, read_gpu, "READ"), "READ")
    if not kw.get("random"):
        assert sum(r["bytes"] for r in res) == sum(len(d) for d in want.values()), what

    res = phase(core, engine_cfg(root, name, read_gpu, "READ", salt=SALT + 1, random=False),
                "READ", ok=False)
    errs = verify_errors(res)
    assert errs and all(count > 1 for _, _, count in errs), (what, "other salt", res)

    if mode == "file":  # dir and tree file names and shares depend on the thread count
        tw, tr = kw["threads"]
        phase(core, engine_cfg(root, name, write_gpu, "WRITE", threads=tr + 1), "WRITE")
        assert_files(want, what + " second write")

    # one bad word in the last file, in its last whole 16 B element before the
    # middle: every file and every block before it still verifies
    path, data = list(want.items())[-1]
    at = (len(data) // 2) // 16 * 16 + 8
    path.write_bytes(flip(data, at + 3))
    res = phase(core, engine_cfg(root, name, read_gpu, "READ", random=False), "READ", ok=False)
    errs = verify_errors(res)
    assert [(off, count) for _, off, count in errs] == [(at, 1)], (what, res)
    block_len = min(kw["block_size"], len(data) - at // kw["block_size"] * kw["block_size"])
    assert errs[0][0] == (bool(read_gpu) and block_len % 16 == 0), (what, res)
