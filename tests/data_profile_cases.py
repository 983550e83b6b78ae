"""The cases of --dataprofile, shared by tests/test_data_profile.py (CPU) and
tests/test_gpu_data_profile.py (MI355X): the kernel case table, and engine
runs through the command line whose JSON profile is compared with the model
(tests/data_profile_model.py) over the bytes of the files.
"""

import base64
import functools
import json
import os

import numpy as np

from tests import data_profile_model as dm

CHUNKS = (512, 4096, 65536)
LENS = (1, 7, 8, 9, 15, 16, 17, 511, 512, 513, 520, 4096, 4096 + 520 + 3, 3 * 4096, 1 << 20)
CONTENTS = ("zeros", "verify", "random", "reduce", "last_byte", "last_real_byte")

MAX_LEN = max(LENS)
FILE_SIZE = 8 * (1 << 20) + 4096 + 523  # the engine file: a 523-byte last chunk


@functools.lru_cache(maxsize=None)
def _base(core, kind):
    """MAX_LEN bytes of each content, made once."""
    if kind == "zeros":
        return bytes(MAX_LEN)
    if kind == "verify":
        return core.fill_checksum(MAX_LEN, 0, 7)
    if kind == "random":
        return np.random.default_rng(20240229).bytes(MAX_LEN)
    if kind == "reduce":  # --dedupepct 50 --compresspct 50 at 4 KiB chunks
        return core.fill_reduce(MAX_LEN, 0, 4096, 2048, 50, core.REDUCE_POOL_CHUNKS, 42, 43)
    raise KeyError(kind)


def content(core, kind, length):
    if kind == "last_byte":  # zeros with only the last byte set
        return bytes(length - 1) + b"\x01"
    if kind == "last_real_byte":
        # zeros whose only set byte is the last real byte before a padded
        # word: with length % 8 != 0 that is the last byte, else (no padding
        # in the last word) the last byte of the word before
        buf = bytearray(length)
        buf[length - 1 if length % 8 else max(length - 9, 0)] = 0x80
        return bytes(buf)
    return _base(core, kind)[:length]


@functools.lru_cache(maxsize=None)
def expected(core, kind, length, chunk):
    """The model's profile of a case, computed once for CPU and GPU tests."""
    return dm.profile(content(core, kind, length), chunk)


def case_table():
    return [(c, n, k) for c in CHUNKS for n in LENS for k in CONTENTS]


def assert_same(got, want, what):
    for key in ("chunks", "bytes", "zero_chunks"):
        assert got[key] == want[key], (what, key, got[key], want[key])
    assert list(got["hist"]) == list(want["hist"]), (what, "hist")
    if bytes(got["regs"]) != bytes(want["regs"]):
        bad = [(i, a, b) for i, (a, b) in enumerate(zip(got["regs"], want["regs"])) if a != b]
        raise AssertionError((what, "regs", len(bad), bad[:8]))


# ---------------------------------------------------------------------------
# engine runs through the command line
# ---------------------------------------------------------------------------

def run_cli(argv):
    from elbencho_amd.__main__ import main
    return main(list(argv) + ["--nolive"])


def json_docs(path):
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]


def profile_of_doc(doc):
    """The dataProfile object of a phase's JSON document, in binding form."""
    p = doc["dataProfile"]
    return {"chunks": p["chunks"], "bytes": p["bytes"], "zero_chunks": p["zeroChunks"],
            "hist": p["byteHistogram"], "regs": base64.b64decode(p["registers"])}


def read_profiles(tmp_path, argv, tag):
    """Run a read with --dataprofile and return the profiles of its READ
    phases (binding form) and the JSON documents."""
    out = os.path.join(str(tmp_path), f"res_{tag}.json")
    rc = run_cli(["-r", "--dataprofile", "--jsonfile", out] + list(argv))
    assert rc == 0, (tag, rc)
    docs = [d for d in json_docs(out) if d["phase_type"] == "READ"]
    return [profile_of_doc(d) for d in docs], docs


def write_reduce_file(tmp_path, gpu_args=()):
    """The engine file: FILE_SIZE bytes with --dedupepct 50 --compresspct 50."""
    path = os.path.join(str(tmp_path), "f")
    rc = run_cli(["-w", "-s", str(FILE_SIZE), "-b", "1m", "--dedupepct", "50",
                  "--compresspct", "50", "--dedupechunk", "4K", *gpu_args, path])
    assert rc == 0
    with open(path, "rb") as f:
        data = f.read()
    assert len(data) == FILE_SIZE
    return path, data


DIR_ARGS = ["-t", "2", "-n", "2", "-N", "3", "-s", "68k", "-b", "64k"]


def write_dir_files(tmp_path, extra=()):
    """Dir mode, 2 threads x 2 dirs x 3 files of 68 KiB (blocks of 64 KiB and
    4 KiB). Returns the directory and the model over all files."""
    root = os.path.join(str(tmp_path), "d")
    os.makedirs(root, exist_ok=True)
    rc = run_cli(["-d", "-w", *DIR_ARGS, "--dedupepct", "50", "--compresspct", "50", *extra,
                  root])
    assert rc == 0
    return root, model_over_tree(root, 4096)


def model_over_tree(root, chunk):
    want = dm.empty()
    count = 0
    for dirpath, _, files in sorted(os.walk(root)):
        for name in sorted(files):
            with open(os.path.join(dirpath, name), "rb") as f:
                want = dm.merge(want, dm.profile(f.read(), chunk))
            count += 1
    assert count, "no files written"
    return want
