"""Pure-Python/numpy model of --dataprofile (the definitions of
elbencho_amd/csrc/dataprofile.h and docs/usage.md, "Data profile"), written
from those definitions alone. profile() returns the dict that the bindings
return: {"chunks", "bytes", "zero_chunks", "hist": [256 ints], "regs": bytes}.
"""

import numpy as np

MASK = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
HLL_P = 14
HLL_M = 1 << HLL_P
RHO_MAX = 64 - HLL_P + 1


def mix(x):
    """The splitmix64 step on an int or a numpy uint64 array (wrapping)."""
    if isinstance(x, np.ndarray):
        with np.errstate(over="ignore"):
            z = x + np.uint64(GOLD)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            return z ^ (z >> np.uint64(31))
    z = (x + GOLD) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def clz64(v):
    """Leading zeros of the non-zero uint64 values in v."""
    v = v.copy()
    n = np.zeros(v.shape, dtype=np.uint64)
    for shift in (32, 16, 8, 4, 2, 1):
        small = (v >> np.uint64(64 - shift)) == 0
        n[small] += np.uint64(shift)
        v[small] <<= np.uint64(shift)
    return n


def registers_of(fps):
    """The sketch after the uint64 fingerprints fps: 16384 uint8 registers."""
    fps = np.asarray(fps, dtype=np.uint64)
    idx = (fps >> np.uint64(64 - HLL_P)).astype(np.int64)
    rest = fps << np.uint64(HLL_P)
    rho = np.full(fps.shape, RHO_MAX, dtype=np.uint64)
    nz = rest != 0
    rho[nz] = clz64(rest[nz]) + np.uint64(1)
    regs = np.zeros(HLL_M, dtype=np.uint8)
    np.maximum.at(regs, idx, rho.astype(np.uint8))
    return regs


def chunk_words(chunk_bytes):
    """ceil(n/8) little-endian u64 words, the last one zero-padded."""
    n = len(chunk_bytes)
    padded = chunk_bytes + bytes(-n % 8)
    return np.frombuffer(padded, dtype="<u8")


def fingerprint(chunk_bytes):
    """fp of one chunk: mix((sum_i mix(w_i + GOLD*(i+1))) ^ n)."""
    w = chunk_words(chunk_bytes)
    with np.errstate(over="ignore"):
        i1 = np.arange(1, len(w) + 1, dtype=np.uint64)
        s = int(np.sum(mix(w + np.uint64(GOLD) * i1), dtype=np.uint64)) if len(w) else 0
    return mix(s ^ len(chunk_bytes))


def empty():
    return {"chunks": 0, "bytes": 0, "zero_chunks": 0, "hist": [0] * 256,
            "regs": bytes(HLL_M)}


def profile(data, chunk):
    """Profile of one block: chunks cut by position in the block."""
    data = bytes(data)
    n = len(data)
    if not n:
        return empty()
    fps = []
    zero_chunks = 0
    full = n // chunk
    if full:
        w = np.frombuffer(data[:full * chunk], dtype="<u8").reshape(full, chunk // 8)
        with np.errstate(over="ignore"):
            i1 = np.arange(1, chunk // 8 + 1, dtype=np.uint64)
            s = np.sum(mix(w + np.uint64(GOLD) * i1), axis=1, dtype=np.uint64)
            fps.extend(mix(s ^ np.uint64(chunk)).tolist())
        zero_chunks += int(np.count_nonzero(~w.any(axis=1)))
    if n % chunk:
        tail = data[full * chunk:]
        fps.append(fingerprint(tail))
        zero_chunks += not any(tail)
    hist = np.bincount(np.frombuffer(data, dtype=np.uint8), minlength=256)
    return {"chunks": len(fps), "bytes": n, "zero_chunks": zero_chunks,
            "hist": [int(v) for v in hist],
            "regs": registers_of(np.array(fps, dtype=np.uint64)).tobytes()}


def merge(a, b):
    return {"chunks": a["chunks"] + b["chunks"], "bytes": a["bytes"] + b["bytes"],
            "zero_chunks": a["zero_chunks"] + b["zero_chunks"],
            "hist": [x + y for x, y in zip(a["hist"], b["hist"])],
            "regs": bytes(map(max, a["regs"], b["regs"]))}


def profile_blocks(blocks, chunk):
    out = empty()
    for b in blocks:
        out = merge(out, profile(b, chunk))
    return out


def profile_file(data, chunk, block):
    """A file read in blocks of `block` bytes (a multiple of chunk): the same
    as profile(data, chunk); stated with the blocks to say so."""
    return profile_blocks([data[o:o + block] for o in range(0, len(data), block)], chunk)
