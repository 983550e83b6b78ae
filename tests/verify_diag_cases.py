"""Shapes and corruptions shared by the CPU and GPU --verifydiag tests.

A geometry is (len, file_off, block_size, mix_len); block_size 0 is the plain
pattern. corrupted_buffers() yields (name, bytes) for every corruption that
fits the geometry, each built from the clean pattern of the model.

The sizes are the smallest at which a piece of the kernel can go wrong: the
kernel handles 16-byte elements, 64 per wave iteration (1024 bytes), 256 per
workgroup (4096 bytes), and the odd final word on thread 0.
"""

from __future__ import annotations

import re

import numpy as np

from tests import verify_diag_model as dm

SALT = 0x0123456789AB
MIB = 1 << 20

LENS = [8, 16, 24, 1024, 1040, 4096, 4112]
OFFS = [0, 8, (1 << 32) - 8, (1 << 64) - 4096]  # the last one wraps past 2^64
# 16 MiB + 48: one grid-stride wrap past 4096 workgroups x 256 elements, an odd
# final word after it
BIG_LEN = 16 * MIB + 48


def mix_geoms(length: int) -> list:
    """(block_size, mix_len) pairs: plain, then the mix boundaries. A launch
    may not exceed the block, so 4112 bytes get a block of 8192."""
    if length <= 4096:
        return [(0, 0), (4096, 0), (4096, 8), (4096, 2048), (4096, 4088), (4096, 4096)]
    return [(0, 0), (8192, 0), (8192, 8), (8192, 2048), (8192, 4104), (8192, 8192)]


def geometries() -> list:
    """Every len with every mix geometry; the file offsets rotate so that each
    meets each len and each geometry, and 4096/4112 bytes meet all of them
    (file_off 8 makes a 4096-byte launch wrap its 4096-byte block)."""
    out = []
    for i, length in enumerate(LENS):
        for j, (bs, m) in enumerate(mix_geoms(length)):
            offs = OFFS if length >= 4096 else [OFFS[(i + j) % len(OFFS)]]
            for off in offs:
                out.append((length, off, bs, m))
    return out


def geom_id(g) -> str:
    length, off, bs, m = g
    return f"len{length}-off{off:#x}-B{bs}-M{m}"


def clean_words(g) -> np.ndarray:
    length, off, bs, m = g
    return dm.expected_words(length, off, SALT, bs, m).copy()


def _flip(w, idx, *bits):
    for b in bits:
        w[idx] ^= np.uint64(1 << b)


def _clear_bit_in_both(w, i):
    """A bit that is 0 in words i and i+1 (so that setting it adds 2^k to both)."""
    for k in range(63, -1, -1):
        if not (int(w[i]) >> k) & 1 and not (int(w[i + 1]) >> k) & 1:
            return k
    return None


def corrupted_buffers(g):
    """(name, bytes) for every corruption that fits geometry g."""
    length, off, bs, m = g
    n = length // 8
    clean = clean_words(g)

    def emit(name, w):
        return name, w.astype("<u8").tobytes()

    # where the hashed words are, if any: each corruption below is also placed
    # at the first hashed word/element
    pos = np.arange(n, dtype=np.uint64) * np.uint64(8) + np.uint64(off & dm.MASK)
    hashed = (pos % np.uint64(bs) < np.uint64(m)) if bs else np.zeros(n, dtype=bool)
    hashed_idx = np.flatnonzero(hashed)
    plain_idx = np.flatnonzero(~hashed)

    # zeroed run of up to 512 words (a lost 4 KiB page), from word 2 if it fits
    start = 2 if n > 4 else 0
    w = clean.copy()
    w[start:start + 512] = 0
    yield emit("zero_run", w)
    if n >= 1024:  # not aligned to anything: words 37..548
        w = clean.copy()
        w[37:37 + 512] = 0
        yield emit("zero_run_odd_start", w)

    # a block that belongs 4096 bytes further up / down the file
    for shift in (4096, -4096):
        cnt = min(512, n)
        w = clean.copy()
        w[n - cnt:] = dm.expected_words(cnt * 8, (off + (n - cnt) * 8 + shift) % (1 << 64),
                                        SALT, bs, m)
        yield emit(f"block_from_{'above' if shift > 0 else 'below'}", w)

    # the whole buffer written with salt + 5
    yield emit("other_salt", dm.expected_words(length, off, SALT + 5, bs, m).copy())

    # flipped bits: one, two, three; at a plain and at a hashed word
    for kind, idx in (("plain", plain_idx), ("hashed", hashed_idx)):
        if not idx.size:
            continue
        i = int(idx[idx.size // 2])
        for name, bits in (("flip1", (17,)), ("flip2", (0, 63)), ("flip3", (3, 31, 40))):
            w = clean.copy()
            _flip(w, i, *bits)
            yield emit(f"{name}_{kind}", w)
        # bit 3 (value 8) flipped in one word, another bit in its partner: the
        # first looks like "delta 8" alone, the deltas differ, so no PATTERN
        if n >= 2:
            e = min(i // 2, n // 2 - 1)
            w = clean.copy()
            _flip(w, 2 * e, 3)
            _flip(w, 2 * e + 1, 5)
            yield emit(f"flip8_partner_differs_{kind}", w)
            w = clean.copy()
            _flip(w, 2 * e, 3)
            yield emit(f"flip8_partner_good_{kind}", w)
            # the documented ambiguity: the same 0->1 flip in both words
            k = _clear_bit_in_both(clean, 2 * e)
            if k is not None:
                w = clean.copy()
                _flip(w, 2 * e, k)
                _flip(w, 2 * e + 1, k)
                yield emit(f"same_flip_in_pair_{kind}", w)

    # a bad .x alone and a bad .y alone: element 0, lanes 0 and 63 of the
    # first two waves, the first element of the second workgroup, the last
    # element; and the odd tail with a good and a bad predecessor
    nvec = n // 2
    elems = sorted({e for e in (0, 63, 64, 127, 128, 255, 256, nvec - 1) if 0 <= e < nvec})
    for e in elems:
        for half, name in ((0, "x"), (1, "y")):
            w = clean.copy()
            w[2 * e + half] ^= np.uint64(0xA5A5A5A5A5A5A5A5)
            yield emit(f"bad_{name}_elem{e}", w)
    if n & 1:
        w = clean.copy()
        w[n - 1] ^= np.uint64(0xA5A5A5A5A5A5A5A5)
        yield emit("bad_tail", w)
        if n >= 2:
            w = w.copy()
            w[n - 2] ^= np.uint64(0x5A)
            yield emit("bad_tail_and_predecessor", w)
        w = clean.copy()
        w[n - 1] = 0
        yield emit("zero_tail", w)

    # runs that straddle a lane (words 9..10), a wave (127..128 and 120..135)
    # and a workgroup boundary (511..512), and one that ends in the odd tail
    for lo, hi in ((9, 11), (127, 129), (120, 136), (511, 513), (500, 520), (n - 3, n)):
        if 0 <= lo and hi <= n:
            w = clean.copy()
            w[lo:hi] ^= np.uint64(0xFFFF0000FFFF)
            yield emit(f"run_{lo}_{hi}", w)
    # two runs whose second one starts at lane 0 of the second wave with a
    # good predecessor, next to one that has a bad predecessor
    if n > 260:
        w = clean.copy()
        w[128] ^= np.uint64(0x7777)
        w[255:257] ^= np.uint64(0x7777)
        yield emit("runs_at_wave_starts", w)

    # everything bad: garbage
    rng = np.random.default_rng(n * 7 + (off & 0xFFFF) + m)
    yield emit("garbage", rng.integers(1, 1 << 63, size=n, dtype=np.uint64))


# ---------------------------------------------------------------------------
# engine end to end: one corrupted block, the message, its parse
# ---------------------------------------------------------------------------

MSG_RE = re.compile(
    r"Data verification failed( \(GPU\))?\. First bad file offset: (\d+)"
    r"; mismatching 8-byte words: (\d+)"
    r"; diagnosis: last bad file offset: (\d+); runs: (\d+); zero: (\d+); pattern: (\d+)"
    r"; bitflip: (\d+); other: (\d+)"
    r"(?:; pattern delta: (-?\d+)(?:\.\.(-?\d+))?)?"
    r"(?:; flipped bits: 0x([0-9a-f]+))?")


def parse_message(err: str):
    """(on_gpu, first offset as printed, record without 'first') of a
    --verifydiag failure message; the whole message must match."""
    mt = MSG_RE.fullmatch(err)
    assert mt, f"not a --verifydiag failure message: {err!r}"
    g = mt.groups()
    rec = dict(nbad=int(g[2]), last=int(g[3]), runs=int(g[4]), zero=int(g[5]),
               pattern=int(g[6]), bitflip=int(g[7]), other=int(g[8]),
               delta_min=dm.I64_MAX, delta_max=dm.I64_MIN, flip_or=0)
    assert (g[9] is not None) == (rec["pattern"] > 0), err
    assert (g[11] is not None) == (rec["bitflip"] > 0), err
    if g[9] is not None:
        rec["delta_min"] = int(g[9])
        rec["delta_max"] = int(g[10]) if g[10] is not None else int(g[9])
        assert g[10] is None or rec["delta_min"] < rec["delta_max"], err
    if g[11] is not None:
        rec["flip_or"] = int(g[11], 16)
    return g[0] is not None, int(g[1]), rec


def without_first(rec: dict) -> dict:
    return {k: v for k, v in rec.items() if k != "first"}


def corrupt_block(clean: bytes, blk: int, bs: int, m: int, mix: bool) -> bytes:
    """The file `clean` with block `blk` (bs >= 32 KiB) damaged four ways: a
    zeroed 4 KiB page, 4 KiB that belong 4096 bytes further up the file, one
    flipped bit and three flipped bits. With mix, the page from elsewhere lies
    in the hashed part when m allows."""
    assert bs >= 32768 and bs % 4096 == 0
    w = np.frombuffer(clean, dtype="<u8").astype(np.uint64)
    base = blk * bs // 8
    w[base + 1024:base + 1536] = 0                      # bytes 8192..12287 of the block
    src = blk * bs + 16384 + 4096                       # the pattern of 4096 bytes further up
    w[base + 2048:base + 2560] = dm.expected_words(4096, src, SALT, bs if mix else 0, m)
    w[base + 5] ^= np.uint64(1 << 21)
    w[base + 3001] ^= np.uint64((1 << 2) | (1 << 33) | (1 << 60))
    return w.astype("<u8").tobytes()


def first_bad_byte(bad: bytes, clean: bytes) -> int:
    return next(i for i in range(len(bad)) if bad[i] != clean[i])
