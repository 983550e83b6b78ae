"""Device CRC-32 / CRC-32C (ebCrcTilesKernel + host fold) on a real MI355X.

Every comparison is an exact 32-bit equality against zlib.crc32 /
core.crc32c of the same bytes.

Sizes key off the kernel's geometry: T = core.gpu_crc_tile_bytes() (one raw
partial CRC per tile), W = core.gpu_crc_wave_bytes() (one wave's share of a
tile). LARGE is the first length at which a workgroup takes a second
grid-stride pass (the grid is capped at 4096 workgroups, one tile each per
pass) plus three more tiles and a 48 B short tile.

Bit flips: at W and T every boundary named below is flipped on its own. At
LARGE there are ~16k wave and tile boundaries and each single flip costs a
64 MiB upload plus a 64 MiB host CRC, so single flips cover the boundaries
that are treated differently by construction (first tile, the tiles on both
sides of the second pass's start, the last full tile, the short tile), and
one more buffer flips a bit on both sides of EVERY wave and tile boundary at
once, so a wrong weight at any of them shows.
"""

import functools
import zlib

import numpy as np
import pytest

from tests import kernel_model as km
from tests.test_crc import start_checking_endpoint
from tests.s3mock import ACCESS_KEY, SECRET_KEY

pytestmark = pytest.mark.gpu

ALGOS = ["CRC32", "CRC32C"]
KINDS = ["pattern", "random", "zero", "ones"]
GRID_CAP = 4096      # gridForBytes
TILES_PER_PASS = 1   # tiles a workgroup takes per grid-stride pass


@pytest.fixture(autouse=True)
def require_gpu(core):
    if core.gpu_device_count() < 1:
        pytest.fail("GPU test run but no HIP device available — the HIP path "
                    "must not silently fall back to CPU")


@functools.lru_cache(maxsize=None)
def geometry():
    from elbencho_amd import load_core
    core = load_core()
    return core.gpu_crc_tile_bytes(), core.gpu_crc_wave_bytes()


def lengths():
    T, W = geometry()
    large = (GRID_CAP * TILES_PER_PASS + 3) * T + 48
    return {"16": 16, "32": 32, "W-16": W - 16, "W": W, "W+16": W + 16,
            "T-16": T - 16, "T": T, "T+16": T + 16, "2T+16": 2 * T + 16,
            "2MiB": 2 << 20, "LARGE": large}


LENGTH_NAMES = ["16", "32", "W-16", "W", "W+16", "T-16", "T", "T+16", "2T+16",
                "2MiB", "LARGE"]


@functools.lru_cache(maxsize=None)
def data(kind: str, n: int) -> bytes:
    if kind == "pattern":
        return km.checksum_pattern(n, 4096, 7)
    if kind == "random":
        return np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    return bytes(n) if kind == "zero" else b"\xff" * n


def oracle(algo: str, buf: bytes) -> int:
    if algo == "CRC32":
        return zlib.crc32(buf) & 0xFFFFFFFF
    from elbencho_amd import load_core
    return load_core().crc32c(buf)


@functools.lru_cache(maxsize=None)
def oracle_cached(algo: str, kind: str, n: int) -> int:
    return oracle(algo, data(kind, n))


def test_geometry(core):
    T, W = geometry()
    assert W % 1024 == 0 and T % W == 0 and T > W


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("name", LENGTH_NAMES)
def test_lengths_and_data(core, name, algo):
    n = lengths()[name]
    assert n % 16 == 0
    for kind in KINDS:
        got = core.gpu_crc(data(kind, n), algo)
        want = oracle_cached(algo, kind, n)
        assert got == want, f"{algo} len={n} ({name}) {kind}: got {got:#010x}, oracle {want:#010x}"


def test_empty(core):
    for algo in ALGOS:
        assert core.gpu_crc(b"", algo) == 0


def boundary_bytes(n: int, every: bool) -> list[int]:
    """Byte positions whose flip is checked: first, last, and the bytes on
    either side of wave and tile boundaries (all of them, or the sample the
    module docstring describes)."""
    T, W = geometry()
    pos = {0, n - 1}
    if every or n <= T:
        bounds = range(W, n, W)  # every wave boundary; tile boundaries are a subset
    else:
        full, last = n // T, T // W
        bounds = [0 * T + W,                       # first wave boundary of all
                  (GRID_CAP - 1) * T + last * W,   # tile boundary where pass 2 starts
                  GRID_CAP * T + W,                # wave boundary in a second-pass tile
                  (full - 1) * T + (last - 1) * W,  # last wave of the last full tile
                  full * T]                        # last full tile | short tile
    for b in bounds:
        if 0 < b < n:
            pos.update((b - 1, b))
    return sorted(pos)


def flipped(buf: bytes, positions, bit: int) -> bytes:
    out = bytearray(buf)
    for p in positions:
        out[p] ^= 1 << bit
    return bytes(out)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("name", ["W", "T"])
def test_single_bit_flips_small(core, name, algo):
    n = lengths()[name]
    base = data("random", n)
    clean = oracle_cached(algo, "random", n)
    for i, p in enumerate(boundary_bytes(n, every=True)):
        buf = flipped(base, [p], i % 8)
        want = oracle(algo, buf)
        assert want != clean
        got = core.gpu_crc(buf, algo)
        assert got == want, f"{algo} len={n}: flip at byte {p}: got {got:#010x}, oracle {want:#010x}"


@pytest.mark.parametrize("algo", ALGOS)
def test_single_bit_flips_large(core, algo):
    n = lengths()["LARGE"]
    base = data("random", n)
    for i, p in enumerate(boundary_bytes(n, every=False)):
        buf = flipped(base, [p], (i * 3) % 8)
        want = oracle(algo, buf)
        got = core.gpu_crc(buf, algo)
        assert got == want, f"{algo} LARGE: flip at byte {p}: got {got:#010x}, oracle {want:#010x}"


@pytest.mark.parametrize("algo", ALGOS)
def test_every_boundary_flipped_large(core, algo):
    n = lengths()["LARGE"]
    buf = flipped(data("random", n), boundary_bytes(n, every=True), 5)
    assert core.gpu_crc(buf, algo) == oracle(algo, buf)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("name", ["16", "W+16", "T-16", "T+16", "2MiB"])
def test_guard_bytes_not_read(core, name, algo):
    """Nothing past len reaches the result: two different sentinels in a
    4 KiB guard behind the data give the oracle's CRC of the data alone."""
    n = lengths()[name]
    want = oracle_cached(algo, "random", n)
    for sentinel in (0xA5, 0x00, 0xFF):
        assert core.gpu_crc(data("random", n), algo, 0, 4096, sentinel) == want


@pytest.mark.parametrize("n", [8, 17, 24, 4096 + 8])
def test_unaligned_length_raises(core, n):
    with pytest.raises(ValueError, match="multiple of 16"):
        core.gpu_crc(bytes(n), "CRC32C")


# ---------------------------------------------------------------------------
# native plane: chunked fill + CRC on one stream, one fetch per object
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("algo", ALGOS)
def test_body_crc_chunks_with_short_tiles(core, algo):
    """max_block = 1 MiB + 16: every chunk ends in a 16 B tile, the body
    ends in a ragged 100 B chunk summed on the host."""
    plane = core.HttpDataPlane("127.0.0.1", 1, 0, (1 << 20) + 16)
    for n, off in [((3 << 20) + 100, 0), ((1 << 20) + 16, 1 << 20), (48, 8), (0, 0)]:
        want = oracle(algo, core.fill_checksum(n, off, 21))
        assert plane.body_crc(n, off, 21, algo) == want, (n, off)
    # unaligned pattern offset: host path of the same plane
    assert plane.body_crc(70000, 3, 21, algo) == oracle(algo, core.fill_checksum(70000, 3, 21))


def test_body_crc_grows_partials(core):
    """More tiles than the partial array starts with (4096): it grows while
    earlier partials of the same object are kept."""
    T, _ = geometry()
    n = (GRID_CAP + 1024) * T
    plane = core.HttpDataPlane("127.0.0.1", 1, 0, 4 << 20)
    assert plane.body_crc(n, 0, 21, "CRC32C") == core.crc32c(km.checksum_pattern(n, 0, 21))
    assert plane.body_crc(n, 0, 21, "CRC32") == \
        zlib.crc32(km.checksum_pattern(n, 0, 21)) & 0xFFFFFFFF


def test_native_put_with_crc32c_on_gpu(core):
    from elbencho_amd.s3 import S3Client

    server, url, handler = start_checking_endpoint()
    try:
        c = S3Client(url, ACCESS_KEY, SECRET_KEY, checksum_algo="CRC32C")
        assert c.attach_native(0, 4 << 20) is True
        c.create_bucket("gchk")
        for key, n in [("a", 4 << 20), ("ragged", (4 << 20) + 24), ("again", 4 << 20)]:
            c.put_object_native("gchk", key, n, 0, 21)
            body = c.get_object("gchk", key)
            assert body == core.fill_checksum(n, 0, 21)
        puts = [s for s in handler.seen if "/gchk/" in s[0]]
        assert len(puts) == 3
        assert all("x-amz-checksum-crc32c" in s[1] for s in puts)
        c.close()
    finally:
        server.shutdown()
        server.server_close()
