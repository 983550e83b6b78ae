"""Device CRC-64/NVME (ebCrc64TilesKernel + host fold) on a real MI355X.

Every comparison is an exact 64-bit equality against
core.crc(buf, "CRC64NVME") of the same bytes; tests/test_crc64.py ties that
to the bit-serial model.

Sizes key off the kernel's geometry, asked for with algo="CRC64NVME":
T = core.gpu_crc_tile_bytes (one raw partial CRC per tile),
W = core.gpu_crc_wave_bytes (one wave's share of a tile). LARGE is the first
length at which a workgroup takes a second grid-stride pass (the grid is
capped at 4096 workgroups, one tile each per pass) plus three more tiles and
a 48 B short tile: 128 MiB at a 32 KiB tile.

Bit flips: at W and T every boundary named below is flipped on its own. At
LARGE each single flip costs an upload and a host CRC of the whole buffer,
so single flips cover the boundaries that are treated differently by
construction (first tile, the tiles on both sides of the second pass's
start, the last full tile, the short tile), one test case each, and one
more buffer flips a bit on both sides of EVERY wave and tile boundary at
once, so a wrong weight at any of them shows.
"""

import functools

import pytest

from tests.s3mock import ACCESS_KEY, SECRET_KEY
from tests.test_crc64 import (ALGO, GRID_CAP, HEADER, KINDS, SMALL_NAMES, data, geometry,
                              lengths, start_crc64_endpoint)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def require_gpu(core):
    if core.gpu_device_count() < 1:
        pytest.fail("GPU test run but no HIP device available — the HIP path "
                    "must not silently fall back to CPU")


def oracle(buf: bytes) -> int:
    from elbencho_amd import load_core
    return load_core().crc(buf, ALGO)


@functools.lru_cache(maxsize=None)
def oracle_cached(kind: str, n: int) -> int:
    return oracle(data(kind, n))


def test_geometry(core):
    T, W = geometry()
    assert W % 1024 == 0 and T % W == 0 and T > W


@pytest.mark.parametrize("name", SMALL_NAMES)
def test_lengths_and_data(core, name):
    n = lengths()[name]
    assert n % 16 == 0
    for kind in KINDS:
        got = core.gpu_crc(data(kind, n), ALGO)
        want = oracle_cached(kind, n)
        assert got == want, f"len={n} ({name}) {kind}: got {got:#018x}, oracle {want:#018x}"


@pytest.mark.parametrize("kind", ["random", "pattern"])
def test_large(core, kind):
    n = lengths()["LARGE"]
    assert n % 16 == 0
    got = core.gpu_crc(data(kind, n), ALGO)
    want = oracle_cached(kind, n)
    assert got == want, f"LARGE {kind}: got {got:#018x}, oracle {want:#018x}"


def test_empty(core):
    assert core.gpu_crc(b"", ALGO) == 0


def large_boundaries() -> list[int]:
    """The five structurally distinct boundaries of LARGE."""
    T, W = geometry()
    n = lengths()["LARGE"]
    full, last = n // T, T // W
    return [0 * T + W,                        # first wave boundary of all
            (GRID_CAP - 1) * T + last * W,    # tile boundary where pass 2 starts
            GRID_CAP * T + W,                 # wave boundary in a second-pass tile
            (full - 1) * T + (last - 1) * W,  # last wave of the last full tile
            full * T]                         # last full tile | short tile


def boundary_bytes(n: int, bounds) -> list[int]:
    """First and last byte, and the bytes on either side of each boundary."""
    pos = {0, n - 1}
    for b in bounds:
        if 0 < b < n:
            pos.update((b - 1, b))
    return sorted(pos)


def flipped(buf: bytes, positions, bit: int) -> bytes:
    out = bytearray(buf)
    for p in positions:
        out[p] ^= 1 << bit
    return bytes(out)


@pytest.mark.parametrize("name", ["W", "T"])
def test_single_bit_flips_small(core, name):
    _, W = geometry()
    n = lengths()[name]
    base = data("random", n)
    clean = oracle_cached("random", n)
    # every wave boundary; tile boundaries are a subset
    for i, p in enumerate(boundary_bytes(n, range(W, n, W))):
        buf = flipped(base, [p], i % 8)
        want = oracle(buf)
        assert want != clean
        got = core.gpu_crc(buf, ALGO)
        assert got == want, f"len={n}: flip at byte {p}: got {got:#018x}, oracle {want:#018x}"


@pytest.mark.parametrize("which", range(5))
def test_single_bit_flips_large(core, which):
    n = lengths()["LARGE"]
    b = large_boundaries()[which]
    assert 0 < b < n
    ends = {0: [0], 4: [n - 1]}.get(which, [])  # first and last byte ride along
    for i, p in enumerate([b - 1, b] + ends):
        buf = flipped(data("random", n), [p], (which + i * 3) % 8)
        want = oracle(buf)
        got = core.gpu_crc(buf, ALGO)
        assert got == want, f"LARGE: flip at byte {p}: got {got:#018x}, oracle {want:#018x}"


def test_every_boundary_flipped_large(core):
    _, W = geometry()
    n = lengths()["LARGE"]
    buf = flipped(data("random", n), boundary_bytes(n, range(W, n, W)), 5)
    assert core.gpu_crc(buf, ALGO) == oracle(buf)


@pytest.mark.parametrize("name", ["16", "W+16", "T-16", "T+16"])
def test_guard_bytes_not_read(core, name):
    """Nothing past len reaches the result: three different sentinels in a
    4 KiB guard behind the data give the oracle's CRC of the data alone."""
    n = lengths()[name]
    want = oracle_cached("random", n)
    for sentinel in (0xA5, 0x00, 0xFF):
        assert core.gpu_crc(data("random", n), ALGO, 0, 4096, sentinel) == want


@pytest.mark.parametrize("n", [8, 17, 24, 4096 + 8])
def test_unaligned_length_raises(core, n):
    with pytest.raises(ValueError, match="multiple of 16"):
        core.gpu_crc(bytes(n), ALGO)


def test_alternating_with_crc32c_on_one_context(core):
    """The two kernels keep separate tables and partials on a context."""
    T, _ = geometry()
    for n in (T + 16, 3 * T + 48):
        buf = data("random", n)
        want = (core.crc32c(buf), oracle(buf))
        assert core.gpu_crc_interleaved(buf, 3) == [want] * 3
    # and through a plane, whose body_crc calls share its one context
    plane = core.HttpDataPlane("127.0.0.1", 1, 0, 1 << 20)
    body = core.fill_checksum((2 << 20) + 32, 0, 21)
    for _ in range(2):
        assert plane.body_crc(len(body), 0, 21, "CRC32C") == core.crc32c(body)
        assert plane.body_crc(len(body), 0, 21, ALGO) == oracle(body)


# ---------------------------------------------------------------------------
# native plane: chunked fill + CRC on one stream, one fetch per object
# ---------------------------------------------------------------------------

def test_body_crc_chunks_with_short_tiles(core):
    """max_block = 1 MiB + 16: every chunk ends in a 16 B tile, the body
    ends in a ragged 100 B chunk summed on the host."""
    plane = core.HttpDataPlane("127.0.0.1", 1, 0, (1 << 20) + 16)
    for n, off in [((3 << 20) + 100, 0), ((1 << 20) + 16, 1 << 20), (48, 8), (0, 0)]:
        want = oracle(core.fill_checksum(n, off, 21))
        assert plane.body_crc(n, off, 21, ALGO) == want, (n, off)
    # unaligned pattern offset: host path of the same plane
    assert plane.body_crc(70000, 3, 21, ALGO) == oracle(core.fill_checksum(70000, 3, 21))


def test_body_crc_grows_partials(core):
    """More tiles than the partial array starts with (4096): it grows while
    earlier partials of the same object are kept."""
    T, _ = geometry()
    n = (4096 + 1024) * T
    plane = core.HttpDataPlane("127.0.0.1", 1, 0, 4 << 20)
    assert plane.body_crc(n, 0, 21, ALGO) == oracle(core.fill_checksum(n, 0, 21))


def test_native_put_with_crc64nvme_on_gpu(core):
    from elbencho_amd.s3 import S3Client

    server, url, handler = start_crc64_endpoint()
    try:
        c = S3Client(url, ACCESS_KEY, SECRET_KEY, checksum_algo=ALGO)
        assert c.attach_native(0, 4 << 20) is True
        c.create_bucket("gchk")
        for key, n in [("a", 4 << 20), ("ragged", (4 << 20) + 24), ("again", 4 << 20)]:
            c.put_object_native("gchk", key, n, 0, 21)
            body = c.get_object("gchk", key)
            assert body == core.fill_checksum(n, 0, 21)
        puts = [s for s in handler.seen if "/gchk/" in s[0]]
        assert len(puts) == 3
        assert all(HEADER in s[1] for s in puts)
        c.close()
    finally:
        server.shutdown()
        server.server_close()


def test_cli_write_phase_with_gpuids(core):
    """--s3chksumalgo CRC64NVME --gpuids 0: a write phase on the native plane
    whose every body passes the checking endpoint."""
    from elbencho_amd.cli import main

    server, url, handler = start_crc64_endpoint()
    try:
        rc = main(["--s3endpoints", url, "--s3key", ACCESS_KEY, "--s3secret", SECRET_KEY,
                   "--nolive", "-d", "-w", "-t", "2", "-N", "2", "-s", "4m", "-b", "2m",
                   "--gpuids", "0", "--s3chksumalgo", "CRC64NVME", "s3://gcli64"])
        assert rc == 0
        sent = [s for s in handler.seen if "/gcli64/" in s[0]]
        assert len(sent) == 2 * 2 * 2  # threads x objects x parts
        assert all(HEADER in s[1] for s in sent)
        assert core.http_dataplane_live() == 0
    finally:
        server.shutdown()
        server.server_close()
