"""CRC-64/NVME (--s3chksumalgo CRC64NVME) without a GPU: the host library
(csrc/crc64.h), the host emulation of the device tile kernel, the native S3
plane's checksummed PUT, config and the Python client.

Oracle: tests/crc64_model.py, a bit-serial model written from the
checksum's parameters. It is slow, so long inputs are tied to it through
core.crc, which the model checks at every length 0-70 and a few above.

The plane tests run against a checking endpoint: the SigV4 mock, extended to
recompute the CRC-64/NVME of every object/part body it receives, to answer
400 when x-amz-checksum-crc64nvme is missing, wrong or unsigned, and to
record the headers of multipart initiations.
"""

import base64
import functools
import struct
import threading
from http.server import ThreadingHTTPServer

import numpy as np
import pytest

from elbencho_amd.s3 import S3Client, S3Error

from tests import crc64_model as model
from tests import kernel_model as km
from tests.s3mock import ACCESS_KEY, SECRET_KEY, S3Handler, S3Store

ALGO = "CRC64NVME"
HEADER = "x-amz-checksum-crc64nvme"
GRID_CAP = 4096      # gridForBytes: the launch in crc64DevAsync
TILES_PER_PASS = 1   # tiles a workgroup takes per grid-stride pass


@functools.lru_cache(maxsize=None)
def rand_bytes(n: int, seed: int = 1) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


# ---------------------------------------------------------------------------
# lengths and data shared with tests/test_gpu_crc64.py
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def geometry():
    from elbencho_amd import load_core
    core = load_core()
    return core.gpu_crc_tile_bytes(ALGO), core.gpu_crc_wave_bytes(ALGO)


def lengths():
    T, W = geometry()
    large = (GRID_CAP * TILES_PER_PASS + 3) * T + 48
    return {"16": 16, "32": 32, "W-16": W - 16, "W": W, "W+16": W + 16,
            "T-16": T - 16, "T": T, "T+16": T + 16, "2T+16": 2 * T + 16,
            "LARGE": large}


SMALL_NAMES = ["16", "32", "W-16", "W", "W+16", "T-16", "T", "T+16", "2T+16"]
KINDS = ["pattern", "random", "zero", "ones"]


@functools.lru_cache(maxsize=None)
def data(kind: str, n: int) -> bytes:
    if kind == "pattern":
        return km.checksum_pattern(n, 4096, 7)
    if kind == "random":
        return np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    return bytes(n) if kind == "zero" else b"\xff" * n


# ---------------------------------------------------------------------------
# known answers, crc64Update
# ---------------------------------------------------------------------------

KNOWN = [(b"123456789", 0xAE8B14860A799888),
         (bytes(4096), 0x6482D367EB22B64E),
         (b"\xff" * 4096, 0xC0DDBA7302ECA3AC),
         (b"", 0)]


def test_known_answers(core):
    for msg, want in KNOWN:
        assert model.crc64nvme(msg) == want
        assert core.crc(msg, ALGO) == want
    assert model.header_value(core.crc(b"123456789", ALGO)) == "rosUhgp5mIg="


@pytest.mark.parametrize("n", list(range(0, 71)) + [4095, 4096, 4097, 65536 + 5])
def test_crc_matches_model(core, n):
    x = rand_bytes(n, 11)
    assert core.crc(x, ALGO) == model.crc64nvme(x)


def test_32_bit_answers_unchanged(core):
    assert core.crc(b"123456789", "CRC32") == 0xCBF43926
    assert core.crc(b"123456789", "CRC32C") == 0xE3069283
    assert core.gpu_crc_tile_bytes() == core.gpu_crc_tile_bytes("CRC32C")
    assert core.gpu_crc_wave_bytes() == core.gpu_crc_wave_bytes("CRC32")
    with pytest.raises(ValueError):
        core.crc(b"x", "SHA256")
    with pytest.raises(ValueError):
        core.gpu_crc_tile_bytes("SHA256")


# ---------------------------------------------------------------------------
# crc64Combine, crc64ShiftPoly
# ---------------------------------------------------------------------------

def test_combine_matches_concatenation(core):
    inputs = [b"", b"\x00", b"\x5a", rand_bytes(8, 2), bytes(1000), bytes(1 << 20),
              rand_bytes(777, 3), rand_bytes(65536 + 1, 4), rand_bytes(1 << 20, 5)]
    crcs = [core.crc(x, ALGO) for x in inputs]
    for a, ca in zip(inputs, crcs):
        for b, cb in zip(inputs, crcs):
            assert core.crc_combine(ALGO, ca, cb, len(b)) == core.crc(a + b, ALGO), \
                (len(a), len(b))


def test_combine_len_zero_returns_a(core):
    for ca in (0, 1, 0xDEADBEEF, 0xFFFFFFFFFFFFFFFF):
        assert core.crc_combine(ALGO, ca, 0, 0) == ca
    with pytest.raises(TypeError):  # the 32-bit algorithms keep 32-bit arguments
        core.crc_combine("CRC32C", 1 << 32, 0, 1)


def _poly_mulmod(a: int, b: int) -> int:
    """a(x) * b(x) mod P in the normal representation (bit i = x^i)."""
    r = 0
    while b:
        if b & 1:
            r ^= a
        b >>= 1
        a <<= 1
        if a >> 64:
            a ^= (1 << 64) | model.POLY
    return r


def model_append_zeros(crc: int, n: int) -> int:
    """Finished CRC of (message with finished CRC `crc`) + n zero bytes: in
    the model's MSB-first register a zero byte is a multiplication by x^8."""
    reg = model._reflect(crc ^ model.MASK, 64)
    xp, sq, e = 1, 2, 8 * n  # x^0, x^1
    while e:
        if e & 1:
            xp = _poly_mulmod(xp, sq)
        sq = _poly_mulmod(sq, sq)
        e >>= 1
    return model._reflect(_poly_mulmod(reg, xp), 64) ^ model.MASK


def test_zeros_appended_past_2_32_by_doubling(core):
    """CRC of 2^k * 4096 zeros by doubling: Z[k] = combine(Z[k-1], Z[k-1]).
    Anchored at real zero blocks up to 1 MiB; above that every level is tied
    to the one below, so each square x^(2^k) used by crc64ShiftPoly is
    checked against the product of the previous one with itself, up to a
    len_b of 2^35. A polynomial-arithmetic model checks the ends."""
    n, z = 4096, core.crc(bytes(4096), ALGO)
    a = rand_bytes(4097, 6)
    ca = core.crc(a, ALGO)
    levels = [(n, z)]
    while n < 1 << 35:
        z = core.crc_combine(ALGO, z, z, n)
        n *= 2
        levels.append((n, z))
        if n <= 1 << 20:
            assert z == core.crc(bytes(n), ALGO), n
    for (half, zh), (full, zf) in zip(levels, levels[1:]):
        step = core.crc_combine(ALGO, core.crc_combine(ALGO, ca, zh, half), zh, half)
        assert core.crc_combine(ALGO, ca, zf, full) == step, full
    assert levels[-1][0] > 1 << 32
    for full, zf in levels[-4:]:
        assert zf == model_append_zeros(0, full), full
        assert core.crc_combine(ALGO, ca, zf, full) == model_append_zeros(ca, full), full
    # a length with many bits set, above 2^32
    odd = (1 << 33) + (1 << 32) + 12345
    zo = model_append_zeros(0, odd)
    assert core.crc_combine(ALGO, ca, zo, odd) == model_append_zeros(ca, odd)


# ---------------------------------------------------------------------------
# host emulation of the device tile kernel: table image, weights, geometry
# ---------------------------------------------------------------------------

def test_geometry(core):
    T, W = geometry()
    assert W % 1024 == 0 and T % W == 0 and T > W


@pytest.mark.parametrize("name", SMALL_NAMES)
def test_tiles_host_matches_crc(core, name):
    n = lengths()[name]
    assert n % 16 == 0
    for kind in KINDS:
        buf = data(kind, n)
        assert core.crc_tiles_host(buf, ALGO) == core.crc(buf, ALGO), (name, kind)


def test_tiles_host_bit_flips_at_wave_boundaries(core):
    """A wrong thread weight or row shift shows as a wrong answer for a
    single flipped bit next to the boundary it serves."""
    T, W = geometry()
    n = T + 16
    base = data("random", n)
    for i, b in enumerate(list(range(W, n, W)) + [1, n]):
        for p in (b - 1, b):
            if p < n:
                buf = bytearray(base)
                buf[p] ^= 1 << (i % 8)
                assert core.crc_tiles_host(bytes(buf), ALGO) == core.crc(bytes(buf), ALGO), p


def test_tiles_host_rejects_unaligned(core):
    with pytest.raises(ValueError, match="multiple of 16"):
        core.crc_tiles_host(bytes(24), ALGO)
    with pytest.raises(ValueError):
        core.crc_tiles_host(bytes(16), "CRC32C")
    assert core.crc_tiles_host(b"", ALGO) == 0


# ---------------------------------------------------------------------------
# config, client headers
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["crc64nvme", "CRC64NVME", "Crc64Nvme"])
def test_config_accepts_crc64nvme(name):
    from elbencho_amd.cli import args_to_config, build_parser
    from elbencho_amd.config import ConfigError
    base = ["--s3endpoints", "http://x:1", "-w", "-N", "1", "-t", "1", "-s", "1M",
            "-b", "1M", "s3://b"]
    p = build_parser()
    cfg = args_to_config(p.parse_args(base + ["--s3chksumalgo", name]))
    assert cfg.s3_chksum_algo.upper() == ALGO
    with pytest.raises(ConfigError, match="CRC64NVME"):
        args_to_config(p.parse_args(base + ["--s3chksumalgo", "CRC64"]))


def test_checksum_headers_base64_form():
    c = S3Client("http://127.0.0.1:1", ACCESS_KEY, SECRET_KEY, checksum_algo="crc64nvme")
    assert c._checksum_headers(b"123456789") == {
        "x-amz-sdk-checksum-algorithm": ALGO, HEADER: "rosUhgp5mIg="}
    body = rand_bytes(1000, 7)
    assert c._checksum_headers(body)[HEADER] == model.header_value(model.crc64nvme(body))


# ---------------------------------------------------------------------------
# native plane against a checking endpoint
# ---------------------------------------------------------------------------

class Crc64CheckingHandler(S3Handler):
    """S3 mock that insists on a correct, signed x-amz-checksum-crc64nvme for
    object and part PUTs, and records PUTs and multipart initiations."""

    seen: list = []        # (path, headers, body length) of object/part PUTs
    initiations: list = []  # headers of multipart initiations

    _put_body = None  # body of the PUT being handled (read once, used twice)

    def _body(self) -> bytes:
        if self._put_body is not None:
            return self._put_body
        return super()._body()

    def do_PUT(self):
        self._put_body = super()._body()
        try:
            return self._checked_put(self._put_body)
        finally:
            self._put_body = None

    def _checked_put(self, body: bytes):
        _, key, _ = self._parse()
        if key is not None:
            hdrs = {k.lower(): v for k, v in self.headers.items()}
            type(self).seen.append((self.path, hdrs, len(body)))
            if hdrs.get("x-amz-sdk-checksum-algorithm") != ALGO:
                return self._err(400, "InvalidRequest")
            from elbencho_amd import load_core
            want = load_core().crc(body, ALGO)
            if len(body) <= 4096:
                assert want == model.crc64nvme(body)
            if hdrs.get(HEADER, "") != base64.b64encode(struct.pack(">Q", want)).decode():
                return self._err(400, "BadDigest")
            if HEADER not in self.headers.get("Authorization", ""):
                return self._err(400, "ChecksumNotSigned")
        return super().do_PUT()

    def do_POST(self):
        _, _, q = self._parse()
        if "uploads" in q:
            type(self).initiations.append({k.lower(): v for k, v in self.headers.items()})
        return super().do_POST()


def start_crc64_endpoint():
    class Handler(Crc64CheckingHandler):
        pass

    Handler.store = S3Store()
    Handler.seen = []
    Handler.initiations = []
    server = ThreadingHTTPServer(("127.0.0.1", 0), Handler)
    server.daemon_threads = True
    threading.Thread(target=server.serve_forever, daemon=True).start()
    return server, f"http://127.0.0.1:{server.server_address[1]}", Handler


@pytest.fixture
def checking():
    server, url, handler = start_crc64_endpoint()
    yield url, handler
    server.shutdown()
    server.server_close()


PUT_LENGTHS = [0, 1, 65536, (1 << 20) + 5, 3 * (1 << 20)]


def test_endpoint_rejects_wrong_checksum(checking):
    url, _ = checking
    c = S3Client(url, ACCESS_KEY, SECRET_KEY)
    c.create_bucket("neg")
    with pytest.raises(S3Error, match="400"):
        c.put_object("neg", "nochk", b"abc")
    status, _, _ = c.request("PUT", "/neg/bad", body=b"123456789", headers={
        "x-amz-sdk-checksum-algorithm": ALGO,
        HEADER: base64.b64encode(struct.pack(">Q", 0xAE8B14860A799889)).decode()})
    assert status == 400
    status, _, _ = c.request("PUT", "/neg/good", body=b"123456789", headers={
        "x-amz-sdk-checksum-algorithm": ALGO, HEADER: "rosUhgp5mIg="})
    assert status == 200
    c.close()


def test_native_put_carries_checksum(checking):
    url, handler = checking
    c = S3Client(url, ACCESS_KEY, SECRET_KEY, checksum_algo=ALGO)
    assert c.attach_native(-1, 1 << 20) is True
    c.create_bucket("chk")
    for salt in (7, -1):
        for n in PUT_LENGTHS:
            c.put_object_native("chk", f"o{salt}_{n}", n, 0, salt)
    # multipart parts: each carries its own checksum; one at an aligned,
    # one at an unaligned pattern offset
    uid = c.create_multipart("chk", "mp")
    e1 = c.put_object_native("chk", "mp", 1 << 20, 0, 7,
                             query={"partNumber": "1", "uploadId": uid})
    e2 = c.put_object_native("chk", "mp", 1 << 20, 1 << 20, 7,
                             query={"partNumber": "2", "uploadId": uid})
    e3 = c.put_object_native("chk", "mp", 70000, 3, 7,
                             query={"partNumber": "3", "uploadId": uid})
    c.complete_multipart("chk", "mp", uid, [(1, e1), (2, e2), (3, e3)])
    puts = [s for s in handler.seen if "/chk/" in s[0]]
    assert len(puts) == 2 * len(PUT_LENGTHS) + 3
    assert all(s[1]["x-amz-sdk-checksum-algorithm"] == ALGO for s in puts)
    assert all(len(base64.b64decode(s[1][HEADER])) == 8 for s in puts)
    assert len(handler.initiations) == 1
    assert handler.initiations[0]["x-amz-checksum-algorithm"] == ALGO
    assert handler.initiations[0]["x-amz-checksum-type"] == "FULL_OBJECT"
    # the Python path: single PUT and part
    c.put_object("chk", "py", rand_bytes(5000, 8))
    uid = c.create_multipart("chk", "mp2")
    etag = c.upload_part("chk", "mp2", uid, 1, rand_bytes(70001, 9))
    c.complete_multipart("chk", "mp2", uid, [(1, etag)])
    assert c.get_object("chk", "mp2") == rand_bytes(70001, 9)
    c.close()
    # the two initiation headers are for this algorithm only
    for algo in ("CRC32C", ""):
        c = S3Client(url, ACCESS_KEY, SECRET_KEY, checksum_algo=algo)
        c.create_multipart("chk", "other")
        c.close()
        assert "x-amz-checksum-algorithm" not in handler.initiations[-1]
        assert "x-amz-checksum-type" not in handler.initiations[-1]
    assert len(handler.initiations) == 4


def test_body_crc_matches_put_body(checking, core):
    """body_crc on a plane without a device is the CRC of the bytes put()
    sends: read them back."""
    url, _ = checking
    c = S3Client(url, ACCESS_KEY, SECRET_KEY, checksum_algo=ALGO)
    assert c.attach_native(-1, 1 << 20)
    c.create_bucket("rb")
    for salt, off, n in [(7, 0, (1 << 20) + 5), (7, 3, 4099), (7, 8, 48), (7, 0, 0),
                         (-1, 0, 3 * (1 << 20)), (-1, 0, (1 << 20) + 5), (-1, 0, 77)]:
        c.put_object_native("rb", "o", n, off, salt)
        got = c.get_object("rb", "o")
        assert len(got) == n
        assert c.native.body_crc(n, off, salt, ALGO) == core.crc(got, ALGO), (salt, off, n)
        # the 32-bit checksums of the same plane are undisturbed
        assert c.native.body_crc(n, off, salt, "CRC32C") == core.crc32c(got)
    c.close()


def test_cli_write_phase_keeps_native_plane(checking, core, monkeypatch):
    """--s3chksumalgo crc64nvme: a multipart write phase through the CLI
    passes the checking endpoint, and its bodies came from the native plane."""
    from elbencho_amd.cli import main

    url, handler = checking
    puts = []
    orig = S3Client.put_object_native

    def spy(self, *a, **kw):
        puts.append(a)
        return orig(self, *a, **kw)

    monkeypatch.setattr(S3Client, "put_object_native", spy)
    rc = main(["--s3endpoints", url, "--s3key", ACCESS_KEY, "--s3secret", SECRET_KEY,
               "--nolive", "-d", "-w", "-t", "2", "-N", "2", "-s", "2m", "-b", "1m",
               "--s3chksumalgo", "crc64nvme", "s3://cli64"])
    assert rc == 0
    assert puts, "the write phase left the native plane"
    sent = [s for s in handler.seen if "/cli64/" in s[0]]
    assert sent and all(HEADER in s[1] for s in sent)
    assert handler.initiations
    assert all(h.get("x-amz-checksum-type") == "FULL_OBJECT" for h in handler.initiations)
    assert core.http_dataplane_live() == 0
