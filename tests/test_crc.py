"""CRC-32 / CRC-32C host library (csrc/crc.h) and the native S3 plane's
checksummed PUT, without a GPU.

The plane tests run against a checking endpoint: the SigV4 mock, extended
to recompute the CRC of every object/part body it receives and to answer
400 when the x-amz-checksum-* header is missing or wrong.
"""

import base64
import functools
import struct
import threading
import zlib
from http.server import ThreadingHTTPServer

import numpy as np
import pytest

from elbencho_amd.s3 import S3Client, S3Error

from tests.s3mock import ACCESS_KEY, SECRET_KEY, S3Handler, S3Store

ALGOS = ["CRC32", "CRC32C"]
LENGTHS = list(range(0, 10)) + [63, 64, 65, 4095, 4096, 4097, (1 << 20) + 3]


@functools.lru_cache(maxsize=None)
def rand_bytes(n: int, seed: int = 1) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def oracle(core, algo: str, data: bytes) -> int:
    return zlib.crc32(data) & 0xFFFFFFFF if algo == "CRC32" else core.crc32c(data)


# ---------------------------------------------------------------------------
# crcUpdate
# ---------------------------------------------------------------------------

def test_known_vectors(core):
    assert core.crc(b"123456789", "CRC32") == 0xCBF43926
    assert core.crc(b"123456789", "CRC32C") == 0xE3069283
    assert core.crc32c(b"123456789") == 0xE3069283


@pytest.mark.parametrize("algo", ALGOS)
def test_empty_is_zero(core, algo):
    assert core.crc(b"", algo) == 0


def test_unknown_algo_rejected(core):
    with pytest.raises(ValueError):
        core.crc(b"x", "SHA256")


@pytest.mark.parametrize("n", LENGTHS)
def test_crc32_matches_zlib(core, n):
    x = rand_bytes(n)
    assert core.crc(x, "CRC32") == zlib.crc32(x) & 0xFFFFFFFF


@pytest.mark.parametrize("n", LENGTHS)
def test_crc32c_matches_crc32c(core, n):
    x = rand_bytes(n)
    assert core.crc(x, "CRC32C") == core.crc32c(x)


# ---------------------------------------------------------------------------
# crcCombine
# ---------------------------------------------------------------------------

def _combine_inputs():
    big = rand_bytes(1 << 20, 2)
    return [b"", b"\x00", b"\x5a", bytes(1000), bytes(1 << 20), rand_bytes(777, 3),
            rand_bytes(65536 + 1, 4), big]


@pytest.mark.parametrize("algo", ALGOS)
def test_combine_matches_concatenation(core, algo):
    inputs = _combine_inputs()
    crcs = [core.crc(x, algo) for x in inputs]
    for a, ca in zip(inputs, crcs):
        for b, cb in zip(inputs, crcs):
            assert core.crc_combine(algo, ca, cb, len(b)) == core.crc(a + b, algo), \
                (algo, len(a), len(b))


@pytest.mark.parametrize("algo", ALGOS)
def test_combine_len_zero_returns_a(core, algo):
    for ca in (0, 1, 0xDEADBEEF, 0xFFFFFFFF):
        assert core.crc_combine(algo, ca, 0, 0) == ca


def test_combine_long_zero_b_against_zlib(core):
    """64 MiB of zeros as B: the exponent's high bits are exercised."""
    n = 64 << 20
    zeros = bytes(n)
    a = rand_bytes(4097, 5)
    cz = zlib.crc32(zeros) & 0xFFFFFFFF
    expect = zlib.crc32(zeros, zlib.crc32(a)) & 0xFFFFFFFF
    assert core.crc(zeros, "CRC32") == cz
    assert core.crc_combine("CRC32", zlib.crc32(a) & 0xFFFFFFFF, cz, n) == expect
    # the same identity for CRC32C, against the incremental oracle
    ca, czc = core.crc32c(a), core.crc32c(zeros)
    assert core.crc_combine("CRC32C", ca, czc, n) == core.crc32c(a + zeros)


# ---------------------------------------------------------------------------
# native plane against a checking endpoint
# ---------------------------------------------------------------------------

class CheckingHandler(S3Handler):
    """S3 mock that insists on a correct x-amz-checksum-* header for object
    and part PUTs when `require` is set, and records what it saw."""

    require = True
    seen: list = []

    _put_body = None  # body of the PUT being handled (read once, used twice)

    def _body(self) -> bytes:
        if self._put_body is not None:
            return self._put_body
        return super()._body()

    def do_PUT(self):
        body = super()._body()
        self._put_body = body
        try:
            return self._checked_put(body)
        finally:
            self._put_body = None

    def _checked_put(self, body: bytes):
        _, key, _ = self._parse()
        if key is not None:
            hdrs = {k.lower(): v for k, v in self.headers.items()}
            type(self).seen.append((self.path, hdrs, len(body)))
            algo = hdrs.get("x-amz-sdk-checksum-algorithm")
            if type(self).require:
                if algo not in ("CRC32", "CRC32C"):
                    return self._err(400, "InvalidRequest")
                from elbencho_amd import load_core
                want = (zlib.crc32(body) & 0xFFFFFFFF if algo == "CRC32"
                        else load_core().crc32c(body))
                got = hdrs.get(f"x-amz-checksum-{algo.lower()}", "")
                if got != base64.b64encode(struct.pack(">I", want)).decode():
                    return self._err(400, "BadDigest")
                signed = self.headers.get("Authorization", "")
                if f"x-amz-checksum-{algo.lower()}" not in signed:
                    return self._err(400, "ChecksumNotSigned")
        return super().do_PUT()


def start_checking_endpoint(require: bool = True):
    class Handler(CheckingHandler):
        pass

    Handler.store = S3Store()
    Handler.require = require
    Handler.seen = []
    server = ThreadingHTTPServer(("127.0.0.1", 0), Handler)
    server.daemon_threads = True
    threading.Thread(target=server.serve_forever, daemon=True).start()
    return server, f"http://127.0.0.1:{server.server_address[1]}", Handler


@pytest.fixture
def checking():
    server, url, handler = start_checking_endpoint()
    yield url, handler
    server.shutdown()
    server.server_close()


PUT_LENGTHS = [0, 1, 65536, (1 << 20) + 5, 3 * (1 << 20)]


def test_checking_endpoint_rejects_wrong_checksum(checking, core):
    """The fixture itself: a wrong or missing checksum is a 400."""
    url, _ = checking
    c = S3Client(url, ACCESS_KEY, SECRET_KEY)
    c.create_bucket("neg")
    with pytest.raises(S3Error, match="400"):
        c.put_object("neg", "nochk", b"abc")
    status, _, _ = c.request("PUT", "/neg/bad", body=b"abc", headers={
        "x-amz-sdk-checksum-algorithm": "CRC32C",
        "x-amz-checksum-crc32c": base64.b64encode(b"\0\0\0\1").decode()})
    assert status == 400
    c.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_native_put_carries_checksum(checking, algo):
    url, handler = checking
    c = S3Client(url, ACCESS_KEY, SECRET_KEY, checksum_algo=algo)
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
    assert all(s[1]["x-amz-sdk-checksum-algorithm"] == algo for s in puts)
    c.close()


def test_body_crc_matches_put_body(checking, core):
    """body_crc is the CRC of the bytes put() sends: read them back."""
    url, _ = checking
    c = S3Client(url, ACCESS_KEY, SECRET_KEY, checksum_algo="CRC32C")
    assert c.attach_native(-1, 1 << 20)
    c.create_bucket("rb")
    for salt, off, n in [(7, 0, (1 << 20) + 5), (7, 3, 4099), (-1, 0, 3 * (1 << 20)),
                         (-1, 0, (1 << 20) + 5)]:
        c.put_object_native("rb", "o", n, off, salt)
        data = c.get_object("rb", "o")
        assert len(data) == n
        for algo in ALGOS:
            assert c.native.body_crc(n, off, salt, algo) == oracle(core, algo, data)
    c.close()


def test_sha256_keeps_python_path():
    c = S3Client("http://127.0.0.1:1", ACCESS_KEY, SECRET_KEY, checksum_algo="SHA256")
    assert c.attach_native(-1, 1 << 20) is False
    assert c.native is None
    c = S3Client("http://127.0.0.1:1", ACCESS_KEY, SECRET_KEY, checksum_algo="SHA1")
    assert c.attach_native(-1, 1 << 20) is False


def test_no_algo_sends_no_checksum_headers():
    server, url, handler = start_checking_endpoint(require=False)
    try:
        c = S3Client(url, ACCESS_KEY, SECRET_KEY)
        assert c.attach_native(-1, 1 << 20)
        c.create_bucket("plain")
        c.put_object_native("plain", "o", 65536, 0, 7)
        c.put_object_native("plain", "r", 4097, 0, -1)
        puts = [s for s in handler.seen if "/plain/" in s[0]]
        assert len(puts) == 2
        for _, hdrs, _ in puts:
            assert not [h for h in hdrs if "checksum" in h]
        c.close()
    finally:
        server.shutdown()
        server.server_close()
