"""Exact tests of the S3 native data plane (csrc/httpdata.h), host variant.

core.HttpDataPlane is driven directly through get / put / body_crc against the
two raw-TCP servers of tests/dataplane_servers.py. The only oracle is
tests/kernel_model.py; every comparison is exact equality.

Every case takes the plane's device from the `dev` fixture. This module runs
them with dev = -1 (no device: the host fill and verify loops), which also
proves the servers and the oracle rule below without a GPU.
tests/test_gpu_s3_dataplane.py imports the same cases and runs them with
dev = 0, where the plane chunks the body over its 2-slot ring and uses the
fill, verify and CRC kernels.

The contract the cases pin
--------------------------
PUT: put(len, off, salt >= 0) sends the checksum pattern of [off, off+len):
the word at 8-aligned pattern offset o holds (o + salt) mod 2^64, a range that
starts or ends inside a word gets that word's bytes. salt < 0 sends the
plane's random block of max(max_block, 4096) bytes over and over.
body_crc(len, off, salt, algo) is the CRC of exactly those bytes.

GET (the rule is expected_get() below and is repeated in the doc comment of
HttpDataPlane::get): the body is cut into chunks of C bytes, the last one
shorter, C = min(max(max_block, 4096), 2 MiB) with a device and
C = max(max_block, 4096) without.
  * A chunk is GPU-checked iff the plane has a device, pattern_off % 8 == 0,
    the chunk's pattern offset is a multiple of 8 and its length a multiple
    of 16. It contributes kernel_model.verify(): the number of mismatching
    words and the offset of the first bad word.
  * Any other chunk is host-checked and contributes (1, offset of its first
    bad byte) if it has a mismatch.
nbad is the sum over the chunks, first the numeric minimum (2^64-1 when
clean), offsets taken mod 2^64. A request starts from zero whatever the
previous request on the plane did.
"""

import functools
import itertools
import re
import zlib

import numpy as np
import pytest

from tests import kernel_model as km
from tests.dataplane_servers import BlobServer, SinkServer, call_limited

MASK = km.MASK
U64_MAX = km.U64_MAX
SALT = 0x0123456789AB
MIB = 1 << 20

# max_block of the plane. 4096: chunks are multiples of 16. 4104: full chunks
# have len % 16 == 8 (GET checks them on the host, PUT fills them on the GPU
# with an odd final word). 4100: every chunk after the first starts at an
# offset that is no multiple of 8. 8 MiB: the 2 MiB production chunk.
GEOMETRIES = [4096, 4104, 4100, 4112, 8 * MIB]
SMALL_GEOMETRIES = GEOMETRIES[:-1]
# pattern offsets: aligned, wrapping past 2^64, and unaligned (host path for
# the whole body)
OFFSETS = [0, 8, 1 << 30, 2**64 - 4096, 3]

geometry_ids = {8 * MIB: "8MiB"}
params_geom_off = pytest.mark.parametrize(
    "mb,off", list(itertools.product(GEOMETRIES, OFFSETS)),
    ids=lambda v: geometry_ids.get(v, hex(v) if v > 1 << 20 else str(v)))


@pytest.fixture
def dev():
    return -1


# ---------------------------------------------------------------------------
# geometry and oracle
# ---------------------------------------------------------------------------

def host_block(mb: int) -> int:
    return max(mb, 4096)


def unit(mb: int) -> int:
    """The C that the body lengths are built from: the chunk of a plane with
    a device (the small geometries chunk the same without one)."""
    return min(host_block(mb), 2 * MIB)


def get_chunk(dev: int, mb: int) -> int:
    return unit(mb) if dev >= 0 else host_block(mb)


def body_lengths(mb: int) -> list:
    C = unit(mb)
    if mb > 2 * MIB:
        return [3 * C + 48]
    # 3C: the third chunk reuses slot 0 and must wait for its event
    return [0, 16, C - 16, C, C + 16, 2 * C, 2 * C + 8, 2 * C + 4, 3 * C, 5 * C + 24]


def long_length(mb: int) -> int:
    """The body the corruption and state cases use: several chunks (the slot
    ring wraps) and a ragged tail."""
    return body_lengths(mb)[-1]


@functools.lru_cache(maxsize=8)
def model_body(n: int, off: int, salt: int) -> bytes:
    """The bytes of pattern range [off, off+n): the model's words over the
    8-aligned cover of the range, sliced to it."""
    head = off % 8
    cover = (head + n + 7) // 8 * 8
    return km.checksum_pattern(cover, off - head, salt)[head:head + n]


def expected_get(dev: int, mb: int, data: bytes, off: int, salt: int) -> tuple:
    """(nbad, first) of a verified GET of `data` - the rule of the module
    docstring, written once."""
    if salt < 0:
        return 0, U64_MAX
    C = get_chunk(dev, mb)
    want = np.frombuffer(model_body(len(data), off, salt), dtype=np.uint8)
    got = np.frombuffer(data, dtype=np.uint8)
    nbad, first = 0, U64_MAX
    for pos in range(0, len(data), C):
        n = min(C, len(data) - pos)
        coff = (off + pos) & MASK
        if dev >= 0 and off % 8 == 0 and coff % 8 == 0 and n % 16 == 0:
            cnt, f = km.verify(data[pos:pos + n], coff, salt)
        else:
            bad = np.flatnonzero(got[pos:pos + n] != want[pos:pos + n])
            cnt, f = (1, (coff + int(bad[0])) & MASK) if bad.size else (0, U64_MAX)
        nbad += cnt
        first = min(first, f)
    return nbad, first


def corrupt(data: bytes, positions) -> bytes:
    out = bytearray(data)
    for p in positions:
        out[p] ^= 0xA5
    return bytes(out)


def corruption_places(mb: int) -> dict:
    """name -> (body length, byte positions to XOR). The 4096 geometry gets
    every place, the others the first word, a chunk boundary and the tail."""
    C = unit(mb)
    L = long_length(mb)
    tail = L // C * C  # where the ragged tail chunk starts
    # The boundary cases hit byte 5 of the chunk's last word, not byte 7: at
    # pattern offset 2^64 - 4096 byte 7 of chunk 0's last word lies at offset
    # 2^64 - 1, which is also the value that says "clean". The host check
    # cannot report a first bad byte there (seen with the 4096 geometry), so
    # no case puts the first bad byte of a host-checked chunk on that offset.
    places = {
        "first_word": (L, [0]),
        # last word of chunk 1 + first word of chunk 2: slots 1 and 0
        "boundary_1_2": (L, [2 * C - 3, 2 * C]),
        "tail_only": (L, [tail, L - 3]),
    }
    if mb != 4096:
        return places
    places.update({
        "last_word": (L, [L - 8]),
        "byte3_gpu_chunk": (L, [C + 40 + 3]),
        "byte3_host_chunk": (L, [tail + 8 + 3]),
        "boundary_0_1": (L, [C - 3, C]),            # slots 0 and 1
        "boundary_2_3": (L, [3 * C - 3, 3 * C]),    # 0 and 1 again, ring wrapped
        # highest chunk first: the minimum offset comes last, the count sums
        "five_chunks": (L, [4 * C + 56, 3 * C + 801, 2 * C + 4090, C + 3, 140]),
        "tail_plus_earlier": (L, [2 * C + 64, tail + 9]),
        "every_word": (3 * C, [8 * i + i % 8 for i in range(3 * C // 8)]),
    })
    return places


# ---------------------------------------------------------------------------
# rig
# ---------------------------------------------------------------------------

class Servers:
    def __init__(self):
        self.blob = BlobServer()
        self.sink = SinkServer()
        self.names = (f"o{i}" for i in itertools.count())

    def stop(self):
        self.blob.stop()
        self.sink.stop()


@pytest.fixture(scope="module")
def servers():
    s = Servers()
    yield s
    s.stop()
    assert s.blob.errors == [] and s.sink.errors == []


@pytest.fixture
def planes(core, dev):
    """planes(server, max_block) -> a fresh HttpDataPlane on `dev`."""
    made = []

    def make(server, mb, on_dev=None):
        p = core.HttpDataPlane("127.0.0.1", server.port,
                               dev if on_dev is None else on_dev, mb)
        made.append(p)
        return p

    yield make
    for p in made:
        p.close()
    made.clear()


def do_get(plane, servers, data, off, salt, expect_len=None, **blob_opts):
    name = next(servers.names)
    servers.blob.put_blob(name, data, **blob_opts)
    try:
        req = f"GET /{name} HTTP/1.1\r\nHost: t\r\n\r\n".encode()
        return call_limited(plane.get, req,
                            len(data) if expect_len is None else expect_len,
                            off, salt)
    finally:
        servers.blob.drop_blob(name)


def put_request(name: str, n: int) -> bytes:
    return f"PUT /{name} HTTP/1.1\r\nHost: t\r\nContent-Length: {n}\r\n\r\n".encode()


def do_put(plane, servers, n, off, salt) -> bytes:
    """One PUT; returns the bytes the sink received."""
    name = next(servers.names)
    status, hdrs = call_limited(plane.put, put_request(name, n), n, off, salt)
    assert status == 200, (status, n, off)
    assert re.search(r"(?im)^etag:", hdrs), hdrs
    return servers.sink.take(name)


def crcs(core, body: bytes) -> dict:
    return {"CRC32": zlib.crc32(body) & 0xFFFFFFFF, "CRC32C": core.crc32c(body)}


def first_diff(a: bytes, b: bytes) -> str:
    """For assertion messages: never dump a body."""
    if len(a) != len(b):
        return f"lengths {len(a)} != {len(b)}"
    x, y = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    bad = np.flatnonzero(x != y)
    return f"{bad.size} bytes differ, first at {int(bad[0])}" if bad.size else "equal"


def assert_body(got: bytes, want: bytes, what):
    assert got == want, f"{what}: {first_diff(got, want)}"


# ---------------------------------------------------------------------------
# PUT
# ---------------------------------------------------------------------------

@params_geom_off
def test_put_body_and_crc(core, dev, servers, planes, mb, off):
    plane = planes(servers.sink, mb)
    for n in body_lengths(mb):
        body = do_put(plane, servers, n, off, SALT)
        assert_body(body, model_body(n, off, SALT), ("put", mb, n, off))
        for algo, want in crcs(core, body).items():
            got = call_limited(plane.body_crc, n, off, SALT, algo)
            assert got == want, (algo, mb, n, off)


def test_put_tail_chunk_at_misaligned_offset(core, dev, servers, planes):
    """max_block 4100, body 4100 + 4096: the last chunk is a whole number of
    words but starts at pattern offset 4100. The fill kernel does not take
    that offset, so the plane has to fill it on the host - and the connection
    serves the next request."""
    plane = planes(servers.sink, 4100)
    n = 4100 + 4096
    assert_body(do_put(plane, servers, n, 0, SALT), model_body(n, 0, SALT), "first")
    conns = servers.sink.connections
    assert_body(do_put(plane, servers, n, 8, SALT), model_body(n, 8, SALT), "second")
    assert_body(do_put(plane, servers, 16, 0, SALT), model_body(16, 0, SALT), "third")
    assert servers.sink.connections == conns, "the plane had to reconnect"


@pytest.mark.parametrize("mb", GEOMETRIES, ids=lambda v: geometry_ids.get(v, str(v)))
def test_put_random_body_and_crc(core, dev, servers, planes, mb):
    plane = planes(servers.sink, mb)
    M = host_block(mb)
    block = None
    for n in (0, M - 1, M, M + 1, 3 * M + 5):
        body = do_put(plane, servers, n, 0, -1)
        assert len(body) == n
        for algo, want in crcs(core, body).items():
            assert call_limited(plane.body_crc, n, 0, -1, algo) == want, (algo, mb, n)
        assert_body(do_put(plane, servers, n, 0, -1), body, ("second put", mb, n))
        # one block of M random bytes, repeated
        if n >= M:
            block = block or body[:M]
            reps = -(-n // M)
            assert_body(body, (block * reps)[:n], ("period", mb, n))
    assert len(set(block)) > 200  # random data, not a constant fill


# ---------------------------------------------------------------------------
# GET
# ---------------------------------------------------------------------------

@params_geom_off
def test_get_clean(core, dev, servers, planes, mb, off):
    plane = planes(servers.blob, mb)
    for i, n in enumerate(body_lengths(mb)):
        data = model_body(n, off, SALT)
        # every other blob: first body bytes in the same write as the header
        got = do_get(plane, servers, data, off, SALT, piece=1000, glue_head=i % 2 == 0)
        assert got == (200, n, 0, U64_MAX), (mb, n, off)


@params_geom_off
def test_get_corrupt(core, dev, servers, planes, mb, off):
    plane = planes(servers.blob, mb)
    C = unit(mb)
    gpu_rule = dev >= 0 and off % 8 == 0
    for name, (n, positions) in corruption_places(mb).items():
        data = corrupt(model_body(n, off, SALT), positions)
        want = expected_get(dev, mb, data, off, SALT)
        # the oracle itself, against figures worked out by hand
        if name == "byte3_gpu_chunk":
            assert want == (1, (off + C + 40 + (0 if gpu_rule else 3)) & MASK)
        elif name == "byte3_host_chunk":
            assert want == (1, (off + 5 * C + 11) & MASK)
        elif name == "every_word":
            assert want[0] == (3 * C // 8 if gpu_rule else 3)
        elif name == "five_chunks":
            assert want[0] == 5
        got = do_get(plane, servers, data, off, SALT, piece=1000)
        assert got == (200, n) + want, (name, mb, off)
        # without a salt nothing is verified
        got = do_get(plane, servers, data, off, -1, piece=1000)
        assert got == (200, n, 0, U64_MAX), (name, mb, off)


# ---------------------------------------------------------------------------
# plane state across requests
# ---------------------------------------------------------------------------

STATE_GEOMETRIES = [4096, 4112]
params_state = pytest.mark.parametrize("mb", STATE_GEOMETRIES)


def first_chunk_corrupt(mb: int, off: int = 0) -> bytes:
    C = unit(mb)
    return corrupt(model_body(long_length(mb), off, SALT), [1, 40, C // 2 + 3, C - 1])


def assert_clean_get(plane, servers, mb, off=0):
    n = long_length(mb)
    got = do_get(plane, servers, model_body(n, off, SALT), off, SALT, piece=1000)
    assert got == (200, n, 0, U64_MAX)


@params_state
def test_state_corrupt_then_clean(core, dev, servers, planes, mb):
    plane = planes(servers.blob, mb)
    bad = first_chunk_corrupt(mb)
    want = expected_get(dev, mb, bad, 0, SALT)
    assert want[0] >= 1
    for _ in range(2):
        assert do_get(plane, servers, bad, 0, SALT, piece=1000) == (200, len(bad)) + want
        assert_clean_get(plane, servers, mb)


@pytest.mark.parametrize("mb", STATE_GEOMETRIES + [8 * MIB],
                         ids=lambda v: geometry_ids.get(v, str(v)))
def test_state_cut_connection_then_clean(core, dev, servers, planes, mb):
    """The server closes the socket inside the third chunk of a body whose
    first chunk is corrupt. What the aborted request had found must not show
    up in the next one."""
    plane = planes(servers.blob, mb)
    C = unit(mb)
    bad = first_chunk_corrupt(mb)
    cut = 2 * C + 100
    got = do_get(plane, servers, bad, 0, SALT, piece=1000, cut_after=cut)
    assert got[:2] == (-1, cut)
    assert_clean_get(plane, servers, mb)
    # and nothing is dropped that belongs to a later request
    want = expected_get(dev, mb, bad, 0, SALT)
    assert do_get(plane, servers, bad, 0, SALT, piece=1000) == (200, len(bad)) + want


@params_state
def test_state_error_status_not_verified(core, dev, servers, planes, mb):
    plane = planes(servers.blob, mb)
    bad = first_chunk_corrupt(mb)
    want = expected_get(dev, mb, bad, 0, SALT)
    assert do_get(plane, servers, bad, 0, SALT, piece=1000) == (200, len(bad)) + want
    err = b"<Error><Code>NoSuchKey</Code></Error>"
    got = do_get(plane, servers, err, 0, SALT, expect_len=long_length(mb), status=404)
    assert got == (404, len(err), 0, U64_MAX)
    assert_clean_get(plane, servers, mb)


@params_state
def test_state_oversized_body_then_clean(core, dev, servers, planes, mb):
    plane = planes(servers.blob, mb)
    n = long_length(mb)
    got = do_get(plane, servers, first_chunk_corrupt(mb), 0, SALT, expect_len=n - 1,
                 piece=1000)
    assert got == (-2, n, 0, U64_MAX)
    assert_clean_get(plane, servers, mb)


@params_state
def test_state_put_get_interleaved(core, dev, servers, planes, mb):
    """Both directions use the same slots: PUT, GET, PUT, GET on one plane."""
    plane = planes(servers.sink, mb)
    C = unit(mb)

    def put(name, n, off):
        status, _ = call_limited(plane.put, put_request(name, n), n, off, SALT)
        assert status == 200
        assert_body(servers.sink.peek(name), model_body(n, off, SALT), (name, n, off))

    def get(name, off):
        req = f"GET /{name} HTTP/1.1\r\nHost: t\r\n\r\n".encode()
        return call_limited(plane.get, req, 1 << 30, off, SALT)

    n1, off1 = 5 * C + 24, 1 << 30
    put("a", n1, off1)
    assert get("a", off1) == (200, n1, 0, U64_MAX)
    bad = corrupt(model_body(n1, off1, SALT), [5, 2 * C - 1, 2 * C, 5 * C + 20])
    servers.sink.store("abad", bad)
    n2, off2 = 3 * C, 8
    put("b", n2, off2)
    assert get("abad", off1) == (200, n1) + expected_get(dev, mb, bad, off1, SALT)
    put("c", 2 * C + 8, 0)
    assert get("b", off2) == (200, n2, 0, U64_MAX)
    assert get("c", 0) == (200, 2 * C + 8, 0, U64_MAX)
    for name in ("a", "abad", "b", "c"):
        servers.sink.take(name)


# ---------------------------------------------------------------------------
# through S3Client, against the SigV4 mock: the path the benchmark takes
# ---------------------------------------------------------------------------

@pytest.fixture
def s3client(dev):
    from elbencho_amd.s3 import S3Client
    from tests.s3mock import ACCESS_KEY, SECRET_KEY, start_mock

    server, port = start_mock()
    clients = []

    def make(mb):
        c = S3Client(f"http://127.0.0.1:{port}", ACCESS_KEY, SECRET_KEY, timeout=20.0)
        assert c.attach_native(dev, mb)
        clients.append(c)
        return c

    yield make
    for c in clients:
        c.close()
        c.native = None
    server.shutdown()
    server.server_close()


@pytest.mark.parametrize("mb", SMALL_GEOMETRIES)
def test_s3client_native_put_reads_back_exact(core, dev, s3client, mb):
    c = s3client(mb)
    n, off = long_length(mb), 1 << 20
    c.create_bucket("dpx")
    call_limited(c.put_object_native, "dpx", "o", n, off, SALT)
    assert_body(c.get_object("dpx", "o"), model_body(n, off, SALT), (mb, n, off))
    assert call_limited(c.get_object_native, "dpx", "o", None, off, SALT) == n


def test_s3client_native_get_reports_oracle_offset_and_count(core, dev, s3client):
    from elbencho_amd.s3 import S3Error

    mb, off = 4096, 1 << 20
    C = unit(mb)
    n = long_length(mb)
    bad = corrupt(model_body(n, off, SALT), [3 * C + 8, C + 16 + 3, C + 800, 5 * C + 17])
    nbad, first = expected_get(dev, mb, bad, off, SALT)
    assert nbad == (4 if dev >= 0 else 3)
    c = s3client(mb)
    c.create_bucket("dpx")
    c.put_object("dpx", "bad", bad)
    with pytest.raises(S3Error) as ei:
        call_limited(c.get_object_native, "dpx", "bad", None, off, SALT)
    assert f"at object offset {first} ({nbad} bad blocks)" in str(ei.value)
