"""S3 engine tests against the in-memory mock (SigV4-verified)."""

import pytest

from elbencho_amd.cli import main
from elbencho_amd.s3 import S3Client, S3Error

from tests.s3mock import ACCESS_KEY, SECRET_KEY, start_mock


@pytest.fixture
def mock_s3():
    server, port = start_mock()
    yield f"http://127.0.0.1:{port}"
    server.shutdown()


@pytest.fixture
def client(mock_s3):
    return S3Client(mock_s3, ACCESS_KEY, SECRET_KEY)


def test_client_bucket_object_roundtrip(client):
    client.create_bucket("b1")
    assert client.head_bucket("b1")
    client.put_object("b1", "k/x", b"hello world")
    assert client.get_object("b1", "k/x") == b"hello world"
    assert client.get_object("b1", "k/x", (6, 10)) == b"world"
    client.head_object("b1", "k/x")
    client.delete_object("b1", "k/x")
    with pytest.raises(S3Error):
        client.get_object("b1", "k/x")
    client.delete_bucket("b1")


def test_client_bad_secret_rejected(mock_s3):
    bad = S3Client(mock_s3, ACCESS_KEY, "wrong")
    with pytest.raises(S3Error, match="403"):
        bad.create_bucket("x")


def test_client_multipart(client):
    client.create_bucket("mp")
    uid = client.create_multipart("mp", "big")
    e1 = client.upload_part("mp", "big", uid, 1, b"A" * 100)
    e2 = client.upload_part("mp", "big", uid, 2, b"B" * 50)
    client.complete_multipart("mp", "big", uid, [(1, e1), (2, e2)])
    assert client.get_object("mp", "big") == b"A" * 100 + b"B" * 50


def test_client_list_pagination(client):
    client.create_bucket("lst")
    for i in range(25):
        client.put_object("lst", f"obj{i:03d}", b"x")
    keys = []
    token = ""
    while True:
        page, token = client.list_objects("lst", max_keys=10, continuation=token)
        keys.extend(k for k, _ in page)
        if not token:
            break
    assert len(keys) == 25


def test_client_multi_delete(client):
    client.create_bucket("md")
    for i in range(5):
        client.put_object("md", f"o{i}", b"x")
    client.multi_delete("md", [f"o{i}" for i in range(5)])
    page, _ = client.list_objects("md")
    assert page == []


def _cli(mock_s3, extra):
    return main(["--s3endpoints", mock_s3, "--s3key", ACCESS_KEY,
                 "--s3secret", SECRET_KEY, "--nolive"] + extra)


def test_s3_full_lifecycle_cli(mock_s3, capsys):
    # mkbuckets -> put (multipart) -> head -> get+verify -> delete -> rmbuckets
    rc = _cli(mock_s3, ["-d", "-w", "--stat", "-r", "-F", "-D", "-t", "2",
                        "-N", "3", "-s", "192k", "-b", "64k", "--verify", "5",
                        "--lat", "s3://tbkt"])
    assert rc == 0
    out = capsys.readouterr().out
    assert "MKBUCKETS" in out
    assert "HEADOBJ" in out
    assert "RMOBJECTS" in out
    assert "RMBUCKETS" in out
    # 2 threads x 3 objects x 192k, multipart of 3 x 64k parts each
    for line in out.splitlines():
        if "Objects total" in line:
            assert line.split()[-1] == "6"
            break
    else:
        raise AssertionError("no Objects total row:\n" + out)


def test_s3_verify_detects_corruption(mock_s3):
    rc = _cli(mock_s3, ["-d", "-w", "-t", "1", "-N", "1", "-s", "64k", "-b", "64k",
                        "--verify", "5", "s3://vbkt"])
    assert rc == 0
    # corrupt the object in the store, then read with verify
    from tests.s3mock import S3Handler
    with S3Handler.store.lock:
        key = next(iter(S3Handler.store.buckets["vbkt"]))
        data = bytearray(S3Handler.store.buckets["vbkt"][key])
        data[1000] ^= 0xFF
        S3Handler.store.buckets["vbkt"][key] = bytes(data)
    rc = _cli(mock_s3, ["-r", "-t", "1", "-N", "1", "-s", "64k", "-b", "64k",
                        "--verify", "5", "s3://vbkt"])
    assert rc == 1


def test_s3_listobj_and_multidel(mock_s3, capsys):
    rc = _cli(mock_s3, ["-d", "-w", "-t", "2", "-N", "4", "-s", "4k", "-b", "4k",
                        "s3://lbkt"])
    assert rc == 0
    rc = _cli(mock_s3, ["--s3listobj", "100", "--s3listverify", "-t", "2", "-N", "4",
                        "-s", "4k", "-b", "4k", "s3://lbkt"])
    assert rc == 0, capsys.readouterr().out
    rc = _cli(mock_s3, ["-F", "--s3multidel", "3", "-t", "2", "-N", "4",
                        "-s", "4k", "-b", "4k", "s3://lbkt"])
    assert rc == 0


def test_s3_acl_and_tagging_phases(mock_s3, capsys):
    rc = _cli(mock_s3, ["-d", "-w", "-t", "2", "-N", "2", "-s", "4k", "-b", "4k",
                        "--s3baclput", "--s3baclget", "--s3btag", "--s3btagverify",
                        "--s3aclput", "--s3aclget", "--s3aclverify",
                        "--s3aclgrants", "public-read",
                        "--s3otag", "--s3otagverify", "-F", "-D", "s3://aclbkt"])
    out = capsys.readouterr().out
    assert rc == 0, out
    for phase in ("PUTBACL", "PUTBUCKETMD", "GETBUCKETMD", "PUTOBJACL", "PUTOBJMD",
                  "GETOBJMD", "GETOBJACL", "DELOBJMD", "GETBACL"):
        assert phase in out, f"{phase} missing in:\n{out}"


def test_s3_randobj(mock_s3):
    rc = _cli(mock_s3, ["-d", "-w", "-t", "2", "-N", "4", "-s", "64k", "-b", "16k",
                        "--verify", "3", "s3://rbkt"])
    assert rc == 0
    rc = _cli(mock_s3, ["-r", "-t", "2", "-N", "4", "-s", "64k", "-b", "16k",
                        "--s3randobj", "--randamount", "256k", "--verify", "3",
                        "s3://rbkt"])
    assert rc == 0


def test_s3_credentials_roundrobin(mock_s3):
    # both workers use valid creds from the list -> phases succeed
    rc = main(["--s3endpoints", mock_s3, "--nolive",
               "--s3credlist", f"{ACCESS_KEY}:{SECRET_KEY},{ACCESS_KEY}:{SECRET_KEY}",
               "-d", "-w", "-F", "-D", "-t", "2", "-N", "2", "-s", "4k", "-b", "4k",
               "s3://credbkt"])
    assert rc == 0


def test_s3_mpu_sharing_cross_instance(mock_s3):
    """--s3nompucompl leaves multipart uploads open; a separate run (another
    'instance') completes them via --s3mpucompl by rediscovering uploadIds
    and part ETags from the endpoint."""
    rc = _cli(mock_s3, ["-d", "-w", "-t", "2", "-N", "2", "-s", "192k", "-b", "64k",
                        "--s3nompucompl", "--verify", "9", "s3://mpubkt"])
    assert rc == 0
    # objects do not exist yet (uploads incomplete)
    from tests.s3mock import S3Handler
    with S3Handler.store.lock:
        assert S3Handler.store.buckets["mpubkt"] == {}
        assert len(S3Handler.store.uploads) == 4  # 2 threads x 2 objects

    rc = _cli(mock_s3, ["--s3mpucompl", "-t", "2", "-N", "2", "-s", "192k",
                        "-b", "64k", "s3://mpubkt"])
    assert rc == 0
    with S3Handler.store.lock:
        assert len(S3Handler.store.buckets["mpubkt"]) == 4
        assert not S3Handler.store.uploads

    # the completed objects verify end to end
    rc = _cli(mock_s3, ["-r", "-t", "2", "-N", "2", "-s", "192k", "-b", "64k",
                        "--verify", "9", "s3://mpubkt"])
    assert rc == 0


def test_s3_opslog(mock_s3, tmp_path):
    log = tmp_path / "s3ops.jsonl"
    rc = _cli(mock_s3, ["-d", "-w", "-r", "-t", "1", "-N", "2", "-s", "8k", "-b", "8k",
                        "--opslog", str(log), "s3://opsbkt"])
    assert rc == 0
    import json as _json
    lines = [_json.loads(ln) for ln in log.read_text().splitlines()]
    assert any(l["op"] == "PutObject" and l["type"] == "pre" for l in lines)
    assert any(l["op"] == "GetObject" and l["type"] == "post" for l in lines)


def test_s3_large_block_payload(mock_s3):
    """block size above the 4 MiB urandom seed chunk (regression: bytearray
    self-append raised BufferError)."""
    rc = _cli(mock_s3, ["-d", "-w", "-r", "-F", "-D", "-t", "1", "-N", "1",
                        "-s", "16m", "-b", "8m", "s3://bigblk"])
    assert rc == 0


def test_s3_versioning_objectlock_statdirs_listpar(mock_s3, capsys):
    rc = _cli(mock_s3, ["-d", "-w", "-t", "2", "-N", "2", "-s", "4k", "-b", "4k",
                        "--s3bversion", "--s3bversionverify",
                        "--s3olockcfg", "--s3olockcfgverify",
                        "--s3statdirs", "--s3listobjpar", "s3://verbkt"])
    out = capsys.readouterr().out
    assert rc == 0, out
    for phase in ("BVERSION", "OLOCKCFG", "STATDIRS", "LISTOBJ_P"):
        assert phase in out, f"{phase} missing:\n{out}"


def test_crc32c_known_vectors():
    from elbencho_amd import load_core
    core = load_core()
    assert core.crc32c(b"123456789") == 0xE3069283  # RFC 3720 test vector
    assert core.crc32c(b"") == 0
    assert core.crc32c(b"a" * 32) == core.crc32c(b"a" * 32)


def test_checksum_headers():
    import base64
    import hashlib as _hl
    import struct
    import zlib
    c = S3Client("http://127.0.0.1:1", "k", "s", checksum_algo="CRC32")
    h = c._checksum_headers(b"hello")
    assert h["x-amz-sdk-checksum-algorithm"] == "CRC32"
    assert base64.b64decode(h["x-amz-checksum-crc32"]) == \
        struct.pack(">I", zlib.crc32(b"hello") & 0xFFFFFFFF)
    c = S3Client("http://127.0.0.1:1", "k", "s", checksum_algo="sha256")
    h = c._checksum_headers(b"hello")
    assert base64.b64decode(h["x-amz-checksum-sha256"]) == \
        _hl.sha256(b"hello").digest()
    c = S3Client("http://127.0.0.1:1", "k", "s", checksum_algo="CRC32C")
    h = c._checksum_headers(b"123456789")
    assert base64.b64decode(h["x-amz-checksum-crc32c"]) == bytes.fromhex("e3069283")


def test_session_token_and_checksum_roundtrip(mock_s3):
    """Session token goes into the signed headers; the SigV4-verifying mock
    accepts the signature, and checksum headers ride along on uploads."""
    c = S3Client(mock_s3, ACCESS_KEY, SECRET_KEY, session_token="tok-123",
                 checksum_algo="CRC32")
    c.create_bucket("tokbkt")
    c.put_object("tokbkt", "o1", b"data-with-token")
    assert c.get_object("tokbkt", "o1") == b"data-with-token"


def test_virtual_addressing_rewrite():
    """--s3virtaddr: bucket moves from the path to the Host header."""
    captured = {}

    class _FakeResp:
        status = 200

        def read(self):
            return b""

        def getheaders(self):
            return {}

    class _FakeConn:
        def request(self, method, url, body=None, headers=None):
            captured.update(method=method, url=url, headers=headers)

        def getresponse(self):
            return _FakeResp()

        def close(self):
            pass

    c = S3Client("http://s3.example.com:9000", "k", "s", virtual_addressing=True)
    c._conn = _FakeConn()
    c._connect = lambda: None
    c.request("GET", "/mybucket/some/key")
    assert captured["url"] == "/some/key"
    assert captured["headers"]["host"] == "mybucket.s3.example.com:9000"
    # authorization must sign that same host header
    assert "host" in captured["headers"]["Authorization"]


def test_acl_value_helper():
    from elbencho_amd.config import BenchConfig
    from elbencho_amd.s3 import acl_value
    cfg = BenchConfig()
    assert acl_value(cfg) == "private"
    cfg.s3_acl_grantee = "public-read"
    assert acl_value(cfg) == "public-read"
    cfg.s3_acl_grantee = "user@example.org"
    cfg.s3_acl_gtype = "emailAddress"
    cfg.s3_acl_grants = "READ,FULL_CONTROL"
    h = acl_value(cfg)
    assert h["x-amz-grant-read"] == 'emailAddress="user@example.org"'
    assert h["x-amz-grant-full-control"] == 'emailAddress="user@example.org"'
    cfg.s3_acl_grants = ""
    with pytest.raises(S3Error):
        acl_value(cfg)


def test_s3_mpu_split_and_sizevar(mock_s3):
    # part size override: 192k object with 48k parts -> 4 parts per object
    rc = _cli(mock_s3, ["-d", "-w", "-r", "-t", "1", "-N", "1", "-s", "192k",
                        "-b", "64k", "--s3mpusplit", "48k", "--verify", "3",
                        "s3://splitbkt"])
    assert rc == 0
    # part size variance: every part shrinks by up to 8k, data still verifies
    rc = _cli(mock_s3, ["-d", "-w", "-r", "-t", "1", "-N", "1", "-s", "192k",
                        "-b", "64k", "--s3mpusizevar", "8k", "--verify", "3",
                        "s3://varbkt"])
    assert rc == 0


def test_s3_mpu_sharing_workers(mock_s3):
    """--s3mpusharing: named objects are uploaded by all workers together
    (round-robin parts of one shared multipart upload per object)."""
    rc = _cli(mock_s3, ["-d", "-w", "-t", "2", "-s", "320k", "-b", "64k",
                        "--s3mpusharing", "--verify", "6",
                        "shbkt/obj1", "shbkt/obj2"])
    assert rc == 0
    from tests.s3mock import S3Handler
    with S3Handler.store.lock:
        assert len(S3Handler.store.buckets["shbkt"]) == 2
        assert len(S3Handler.store.buckets["shbkt"]["obj1"]) == 320 * 1024
        assert not S3Handler.store.uploads  # completed by the last finisher
    # shared ranged read-back with verification, then stat + delete
    rc = _cli(mock_s3, ["-r", "--stat", "-F", "-t", "2", "-s", "320k", "-b", "64k",
                        "--s3mpusharing", "--verify", "6",
                        "shbkt/obj1", "shbkt/obj2"])
    assert rc == 0
    with S3Handler.store.lock:
        assert S3Handler.store.buckets["shbkt"] == {}


def test_s3_single_shared_client(mock_s3, capsys):
    rc = _cli(mock_s3, ["-d", "-w", "-r", "-F", "-t", "4", "-N", "2", "-s", "32k",
                        "-b", "32k", "--s3single", "--verify", "2", "s3://snglbkt"])
    assert rc == 0
    out = capsys.readouterr().out
    for line in out.splitlines():
        if "Objects total" in line:
            assert line.split()[-1] == "8"
            break


def test_s3_10k_part_check():
    from elbencho_amd.cli import build_parser, args_to_config
    from elbencho_amd.config import ConfigError
    base = ["--s3endpoints", "http://x:1", "-w", "-N", "1", "-t", "1",
            "-s", "11M", "-b", "1k", "s3://b"]
    p = build_parser()
    with pytest.raises(ConfigError, match="10,000 parts"):
        args_to_config(p.parse_args(base))
    cfg = args_to_config(p.parse_args(base + ["--s3nompcheck"]))
    assert cfg.s3_no_mp_check


def test_s3_fastput_unsigned_payload(mock_s3, capsys):
    """--s3fastput: uploads go out with UNSIGNED-PAYLOAD (no per-block
    SHA256); the SigV4 mock accepts the signature."""
    rc = _cli(mock_s3, ["-d", "-w", "-r", "-t", "1", "-N", "2", "-s", "64k",
                        "-b", "64k", "--s3fastput", "s3://fastbkt"])
    assert rc == 0
    c = S3Client(mock_s3, ACCESS_KEY, SECRET_KEY, sign_payload=False)
    c.create_bucket("fp2")
    c.put_object("fp2", "o", b"x" * 100)
    assert c.get_object("fp2", "o") == b"x" * 100


def test_s3_iodepth_pipelined(mock_s3, capsys):
    """--iodepth pipelines part uploads and ranged downloads per worker
    (reference async multipart pipelining)."""
    rc = _cli(mock_s3, ["-d", "-w", "-r", "-t", "2", "-N", "2", "-s", "256k",
                        "-b", "32k", "--iodepth", "4", "--verify", "9",
                        "--lat", "s3://pipebkt"])
    assert rc == 0
    out = capsys.readouterr().out
    for line in out.splitlines():
        if "Objects total" in line:
            assert line.split()[-1] == "4"
            break
    else:
        raise AssertionError("no Objects total row")


def test_s3_worker_error_does_not_hang_pipeline(mock_s3):
    """A failing pipelined download (missing object) aborts cleanly without
    hanging the pool or the phase."""
    c = S3Client(mock_s3, ACCESS_KEY, SECRET_KEY)
    c.create_bucket("errbkt")
    c.put_object("errbkt", "r0-f0", b"x" * (64 * 1024))  # only one of two
    rc = _cli(mock_s3, ["-r", "-t", "1", "-N", "2", "-s", "64k", "-b", "16k",
                        "--iodepth", "4", "s3://errbkt"])
    assert rc != 0  # r0-f1 is missing -> phase fails, process exits promptly


def test_s3_rwmix_dedicated_readers(mock_s3, capsys):
    """--rwmixthr in the S3 WRITE phase: the first K threads download the
    pre-written objects while the rest upload (reference
    s3ModeIterateObjects isRWMixedReader); read results appear in the rwmix
    read columns."""
    # pre-write the reader threads' objects (mix reads need existing data)
    rc = _cli(mock_s3, ["-d", "-w", "-t", "4", "-N", "2", "-s", "64k",
                        "-b", "64k", "--verify", "4", "s3://mixbkt"])
    assert rc == 0
    capsys.readouterr()  # drop the pre-write output
    rc = _cli(mock_s3, ["-w", "-t", "4", "--rwmixthr", "2", "-N", "2",
                        "-s", "64k", "-b", "64k", "--verify", "4",
                        "s3://mixbkt"])
    assert rc == 0
    out = capsys.readouterr().out
    assert "MiB/s read" in out  # rwmix read rows present
    for line in out.splitlines():
        if "Objects total" in line:
            # 2 writer threads x 2 objects written; readers tracked separately
            assert line.split()[-1] == "4"
            break


def test_native_dataplane_roundtrip_and_verify():
    """Native C++ data plane (csrc/httpdata.h) against the native bench
    server: PUT/GET with pattern bodies verify clean; a salt mismatch is
    detected as corruption."""
    from elbencho_amd import load_core
    from elbencho_amd.s3 import S3Client

    core = load_core()
    srv = core.S3BenchServer(0, 7)
    try:
        c = S3Client(f"http://127.0.0.1:{srv.port()}", "k", "s")
        assert c.attach_native(-1, 1 << 20)
        c.create_bucket("nb")
        etag = c.put_object_native("nb", "obj", 4 * 1024 * 1024, 0, 7)
        assert etag
        got = c.get_object_native("nb", "obj", (0, 1024 * 1024 - 1), 0, 7)
        assert got == 1024 * 1024
        # middle range: pattern offset = range start
        got = c.get_object_native("nb", "obj", (1 << 20, (2 << 20) - 1),
                                  1 << 20, 7)
        assert got == 1 << 20
        # wrong salt -> verification failure
        import pytest as _pytest
        from elbencho_amd.s3 import S3Error
        with _pytest.raises(S3Error, match="verification failed"):
            c.get_object_native("nb", "obj", (0, (1 << 20) - 1), 0, 5)
        # multipart via native part PUTs
        uid = c.create_multipart("nb", "mp")
        e1 = c.put_object_native("nb", "mp", 1 << 20, 0, 7,
                                 query={"partNumber": "1", "uploadId": uid})
        e2 = c.put_object_native("nb", "mp", 1 << 20, 1 << 20, 7,
                                 query={"partNumber": "2", "uploadId": uid})
        c.complete_multipart("nb", "mp", uid, [(1, e1), (2, e2)])
        assert c.get_object_native("nb", "mp", (0, (2 << 20) - 1), 0, 7) \
            == 2 << 20
        c.close()
    finally:
        srv.stop()


def test_native_dataplane_cli_end_to_end():
    """CLI S3 write+read against the native server with the native client
    data plane on (default): full phase accounting."""
    import json
    import os
    import tempfile

    from elbencho_amd import load_core
    from elbencho_amd.cli import main

    core = load_core()
    srv = core.S3BenchServer(0, 3)
    try:
        with tempfile.TemporaryDirectory() as td:
            jf = os.path.join(td, "r.json")
            rc = main(["--s3endpoints", f"http://127.0.0.1:{srv.port()}",
                       "--s3key", "k", "--s3secret", "s", "--nolive",
                       "-w", "-r", "-t", "2", "-N", "2", "-s", "24m",
                       "-b", "8m", "--verify", "3", "--jsonfile", jf,
                       "s3://clibkt"])
            assert rc == 0
            docs = [json.loads(ln) for ln in open(jf)]
            assert [d["phase_type"] for d in docs] == ["WRITE", "READ"]
            for d in docs:
                assert d["last_done"]["bytes"] == 2 * 2 * 24 * 1024 * 1024
    finally:
        srv.stop()


def test_native_dataplane_against_sigv4_mock(mock_s3):
    """The native plane signs UNSIGNED-PAYLOAD requests the strict mock
    accepts, and PUT bodies carry the real checksum pattern (read back
    through the pure-python path and verified on CPU)."""
    from elbencho_amd import load_core
    from elbencho_amd.s3 import S3Client
    from tests.s3mock import ACCESS_KEY, SECRET_KEY

    c = S3Client(mock_s3, ACCESS_KEY, SECRET_KEY)
    assert c.attach_native(-1, 1 << 20)
    c.create_bucket("nmock")
    c.put_object_native("nmock", "o", 65536, 0, 9)
    data = c.get_object("nmock", "o")
    assert load_core().verify_checksum(data, 0, 9) == 2**64 - 1
    assert c.get_object_native("nmock", "o", (0, 65535), 0, 9) == 65536
    c.close()


def test_native_dataplane_released_after_run(mock_s3):
    """Native planes (and their GPU contexts) are torn down eagerly when a
    run ends — not left to the cyclic GC (VRAM leak regression, r02 soak)."""
    from elbencho_amd import load_core
    from elbencho_amd.cli import main
    from tests.s3mock import ACCESS_KEY, SECRET_KEY

    core = load_core()
    for _ in range(2):
        rc = main(["--s3endpoints", mock_s3, "--s3key", ACCESS_KEY,
                   "--s3secret", SECRET_KEY, "--nolive", "-d", "-w", "-r",
                   "-F", "-D", "-t", "4", "-N", "2", "-s", "2m", "-b", "1m",
                   "--verify", "5", "s3://relchk"])
        assert rc == 0
        assert core.http_dataplane_live() == 0


def test_native_dataplane_released_after_failed_pipeline(mock_s3):
    """A failed --iodepth run releases its native planes without the cyclic
    GC: the failed task's traceback keeps its client alive in a reference
    cycle, which must not keep the plane with it."""
    import gc

    from elbencho_amd import load_core

    core = load_core()
    c = S3Client(mock_s3, ACCESS_KEY, SECRET_KEY)
    c.create_bucket("errrel")
    c.put_object("errrel", "r0-f0", b"x" * (64 * 1024))  # only one of two
    gc.collect()
    before = core.http_dataplane_live()
    gc.disable()
    try:
        rc = _cli(mock_s3, ["-r", "-t", "1", "-N", "2", "-s", "64k", "-b",
                            "16k", "--iodepth", "4", "s3://errrel"])
        assert rc != 0
        assert core.http_dataplane_live() == before
    finally:
        gc.enable()


@pytest.mark.parametrize("seed", range(10))
def test_fuzz_native_endpoint_flags(seed, tmp_path):
    """Flag-combination fuzz against the native C++ endpoint with the
    native data plane on: no tracebacks, rc in {0,1}."""
    import contextlib
    import io
    import random

    from elbencho_amd import load_core
    from elbencho_amd.cli import main

    core = load_core()
    srv = core.S3BenchServer(0, 3)
    try:
        ep = f"http://127.0.0.1:{srv.port()}"
        rng = random.Random(7000 + seed)
        argv = ["--nolive", "--timelimit", "30", "--s3endpoints", ep,
                "--s3key", "k", "--s3secret", "s"]
        pool = [
            ("-w", None), ("-r", None), ("--stat", None), ("-F", None),
            ("-d", None), ("-D", None), ("-t", ["1", "2"]),
            ("-n", ["0", "2"]), ("-N", ["1", "4"]),
            ("-s", ["0", "4k", "12m"]), ("-b", ["4k", "1m", "8m"]),
            ("--iodepth", ["1", "4"]), ("--verify", ["3"]), ("--lat", None),
            ("--s3fastget", None), ("--s3single", None),
            ("--s3nompucompl", None), ("--s3mpusplit", ["2m"]),
            ("--rwmixthr", ["1"]), ("--s3randobj", None),
            ("--randamount", ["8m"]),
        ]
        for flag, values in pool:
            if rng.random() < 0.3:
                argv.append(flag)
                if values:
                    argv.append(rng.choice(values))
        argv.append(f"s3://fz{seed}")
        buf = io.StringIO()
        try:
            with contextlib.redirect_stdout(buf), \
                    contextlib.redirect_stderr(buf):
                rc = main(list(argv))
        except SystemExit:
            return
        assert rc in (0, 1), (rc, argv, buf.getvalue()[-500:])
        assert "Traceback" not in buf.getvalue(), (argv, buf.getvalue()[-800:])
    finally:
        srv.stop()
