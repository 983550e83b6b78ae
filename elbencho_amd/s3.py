"""S3 object storage engine.

Reference analogue: the LocalWorker S3 engine (+ toolkits/S3Tk,
S3UploadStore) — /root/reference/source/workers/LocalWorker.cpp:3822-7290:
bucket create/delete, single-part and multipart upload, (ranged) download,
HEAD, listing (+verify), multi-delete, random-object reads, object prefix,
integrity verify. Independent implementation: a minimal SigV4 REST client on
http.client with one persistent connection per worker thread (the reference
links the AWS SDK; this environment has no SDK and S3 throughput is
network-bound, so a native-C++ client is not the bottleneck).

Endpoint round-robin across workers matches S3Tk.cpp:167.
"""

from __future__ import annotations

import datetime
import hashlib
import os
import re
import hmac
import http.client
import threading
import time
import urllib.parse
import xml.etree.ElementTree as ET
from dataclasses import dataclass
from typing import Any, Optional

from elbencho_amd import load_core
from elbencho_amd.config import BenchConfig
from elbencho_amd.histogram import Histogram
from elbencho_amd.stats import WorkerStats

EMPTY_SHA256 = hashlib.sha256(b"").hexdigest()
# --s3chksumalgo values whose checksum the native data plane computes itself
NATIVE_CRC_ALGOS = ("CRC32", "CRC32C", "CRC64NVME")


class S3Error(RuntimeError):
    pass


# ---------------------------------------------------------------------------
# SigV4 signing + REST client
# ---------------------------------------------------------------------------

class S3Client:
    """One S3 endpoint connection with AWS Signature V4 (path-style URLs)."""

    def __init__(self, endpoint: str, access_key: str, secret_key: str,
                 region: str = "us-east-1", timeout: float = 60.0,
                 extra_put_headers: dict[str, str] | None = None,
                 session_token: str = "", virtual_addressing: bool = False,
                 checksum_algo: str = "", trace=None, sign_payload: bool = True):
        self.extra_put_headers = extra_put_headers or {}
        u = urllib.parse.urlparse(endpoint if "//" in endpoint else "http://" + endpoint)
        self.host = u.hostname or "localhost"
        self.port = u.port or (443 if u.scheme == "https" else 80)
        self.secure = u.scheme == "https"
        self.access_key = access_key
        self.secret_key = secret_key
        self.region = region or "us-east-1"
        self.timeout = timeout
        self.session_token = session_token        # --s3sessiontoken
        self.virtual_addressing = virtual_addressing  # --s3virtaddr
        self.checksum_algo = checksum_algo.upper()    # --s3chksumalgo
        self.trace = trace                        # --s3log sink: fn(str)
        # --s3sign 2 / --s3fastput: skip the per-block SHA256 of upload
        # payloads (UNSIGNED-PAYLOAD); a real CPU saving in this native
        # client, unlike the SDK (reference ProgArgs.cpp:738-741)
        self.sign_payload = sign_payload
        # --s3single shares one client across worker threads; the connection
        # handles one request at a time, so serialize (uncontended otherwise)
        self.lock = threading.Lock()
        self._conn: Optional[http.client.HTTPConnection] = None
        self.native = None  # HttpDataPlane (attach_native)

    # --- low level ---
    def _connect(self):
        cls = http.client.HTTPSConnection if self.secure else http.client.HTTPConnection
        self._conn = cls(self.host, self.port, timeout=self.timeout)

    def close(self):
        if self._conn:
            self._conn.close()
            self._conn = None
        if self.native:
            self.native.close()

    # --- native data plane (csrc/httpdata.h): block bodies in C++ ---
    def attach_native(self, dev: int, max_block: int) -> bool:
        """Route object-body transfers through the native data plane
        (SigV4 signing stays here). Not used with HTTPS, nor with SHA1 /
        SHA256 checksums (those need the body bytes in Python). CRC32,
        CRC32C and CRC64NVME stay native: the plane computes the checksum of
        the body it is about to generate (HttpDataPlane.body_crc — in HBM for
        pattern bodies when a device is attached)."""
        if self.secure or self.checksum_algo not in ("",) + NATIVE_CRC_ALGOS:
            return False
        self.native = load_core().HttpDataPlane(
            self.host, self.port, dev, max_block,
            0x243F6A8885A308D3 ^ (dev + 2))
        return True

    def _native_raw_request(self, method: str, path: str,
                            query: dict[str, str] | None,
                            headers: dict[str, str], content_len: int) -> bytes:
        headers = self._sign(method, path, query or {}, headers,
                             "UNSIGNED-PAYLOAD")
        qs = urllib.parse.urlencode(query or {}, quote_via=urllib.parse.quote)
        url = urllib.parse.quote(path) + ("?" + qs if qs else "")
        lines = [f"{method} {url} HTTP/1.1"]
        lines += [f"{k}: {v}" for k, v in headers.items()]
        lines.append(f"content-length: {content_len}")
        return ("\r\n".join(lines) + "\r\n\r\n").encode()

    def put_object_native(self, bucket: str, key: str, length: int,
                          pattern_off: int, salt: int,
                          query: dict[str, str] | None = None) -> str:
        """PUT with a natively generated body (checksum pattern when
        salt >= 0, random otherwise). Returns the ETag. With a CRC32 /
        CRC32C / CRC64NVME checksum_algo the plane computes the body's
        checksum first and it rides in the signed headers (multipart parts
        included)."""
        with self.lock:
            headers = dict(self.extra_put_headers)
            if self.checksum_algo:
                import base64
                import struct
                algo = self.checksum_algo
                crc = self.native.body_crc(length, pattern_off, salt, algo)
                headers["x-amz-sdk-checksum-algorithm"] = algo
                headers[f"x-amz-checksum-{algo.lower()}"] = \
                    base64.b64encode(struct.pack(
                        ">Q" if algo == "CRC64NVME" else ">I", crc)).decode()
            req = self._native_raw_request(
                "PUT", f"/{bucket}/{key}", query, dict(headers), length)
            status, raw_hdrs = self.native.put(req, length, pattern_off, salt)
            if status < 0:  # connection problem: one clean retry
                req = self._native_raw_request(
                    "PUT", f"/{bucket}/{key}", query, dict(headers), length)
                status, raw_hdrs = self.native.put(req, length, pattern_off,
                                                   salt)
        self._check(status if status > 0 else 599, b"",
                    f"native put {bucket}/{key}")
        m = re.search(r"(?im)^etag:\s*(\S+)\s*$", raw_hdrs)
        return m.group(1) if m else '"native"'

    def get_object_native(self, bucket: str, key: str,
                          byte_range: tuple[int, int] | None,
                          pattern_off: int, salt: int) -> int:
        """Ranged GET received and (when salt >= 0) verified natively.
        Returns bytes received; raises on HTTP error or verify mismatch."""
        headers = {}
        expect = 1 << 30
        if byte_range:
            headers["range"] = f"bytes={byte_range[0]}-{byte_range[1]}"
            expect = byte_range[1] - byte_range[0] + 1
        with self.lock:
            req = self._native_raw_request("GET", f"/{bucket}/{key}",
                                           None, headers, 0)
            status, got, nbad, first = self.native.get(req, expect,
                                                       pattern_off, salt)
            if status < 0:
                req = self._native_raw_request("GET", f"/{bucket}/{key}",
                                               None, headers, 0)
                status, got, nbad, first = self.native.get(req, expect,
                                                           pattern_off, salt)
        self._check(status if status > 0 else 599, b"",
                    f"native get {bucket}/{key}")
        if nbad:
            raise S3Error(f"S3 data verification failed for {bucket}/{key} "
                          f"at object offset {first} ({nbad} bad blocks)")
        return got

    def _sign(self, method: str, path: str, query: dict[str, str],
              headers: dict[str, str], payload_hash: str,
              host: str | None = None) -> dict[str, str]:
        now = datetime.datetime.now(datetime.timezone.utc)
        amz_date = now.strftime("%Y%m%dT%H%M%SZ")
        datestamp = now.strftime("%Y%m%d")

        headers = dict(headers)
        headers["host"] = host or f"{self.host}:{self.port}"
        headers["x-amz-date"] = amz_date
        headers["x-amz-content-sha256"] = payload_hash
        if self.session_token:
            headers["x-amz-security-token"] = self.session_token

        canonical_query = "&".join(
            f"{urllib.parse.quote(k, safe='')}={urllib.parse.quote(v, safe='')}"
            for k, v in sorted(query.items()))
        signed_headers = ";".join(sorted(h.lower() for h in headers))
        canonical_headers = "".join(
            f"{k.lower()}:{headers[k].strip()}\n" for k in sorted(headers, key=str.lower))
        canonical_request = "\n".join([
            method, urllib.parse.quote(path), canonical_query, canonical_headers,
            signed_headers, payload_hash])

        scope = f"{datestamp}/{self.region}/s3/aws4_request"
        string_to_sign = "\n".join([
            "AWS4-HMAC-SHA256", amz_date, scope,
            hashlib.sha256(canonical_request.encode()).hexdigest()])

        def hmac_sha256(key: bytes, msg: str) -> bytes:
            return hmac.new(key, msg.encode(), hashlib.sha256).digest()

        k = hmac_sha256(("AWS4" + self.secret_key).encode(), datestamp)
        k = hmac_sha256(k, self.region)
        k = hmac_sha256(k, "s3")
        k = hmac_sha256(k, "aws4_request")
        sig = hmac.new(k, string_to_sign.encode(), hashlib.sha256).hexdigest()

        headers["Authorization"] = (
            f"AWS4-HMAC-SHA256 Credential={self.access_key}/{scope}, "
            f"SignedHeaders={signed_headers}, Signature={sig}")
        return headers

    def request(self, method: str, path: str, query: dict[str, str] | None = None,
                body: bytes = b"", headers: dict[str, str] | None = None,
                want_body: bool = True) -> tuple[int, bytes, dict[str, str]]:
        query = query or {}
        headers = headers or {}
        host = None
        if self.virtual_addressing and len(path) > 1:
            # bucket as subdomain of the endpoint host (the TCP connection
            # stays on the configured endpoint, like curl --resolve)
            bucket, _, rest = path[1:].partition("/")
            path = "/" + rest
            host = f"{bucket}.{self.host}:{self.port}"
        if body and not self.sign_payload:
            payload_hash = "UNSIGNED-PAYLOAD"
        else:
            payload_hash = hashlib.sha256(body).hexdigest() if body else EMPTY_SHA256
        headers = self._sign(method, path, query, headers, payload_hash, host=host)

        # Must match the canonical query encoding used in _sign (quote with
        # safe='', space -> %20): urlencode's quote_plus would produce '+' and
        # strict servers reject the signature.
        qs = urllib.parse.urlencode(query, quote_via=urllib.parse.quote)
        url = path + ("?" + qs if qs else "")

        with self.lock:
            for attempt in (0, 1):  # one reconnect retry on stale connections
                if self._conn is None:
                    self._connect()
                try:
                    self._conn.request(method, url, body=body or None, headers=headers)
                    resp = self._conn.getresponse()
                    data = resp.read() if want_body else resp.read()
                    if self.trace:
                        self.trace(f"{method} {headers['host']}{url} "
                                   f"len={len(body)} -> {resp.status}")
                    return resp.status, data, dict(resp.getheaders())
                except (ConnectionError, http.client.HTTPException, OSError):
                    self.close()
                    if attempt:
                        if self.trace:
                            self.trace(f"{method} {url} -> connection error")
                        raise
        raise S3Error("unreachable")

    # --s3chksumalgo: x-amz-sdk-checksum-algorithm + the computed
    # x-amz-checksum-* trailer header (the reference delegates to the AWS SDK;
    # this client computes the digest itself — CRC32C via the native core)
    def _checksum_headers(self, body: bytes) -> dict[str, str]:
        if not self.checksum_algo:
            return {}
        import base64
        import struct
        import zlib
        algo = self.checksum_algo
        if algo == "CRC32":
            digest = struct.pack(">I", zlib.crc32(body) & 0xFFFFFFFF)
        elif algo == "CRC32C":
            digest = struct.pack(">I", load_core().crc32c(body))
        elif algo == "CRC64NVME":
            digest = struct.pack(">Q", load_core().crc(body, "CRC64NVME"))
        elif algo == "SHA1":
            digest = hashlib.sha1(body).digest()
        else:  # SHA256
            digest = hashlib.sha256(body).digest()
        return {"x-amz-sdk-checksum-algorithm": algo,
                f"x-amz-checksum-{algo.lower()}": base64.b64encode(digest).decode()}

    def _check(self, status: int, data: bytes, what: str):
        if status >= 300:
            raise S3Error(f"{what} failed: HTTP {status}: {data[:300].decode(errors='replace')}")

    # --- bucket ops ---
    def create_bucket(self, bucket: str):
        status, data, _ = self.request("PUT", f"/{bucket}")
        if status == 409:  # BucketAlreadyOwnedByYou — idempotent like the reference
            return
        self._check(status, data, f"create bucket {bucket}")

    def delete_bucket(self, bucket: str):
        status, data, _ = self.request("DELETE", f"/{bucket}")
        self._check(status, data, f"delete bucket {bucket}")

    def head_bucket(self, bucket: str) -> bool:
        status, _, _ = self.request("HEAD", f"/{bucket}", want_body=False)
        return status < 300

    # --- object ops ---
    def put_object(self, bucket: str, key: str, body: bytes):
        headers = dict(self.extra_put_headers)
        headers.update(self._checksum_headers(body))
        status, data, _ = self.request("PUT", f"/{bucket}/{key}", body=body,
                                       headers=headers)
        self._check(status, data, f"put {bucket}/{key}")

    def get_object(self, bucket: str, key: str,
                   byte_range: tuple[int, int] | None = None) -> bytes:
        headers = {}
        if byte_range:
            headers["Range"] = f"bytes={byte_range[0]}-{byte_range[1]}"
        status, data, _ = self.request("GET", f"/{bucket}/{key}", headers=headers)
        self._check(status, data, f"get {bucket}/{key}")
        return data

    def head_object(self, bucket: str, key: str) -> dict[str, str]:
        status, data, headers = self.request("HEAD", f"/{bucket}/{key}", want_body=False)
        self._check(status, b"", f"head {bucket}/{key}")
        return headers

    def delete_object(self, bucket: str, key: str):
        status, data, _ = self.request("DELETE", f"/{bucket}/{key}")
        self._check(status, data, f"delete {bucket}/{key}")

    def multi_delete(self, bucket: str, keys: list[str]):
        objs = "".join(f"<Object><Key>{k}</Key></Object>" for k in keys)
        body = (f"<Delete><Quiet>true</Quiet>{objs}</Delete>").encode()
        md5 = __import__("base64").b64encode(hashlib.md5(body).digest()).decode()
        status, data, _ = self.request("POST", f"/{bucket}", query={"delete": ""},
                                       body=body, headers={"Content-MD5": md5})
        self._check(status, data, f"multi-delete in {bucket}")

    def list_objects(self, bucket: str, prefix: str = "", max_keys: int = 1000,
                     continuation: str = "") -> tuple[list[tuple[str, int]], str]:
        q = {"list-type": "2", "max-keys": str(max_keys)}
        if prefix:
            q["prefix"] = prefix
        if continuation:
            q["continuation-token"] = continuation
        status, data, _ = self.request("GET", f"/{bucket}", query=q)
        self._check(status, data, f"list {bucket}")
        root = ET.fromstring(data)
        ns = root.tag.split("}")[0] + "}" if "}" in root.tag else ""
        out = []
        for c in root.findall(f"{ns}Contents"):
            key = c.find(f"{ns}Key").text
            size = int(c.find(f"{ns}Size").text)
            out.append((key, size))
        token_el = root.find(f"{ns}NextContinuationToken")
        return out, (token_el.text if token_el is not None else "")

    # --- ACL (canned or grantee headers) ---
    def put_object_acl(self, bucket: str, key: str, acl):
        headers = {"x-amz-acl": acl} if isinstance(acl, str) else dict(acl)
        status, data, _ = self.request("PUT", f"/{bucket}/{key}", query={"acl": ""},
                                       headers=headers)
        self._check(status, data, f"put acl {bucket}/{key}")

    def get_object_acl(self, bucket: str, key: str) -> bytes:
        status, data, _ = self.request("GET", f"/{bucket}/{key}", query={"acl": ""})
        self._check(status, data, f"get acl {bucket}/{key}")
        return data

    def put_bucket_acl(self, bucket: str, acl):
        headers = {"x-amz-acl": acl} if isinstance(acl, str) else dict(acl)
        status, data, _ = self.request("PUT", f"/{bucket}", query={"acl": ""},
                                       headers=headers)
        self._check(status, data, f"put bucket acl {bucket}")

    def get_bucket_acl(self, bucket: str) -> bytes:
        status, data, _ = self.request("GET", f"/{bucket}", query={"acl": ""})
        self._check(status, data, f"get bucket acl {bucket}")
        return data

    # --- tagging ---
    @staticmethod
    def _tagset_xml(tags: dict[str, str]) -> bytes:
        inner = "".join(f"<Tag><Key>{k}</Key><Value>{v}</Value></Tag>"
                        for k, v in tags.items())
        return f"<Tagging><TagSet>{inner}</TagSet></Tagging>".encode()

    def put_object_tagging(self, bucket: str, key: str, tags: dict[str, str]):
        status, data, _ = self.request("PUT", f"/{bucket}/{key}", query={"tagging": ""},
                                       body=self._tagset_xml(tags))
        self._check(status, data, f"put tagging {bucket}/{key}")

    def get_object_tagging(self, bucket: str, key: str) -> dict[str, str]:
        status, data, _ = self.request("GET", f"/{bucket}/{key}", query={"tagging": ""})
        self._check(status, data, f"get tagging {bucket}/{key}")
        import re as _re
        return dict(_re.findall(r"<Key>([^<]*)</Key><Value>([^<]*)</Value>",
                                data.decode()))

    def delete_object_tagging(self, bucket: str, key: str):
        status, data, _ = self.request("DELETE", f"/{bucket}/{key}", query={"tagging": ""})
        if status not in (200, 204):
            self._check(status, data, f"delete tagging {bucket}/{key}")

    def put_bucket_tagging(self, bucket: str, tags: dict[str, str]):
        status, data, _ = self.request("PUT", f"/{bucket}", query={"tagging": ""},
                                       body=self._tagset_xml(tags))
        self._check(status, data, f"put bucket tagging {bucket}")

    def get_bucket_tagging(self, bucket: str) -> dict[str, str]:
        status, data, _ = self.request("GET", f"/{bucket}", query={"tagging": ""})
        self._check(status, data, f"get bucket tagging {bucket}")
        import re as _re
        return dict(_re.findall(r"<Key>([^<]*)</Key><Value>([^<]*)</Value>",
                                data.decode()))

    # --- versioning / object lock ---
    def put_bucket_versioning(self, bucket: str, enabled: bool):
        body = (f"<VersioningConfiguration><Status>"
                f"{'Enabled' if enabled else 'Suspended'}</Status>"
                f"</VersioningConfiguration>").encode()
        status, data, _ = self.request("PUT", f"/{bucket}", query={"versioning": ""},
                                       body=body)
        self._check(status, data, f"put bucket versioning {bucket}")

    def get_bucket_versioning(self, bucket: str) -> str:
        status, data, _ = self.request("GET", f"/{bucket}", query={"versioning": ""})
        self._check(status, data, f"get bucket versioning {bucket}")
        import re as _re
        m = _re.search(r"<Status>([^<]*)</Status>", data.decode())
        return m.group(1) if m else ""

    def put_object_lock_config(self, bucket: str, mode: str = "GOVERNANCE",
                               days: int = 1):
        body = (f"<ObjectLockConfiguration><ObjectLockEnabled>Enabled"
                f"</ObjectLockEnabled><Rule><DefaultRetention><Mode>{mode}</Mode>"
                f"<Days>{days}</Days></DefaultRetention></Rule>"
                f"</ObjectLockConfiguration>").encode()
        status, data, _ = self.request("PUT", f"/{bucket}", query={"object-lock": ""},
                                       body=body)
        self._check(status, data, f"put object lock config {bucket}")

    def get_object_lock_config(self, bucket: str) -> bytes:
        status, data, _ = self.request("GET", f"/{bucket}", query={"object-lock": ""})
        self._check(status, data, f"get object lock config {bucket}")
        return data

    # --- multipart ---
    def create_multipart(self, bucket: str, key: str) -> str:
        headers = dict(self.extra_put_headers)
        if self.checksum_algo == "CRC64NVME":
            # the only S3 checksum defined over the whole object of a
            # multipart upload; S3 wants both declared at initiation before
            # it accepts parts that carry x-amz-checksum-crc64nvme
            headers["x-amz-checksum-algorithm"] = "CRC64NVME"
            headers["x-amz-checksum-type"] = "FULL_OBJECT"
        status, data, _ = self.request("POST", f"/{bucket}/{key}", query={"uploads": ""},
                                       headers=headers)
        self._check(status, data, f"initiate multipart {bucket}/{key}")
        root = ET.fromstring(data)
        ns = root.tag.split("}")[0] + "}" if "}" in root.tag else ""
        return root.find(f"{ns}UploadId").text

    def upload_part(self, bucket: str, key: str, upload_id: str, part_num: int,
                    body: bytes) -> str:
        status, data, headers = self.request(
            "PUT", f"/{bucket}/{key}",
            query={"partNumber": str(part_num), "uploadId": upload_id}, body=body,
            headers=self._checksum_headers(body))
        self._check(status, data, f"upload part {part_num} of {bucket}/{key}")
        return headers.get("ETag", headers.get("etag", f'"{part_num}"'))

    def complete_multipart(self, bucket: str, key: str, upload_id: str,
                           parts: list[tuple[int, str]]):
        parts_xml = "".join(
            f"<Part><PartNumber>{n}</PartNumber><ETag>{etag}</ETag></Part>"
            for n, etag in sorted(parts))
        body = f"<CompleteMultipartUpload>{parts_xml}</CompleteMultipartUpload>".encode()
        status, data, _ = self.request("POST", f"/{bucket}/{key}",
                                       query={"uploadId": upload_id}, body=body)
        self._check(status, data, f"complete multipart {bucket}/{key}")

    def list_multipart_uploads(self, bucket: str,
                               prefix: str = "") -> list[tuple[str, str]]:
        """[(key, uploadId)] of in-progress multipart uploads."""
        q = {"uploads": ""}
        if prefix:
            q["prefix"] = prefix
        status, data, _ = self.request("GET", f"/{bucket}", query=q)
        self._check(status, data, f"list multipart uploads {bucket}")
        import re as _re
        return _re.findall(r"<Key>([^<]*)</Key><UploadId>([^<]*)</UploadId>",
                           data.decode())

    def list_parts(self, bucket: str, key: str, upload_id: str) -> list[tuple[int, str]]:
        status, data, _ = self.request("GET", f"/{bucket}/{key}",
                                       query={"uploadId": upload_id})
        self._check(status, data, f"list parts {bucket}/{key}")
        import re as _re
        return [(int(n), e) for n, e in
                _re.findall(r"<PartNumber>(\d+)</PartNumber><ETag>([^<]*)</ETag>",
                            data.decode())]

    def abort_multipart(self, bucket: str, key: str, upload_id: str):
        status, data, _ = self.request("DELETE", f"/{bucket}/{key}",
                                       query={"uploadId": upload_id})
        if status not in (204, 404):
            self._check(status, data, f"abort multipart {bucket}/{key}")


# canned ACL values accepted as --s3aclgrantee (reference ProgArgs.cpp:576-579)
_CANNED_ACLS = {"private", "public-read", "public-read-write", "authenticated-read"}
_ACL_PERM_HEADERS = {"READ": "x-amz-grant-read", "WRITE": "x-amz-grant-write",
                     "READ_ACP": "x-amz-grant-read-acp",
                     "WRITE_ACP": "x-amz-grant-write-acp",
                     "FULL_CONTROL": "x-amz-grant-full-control"}


def precreate_upload_ids(cfg: BenchConfig) -> dict[str, str]:
    """Create one multipart upload per shared object ("bucket/key" paths) for
    cross-instance --s3mpusharing; the ids are distributed to every instance
    so all of them add parts to the SAME upload (reference
    ProgArgs::precreateMpuIDs, ProgArgs.cpp:2950-2990)."""
    part_size = cfg.s3_mpu_split or cfg.block_size
    if cfg.file_size <= part_size:
        raise S3Error("S3 MPU sharing mode selected but object size is not "
                      "larger than part block size")
    client = S3Client(cfg.s3_endpoints[0], cfg.s3_key, cfg.s3_secret,
                      cfg.s3_region, session_token=cfg.s3_session_token,
                      virtual_addressing=cfg.s3_virt_addr)
    ids: dict[str, str] = {}
    try:
        for p in cfg.paths:
            p = p[len("s3://"):] if p.startswith("s3://") else p
            bucket, _, key = p.partition("/")
            if not key:
                raise S3Error("--s3mpusharing requires bucket/object paths")
            ids[f"{bucket}/{key}"] = client.create_multipart(bucket, key)
    finally:
        client.close()
    return ids


def build_put_headers(cfg: BenchConfig) -> dict[str, str]:
    """Upload headers from SSE (--s3sse/--s3sseckey/--s3ssekmskey) and
    inline-ACL (--s3aclputinl) options."""
    put_headers: dict[str, str] = {}
    if cfg.s3_sse:  # SSE-S3 (AES256) passthrough header
        put_headers["x-amz-server-side-encryption"] = "AES256"
    if cfg.s3_sse_kms_key:  # --s3ssekmskey
        put_headers["x-amz-server-side-encryption"] = "aws:kms"
        put_headers["x-amz-server-side-encryption-aws-kms-key-id"] = cfg.s3_sse_kms_key
    if cfg.s3_sse_c_key:  # --s3sseckey (base64 customer key + MD5)
        import base64 as _b64
        raw = _b64.b64decode(cfg.s3_sse_c_key)
        put_headers["x-amz-server-side-encryption-customer-algorithm"] = "AES256"
        put_headers["x-amz-server-side-encryption-customer-key"] = cfg.s3_sse_c_key
        put_headers["x-amz-server-side-encryption-customer-key-MD5"] = \
            _b64.b64encode(hashlib.md5(raw).digest()).decode()
    if cfg.s3_acl_put_inline:  # --s3aclputinl: ACL headers on every PUT
        acl = acl_value(cfg)
        put_headers.update({"x-amz-acl": acl} if isinstance(acl, str) else acl)
    return put_headers


def acl_value(cfg: BenchConfig):
    """Canned-ACL string or x-amz-grant-* header dict from --s3aclgrantee /
    --s3aclgtype / --s3aclgrants (reference S3 ACL grant building)."""
    grantee = cfg.s3_acl_grantee
    if not grantee:
        return cfg.s3_acl_grants or "private"  # legacy: grants as canned ACL
    if grantee in _CANNED_ACLS:
        return grantee
    gtype = cfg.s3_acl_gtype or "id"
    headers: dict[str, str] = {}
    for perm in (p.strip().upper() for p in (cfg.s3_acl_grants or "").split(",")):
        if not perm:
            continue
        if perm not in _ACL_PERM_HEADERS:
            raise S3Error(f"unknown S3 ACL permission: {perm}")
        headers[_ACL_PERM_HEADERS[perm]] = f'{gtype}="{grantee}"'
    if not headers:
        raise S3Error("--s3aclgrantee requires --s3aclgrants permissions "
                      "(READ, WRITE, READ_ACP, WRITE_ACP, FULL_CONTROL)")
    return headers


# ---------------------------------------------------------------------------
# shared multipart upload registry (reference S3UploadStore.{h,cpp})
# ---------------------------------------------------------------------------

class SharedUploadStore:
    """First-writer-wins uploadId registry + completed-part collection, so
    multiple workers can upload disjoint part ranges of one object."""

    def __init__(self):
        self.lock = threading.Lock()
        self.uploads: dict[tuple[str, str], dict] = {}

    def get_or_create(self, client: S3Client, bucket: str, key: str,
                      num_parts_total: int) -> str:
        with self.lock:
            ent = self.uploads.get((bucket, key))
            if ent is None:
                upload_id = client.create_multipart(bucket, key)
                ent = {"id": upload_id, "parts": [], "total": num_parts_total}
                self.uploads[(bucket, key)] = ent
            return ent["id"]

    def seed(self, bucket: str, key: str, upload_id: str) -> None:
        """Pre-register a master-created uploadId (cross-service
        --s3mpusharing): this instance adds parts but never completes or
        aborts the upload (total unreachable, external owner)."""
        with self.lock:
            self.uploads[(bucket, key)] = {"id": upload_id, "parts": [],
                                           "total": 1 << 62, "external": True}

    def add_part(self, bucket: str, key: str, part_num: int, etag: str) -> bool:
        """Record a completed part; True when all parts are done (the caller
        that gets True completes the upload — 'whoever finishes last')."""
        with self.lock:
            ent = self.uploads[(bucket, key)]
            ent["parts"].append((part_num, etag))
            return len(ent["parts"]) >= ent["total"]

    def get_parts(self, bucket: str, key: str) -> list[tuple[int, str]]:
        with self.lock:
            return list(self.uploads[(bucket, key)]["parts"])

    def abort_unfinished(self, client: S3Client):
        with self.lock:
            for (bucket, key), ent in self.uploads.items():
                if ent.get("external"):
                    continue  # master-owned shared upload: never abort here
                if len(ent["parts"]) < ent["total"]:
                    try:
                        client.abort_multipart(bucket, key, ent["id"])
                    except (S3Error, OSError):
                        pass


# ---------------------------------------------------------------------------
# the S3 benchmark runner (Coordinator backend)
# ---------------------------------------------------------------------------

@dataclass
class _Counters:
    entries: int = 0
    bytes: int = 0
    iops: int = 0


class S3Worker(threading.Thread):
    def __init__(self, runner: "S3Runner", local_rank: int, phase: str):
        super().__init__(daemon=True)
        self.r = runner
        self.local_rank = local_rank
        self.rank = runner.cfg.rank_offset + local_rank
        self.phase = phase
        self.ops = _Counters()
        self.sw: Optional[_Counters] = None
        self.sw_elapsed_us = 0
        self.io_lat = Histogram()
        self.entry_lat = Histogram()
        self.error = ""
        self.elapsed_us = 0
        cfg = runner.cfg
        # --rwmixthr: the first K threads of a WRITE phase read instead
        # (reference s3ModeIterateObjects isRWMixedReader); their results go
        # to the rwmix-read counter set
        self.is_mix_reader = (phase == "WRITE" and
                              local_rank < cfg._rwmix_threads_effective())
        self.rm_ops = _Counters()
        self.rm_sw: Optional[_Counters] = None
        self.io_lat_rm = Histogram()
        self.entry_lat_rm = Histogram()
        ep = cfg.s3_endpoints[self.rank % len(cfg.s3_endpoints)]
        key, secret = cfg.s3_key, cfg.s3_secret
        if runner.credentials:  # --s3credfile/--s3credlist round-robin
            key, secret = runner.credentials[self.rank % len(runner.credentials)]
        self._client_args = (ep, key, secret)
        self._pool = None  # lazy --iodepth pipelining pool
        if cfg.s3_single:
            # --s3single: one shared client instance for all worker threads
            self.client = runner.shared_client
        else:
            self.client = self._new_client()
        self.core = load_core()
        # --gpuids + --verify: verify/generate object data with the gfx950
        # kernels in HBM (BASELINE config 5); one persistent context per worker
        self.gpu = None
        if cfg.gpu_ids and cfg.verify >= 0 and self.core.gpu_device_count() > 0:
            dev = cfg.gpu_ids[self.rank % len(cfg.gpu_ids)]
            self.gpu = self.core.GpuBufferOps(dev, cfg.block_size)
        elif cfg.gpu_ids and self.core.gpu_device_count() <= 0:
            raise S3Error("GPU requested (gpuids) but no HIP device is available")

    def _new_client(self) -> S3Client:
        cfg = self.r.cfg
        ep, key, secret = self._client_args
        c = S3Client(ep, key, secret, cfg.s3_region,
                     extra_put_headers=build_put_headers(cfg),
                     session_token=cfg.s3_session_token,
                     virtual_addressing=cfg.s3_virt_addr,
                     checksum_algo=cfg.s3_chksum_algo,
                     trace=self.r.trace,
                     sign_payload=cfg.s3_sign_policy != 2)
        # native data plane (C++ block transfers; EB_S3_NATIVE=0 disables).
        # Rwmix readers always verify-read their own rank's pattern, so the
        # native path covers every body the hot loops move.
        if os.environ.get("EB_S3_NATIVE", "1") != "0":
            dev = -1
            if cfg.gpu_ids and load_core().gpu_device_count() > 0:
                dev = cfg.gpu_ids[self.rank % len(cfg.gpu_ids)]
            max_block = max(cfg.block_size, cfg.s3_mpu_split or 0, 1 << 20)
            try:
                c.attach_native(dev, max_block)
            except Exception:  # noqa: BLE001 — fall back to pure python
                c.native = None
        return c

    def _pipeline(self):
        """(executor, client queue, depth) for --iodepth S3 pipelining: up to
        iodepth part uploads / ranged downloads of one object in flight per
        worker, each pool thread with its own connection (reference async
        multipart pipelining, LocalWorker.cpp:5155/:6280)."""
        if self._pool is None:
            import queue
            from concurrent.futures import ThreadPoolExecutor
            cfg = self.r.cfg
            # --s3maxconns caps the per-worker connection count
            n = min(cfg.iodepth, cfg.s3_max_conns or 16, 16)
            clients: queue.Queue = queue.Queue()
            for _ in range(n):
                clients.put(self._new_client())
            self._pool = (ThreadPoolExecutor(max_workers=n), clients, n)
        return self._pool

    # --- object name layout mirrors dir mode: r{rank}/d{dir}/r{rank}-f{file} ---
    def _object_names(self):
        cfg = self.r.cfg
        dirs = max(cfg.dirs, 1)
        for d in range(dirs):
            for f in range(cfg.files):
                if cfg.dirs > 0:
                    yield f"{cfg.s3_obj_prefix}r{self.rank}/d{d}/r{self.rank}-f{f}"
                else:
                    yield f"{cfg.s3_obj_prefix}r{self.rank}-f{f}"

    def _bucket(self, idx: int = 0) -> str:
        buckets = self.r.buckets
        return buckets[(self.rank + idx) % len(buckets)]

    def _check_interrupt(self):
        if self.r.interrupt_flag.is_set():
            raise KeyboardInterrupt

    def _oplog(self, op: str, entry: str, offset: int, length: int, pre: bool,
               err: bool = False):
        log = self.r.ops_log
        if not log:
            return
        import json as _json
        line = _json.dumps({"rank": self.rank, "op": op, "entry": entry,
                            "offset": offset, "len": length,
                            "type": "pre" if pre else "post",
                            **({"error": True} if err else {})})
        with self.r.ops_log_lock:
            log.write(line + "\n")
            log.flush()

    def run(self):
        try:
            self.r.start_gate.wait()
            t0 = time.monotonic()
            try:
                self._run_phase()
            except S3Error as e:
                if not self.r.cfg.s3_ignore_errors:
                    raise
                # --s3ignoreerrors: record and carry on (stress-mode knob)
                self.error = f"(ignored) {e}"
            self.elapsed_us = int((time.monotonic() - t0) * 1e6)
        except KeyboardInterrupt:
            self.error = "interrupted"
        except Exception as e:  # noqa: BLE001
            self.error = str(e)
            self.r.interrupt_flag.set()
        finally:
            if self._pool is not None:
                ex, clients, _ = self._pool
                ex.shutdown(wait=True)
                while not clients.empty():
                    c = clients.get_nowait()
                    c.close()
                    # drop the plane now: a failed task's traceback keeps
                    # its client (a reference cycle) until the cyclic GC runs
                    c.native = None
                self._pool = None
            self.elapsed_us = self.elapsed_us or int(
                (time.monotonic() - self.r.phase_start) * 1e6)
            self.r.on_worker_done(self)

    # ------------------------------------------------------------------
    def _run_phase(self):
        cfg = self.r.cfg
        ph = self.phase
        if ph == "MKDIRS":  # MKBUCKETS
            for i, b in enumerate(self.r.buckets):
                if i % cfg.num_dataset_threads == self.rank:
                    self.client.create_bucket(b)
                    self.ops.entries += 1
        elif ph == "RMDIRS":  # RMBUCKETS
            for i, b in enumerate(self.r.buckets):
                if i % cfg.num_dataset_threads == self.rank:
                    self.client.delete_bucket(b)
                    self.ops.entries += 1
        elif ph == "WRITE":
            if self.is_mix_reader:
                # account into the rwmix-read counters via a counter swap
                # (the read loop only touches ops/io_lat/entry_lat)
                self.ops, self.rm_ops = self.rm_ops, self.ops
                self.io_lat, self.io_lat_rm = self.io_lat_rm, self.io_lat
                self.entry_lat, self.entry_lat_rm = self.entry_lat_rm, self.entry_lat
                try:
                    self._get_objects()
                finally:
                    self.ops, self.rm_ops = self.rm_ops, self.ops
                    self.io_lat, self.io_lat_rm = self.io_lat_rm, self.io_lat
                    self.entry_lat, self.entry_lat_rm = \
                        self.entry_lat_rm, self.entry_lat
            else:
                self._put_objects()
        elif ph == "READ":
            self._get_objects()
        elif ph == "STAT":  # HEADOBJ
            num_ranks = max(cfg.num_dataset_threads, 1)
            if cfg.s3_mpu_sharing:
                for i, (b, k) in enumerate(self.r.shared_objects):
                    if i % num_ranks != self.rank % num_ranks:
                        continue
                    self._check_interrupt()
                    t0 = time.monotonic()
                    self.client.head_object(b, k)
                    self.entry_lat.vec = _add_lat(self.entry_lat, t0)
                    self.ops.entries += 1
                return
            for name in self._object_names():
                self._check_interrupt()
                t0 = time.monotonic()
                self.client.head_object(self._bucket(), name)
                self.entry_lat.vec = _add_lat(self.entry_lat, t0)
                self.ops.entries += 1
        elif ph == "RMFILES":  # RMOBJECTS / MULTIDEL
            num_ranks = max(cfg.num_dataset_threads, 1)
            if cfg.s3_mpu_sharing:
                for i, (b, k) in enumerate(self.r.shared_objects):
                    if i % num_ranks != self.rank % num_ranks:
                        continue
                    self._check_interrupt()
                    t0 = time.monotonic()
                    self.client.delete_object(b, k)
                    self.entry_lat.vec = _add_lat(self.entry_lat, t0)
                    self.ops.entries += 1
                return
            if cfg.s3_multi_del > 0:
                batch: list[str] = []
                for name in self._object_names():
                    batch.append(name)
                    if len(batch) >= cfg.s3_multi_del:
                        self._check_interrupt()
                        self.client.multi_delete(self._bucket(), batch)
                        self.ops.entries += len(batch)
                        batch = []
                if batch:
                    self.client.multi_delete(self._bucket(), batch)
                    self.ops.entries += len(batch)
            else:
                for name in self._object_names():
                    self._check_interrupt()
                    t0 = time.monotonic()
                    self.client.delete_object(self._bucket(), name)
                    self.entry_lat.vec = _add_lat(self.entry_lat, t0)
                    self.ops.entries += 1
        elif ph == "LISTOBJ":
            self._list_objects()
        elif ph == "PUTOBJACL":
            acl = acl_value(cfg)
            for name in self._object_names():
                self._check_interrupt()
                self.client.put_object_acl(self._bucket(), name, acl)
                self.ops.entries += 1
        elif ph == "GETOBJACL":
            expect = acl_value(cfg)
            expect_str = expect if isinstance(expect, str) else cfg.s3_acl_grantee
            for name in self._object_names():
                self._check_interrupt()
                acl = self.client.get_object_acl(self._bucket(), name)
                if cfg.s3_acl_verify and expect_str not in acl.decode():
                    raise S3Error(f"object ACL verification failed for {name}")
                self.ops.entries += 1
        elif ph == "PUTBACL":
            if self.local_rank == 0:
                acl = acl_value(cfg)
                for b in self.r.buckets:
                    self.client.put_bucket_acl(b, acl)
                    self.ops.entries += 1
        elif ph == "GETBACL":
            if self.local_rank == 0:
                for b in self.r.buckets:
                    self.client.get_bucket_acl(b)
                    self.ops.entries += 1
        elif ph == "PUTOTAG":
            for name in self._object_names():
                self._check_interrupt()
                self.client.put_object_tagging(self._bucket(), name,
                                               {"elbencho-amd": str(self.rank)})
                self.ops.entries += 1
        elif ph == "GETOTAG":
            for name in self._object_names():
                self._check_interrupt()
                tags = self.client.get_object_tagging(self._bucket(), name)
                if cfg.s3_otag_verify and tags.get("elbencho-amd") != str(self.rank):
                    raise S3Error(f"object tagging verification failed for {name}: {tags}")
                self.ops.entries += 1
        elif ph == "DELOTAG":
            for name in self._object_names():
                self._check_interrupt()
                self.client.delete_object_tagging(self._bucket(), name)
                self.ops.entries += 1
        elif ph == "PUTBTAG":
            if self.local_rank == 0:
                for b in self.r.buckets:
                    self.client.put_bucket_tagging(b, {"elbencho-amd": "bucket"})
                    self.ops.entries += 1
        elif ph == "GETBTAG":
            if self.local_rank == 0:
                for b in self.r.buckets:
                    tags = self.client.get_bucket_tagging(b)
                    if cfg.s3_btag_verify and tags.get("elbencho-amd") != "bucket":
                        raise S3Error(f"bucket tagging verification failed for {b}")
                    self.ops.entries += 1
        elif ph == "BVERSION":
            if self.local_rank == 0:
                for b in self.r.buckets:
                    self.client.put_bucket_versioning(b, True)
                    if cfg.s3_bversion_verify:
                        st = self.client.get_bucket_versioning(b)
                        if st != "Enabled":
                            raise S3Error(f"bucket versioning verification failed "
                                          f"for {b}: {st!r}")
                    self.ops.entries += 1
        elif ph == "OLOCKCFG":
            if self.local_rank == 0:
                for b in self.r.buckets:
                    self.client.put_object_lock_config(b)
                    if cfg.s3_olock_verify:
                        data = self.client.get_object_lock_config(b).decode()
                        if "Enabled" not in data:
                            raise S3Error(f"object lock verification failed for {b}")
                    self.ops.entries += 1
        elif ph == "STATDIRS":
            # HEAD the buckets (reference --statdirs in S3 mode)
            for i, b in enumerate(self.r.buckets):
                if i % cfg.num_dataset_threads == self.rank:
                    if not self.client.head_bucket(b):
                        raise S3Error(f"bucket {b} does not exist")
                    self.ops.entries += 1
        elif ph == "LISTOBJPAR":
            # parallel listing: each worker lists its own prefix slice
            prefix = f"{cfg.s3_obj_prefix}r{self.rank}"
            for bucket in self.r.buckets:
                token = ""
                while True:
                    self._check_interrupt()
                    objs, token = self.client.list_objects(
                        bucket, prefix=prefix, max_keys=1000, continuation=token)
                    self.ops.entries += len(objs)
                    if not token:
                        break
        elif ph == "S3MPUCOMPLETE":
            # complete multipart uploads left open by an earlier --s3nompucompl
            # or --s3mpusharing run — possibly by ANOTHER instance: uploadIds
            # and part ETags are rediscovered from S3 itself (reference
            # S3MPUCOMPLETE phase + shared MPU store, Common.h:196)
            if cfg.files:
                for name in self._object_names():
                    self._check_interrupt()
                    bucket = self._bucket()
                    uploads = [u for k, u in
                               self.client.list_multipart_uploads(bucket, prefix=name)
                               if k == name]
                    for upload_id in uploads:
                        parts = self.client.list_parts(bucket, name, upload_id)
                        self.client.complete_multipart(bucket, name, upload_id, parts)
                        self.ops.entries += 1
            elif self.local_rank == 0:
                # no object layout given (bucket-only path, e.g. after an
                # --s3mpusharing run): complete every open upload per bucket
                for bucket in self.r.buckets:
                    self._check_interrupt()
                    for key, upload_id in self.client.list_multipart_uploads(bucket):
                        parts = self.client.list_parts(bucket, key, upload_id)
                        self.client.complete_multipart(bucket, key, upload_id, parts)
                        self.ops.entries += 1
        else:
            raise S3Error(f"S3 phase not supported: {ph}")

    # ------------------------------------------------------------------
    def _make_block(self, length: int, obj_off: int) -> bytes:
        cfg = self.r.cfg
        if cfg.verify >= 0:
            # generate the pattern in HBM with the fill kernel (whole u64
            # words only; the kernel wrapper rejects anything else)
            if self.gpu and obj_off % 8 == 0 and length % 8 == 0:
                return self.gpu.fill_checksum(length, obj_off, cfg.verify)
            return self.core.fill_checksum(length, obj_off, cfg.verify)
        return bytes(self.r.rand_block[:length])

    def _part_sizes(self, size: int, seed_extra: int = 0) -> list[tuple[int, int]]:
        """[(offset, length)] parts of one object: part size is -b (or
        --s3mpusplit) with optional --s3mpusizevar random shrink per part;
        the final part absorbs the difference (reference s3MpuSizeVariance).
        seed_extra must be identical across ranks for shared uploads."""
        cfg = self.r.cfg
        ps = cfg.s3_mpu_split or cfg.block_size
        out = []
        off = 0
        if cfg.s3_mpu_size_var:
            import random as _random
            rng = _random.Random((cfg.bench_seed or 1) ^ 0x9E3779B9 ^ seed_extra)
            while off < size:
                ln = min(ps, size - off)
                if size - off > ln:  # not the last part: shrink by variance
                    ln = max(1, ln - rng.randrange(cfg.s3_mpu_size_var + 1))
                out.append((off, ln))
                off += ln
        else:
            while off < size:
                ln = min(ps, size - off)
                out.append((off, ln))
                off += ln
        return out

    def _put_objects(self):
        cfg = self.r.cfg
        if cfg.s3_mpu_sharing:
            return self._put_objects_shared()
        size = cfg.file_size
        ps = cfg.s3_mpu_split or cfg.block_size
        for name in self._object_names():
            self._check_interrupt()
            te = time.monotonic()
            bucket = self._bucket()
            if size <= ps and not cfg.s3_mpu_size_var:  # single part
                t0 = time.monotonic()
                self._oplog("PutObject", name, 0, size, True)
                if self.client.native:
                    self.client.put_object_native(bucket, name, size, 0,
                                                  cfg.verify)
                else:
                    self.client.put_object(bucket, name,
                                           self._make_block(size, 0))
                self._oplog("PutObject", name, 0, size, False)
                self.io_lat.vec = _add_lat(self.io_lat, t0)
                self.ops.bytes += size
                self.ops.iops += 1
            else:  # multipart: block size = part size (reference -b semantics)
                upload_id = self.client.create_multipart(bucket, name)
                try:
                    if cfg.iodepth > 1 and not cfg.s3_single:
                        parts = self._put_parts_pipelined(bucket, name, upload_id,
                                                          size)
                    else:
                        parts = []
                        for part_num, (off, ln) in enumerate(
                                self._part_sizes(size, self.rank), 1):
                            self._check_interrupt()
                            t0 = time.monotonic()
                            if self.client.native:
                                etag = self.client.put_object_native(
                                    bucket, name, ln, off, cfg.verify,
                                    query={"partNumber": str(part_num),
                                           "uploadId": upload_id})
                            else:
                                etag = self.client.upload_part(
                                    bucket, name, upload_id, part_num,
                                    self._make_block(ln, off))
                            self.io_lat.vec = _add_lat(self.io_lat, t0)
                            parts.append((part_num, etag))
                            self.ops.bytes += ln
                            self.ops.iops += 1
                    if not cfg.s3_no_mpu_compl:
                        self.client.complete_multipart(bucket, name, upload_id, parts)
                    # else: left open for a later S3MPUCOMPLETE phase
                except BaseException:
                    self.client.abort_multipart(bucket, name, upload_id)
                    raise
            self.entry_lat.vec = _add_lat(self.entry_lat, te)
            self.ops.entries += 1

    def _put_parts_pipelined(self, bucket: str, name: str, upload_id: str,
                             size: int) -> list[tuple[int, str]]:
        """--iodepth > 1: keep up to iodepth part uploads of one object in
        flight (blocks are generated in the worker thread, uploads overlap
        on per-slot connections)."""
        import threading as _threading
        from concurrent.futures import as_completed

        ex, clients, depth = self._pipeline()
        inflight = _threading.Semaphore(depth * 2)  # bound queued block memory

        cfg = self.r.cfg
        use_native = self.client.native is not None

        def task(pn: int, off: int, ln: int, body):
            try:
                c = clients.get()
                try:
                    t0 = time.monotonic()
                    if use_native and c.native:
                        # body generated inside the native plane (GIL-free)
                        etag = c.put_object_native(
                            bucket, name, ln, off, cfg.verify,
                            query={"partNumber": str(pn),
                                   "uploadId": upload_id})
                    else:
                        etag = c.upload_part(bucket, name, upload_id, pn, body)
                    return pn, etag, ln, int((time.monotonic() - t0) * 1e6)
                finally:
                    clients.put(c)
            finally:
                inflight.release()

        futs = []
        try:
            for part_num, (off, ln) in enumerate(self._part_sizes(size, self.rank), 1):
                self._check_interrupt()
                inflight.acquire()
                # non-native: block generated HERE (worker thread owns the
                # GPU fill context; pool threads must not share it)
                body = None if use_native else self._make_block(ln, off)
                futs.append(ex.submit(task, part_num, off, ln, body))
            parts = []
            for f in as_completed(futs):
                pn, etag, ln, lat_us = f.result()
                parts.append((pn, etag))
                self.io_lat.vec = _add_lat_us(self.io_lat, lat_us)
                self.ops.bytes += ln
                self.ops.iops += 1
            return parts
        except BaseException:
            for f in futs:
                f.cancel()
            raise

    def _put_objects_shared(self):
        """--s3mpusharing: every worker uploads its round-robin share of parts
        of each named object through one shared multipart upload; whichever
        worker records the final part completes the upload (reference
        S3UploadStore first-writer-wins + LocalWorker.cpp:5455)."""
        cfg = self.r.cfg
        size = cfg.file_size
        ps = cfg.s3_mpu_split or cfg.block_size
        num_ranks = max(cfg.num_dataset_threads, 1)
        store = self.r.upload_store
        for bucket, key in self.r.shared_objects:
            self._check_interrupt()
            te = time.monotonic()
            # seed by object name so every rank computes identical part bounds
            name_seed = int(hashlib.md5(f"{bucket}/{key}".encode()).hexdigest()[:8], 16)
            all_parts = [(n, off, ln) for n, (off, ln)
                         in enumerate(self._part_sizes(size, name_seed), 1)]
            upload_id = store.get_or_create(self.client, bucket, key, len(all_parts))
            did_any = False
            for part_num, off, ln in all_parts:
                if (part_num - 1) % num_ranks != self.rank % num_ranks:
                    continue
                self._check_interrupt()
                t0 = time.monotonic()
                self._oplog("UploadPart", f"{bucket}/{key}", off, ln, True)
                etag = self.client.upload_part(bucket, key, upload_id, part_num,
                                               self._make_block(ln, off))
                self._oplog("UploadPart", f"{bucket}/{key}", off, ln, False)
                self.io_lat.vec = _add_lat(self.io_lat, t0)
                self.ops.bytes += ln
                self.ops.iops += 1
                did_any = True
                is_last = store.add_part(bucket, key, part_num, etag)
                if is_last and not cfg.s3_no_mpu_compl:
                    self.client.complete_multipart(bucket, key, upload_id,
                                                   store.get_parts(bucket, key))
            if did_any:
                self.entry_lat.vec = _add_lat(self.entry_lat, te)
                self.ops.entries += 1

    def _get_objects_shared(self):
        """--s3mpusharing READ: each rank downloads its round-robin block
        share of every named shared object (ranged GETs)."""
        cfg = self.r.cfg
        size = cfg.file_size
        bs = cfg.block_size
        num_ranks = max(cfg.num_dataset_threads, 1)
        for bucket, key in self.r.shared_objects:
            self._check_interrupt()
            te = time.monotonic()
            did_any = False
            off = 0
            blk = 0
            while off < size:
                ln = min(bs, size - off)
                if blk % num_ranks == self.rank % num_ranks:
                    self._check_interrupt()
                    t0 = time.monotonic()
                    data = self.client.get_object(bucket, key, (off, off + ln - 1))
                    self.io_lat.vec = _add_lat(self.io_lat, t0)
                    if len(data) != ln:
                        raise S3Error(f"short ranged read of {bucket}/{key}: "
                                      f"{len(data)} != {ln}")
                    if cfg.verify >= 0 and not cfg.s3_fastget:
                        bad = self.core.verify_checksum(data, off, cfg.verify)
                        if bad != 2**64 - 1:
                            raise S3Error(f"S3 data verification failed for "
                                          f"{bucket}/{key} at object offset {bad}")
                    self.ops.bytes += ln
                    self.ops.iops += 1
                    did_any = True
                off += ln
                blk += 1
            if did_any:
                self.entry_lat.vec = _add_lat(self.entry_lat, te)
                self.ops.entries += 1

    def _get_objects(self):
        cfg = self.r.cfg
        size = cfg.file_size
        bs = cfg.block_size
        if cfg.s3_mpu_sharing:
            return self._get_objects_shared()
        if cfg.s3_rand_obj:
            return self._get_random_objects()
        pipelined = cfg.iodepth > 1 and not cfg.s3_single and size > bs
        for name in self._object_names():
            self._check_interrupt()
            te = time.monotonic()
            bucket = self._bucket()
            if pipelined:
                self._get_ranges_pipelined(bucket, name, size, bs)
            else:
                off = 0
                while off < size:
                    ln = min(bs, size - off)
                    t0 = time.monotonic()
                    self._oplog("GetObject", name, off, ln, True)
                    if self.client.native:
                        salt = cfg.verify if (cfg.verify >= 0 and
                                              not cfg.s3_fastget) else -1
                        got = self.client.get_object_native(
                            bucket, name, (off, off + ln - 1), off, salt)
                        if got != ln:
                            raise S3Error(f"short ranged read of {name}: "
                                          f"{got} != {ln}")
                    else:
                        data = self.client.get_object(bucket, name,
                                                      (off, off + ln - 1))
                        if len(data) != ln:
                            raise S3Error(f"short ranged read of {name}: "
                                          f"{len(data)} != {ln}")
                        if cfg.verify >= 0 and not cfg.s3_fastget:
                            self._verify_block(name, data, off)
                    self._oplog("GetObject", name, off, ln, False)
                    self.io_lat.vec = _add_lat(self.io_lat, t0)
                    self.ops.bytes += ln
                    self.ops.iops += 1
                    off += ln
            self.entry_lat.vec = _add_lat(self.entry_lat, te)
            self.ops.entries += 1

    def _verify_block(self, name: str, data: bytes, off: int) -> None:
        cfg = self.r.cfg
        if self.gpu and off % 8 == 0 and len(data) % 16 == 0:
            nbad, first = self.gpu.verify(data, off, cfg.verify)
            if nbad:
                raise S3Error(f"S3 data verification failed (GPU) for "
                              f"{name} at object offset {first}")
        else:
            bad = self.core.verify_checksum(data, off, cfg.verify)
            if bad != 2**64 - 1:
                raise S3Error(f"S3 data verification failed for {name} at "
                              f"object offset {bad}")

    def _get_ranges_pipelined(self, bucket: str, name: str, size: int,
                              bs: int) -> None:
        """--iodepth > 1: up to iodepth ranged GETs of one object in flight;
        verification happens in the worker thread as downloads complete
        (reference async download pipelining, LocalWorker.cpp:6280)."""
        import threading as _threading
        from concurrent.futures import as_completed

        cfg = self.r.cfg
        ex, clients, depth = self._pipeline()
        inflight = _threading.Semaphore(depth * 2)

        use_native = self.client.native is not None
        native_salt = cfg.verify if (cfg.verify >= 0 and
                                     not cfg.s3_fastget) else -1

        def task(off: int, ln: int):
            try:
                c = clients.get()
                try:
                    t0 = time.monotonic()
                    if use_native and c.native:
                        # receive + verify natively (per-connection plane)
                        got = c.get_object_native(bucket, name,
                                                  (off, off + ln - 1), off,
                                                  native_salt)
                        if got != ln:
                            raise S3Error(f"short ranged read of {name}: "
                                          f"{got} != {ln}")
                        return off, ln, None, \
                            int((time.monotonic() - t0) * 1e6)
                    data = c.get_object(bucket, name, (off, off + ln - 1))
                    return off, ln, data, int((time.monotonic() - t0) * 1e6)
                finally:
                    clients.put(c)
            finally:
                inflight.release()

        futs = []
        try:
            off = 0
            while off < size:
                self._check_interrupt()
                ln = min(bs, size - off)
                inflight.acquire()
                futs.append(ex.submit(task, off, ln))
                off += ln
            for f in as_completed(futs):
                off, ln, data, lat_us = f.result()
                if data is not None:  # pure-python path: verify here
                    if len(data) != ln:
                        raise S3Error(f"short ranged read of {name}: "
                                      f"{len(data)} != {ln}")
                    if cfg.verify >= 0 and not cfg.s3_fastget:
                        self._verify_block(name, data, off)
                self.io_lat.vec = _add_lat_us(self.io_lat, lat_us)
                self.ops.bytes += ln
                self.ops.iops += 1
        except BaseException:
            for f in futs:
                f.cancel()
            raise

    def _get_random_objects(self):
        """--s3randobj: ranged reads at random offsets of random objects
        (reference LocalWorker.cpp:4069). Amount: randamount/threads bytes."""
        import random as _random

        cfg = self.r.cfg
        size = cfg.file_size
        bs = min(cfg.block_size, size)
        amount = (cfg.rand_amount or
                  cfg.num_dataset_threads * max(cfg.dirs, 1) * cfg.files * size)
        amount //= cfg.num_dataset_threads
        rng = _random.Random(0x5EED ^ self.rank)
        # any rank may read any rank's objects
        all_names = []
        for r in range(cfg.num_dataset_threads):
            for d in range(max(cfg.dirs, 1)):
                for f in range(cfg.files):
                    if cfg.dirs > 0:
                        all_names.append(f"{cfg.s3_obj_prefix}r{r}/d{d}/r{r}-f{f}")
                    else:
                        all_names.append(f"{cfg.s3_obj_prefix}r{r}-f{f}")
        done = 0
        while done < amount:
            self._check_interrupt()
            name = all_names[rng.randrange(len(all_names))]
            ln = min(bs, amount - done, size)
            off = rng.randrange(max(size - ln, 0) + 1)
            t0 = time.monotonic()
            data = self.client.get_object(self._bucket(), name, (off, off + ln - 1))
            self.io_lat.vec = _add_lat(self.io_lat, t0)
            if len(data) != ln:
                raise S3Error(f"short random read of {name}")
            if cfg.verify >= 0 and not cfg.s3_fastget:
                bad = self.core.verify_checksum(data, off, cfg.verify)
                if bad != 2**64 - 1:
                    raise S3Error(f"S3 verification failed for {name} at offset {bad}")
            self.ops.bytes += ln
            self.ops.iops += 1
            done += ln

    def _list_objects(self):
        cfg = self.r.cfg
        if self.local_rank != 0:
            return
        for bucket in self.r.buckets:
            token = ""
            seen = 0
            while True:
                self._check_interrupt()
                objs, token = self.client.list_objects(
                    bucket, prefix=cfg.s3_obj_prefix,
                    max_keys=min(1000, cfg.s3_list_obj or 1000),
                    continuation=token)
                seen += len(objs)
                self.ops.entries += len(objs)
                if not token or (cfg.s3_list_obj and seen >= cfg.s3_list_obj):
                    break
            if cfg.s3_list_verify:
                expected = (cfg.num_dataset_threads * max(cfg.dirs, 1) * cfg.files)
                if seen != expected:
                    raise S3Error(f"listing verification failed for {bucket}: "
                                  f"saw {seen} objects, expected {expected}")


def _add_lat(h: Histogram, t0: float) -> list[int]:
    return _add_lat_us(h, int((time.monotonic() - t0) * 1e6))


def _add_lat_us(h: Histogram, us: int) -> list[int]:
    idx = _bucket_index(us)
    v = h.vec
    v[0] += 1
    v[1] += us
    v[2] = min(v[2], us)
    v[3] = max(v[3], us)
    v[4 + idx] += 1
    return v


def _bucket_index(v: int) -> int:
    if v < 4:
        return v
    log2v = v.bit_length() - 1
    frac = (v >> (log2v - 2)) & 3
    return log2v * 4 + frac - 4


class S3Runner:
    """Coordinator backend for S3 mode (bench_mode == "s3")."""

    def __init__(self, cfg: BenchConfig):
        if not cfg.s3_endpoints:
            raise S3Error("S3 mode requires --s3endpoints")
        self.cfg = cfg
        stripped = [p[len("s3://"):] if p.startswith("s3://") else p
                    for p in cfg.paths]
        # --s3mpusharing: "bucket/object" path entries name shared objects that
        # all workers upload/download together (reference s3mpusharing mode,
        # object names as parameters)
        self.shared_objects: list[tuple[str, str]] = []
        if cfg.s3_mpu_sharing:
            for p in stripped:
                if "/" not in p:
                    raise S3Error("--s3mpusharing requires bucket/object paths")
                b, _, k = p.partition("/")
                self.shared_objects.append((b, k))
            self.buckets = sorted({b for b, _ in self.shared_objects})
        else:
            self.buckets = stripped
        if not self.buckets:
            raise S3Error("S3 mode requires s3://bucket paths")
        # --s3log: client request trace (reference AWS SDK logging)
        self.trace = None
        self._trace_file = None
        if cfg.s3_log > 0:
            import datetime as _dt
            prefix = cfg.s3_log_prefix or "s3_client_"
            path = f"{prefix}{_dt.date.today().strftime('%Y%m%d')}.log"
            self._trace_file = open(path, "a")
            tl = threading.Lock()

            def _trace(line: str, _f=self._trace_file, _l=tl):
                with _l:
                    _f.write(f"{time.time():.6f} {line}\n")
                    _f.flush()
            self.trace = _trace
        # --s3single: one client shared by every worker thread
        self.shared_client = None
        if cfg.s3_single:
            self.shared_client = S3Client(
                cfg.s3_endpoints[0], cfg.s3_key, cfg.s3_secret, cfg.s3_region,
                extra_put_headers=build_put_headers(cfg),
                session_token=cfg.s3_session_token,
                virtual_addressing=cfg.s3_virt_addr,
                checksum_algo=cfg.s3_chksum_algo, trace=self.trace,
                sign_payload=cfg.s3_sign_policy != 2)
        self.credentials: list[tuple[str, str]] = []
        if cfg.s3_cred_list:
            for ent in cfg.s3_cred_list.split(","):
                if ":" in ent:
                    k, sec = ent.split(":", 1)
                    self.credentials.append((k, sec))
        elif cfg.s3_cred_file:
            with open(cfg.s3_cred_file) as f:
                for ln in f:
                    ln = ln.strip()
                    if ln and ":" in ln and not ln.startswith("#"):
                        k, sec = ln.split(":", 1)
                        self.credentials.append((k, sec))
        self.ops_log = None
        if cfg.ops_log_path:
            self.ops_log_lock = threading.Lock()
            self.ops_log = open(cfg.ops_log_path, "a")
        self.workers: list[S3Worker] = []
        self.interrupt_flag = threading.Event()
        self.start_gate = threading.Event()
        self.done_count = 0
        self.done_lock = threading.Lock()
        self.done_cv = threading.Condition(self.done_lock)
        self.stonewalled = False
        self.phase_start = 0.0
        # pre-generated random payload block (like the engine's host buffers)
        import os as _os
        blk = _os.urandom(min(max(cfg.block_size, 1), 1 << 22))
        while len(blk) < cfg.block_size:
            blk = blk + blk  # bytes concat (a bytearray cannot resize itself)
        self.rand_block = blk[:cfg.block_size]
        self.upload_store = SharedUploadStore()
        # cross-service sharing: uploadIds pre-created by the master
        for objpath, upload_id in (cfg.s3_mpu_upload_ids or {}).items():
            b, _, k = objpath.partition("/")
            self.upload_store.seed(b, k, upload_id)

    # --- runner interface ---
    def start(self, phase_name: str) -> None:
        self.interrupt_flag.clear()
        self.start_gate.clear()
        self.done_count = 0
        self.stonewalled = False
        self.workers = [S3Worker(self, i, phase_name) for i in range(self.cfg.threads)]
        for w in self.workers:
            w.start()
        self.phase_start = time.monotonic()
        self.start_gate.set()

    def on_worker_done(self, w: S3Worker) -> None:
        with self.done_cv:
            if not self.stonewalled and not w.error and (
                    w.ops.bytes or w.ops.entries or w.ops.iops or
                    w.rm_ops.bytes or w.rm_ops.iops):
                elapsed = int((time.monotonic() - self.phase_start) * 1e6)
                for peer in self.workers:
                    peer.sw = _Counters(peer.ops.entries, peer.ops.bytes, peer.ops.iops)
                    peer.rm_sw = _Counters(peer.rm_ops.entries, peer.rm_ops.bytes,
                                           peer.rm_ops.iops)
                    peer.sw_elapsed_us = elapsed
                self.stonewalled = True
            self.done_count += 1
            self.done_cv.notify_all()

    def wait(self, timeout_ms: int) -> bool:
        with self.done_cv:
            return self.done_cv.wait_for(
                lambda: self.done_count >= len(self.workers),
                timeout=None if timeout_ms < 0 else timeout_ms / 1000.0)

    def poll(self) -> dict[str, Any]:
        agg = {"entries": 0, "bytes": 0, "iops": 0,
               "workers_done": self.done_count, "workers_total": len(self.workers),
               "workers_with_error": sum(1 for w in self.workers if w.error),
               "elapsed_usec": int((time.monotonic() - self.phase_start) * 1e6),
               "stonewall_triggered": self.stonewalled,
               "lat_num_ios": 0, "lat_sum_ios": 0, "lat_num_entries": 0,
               "lat_sum_entries": 0}
        for w in self.workers:
            agg["entries"] += w.ops.entries
            agg["bytes"] += w.ops.bytes
            agg["iops"] += w.ops.iops
            agg["lat_num_ios"] += w.io_lat.vec[0]
            agg["lat_sum_ios"] += w.io_lat.vec[1]
        return agg

    def interrupt(self) -> None:
        self.interrupt_flag.set()

    def trigger_stonewall(self) -> None:
        """Remote stonewall propagation (/triggerstonewall): snapshot every
        worker's live counters now (reference RemoteWorker poll loop)."""
        with self.done_cv:
            if not self.stonewalled:
                elapsed = int((time.monotonic() - self.phase_start) * 1e6)
                for peer in self.workers:
                    peer.sw = _Counters(peer.ops.entries, peer.ops.bytes,
                                        peer.ops.iops)
                    peer.rm_sw = _Counters(peer.rm_ops.entries,
                                           peer.rm_ops.bytes, peer.rm_ops.iops)
                    peer.sw_elapsed_us = elapsed
                self.stonewalled = True

    def poll_workers(self):
        """Per-worker rows for the fullscreen dashboard / --livecsvex."""
        return [{"rank": w.rank,
                 "entries": w.ops.entries + w.rm_ops.entries,
                 "bytes": w.ops.bytes + w.rm_ops.bytes,
                 "iops": w.ops.iops + w.rm_ops.iops} for w in self.workers]

    def finish(self) -> list[WorkerStats]:
        for w in self.workers:
            w.join()
        out = []
        for w in self.workers:
            sw = w.sw or w.ops
            rm_sw = w.rm_sw or w.rm_ops
            out.append(WorkerStats(
                rank=w.rank,
                elapsed_usec=w.elapsed_us,
                entries=w.ops.entries, bytes=w.ops.bytes, iops=w.ops.iops,
                stonewall_elapsed_usec=w.sw_elapsed_us or w.elapsed_us,
                stonewall_entries=sw.entries, stonewall_bytes=sw.bytes,
                stonewall_iops=sw.iops,
                rm_entries=w.rm_ops.entries, rm_bytes=w.rm_ops.bytes,
                rm_iops=w.rm_ops.iops,
                rm_stonewall_entries=rm_sw.entries,
                rm_stonewall_bytes=rm_sw.bytes, rm_stonewall_iops=rm_sw.iops,
                io_lat=list(w.io_lat.vec), entry_lat=list(w.entry_lat.vec),
                io_lat_rm=list(w.io_lat_rm.vec),
                entry_lat_rm=list(w.entry_lat_rm.vec),
                error=w.error))
        return out

    def planned_work(self, phase_name: str) -> tuple[int, int]:
        cfg = self.cfg
        if cfg.s3_mpu_sharing:
            nobj = len(self.shared_objects)
            if phase_name in ("WRITE", "READ"):
                return nobj, nobj * cfg.file_size
            if phase_name in ("STAT", "RMFILES"):
                return nobj, 0
            return 0, 0
        nobj = max(cfg.dirs, 1) * cfg.files * cfg.threads
        if phase_name in ("WRITE", "READ"):
            return nobj, nobj * cfg.file_size
        if phase_name in ("STAT", "RMFILES"):
            return nobj, 0
        if phase_name in ("MKDIRS", "RMDIRS"):
            return len(self.buckets), 0
        if phase_name in ("PUTOBJACL", "GETOBJACL", "PUTOTAG", "GETOTAG", "DELOTAG"):
            return nobj, 0
        return 0, 0

    def close(self) -> None:
        for w in self.workers:
            if w.is_alive():
                self.interrupt_flag.set()
        # abort unfinished shared multipart uploads (reference behavior)
        if self.workers:
            try:
                self.upload_store.abort_unfinished(self.workers[0].client)
            except (S3Error, OSError):
                pass
        # tear down every worker's clients EAGERLY: the native data planes
        # hold GpuCtx allocations in HBM, and waiting for the cyclic GC to
        # find them leaks VRAM across repeated in-process runs
        for w in self.workers:
            try:
                if w.client:
                    w.client.close()
                    w.client.native = None
                if w._pool:
                    ex, clients, _ = w._pool
                    ex.shutdown(wait=False)
                    while not clients.empty():
                        c = clients.get_nowait()
                        c.close()
                        c.native = None
                    w._pool = None
            except Exception:  # noqa: BLE001 — teardown is best effort
                pass
        self.workers = []
        if self._trace_file:
            self._trace_file.close()
            self._trace_file = None
