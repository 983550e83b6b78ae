"""Two small raw-TCP HTTP/1.1 servers for driving core.HttpDataPlane directly.

The data plane only executes fully formed requests, so it can be pointed at
anything that speaks enough HTTP/1.1 - no SigV4, no S3 semantics:

* BlobServer - ``GET /<name>`` answers with the stored bytes over keep-alive.
  Per blob it can split the body into fixed-size writes, glue the first body
  bytes to the header write, answer with an error status, or close the socket
  after part of the body.
* SinkServer - ``PUT /<name>`` reads exactly Content-Length bytes, keeps them
  under the path and answers 200 with an ETag and an empty body. ``GET`` of a
  stored path sends it back, so one plane can alternate both directions.

Every socket has a timeout: a client that stops reading or writing makes the
connection thread give up and close, which the client sees as a connection
error. call_limited() bounds the client side the same way.
"""

from __future__ import annotations

import socket
import threading
import zlib

SOCK_TIMEOUT = 20.0   # per socket operation, server side
CALL_LIMIT = 60.0     # per data-plane call, client side


def call_limited(fn, *args, limit: float = CALL_LIMIT):
    """fn(*args) on a helper thread; AssertionError if it is not back within
    `limit` seconds (the thread is a daemon, a stuck call cannot hold the
    process). Exceptions of fn are re-raised here."""
    box = {}

    def run():
        try:
            box["ret"] = fn(*args)
        except BaseException as e:  # noqa: BLE001 - handed to the caller
            box["exc"] = e

    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(limit)
    if t.is_alive():
        raise AssertionError(f"{getattr(fn, '__name__', fn)}{args[1:]} still "
                             f"running after {limit} s")
    if "exc" in box:
        raise box["exc"]
    return box["ret"]


class _Server:
    """Listener + one thread per connection; subclasses answer requests."""

    def __init__(self):
        self._lsock = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
        self._lsock.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
        self._lsock.bind(("127.0.0.1", 0))
        self._lsock.listen(16)
        self._lsock.settimeout(0.1)
        self.port = self._lsock.getsockname()[1]
        self.lock = threading.Lock()
        self.errors: list[str] = []   # what connection threads could not do
        self.requests = 0             # requests answered (or cut) so far
        self.connections = 0          # connections accepted so far
        self._stop = threading.Event()
        self._conns: list[socket.socket] = []
        self._threads: list[threading.Thread] = []
        self._acceptor = threading.Thread(target=self._accept_loop, daemon=True)
        self._acceptor.start()

    def stop(self):
        self._stop.set()
        self._acceptor.join(5)
        self._lsock.close()
        with self.lock:
            conns = list(self._conns)
        for c in conns:
            try:
                c.shutdown(socket.SHUT_RDWR)
            except OSError:
                pass
        for t in self._threads:
            t.join(5)

    def _accept_loop(self):
        while not self._stop.is_set():
            try:
                conn, _ = self._lsock.accept()
            except socket.timeout:
                continue
            except OSError:
                return
            conn.settimeout(SOCK_TIMEOUT)
            conn.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
            with self.lock:
                self._conns.append(conn)
                self.connections += 1
            t = threading.Thread(target=self._serve, args=(conn,), daemon=True)
            self._threads.append(t)
            t.start()

    def _serve(self, conn: socket.socket):
        buf = b""
        try:
            while not self._stop.is_set():
                while b"\r\n\r\n" not in buf:
                    try:
                        got = conn.recv(65536)
                    except socket.timeout:
                        if buf:
                            raise
                        continue  # idle keep-alive connection: not an error
                    if not got:
                        return
                    buf += got
                head, buf = buf.split(b"\r\n\r\n", 1)
                lines = head.decode("latin-1").split("\r\n")
                method, path, _ = lines[0].split(" ", 2)
                headers = {}
                for ln in lines[1:]:
                    k, _, v = ln.partition(":")
                    headers[k.strip().lower()] = v.strip()
                keep, buf = self.answer(conn, method, path, headers, buf)
                with self.lock:
                    self.requests += 1
                if not keep:
                    return
        except socket.timeout:
            with self.lock:
                self.errors.append("socket timeout: the client stopped "
                                   "reading or writing")
        except OSError:
            pass  # the client closed on us (it may: oversized body, close())
        finally:
            conn.close()
            with self.lock:
                self._conns.remove(conn)

    def answer(self, conn, method, path, headers, rest):
        """Handle one request; `rest` is what was read past the header.
        Returns (keep the connection, unconsumed bytes)."""
        raise NotImplementedError


def _head(status: int, length: int, extra: str = "") -> bytes:
    reason = {200: "OK", 404: "Not Found"}.get(status, "Status")
    return (f"HTTP/1.1 {status} {reason}\r\n{extra}"
            f"Content-Length: {length}\r\n\r\n").encode()


class BlobServer(_Server):
    def __init__(self):
        self.blobs: dict[str, dict] = {}
        super().__init__()

    def put_blob(self, name: str, data: bytes, piece: int = 0, status: int = 200,
                 cut_after: int | None = None, glue_head: bool = False):
        """piece: body goes out in writes of this many bytes (0: one write);
        glue_head: the first piece shares a write with the header;
        cut_after: announce the whole body, send this many bytes, close."""
        with self.lock:
            self.blobs[name] = dict(data=data, piece=piece, status=status,
                                    cut_after=cut_after, glue_head=glue_head)

    def drop_blob(self, name: str):
        with self.lock:
            self.blobs.pop(name, None)

    def answer(self, conn, method, path, headers, rest):
        with self.lock:
            blob = self.blobs.get(path.lstrip("/"))
        if method != "GET" or blob is None:
            body = b"<Error><Code>NoSuchKey</Code></Error>"
            conn.sendall(_head(404, len(body)) + body)
            return True, rest
        data = blob["data"]
        head = _head(blob["status"], len(data))
        end = len(data) if blob["cut_after"] is None else blob["cut_after"]
        piece = blob["piece"] or max(end, 1)
        pos = 0
        if blob["glue_head"]:
            pos = min(piece, end)
            conn.sendall(head + data[:pos])
        else:
            conn.sendall(head)
        view = memoryview(data)
        while pos < end:
            n = min(piece, end - pos)
            conn.sendall(view[pos:pos + n])
            pos += n
        return blob["cut_after"] is None, rest


class SinkServer(_Server):
    def __init__(self):
        self.objects: dict[str, bytes] = {}
        super().__init__()

    def take(self, name: str) -> bytes:
        """The body stored under /name; it is forgotten afterwards."""
        with self.lock:
            return self.objects.pop(name)

    def peek(self, name: str) -> bytes:
        with self.lock:
            return self.objects[name]

    def store(self, name: str, data: bytes):
        with self.lock:
            self.objects[name] = data

    def answer(self, conn, method, path, headers, rest):
        if method == "GET":  # read a stored body back, in one write
            with self.lock:
                data = self.objects.get(path.lstrip("/"))
            if data is None:
                conn.sendall(_head(404, 0))
            else:
                conn.sendall(_head(200, len(data)) + data)
            return True, rest
        if method != "PUT":
            conn.sendall(_head(404, 0))
            return True, rest
        length = int(headers["content-length"])
        body = bytearray(length)
        have = min(len(rest), length)
        body[:have] = rest[:have]
        rest = rest[have:]
        view = memoryview(body)
        while have < length:
            n = conn.recv_into(view[have:])
            if n == 0:
                return False, b""
            have += n
        body = bytes(body)
        with self.lock:
            self.objects[path.lstrip("/")] = body
        conn.sendall(_head(200, 0, f'ETag: "{zlib.crc32(body):08x}"\r\n'))
        return True, rest
