"""Master-side remote service driver.

Reference analogue: /root/reference/source/workers/RemoteWorker.cpp — one
thread per service host, POST /preparephase with the serialized config,
GET /startphase, adaptive /status poll loop (:447-584, 25ms -> svcupint),
GET /benchresult collection, stonewall propagation. Independent
implementation on http.client.
"""

from __future__ import annotations

import hashlib
import http.client
import json
import threading
import time
import urllib.parse
from dataclasses import dataclass, field
from typing import Any

from elbencho_amd import HTTP_PROTOCOL_VERSION
from elbencho_amd.config import BenchConfig
from elbencho_amd.dataprofile import DataProfile
from elbencho_amd.stats import WorkerStats

DEFAULT_PORT = 1611
FIRST_POLL_MS = 25  # adaptive poll start (reference RemoteWorker.cpp:699)


def split_host(h: str) -> tuple[str, int]:
    if ":" in h:
        host, port = h.rsplit(":", 1)
        return host, int(port)
    return h, DEFAULT_PORT


class ServiceClient:
    """HTTP client for one service host."""

    def __init__(self, hostport: str, auth: str = "", timeout: float = 30.0):
        self.hostport = hostport
        self.host, self.port = split_host(hostport)
        self.auth = auth
        self.timeout = timeout

    def _headers(self) -> dict[str, str]:
        h = {}
        if self.auth:
            h["X-Service-Auth"] = self.auth
        return h

    def get(self, path: str, timeout: float | None = None) -> Any:
        conn = http.client.HTTPConnection(self.host, self.port,
                                          timeout=timeout or self.timeout)
        try:
            conn.request("GET", path, headers=self._headers())
            resp = conn.getresponse()
            body = resp.read()
            if resp.status != 200:
                raise RuntimeError(self._frame_err(path, resp.status, body))
            ctype = resp.getheader("Content-Type", "")
            return json.loads(body) if "json" in ctype else body.decode()
        finally:
            conn.close()

    def post(self, path: str, obj: Any) -> Any:
        conn = http.client.HTTPConnection(self.host, self.port, timeout=self.timeout)
        try:
            body = json.dumps(obj).encode()
            hdrs = self._headers()
            hdrs["Content-Type"] = "application/json"
            conn.request("POST", path, body=body, headers=hdrs)
            resp = conn.getresponse()
            rbody = resp.read()
            if resp.status != 200:
                raise RuntimeError(self._frame_err(path, resp.status, rbody))
            return json.loads(rbody)
        finally:
            conn.close()

    def _frame_err(self, path: str, status: int, body: bytes) -> str:
        try:
            msg = json.loads(body).get("error", body.decode())
        except (ValueError, UnicodeDecodeError):
            msg = body.decode(errors="replace")
        return f"Service {self.hostport}{path} returned HTTP {status}: {msg}"


@dataclass
class HostState:
    client: ServiceClient
    last_status: dict = field(default_factory=dict)
    done: bool = False
    error: str = ""
    ping_us: int = 0  # --svcping: last /status round-trip


class RemoteRunner:
    """Coordinator backend driving N remote services (master mode)."""

    def __init__(self, cfg: BenchConfig):
        self.cfg = cfg
        auth = ""
        if cfg.svc_pw_file:
            with open(cfg.svc_pw_file) as f:
                auth = hashlib.sha256(f.read().strip().encode()).hexdigest()

        hosts = cfg.hosts
        if cfg.num_hosts >= 0:
            hosts = hosts[: cfg.num_hosts]
        self.hosts = [HostState(ServiceClient(h, auth)) for h in hosts]
        self._phase = ""
        self._bench_id = ""
        self._poll_ms = FIRST_POLL_MS
        self._wait_for_services()

    # ------------------------------------------------------------------
    def _wait_for_services(self, timeout: float = 10.0) -> None:
        if getattr(self.cfg, "svc_wait", False):
            timeout = 365 * 24 * 3600.0  # --svcwait: wait for services forever
        deadline = time.monotonic() + timeout
        for hs in self.hosts:
            while True:
                try:
                    ver = hs.client.get("/protocolversion", timeout=2.0)
                    if ver != HTTP_PROTOCOL_VERSION:
                        raise RuntimeError(
                            f"Service {hs.client.hostport} protocol version {ver!r} does "
                            f"not match master {HTTP_PROTOCOL_VERSION!r}")
                    break
                except (ConnectionError, OSError) as e:
                    if time.monotonic() > deadline:
                        raise RuntimeError(
                            f"Service {hs.client.hostport} is not reachable: {e}") from e
                    time.sleep(0.25)

    # ------------------------------------------------------------------
    def _for_all(self, fn) -> list[Any]:
        """Run fn(hostIdx, HostState) on all hosts in parallel; raise first error."""
        results: list[Any] = [None] * len(self.hosts)
        errors: list[str] = []

        def run(i: int, hs: HostState):
            try:
                results[i] = fn(i, hs)
            except Exception as e:  # noqa: BLE001
                errors.append(str(e))

        threads = [threading.Thread(target=run, args=(i, hs))
                   for i, hs in enumerate(self.hosts)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errors:
            raise RuntimeError("; ".join(errors))
        return results

    # ------------------------------------------------------------------
    def start(self, phase_name: str) -> None:
        import uuid

        cfg = self.cfg
        self._phase = phase_name
        self._bench_id = str(uuid.uuid4())
        self._poll_ms = FIRST_POLL_MS
        self._stonewall_sent = False
        shared = not cfg.no_svc_share and cfg.path_type != "dir"
        num_hosts = len(self.hosts)

        # --s3mpusharing across services: the master pre-creates one
        # multipart upload per shared object and distributes the uploadIds in
        # the wire config, so every service adds parts to the SAME upload
        # (reference ProgArgs::precreateMpuIDs + the /preparefile MPU file,
        # ProgArgs.cpp:2950-2990). Nobody completes in this mode — a later
        # --s3mpucompl run does (or --s3nompucompl semantics apply).
        if (cfg.bench_mode == "s3" and cfg.s3_mpu_sharing and
                phase_name == "WRITE" and not cfg.s3_mpu_upload_ids):
            from elbencho_amd.s3 import precreate_upload_ids
            cfg.s3_mpu_upload_ids = precreate_upload_ids(cfg)

        # netbench role assignment: hosts named in --servers act as servers,
        # the rest are clients (reference scale-out semantics)
        server_hosts = set()
        if cfg.bench_mode == "netbench":
            # exact host:port match when the server spec names a port;
            # hostname-only specs match any port of that host
            with_port = {s for s in cfg.servers if ":" in s}
            name_only = {s for s in cfg.servers if ":" not in s}
            for hs in self.hosts:
                hp = hs.client.hostport
                if hp in with_port or hp.rsplit(":", 1)[0] in name_only:
                    server_hosts.add(hp)
            if not server_hosts:
                raise RuntimeError("--netbench: none of --hosts matches --servers")
            n_clients = len(self.hosts) - len(server_hosts)
            if n_clients < 1:
                raise RuntimeError("--netbench needs at least one non-server host")
            self._nb_total_client_threads = n_clients * cfg.threads
            self._nb_num_servers = len(server_hosts)

        client_rank = [0]  # contiguous rank offsets over client hosts only

        def prep(i: int, hs: HostState):
            wire = cfg.to_wire()
            wire["service_index"] = i
            wire["threads"] = cfg.threads
            wire["num_dataset_threads"] = (cfg.threads * num_hosts) if shared else cfg.threads
            if cfg.bench_mode == "netbench":
                is_server = hs.client.hostport in server_hosts
                wire["netbench_is_server"] = is_server
                svc_port = hs.client.port
                wire["service_port"] = svc_port  # server listens on port+1000
                if is_server:
                    # this server's share of client connections (clients pick
                    # servers round-robin by global rank)
                    srv_list = sorted(server_hosts)
                    j = srv_list.index(hs.client.hostport)
                    n = self._nb_total_client_threads
                    k = self._nb_num_servers
                    wire["netbench_num_conns"] = n // k + (1 if (n % k) > j else 0)
                    wire["rank_offset"] = 0
                else:
                    wire["rank_offset"] = client_rank[0]
                    client_rank[0] += cfg.threads
                # rewrite servers list to hostport form for the engine
                srv_list = sorted(server_hosts)
                wire["servers"] = srv_list
            elif cfg.no_svc_share:
                # private whole dataset per host: every host runs ranks
                # 0..threads-1 over the full work (a global offset would
                # push later hosts past the dataset into empty slices)
                wire["rank_offset"] = 0
            else:
                wire["rank_offset"] = i * cfg.threads
            hs.done = False
            hs.error = ""
            hs.last_status = {}
            return hs.client.post("/preparephase",
                                  {"protocol_version": HTTP_PROTOCOL_VERSION, "config": wire})

        infos = self._for_all(prep)
        self._check_bench_path_infos(infos)
        self._for_all(lambda i, hs: hs.client.get(
            f"/startphase?phase={urllib.parse.quote(phase_name)}&benchid={self._bench_id}"))

    # ------------------------------------------------------------------
    def _check_bench_path_infos(self, infos: list[dict]) -> None:
        """Cross-check the BenchPathInfo each service returned from
        /preparephase: conflicting path types or path counts between
        services fail fast; size adaptations are reported as NOTEs
        (reference WorkerManager::checkServiceBenchPathInfos,
        WorkerManager.cpp:498 + ProgArgs.cpp:4206)."""
        infos = [i for i in infos if isinstance(i, dict)]
        if not infos:
            return
        first = infos[0]
        host0 = self.hosts[0].client.hostport

        if first.get("num_paths") is not None and self.cfg.paths and \
                first["num_paths"] != len(self.cfg.paths):
            raise RuntimeError(
                "Service instance benchmark paths count does not match master "
                f"paths count. Service: {host0}; "
                f"Master paths: {len(self.cfg.paths)} ({','.join(self.cfg.paths)}); "
                f"Service paths: {first['num_paths']} ({first.get('paths_str', '')})")
        if first.get("file_size") not in (None, self.cfg.file_size):
            print(f"NOTE: Service instance adapted file size. "
                  f"New file size: {first['file_size']}; Service: {host0}")
        if first.get("block_size") not in (None, self.cfg.block_size):
            print(f"NOTE: Service instance adapted block size. "
                  f"New block size: {first['block_size']}; Service: {host0}")

        for i, other in enumerate(infos[1:], start=1):
            hosti = self.hosts[i].client.hostport
            if first.get("path_type") != other.get("path_type"):
                raise RuntimeError(
                    "Conflicting benchmark path types on different service "
                    f"instances. Service_A: {host0}; Service_B: {hosti}; "
                    f"Service_A paths: {first.get('paths_str', '')}; "
                    f"Service_B paths: {other.get('paths_str', '')}")
            if first.get("num_paths") != other.get("num_paths"):
                raise RuntimeError(
                    "Conflicting number of benchmark paths on different "
                    f"service instances. Service_A: {host0}; "
                    f"Service_B: {hosti}; "
                    f"Service_A paths: {first.get('num_paths')}; "
                    f"Service_B paths: {other.get('num_paths')}")
            if first.get("file_size") != other.get("file_size"):
                raise RuntimeError(
                    "Conflicting file sizes on different service instances. "
                    f"Service_A: {host0} ({first.get('file_size')}); "
                    f"Service_B: {hosti} ({other.get('file_size')})")

    # ------------------------------------------------------------------
    def wait(self, timeout_ms: int) -> bool:
        """Poll all services once (after an adaptive sleep); True when all done."""
        time.sleep(min(self._poll_ms, timeout_ms if timeout_ms > 0 else self._poll_ms) / 1000.0)
        self._poll_ms = min(self._poll_ms * 2, max(self.cfg.svc_update_int_ms, 50))

        def poll(i: int, hs: HostState):
            if hs.done:
                return
            t0 = time.monotonic()
            st = hs.client.get("/status")
            # --svcping: /status round-trip per service for the dashboard
            # (reference RemoteWorker pingMicroSecs, RemoteWorker.cpp:479)
            hs.ping_us = int((time.monotonic() - t0) * 1e6)
            if st.get("bench_id") and st["bench_id"] != self._bench_id:
                raise RuntimeError(
                    f"Service {hs.client.hostport} reports foreign benchmark ID "
                    f"(service hijacked?): {st['bench_id']} != {self._bench_id}")
            hs.last_status = st
            if st.get("workers_total") and st["workers_done"] >= st["workers_total"]:
                hs.done = True

        self._for_all(poll)

        # stonewall propagation: the first service whose worker finished its
        # fair share defines the whole job's first-done point — tell the
        # other services to snapshot now (reference RemoteWorker :453-583)
        if not self._stonewall_sent and any(
                hs.last_status.get("stonewall_triggered") for hs in self.hosts):
            self._stonewall_sent = True

            def sw(i: int, hs: HostState):
                if not hs.last_status.get("stonewall_triggered"):
                    hs.client.get("/triggerstonewall")

            try:
                self._for_all(sw)
            except RuntimeError:
                pass  # best effort; local finish times still bound the result

        return all(hs.done for hs in self.hosts)

    # ------------------------------------------------------------------
    def poll(self) -> dict[str, Any]:
        agg = {"entries": 0, "bytes": 0, "iops": 0, "workers_done": 0, "workers_total": 0,
               "workers_with_error": 0, "elapsed_usec": 0, "stonewall_triggered": False,
               "lat_num_ios": 0, "lat_sum_ios": 0, "lat_num_entries": 0,
               "lat_sum_entries": 0}
        for hs in self.hosts:
            st = hs.last_status
            if not st or st.get("idle"):
                continue
            for k in ("entries", "bytes", "iops", "workers_done", "workers_total",
                      "workers_with_error", "lat_num_ios", "lat_sum_ios",
                      "lat_num_entries", "lat_sum_entries"):
                agg[k] += st.get(k, 0)
            agg["elapsed_usec"] = max(agg["elapsed_usec"], st.get("elapsed_usec", 0))
            agg["stonewall_triggered"] |= bool(st.get("stonewall_triggered"))
        return agg

    # ------------------------------------------------------------------
    def poll_workers(self):
        """Per-service rows for the fullscreen dashboard."""
        rows = []
        for i, hs in enumerate(self.hosts):
            st = hs.last_status
            if not st or st.get("idle"):
                continue
            row = {"rank": i, "entries": st.get("entries", 0),
                   "bytes": st.get("bytes", 0), "iops": st.get("iops", 0)}
            if self.cfg.svc_ping:
                row["ping_us"] = hs.ping_us
            rows.append(row)
        return rows

    # ------------------------------------------------------------------
    def rotate_hosts(self, n: int) -> None:
        """--rotatehosts: rotate the service list by n between phases
        (reference Coordinator::rotateHosts, Coordinator.cpp:384)."""
        if not n or len(self.hosts) < 2:
            return
        n %= len(self.hosts)
        self.hosts = self.hosts[n:] + self.hosts[:n]

    # ------------------------------------------------------------------
    def interrupt(self) -> None:
        try:
            self._for_all(lambda i, hs: hs.client.get("/interruptphase"))
        except RuntimeError:
            pass

    # ------------------------------------------------------------------
    def finish(self) -> list[WorkerStats]:
        def collect(i: int, hs: HostState):
            return hs.client.get("/benchresult")

        all_workers: list[WorkerStats] = []
        self.last_service_elapsed = []  # (hostport, max elapsed usec)
        for hs, res in zip(self.hosts, self._for_all(collect)):
            host_workers = []
            for w in res["workers"]:
                ws = WorkerStats(**{k: w[k] for k in w if k in WorkerStats.__dataclass_fields__})
                if ws.error:
                    # frame remote errors with the origin host (reference
                    # RemoteWorker::frameHostErrorMsg, RemoteWorker.cpp:650)
                    ws.error = f"[{hs.client.hostport}] {ws.error}"
                host_workers.append(ws)
            # --dataprofile: the service's merged profile (optional keys; a
            # service that sends none contributes none)
            if res.get("data_profile") and host_workers:
                host_workers[0].data_profile = DataProfile.from_wire(res["data_profile"])
            all_workers.extend(host_workers)
            self.last_service_elapsed.append(
                (hs.client.hostport,
                 max((w.elapsed_usec for w in host_workers), default=0)))
        return all_workers

    # ------------------------------------------------------------------
    def planned_work(self, phase_name: str) -> tuple[int, int]:
        cfg = self.cfg
        if cfg.path_type == "dir":
            n_hosts = len(self.hosts)
            dirs = cfg.dirs or 1
            if phase_name in ("MKDIRS", "RMDIRS"):
                return cfg.dirs * cfg.threads * n_hosts, 0
            if phase_name in ("WRITE", "READ"):
                e = dirs * cfg.files * cfg.threads * n_hosts
                return e, e * cfg.file_size
            if phase_name in ("STAT", "RMFILES"):
                return dirs * cfg.files * cfg.threads * n_hosts, 0
            return 0, 0
        if phase_name == "NETBENCH":
            n_clients = getattr(self, "_nb_total_client_threads",
                                len(self.hosts) * cfg.threads)
            return 0, cfg.file_size * n_clients
        if phase_name in ("WRITE", "READ"):
            total = cfg.file_size * len(cfg.paths)
            if cfg.no_svc_share:
                total *= len(self.hosts)
            if cfg.random and cfg.rand_amount:
                total = cfg.rand_amount
            return 0, total
        return 0, 0

    def close(self) -> None:
        pass


def send_control(cfg: BenchConfig, quit: bool = False) -> None:
    """--interrupt / --quit: stop the phase (and optionally the services)."""
    auth = ""
    if cfg.svc_pw_file:
        with open(cfg.svc_pw_file) as f:
            auth = hashlib.sha256(f.read().strip().encode()).hexdigest()
    for h in cfg.hosts:
        client = ServiceClient(h, auth)
        try:
            client.get(f"/interruptphase?quit={'1' if quit else '0'}")
            print(f"Service {h}: {'quit' if quit else 'interrupt'} requested.")
        except (ConnectionError, OSError, RuntimeError) as e:
            print(f"Service {h}: {e}")
