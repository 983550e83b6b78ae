"""Distributed service/master mode over localhost HTTP (no real cluster),
mirroring reference tools/test-examples.sh:293-342."""

import json
import os
import socket
import subprocess
import sys
import time
import urllib.request

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def free_port() -> int:
    s = socket.socket()
    s.bind(("", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture
def services():
    ports = [free_port(), free_port()]
    procs = []
    env = dict(os.environ, PYTHONPATH=REPO)
    for p in ports:
        procs.append(subprocess.Popen(
            [sys.executable, "-m", "elbencho_amd", "--service", "--foreground",
             "--port", str(p)],
            env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    # wait for readiness
    deadline = time.monotonic() + 40
    for p in ports:
        while True:
            try:
                with urllib.request.urlopen(
                        f"http://127.0.0.1:{p}/protocolversion", timeout=1) as r:
                    r.read()
                break
            except OSError:
                if time.monotonic() > deadline:
                    for pr in procs:
                        pr.kill()
                    raise RuntimeError("service did not become ready")
                time.sleep(0.1)
    yield ports
    for pr in procs:
        pr.terminate()
        try:
            pr.wait(5)
        except subprocess.TimeoutExpired:
            pr.kill()


def run_master(args):
    env = dict(os.environ, PYTHONPATH=REPO)
    return subprocess.run([sys.executable, "-m", "elbencho_amd", "--nolive"] + args,
                          env=env, capture_output=True, text=True, timeout=120)


def test_service_endpoints(services):
    port = services[0]
    with urllib.request.urlopen(f"http://127.0.0.1:{port}/info", timeout=5) as r:
        assert b"elbencho-amd service" in r.read()
    with urllib.request.urlopen(f"http://127.0.0.1:{port}/status", timeout=5) as r:
        st = json.loads(r.read())
    assert st["idle"] is True


def test_distributed_dir_mode(services, tmp_path):
    hosts = ",".join(f"127.0.0.1:{p}" for p in services)
    res = run_master(["--hosts", hosts, "-t", "2", "-d", "-n", "2", "-w", "-r",
                      "-N", "3", "-s", "16k", "-F", "-D", "--verify", "1",
                      str(tmp_path)])
    assert res.returncode == 0, res.stdout + res.stderr
    # 2 services x 2 threads x 2 dirs x 3 files
    assert "Files total" in res.stdout
    assert list(tmp_path.iterdir()) == []
    # master output must aggregate both services:
    # 2 services x 2 threads x 2 dirs x 3 files = 24
    for line in res.stdout.splitlines():
        if "Files total" in line:
            assert line.split()[-1] == "24"
            break


def test_distributed_shared_file(services, tmp_path):
    hosts = ",".join(f"127.0.0.1:{p}" for p in services)
    f = tmp_path / "shared"
    res = run_master(["--hosts", hosts, "-t", "2", "-w", "-r", "-s", "1m",
                      "-b", "64k", "--verify", "2", str(f)])
    assert res.returncode == 0, res.stdout + res.stderr
    assert f.stat().st_size == 1024 * 1024
    # whole file written exactly once across 2 services x 2 threads
    from elbencho_amd import load_core
    core = load_core()
    assert core.verify_checksum(f.read_bytes(), 0, 2) == 2**64 - 1


def test_quit_services(services):
    hosts = ",".join(f"127.0.0.1:{p}" for p in services)
    res = run_master(["--hosts", hosts, "--quit"])
    assert res.returncode == 0
    # services exit shortly after
    deadline = time.monotonic() + 10
    while time.monotonic() < deadline:
        try:
            urllib.request.urlopen(
                f"http://127.0.0.1:{services[0]}/status", timeout=1).read()
            time.sleep(0.2)
        except OSError:
            return
    raise AssertionError("service did not quit")


def test_netbench(services, tmp_path):
    """Netbench: first host is server, second is client (reference
    tools/test-examples.sh has no netbench case; this mirrors docs usage)."""
    hosts = ",".join(f"127.0.0.1:{p}" for p in services)
    server = f"127.0.0.1:{services[0]}"
    res = run_master(["--hosts", hosts, "--netbench", "-w", "-t", "2", "-s", "4m",
                      "-b", "64k", "--servers", server, "--respsize", "1k",
                      "--lat", str(tmp_path)])
    assert res.returncode == 0, res.stdout + res.stderr
    assert "NETBENCH" in res.stdout
    # 2 client threads x 4 MiB = 8 MiB transferred
    for line in res.stdout.splitlines():
        if "Total MiB" in line:
            assert line.split()[-1] == "8"
            break
    else:
        raise AssertionError("no Total MiB row in:\n" + res.stdout)


def test_master_interrupt_rpc(services, tmp_path):
    """--interrupt stops a running phase on the services."""
    import threading

    hosts = ",".join(f"127.0.0.1:{p}" for p in services)
    f = tmp_path / "big"

    results = {}

    def run():
        results["res"] = run_master(["--hosts", hosts, "-t", "1", "-w", "-s", "1g",
                                     "-b", "64k", "--limitwrite", "2m", str(f)])

    t = threading.Thread(target=run)
    t.start()
    time.sleep(3)  # let the write phase start
    intr = run_master(["--hosts", hosts, "--interrupt"])
    assert intr.returncode == 0
    t.join(60)
    assert not t.is_alive()
    # interrupted phase -> master exits nonzero with the interrupt reported
    assert results["res"].returncode != 0
    assert "interrupt" in (results["res"].stdout + results["res"].stderr).lower()


def test_rotatehosts(services, tmp_path):
    """--rotatehosts shifts service rank assignment between phases."""
    hosts = ",".join(f"127.0.0.1:{p}" for p in services)
    res = run_master(["--hosts", hosts, "--rotatehosts", "1", "-t", "1", "-d",
                      "-n", "1", "-w", "-r", "-N", "2", "-s", "4k", "-F", "-D",
                      str(tmp_path)])
    assert res.returncode == 0, res.stdout + res.stderr


def test_distributed_custom_tree(services, tmp_path):
    """Custom tree partitioning across two services (tree shipped in the
    wire config; shared big file range-sliced across all ranks)."""
    from elbencho_amd.pathstore import CustomTree, write_treefile

    base = tmp_path / "bench"
    base.mkdir()
    tf = tmp_path / "tree.txt"
    tree = CustomTree(dirs=["a", "a/b"],
                      files=[("a/small1", 4096), ("a/b/small2", 8192),
                             ("bigshared", 1 << 20)])
    write_treefile(tree, str(tf))
    hosts = ",".join(f"127.0.0.1:{p}" for p in services)
    res = run_master(["--hosts", hosts, "-t", "2", "-d", "-w", "-r", "-F", "-D",
                      "-b", "64k", "--treefile", str(tf), "--sharesize", "512k",
                      "--verify", "6", str(base)])
    assert res.returncode == 0, res.stdout + res.stderr
    assert not (base / "a").exists()
    assert not (base / "bigshared").exists()


def test_service_error_history_framed(tmp_path, services):
    """Worker errors surface in the service error history (/benchresult) and
    the master frames them with the origin host (reference Logger error
    history + RemoteWorker::frameHostErrorMsg)."""
    port = services[0]
    res = run_master(["--hosts", f"127.0.0.1:{port}", "-r", "-t", "1",
                      "-s", "1m", "-b", "1m", "--nolive",
                      str(tmp_path / "missing_file")])
    out = res.stdout + res.stderr
    assert res.returncode != 0
    assert f"[127.0.0.1:{port}]" in out  # framed host in the error line


def test_s3_mpu_sharing_across_services(services, tmp_path):
    """Cross-service --s3mpusharing: the master pre-creates the multipart
    uploads and all services add disjoint parts to the SAME uploadId; a
    later --s3mpucompl run completes, then a read verifies the data."""
    from tests.s3mock import ACCESS_KEY, SECRET_KEY, S3Handler, start_mock

    server, port = start_mock()
    try:
        ep = f"http://127.0.0.1:{port}"
        hosts = ",".join(f"127.0.0.1:{p}" for p in services)
        s3args = ["--s3endpoints", ep, "--s3key", ACCESS_KEY,
                  "--s3secret", SECRET_KEY]
        res = run_master(s3args + ["--hosts", hosts, "-d", "-w", "-t", "2",
                                   "-s", "512k", "-b", "64k", "--s3mpusharing",
                                   "--verify", "8", "shsvc/obj1", "shsvc/obj2"])
        assert res.returncode == 0, res.stdout + res.stderr
        with S3Handler.store.lock:
            # one shared upload per object, parts from all 4 ranks, still open
            assert len(S3Handler.store.uploads) == 2
            assert all(len(parts) == 8 for parts in
                       S3Handler.store.uploads.values())
            assert S3Handler.store.buckets["shsvc"] == {}
        # completion from a separate instance (standalone, no services)
        res = run_master(s3args + ["--s3mpucompl", "-t", "1", "-s", "512k",
                                   "-b", "64k", "s3://shsvc"])
        assert res.returncode == 0, res.stdout + res.stderr
        with S3Handler.store.lock:
            assert not S3Handler.store.uploads
            assert len(S3Handler.store.buckets["shsvc"]["obj1"]) == 512 * 1024
        res = run_master(s3args + ["--hosts", hosts, "-r", "-t", "2",
                                   "-s", "512k", "-b", "64k", "--s3mpusharing",
                                   "--verify", "8", "shsvc/obj1", "shsvc/obj2"])
        assert res.returncode == 0, res.stdout + res.stderr
    finally:
        server.shutdown()


def test_svcpwfile_auth(tmp_path):
    """--svcpwfile: master requests must carry the shared-secret hash; a
    master without the password is rejected (reference HashTk + svcpwfile)."""
    pw = tmp_path / "secret.txt"
    pw.write_text("hunter2\n")
    port = free_port()
    env = dict(os.environ, PYTHONPATH=REPO)
    proc = subprocess.Popen(
        [sys.executable, "-m", "elbencho_amd", "--service", "--foreground",
         "--port", str(port), "--svcpwfile", str(pw)],
        env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    try:
        deadline = time.monotonic() + 40
        while True:
            try:
                with urllib.request.urlopen(
                        f"http://127.0.0.1:{port}/protocolversion", timeout=1) as r:
                    r.read()
                break
            except urllib.error.HTTPError:
                break  # 403 = up, but auth required (expected)
            except OSError:
                if time.monotonic() > deadline:
                    raise
                time.sleep(0.1)
        bench = tmp_path / "f1"
        res = run_master(["--hosts", f"127.0.0.1:{port}", "-w", "-t", "1",
                          "-s", "64k", "-b", "64k", str(bench)])
        assert res.returncode != 0  # no password -> rejected
        res = run_master(["--hosts", f"127.0.0.1:{port}", "--svcpwfile", str(pw),
                          "-w", "-t", "1", "-s", "64k", "-b", "64k", str(bench)])
        assert res.returncode == 0, res.stdout + res.stderr
    finally:
        proc.terminate()
        proc.wait(5)


def test_numhosts_limits_services(services, tmp_path):
    """--numhosts 1: only the first of the two services runs the phase."""
    hosts = ",".join(f"127.0.0.1:{p}" for p in services)
    res = run_master(["--hosts", hosts, "--numhosts", "1", "-d", "-w", "-t", "2",
                      "-n", "1", "-N", "2", "-s", "16k", "-F", "-D",
                      str(tmp_path)])
    assert res.returncode == 0, res.stdout + res.stderr
    for line in res.stdout.splitlines():
        if "Files total" in line:
            # 1 host x 2 threads x 1 dir x 2 files (2 hosts would give 8)
            assert line.split()[-1] == "4"
            break
    else:
        raise AssertionError("no Files total row:\n" + res.stdout)


def test_nosvcshare_whole_dataset_per_host(services, tmp_path):
    """--nosvcshare: every service host writes the whole dataset instead of
    a partition (total bytes = hosts x size)."""
    hosts = ",".join(f"127.0.0.1:{p}" for p in services)
    res = run_master(["--hosts", hosts, "--nosvcshare", "-w", "-t", "2",
                      "-s", "2m", "-b", "1m", str(tmp_path / "shared")])
    assert res.returncode == 0, res.stdout + res.stderr
    for line in res.stdout.splitlines():
        if "Total MiB" in line:
            assert line.split()[-1] == "4"  # 2 hosts x 2 MiB
            break
    else:
        raise AssertionError("no Total MiB row:\n" + res.stdout)


def test_gpuperservice_override_unit():
    """--gpuperservice: each service keeps one GPU (set) from the list,
    selected by its service index (reference ProgArgs.h:378)."""
    from elbencho_amd.config import BenchConfig
    from elbencho_amd.service import ServiceState

    st = ServiceState(BenchConfig())
    cfg = BenchConfig()
    cfg.threads = 1
    cfg.gpu_ids = [0, 1, 2, 3]
    cfg.gpu_per_service = True
    cfg.paths = []
    wire = cfg.to_wire()
    wire["service_index"] = 2
    # prepare builds the runner; no paths and no phases -> engine with no work
    st.prepare_phase(wire)
    assert st.cfg.gpu_ids == [2]


def test_service_reuse_after_interrupt(services, tmp_path):
    """A service stays usable after a phase is interrupted mid-flight
    (reference /interruptphase semantics: reset, no quit)."""
    hosts = ",".join(f"127.0.0.1:{p}" for p in services)
    env = dict(os.environ, PYTHONPATH=REPO)
    # long-running write (rate-limited to 64 MiB/s per thread, so 8 GiB
    # takes a minute on any machine, however fast its tmpfs) with a 1s
    # timelimit -> master interrupts the phase and reports failure
    res = run_master(["--hosts", hosts, "-w", "-t", "1", "-s", "8g", "-b", "1m",
                      "--limitwrite", "64m", "--timelimit", "1",
                      str(tmp_path / "big")])
    assert res.returncode != 0
    # the same services then run a normal benchmark cleanly
    res = run_master(["--hosts", hosts, "-w", "-r", "-t", "1", "-s", "1m",
                      "-b", "1m", "--verify", "2", str(tmp_path / "small")])
    assert res.returncode == 0, res.stdout + res.stderr


def test_distributed_hdfs(services, tmp_path):
    """Services route HDFS configs to the WebHDFS engine."""
    from tests.webhdfsmock import WebHdfsHandler, start_mock

    server, port = start_mock()
    try:
        hosts = ",".join(f"127.0.0.1:{p}" for p in services)
        res = run_master(["--hosts", hosts, "-d", "-w", "-r", "-F", "-D",
                          "-t", "2", "-n", "1", "-N", "2", "-s", "32k",
                          "-b", "32k", "--verify", "6",
                          f"hdfs://127.0.0.1:{port}/dbench"])
        assert res.returncode == 0, res.stdout + res.stderr
        for line in res.stdout.splitlines():
            if "Files total" in line:
                # 2 services x 2 threads x 1 dir x 2 files
                assert line.split()[-1] == "8"
                break
        else:
            raise AssertionError("no Files total row:\n" + res.stdout)
        with WebHdfsHandler.store.lock:
            assert not WebHdfsHandler.store.files
    finally:
        server.shutdown()


def test_protocol_version_mismatch_rejected(services):
    """A master with a different wire version is refused at /preparephase
    (reference protocol-version check, HTTPServiceSWS.cpp:268)."""
    import http.client

    port = services[0]
    conn = http.client.HTTPConnection("127.0.0.1", port, timeout=10)
    body = json.dumps({"protocol_version": "99.0.0", "config": {}}).encode()
    conn.request("POST", "/preparephase", body=body,
                 headers={"Content-Type": "application/json"})
    resp = conn.getresponse()
    data = resp.read()
    conn.close()
    assert resp.status == 400
    assert b"protocol version mismatch" in data


def test_daemonized_service_lifecycle(tmp_path):
    """Default (non-foreground) service: double-fork daemonize, serve, obey
    a master --quit (the suite otherwise only covers --foreground)."""
    port = free_port()
    env = dict(os.environ, PYTHONPATH=REPO, TMPDIR=str(tmp_path))
    # parent exits immediately after daemonizing
    res = subprocess.run([sys.executable, "-m", "elbencho_amd", "--service",
                          "--port", str(port)], env=env, capture_output=True,
                         text=True, timeout=60, cwd=str(tmp_path))
    assert res.returncode == 0, res.stdout + res.stderr
    try:
        deadline = time.monotonic() + 30
        while True:
            try:
                with urllib.request.urlopen(
                        f"http://127.0.0.1:{port}/info", timeout=1) as r:
                    assert b"elbencho-amd service" in r.read()
                break
            except OSError:
                assert time.monotonic() < deadline, "daemon never came up"
                time.sleep(0.2)
        bench = run_master(["--hosts", f"127.0.0.1:{port}", "-w", "-r",
                            "-t", "1", "-s", "64k", "-b", "64k",
                            str(tmp_path / "f1")])
        assert bench.returncode == 0, bench.stdout + bench.stderr
    finally:
        subprocess.run([sys.executable, "-m", "elbencho_amd",
                        "--hosts", f"127.0.0.1:{port}", "--quit"],
                       env=env, capture_output=True, timeout=30)


def test_bench_path_info_consistency_check(tmp_path):
    """Master cross-checks the BenchPathInfo from /preparephase (reference
    WorkerManager::checkServiceBenchPathInfos): a service whose path
    override yields a different path count fails the run fast."""
    ports = [free_port(), free_port()]
    env = dict(os.environ, PYTHONPATH=REPO)
    d1, d2a, d2b = tmp_path / "a", tmp_path / "b1", tmp_path / "b2"
    for d in (d1, d2a, d2b):
        d.mkdir()
    procs = [
        subprocess.Popen([sys.executable, "-m", "elbencho_amd", "--service",
                          "--foreground", "--port", str(ports[0])],
                         env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT),
        # this one overrides the bench path with TWO paths
        subprocess.Popen([sys.executable, "-m", "elbencho_amd", "--service",
                          "--foreground", "--port", str(ports[1]),
                          "--path", str(d2a), "--path", str(d2b)],
                         env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT),
    ]
    try:
        deadline = time.monotonic() + 40
        for p in ports:
            while True:
                try:
                    with urllib.request.urlopen(
                            f"http://127.0.0.1:{p}/protocolversion",
                            timeout=1) as r:
                        r.read()
                    break
                except OSError:
                    if time.monotonic() > deadline:
                        raise RuntimeError("service did not become ready")
                    time.sleep(0.1)

        res = run_master(["--hosts",
                          f"localhost:{ports[0]},localhost:{ports[1]}",
                          "-t", "1", "-d", "-n", "1", "-w", "-N", "1",
                          "-s", "4k", str(d1)])
        assert res.returncode != 0
        out = res.stdout + res.stderr
        assert "paths count" in out or "number of benchmark paths" in out, out
    finally:
        for pr in procs:
            pr.terminate()
            try:
                pr.wait(5)
            except subprocess.TimeoutExpired:
                pr.kill()


def test_service_many_sequential_runs(services, tmp_path):
    """A persistent service survives many master runs (per-/preparephase
    runner teardown; 50-run one-off also clean)."""
    for i in range(8):
        res = run_master(["--hosts",
                          f"localhost:{services[0]},localhost:{services[1]}",
                          "-t", "2", "-d", "-n", "1", "-w", "-r", "-N", "3",
                          "-s", "128k", "-b", "64k", "--verify", str(i),
                          "-F", "-D", "--no0usecerr", str(tmp_path)])
        assert res.returncode == 0, (i, res.stdout[-300:], res.stderr[-300:])


def test_svcwait_master_waits_for_late_service(tmp_path):
    """--svcwait: the master keeps retrying until the service appears
    (reference --svcwait semantics) instead of failing after the default
    10 s readiness window."""
    import threading

    port = free_port()
    env = dict(os.environ, PYTHONPATH=REPO)

    svc_holder = {}

    def start_service_late():
        time.sleep(2.0)
        svc_holder["proc"] = subprocess.Popen(
            [sys.executable, "-m", "elbencho_amd", "--service",
             "--foreground", "--port", str(port)],
            env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)

    t = threading.Thread(target=start_service_late)
    t.start()
    try:
        res = run_master(["--svcwait", "--hosts", f"localhost:{port}",
                          "-t", "1", "-w", "-s", "64k", "-b", "64k",
                          str(tmp_path / "f")])
        assert res.returncode == 0, res.stdout + res.stderr
    finally:
        t.join()
        pr = svc_holder.get("proc")
        if pr:
            subprocess.run([sys.executable, "-m", "elbencho_amd", "--hosts",
                            f"localhost:{port}", "--quit"], env=env,
                           capture_output=True, timeout=30)
            try:
                pr.wait(10)
            except subprocess.TimeoutExpired:
                pr.kill()
