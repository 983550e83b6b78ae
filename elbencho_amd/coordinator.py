"""Run control: phase ordering, iterations, live stats loop, time limit.

Reference analogue: /root/reference/source/Coordinator.cpp (phase order
:311-334, sync/dropcaches interleave :278, SIGINT handling :420) and the
WorkerManager phase barrier. Independent implementation: the local engine is
the native _core.Engine; remote services are driven via elbencho_amd.remote;
multi-GPU lockstep uses RCCL via elbencho_amd.parallel when torch.distributed
is initialized.
"""

from __future__ import annotations

import signal
import sys
import time
import uuid
from typing import Any, Optional

from elbencho_amd import load_core
from elbencho_amd.config import BenchConfig, PATH_DIR
from elbencho_amd.stats import (CpuUtil, LiveCsvWriter, LiveStatsPrinter, PhaseResults,
                                WorkerStats, aggregate_phase, append_csv_result,
                                append_json_result, print_phase_results,
                                print_results_table_header)

PHASE_CODES: dict[str, int] = {}


def phase_code(name: str) -> int:
    global PHASE_CODES
    if not PHASE_CODES:
        PHASE_CODES = dict(load_core().PHASES)
    return PHASE_CODES[name]


class LocalRunner:
    """Drives the native engine for one instance (standalone or service)."""

    def __init__(self, cfg: BenchConfig):
        self.cfg = cfg
        self.core = load_core()
        self.engine = self.core.Engine(cfg.engine_dict())
        self.engine.prepare()

    def start(self, phase_name: str) -> None:
        self.engine.start_phase(phase_code(phase_name))

    def poll(self) -> dict[str, Any]:
        return self.engine.poll()

    def poll_workers(self) -> list[dict[str, Any]]:
        return self.engine.poll_workers()

    def wait(self, timeout_ms: int) -> bool:
        return self.engine.wait_phase_done(timeout_ms)

    def interrupt(self) -> None:
        self.engine.interrupt()

    def trigger_stonewall(self) -> None:
        self.engine.trigger_stonewall()

    def finish(self) -> list[WorkerStats]:
        return [WorkerStats.from_engine(d) for d in self.engine.finish_phase()]

    def planned_work(self, phase_name: str) -> tuple[int, int]:
        return tuple(self.engine.planned_work(phase_code(phase_name)))


class Coordinator:
    def __init__(self, cfg: BenchConfig, out=None):
        self.cfg = cfg
        self.out = out or sys.stdout
        self.interrupted = False
        self._sigint_count = 0
        self.runner: Any = None
        self.dist = None  # parallel.PhaseSync when torch.distributed is up

    # ------------------------------------------------------------------
    def main(self) -> int:
        cfg = self.cfg

        if cfg.quit_services or cfg.interrupt_services:
            from elbencho_amd.remote import send_control
            send_control(cfg, quit=cfg.quit_services)
            return 0

        if cfg.service_mode:
            from elbencho_amd.service import run_service
            return run_service(cfg)

        if cfg.tree_scan:
            from elbencho_amd.pathstore import scan_path, write_treefile
            if not cfg.treefile:
                print("ERROR: --treescan requires --treefile as output path",
                      file=sys.stderr)
                return 1
            tree = scan_path(cfg.tree_scan)
            write_treefile(tree, cfg.treefile)
            print(f"Scanned {cfg.tree_scan}: {len(tree.dirs)} dirs, "
                  f"{len(tree.files)} files -> {cfg.treefile}", file=self.out)
            return 0

        old_sigint = None
        try:
            old_sigint = signal.signal(signal.SIGINT, self._on_sigint)
        except ValueError:
            pass  # not in main thread (tests)

        if cfg.hosts:
            from elbencho_amd.remote import RemoteRunner
            self.runner = RemoteRunner(cfg)
        else:
            import os
            if "RANK" in os.environ and "WORLD_SIZE" in os.environ:
                # launched under torch.distributed.run: one instance per GPU,
                # RCCL barrier + all-reduce replace the HTTP master poll —
                # applies to the posix engine AND the S3 object engine
                from elbencho_amd import parallel
                self.dist = parallel.init_from_env()
                if self.dist:
                    rank, world = self.dist.rank, self.dist.world_size
                    if cfg.gpu_ids:
                        local = int(os.environ.get("LOCAL_RANK", rank))
                        cfg.gpu_ids = [cfg.gpu_ids[local % len(cfg.gpu_ids)]]
                    cfg.rank_offset = rank * cfg.threads
                    if cfg.bench_mode == "s3" or (
                            not cfg.no_svc_share and cfg.path_type != PATH_DIR):
                        cfg.num_dataset_threads = cfg.threads * world
                    else:
                        cfg.num_dataset_threads = cfg.threads
            if cfg.bench_mode == "s3":
                from elbencho_amd.s3 import S3Runner
                self.runner = S3Runner(cfg)
            elif cfg.bench_mode == "hdfs":
                from elbencho_amd.hdfs import HdfsRunner
                self.runner = HdfsRunner(cfg)
            else:
                self.runner = LocalRunner(cfg)

        try:
            if cfg.dryrun:
                self._print_dryrun()
                return 0
            return self.run_benchmarks()
        finally:
            closer = getattr(self.runner, "close", None)
            if closer:
                closer()
            # drop the SIGINT closure: it references this Coordinator (and
            # through it the runner + clients + GPU contexts) globally, which
            # would pin the whole object graph after the run ends
            if old_sigint is not None:
                try:
                    signal.signal(signal.SIGINT, old_sigint)
                except ValueError:
                    pass

    # ------------------------------------------------------------------
    def _on_sigint(self, signum, frame):
        self._sigint_count += 1
        if self._sigint_count == 1:
            print("\nReceived interrupt. Finishing current phase gracefully "
                  "(interrupt again to abort)...", file=sys.stderr)
            self.interrupted = True
            if self.runner:
                self.runner.interrupt()
        else:
            print("\nAborting.", file=sys.stderr)
            sys.exit(130)

    # ------------------------------------------------------------------
    def _print_dryrun(self) -> None:
        cfg = self.cfg
        print("DRY RUN (no I/O will be done)", file=self.out)
        for name in cfg.phase_list():
            entries, nbytes = self.runner.planned_work(name)
            print(f"  {name}: entries={entries} bytes={nbytes}", file=self.out)

    # ------------------------------------------------------------------
    def run_benchmarks(self) -> int:
        cfg = self.cfg
        phases = cfg.phase_list()
        if not phases and not (cfg.run_sync or cfg.run_dropcaches):
            print("No benchmark phase selected (e.g. -w to write or -r to read).",
                  file=sys.stderr)
            return 1

        if cfg.start_time:
            delay = cfg.start_time - time.time()
            if delay > 0:
                time.sleep(delay)

        rc = 0
        for it in range(cfg.iterations):
            if cfg.iterations > 1:
                print(f"[Starting iteration {it + 1} of {cfg.iterations}...]", file=self.out)
            print_results_table_header(self.out)

            self._run_sync_and_dropcaches()

            for i, name in enumerate(phases):
                if self.interrupted:
                    rc = 130
                    break
                ok = self.run_phase(name)
                if not ok:
                    rc = 1
                    break
                self._run_sync_and_dropcaches()
                if i < len(phases) - 1:
                    if cfg.phase_delay_secs:
                        time.sleep(cfg.phase_delay_secs)
                    if cfg.rotate_hosts:
                        rot = getattr(self.runner, "rotate_hosts", None)
                        if rot:
                            rot(cfg.rotate_hosts)
            if rc:
                break
        return rc

    def _run_sync_and_dropcaches(self) -> None:
        if self.cfg.run_sync:
            self.run_phase("SYNC", quiet=False)
        if self.cfg.run_dropcaches:
            self.run_phase("DROPCACHES", quiet=False)

    # ------------------------------------------------------------------
    S3_DISPLAY = {"MKDIRS": "MKBUCKETS", "RMDIRS": "RMBUCKETS", "WRITE": "WRITE",
                  "READ": "READ", "STAT": "HEADOBJ", "RMFILES": "RMOBJECTS",
                  "LISTOBJ": "LISTOBJ", "PUTOBJACL": "PUTOBJACL",
                  "GETOBJACL": "GETOBJACL", "PUTBACL": "PUTBACL",
                  "GETBACL": "GETBACL", "PUTOTAG": "PUTOBJMD",
                  "GETOTAG": "GETOBJMD", "DELOTAG": "DELOBJMD",
                  "PUTBTAG": "PUTBUCKETMD", "GETBTAG": "GETBUCKETMD",
                  "S3MPUCOMPLETE": "MPUCOMPL", "BVERSION": "BVERSION",
                  "OLOCKCFG": "OLOCKCFG", "STATDIRS": "STATDIRS",
                  "LISTOBJPAR": "LISTOBJ_P"}

    def run_phase(self, name: str, quiet: bool = False) -> bool:
        cfg = self.cfg
        phase_id = str(uuid.uuid4())
        start_time = time.time()
        display = (self.S3_DISPLAY.get(name, name)
                   if cfg.bench_mode == "s3" else name)

        planned_entries, planned_bytes = self.runner.planned_work(name)

        cpu_first_meter = CpuUtil()  # phase start -> stonewall
        cpu_last_meter = CpuUtil()   # phase start -> phase end

        # live display: fullscreen per-worker dashboard on a TTY by default,
        # --live1 single line, --live1n newline mode (reference behavior)
        from elbencho_amd.livestats import (FullscreenLiveStats, LiveCsvExWriter,
                                            NewlineLiveStats)
        if cfg.live1 or not sys.stderr.isatty():
            live = LiveStatsPrinter(cfg, display, planned_entries, planned_bytes)
        elif getattr(cfg, "live1n", False):
            live = NewlineLiveStats(cfg, display)
        else:
            live = FullscreenLiveStats(cfg, display, planned_bytes, planned_entries)
        want_worker_rows = isinstance(live, FullscreenLiveStats) or cfg.live_csv_ex
        if cfg.live_csv and cfg.live_csv_ex:
            live_csv = LiveCsvExWriter(cfg.live_csv, cfg, name)
        elif cfg.live_csv:
            live_csv = LiveCsvWriter(cfg.live_csv, cfg, name)
        else:
            live_csv = None

        if self.dist:
            # cross-rank --s3mpusharing: rank 0 pre-creates the shared
            # multipart uploads, all ranks receive the uploadIds (same
            # mechanism as the HTTP master's wire distribution)
            if (cfg.bench_mode == "s3" and cfg.s3_mpu_sharing and
                    name == "WRITE" and not cfg.s3_mpu_upload_ids):
                import torch.distributed as torch_dist

                from elbencho_amd.s3 import precreate_upload_ids
                box = [precreate_upload_ids(cfg) if self.dist.rank == 0 else None]
                torch_dist.broadcast_object_list(box, src=0)
                cfg.s3_mpu_upload_ids = box[0]
                for objpath, upload_id in cfg.s3_mpu_upload_ids.items():
                    b, _, k = objpath.partition("/")
                    self.runner.upload_store.seed(b, k, upload_id)
            self.dist.barrier()  # lockstep phase start across GPU ranks

        if cfg.log_level >= 1:
            print(f"[phase {display}] id={phase_id} planned_entries={planned_entries} "
                  f"planned_bytes={planned_bytes}", file=sys.stderr)

        self.runner.start(name)

        deadline = time.monotonic() + cfg.timelimit if cfg.timelimit else None
        poll_int = max(0.05, cfg.live_int_ms / 1000.0)
        cpu_first: Optional[int] = None

        while not self.runner.wait(int(poll_int * 1000)):
            p = self.runner.poll()
            if cpu_first is None and p.get("stonewall_triggered"):
                cpu_first = cpu_first_meter.percent_since_last()
            rows = None
            if want_worker_rows:
                getter = getattr(self.runner, "poll_workers", None)
                rows = getter() if getter else None
            live.update(p, rows)
            if live_csv:
                if isinstance(live_csv, LiveCsvExWriter):
                    live_csv.update(p, rows or [])
                else:
                    live_csv.update(p)
            if deadline and time.monotonic() > deadline:
                print(f"\nPhase time limit reached ({cfg.timelimit}s); "
                      "interrupting workers...", file=sys.stderr)
                self.runner.interrupt()
                deadline = None

        live.finish()
        if live_csv:
            live_csv.close()

        cpu_last = cpu_last_meter.percent_since_last()
        if cpu_first is None:
            cpu_first = cpu_last
        workers = self.runner.finish()

        results = aggregate_phase(display, phase_id, start_time, workers,
                                  cpu_first, cpu_last)

        if self.dist:
            results = self.dist.allreduce_results(
                results, with_profile=cfg.data_profile and name == "READ")

        if not quiet or results.errors:
            if self.dist is None or self.dist.rank == 0:
                print_phase_results(cfg, results, self.out)
                if cfg.svc_elapsed:
                    for hostport, us in getattr(self.runner, "last_service_elapsed", []):
                        from elbencho_amd.units import elapsed_ms_to_human
                        print(f"{'':<11} {'Svc ' + hostport:<17}: "
                              f"{elapsed_ms_to_human(us // 1000):>11}", file=self.out)

        if cfg.csv_file and (self.dist is None or self.dist.rank == 0):
            append_csv_result(cfg, results, cfg.csv_file)
        if cfg.json_file and (self.dist is None or self.dist.rank == 0):
            append_json_result(cfg, results, cfg.json_file)
        if cfg.res_file and (self.dist is None or self.dist.rank == 0):
            with open(cfg.res_file, "a") as f:
                print_phase_results(cfg, results, f)

        # sub-microsecond phases usually mean a mis-configured benchmark
        # (reference --no0usecerr contract)
        did_work = results.bytes or results.entries or results.iops
        if (did_work and results.last_finish_usec == 0
                and not cfg.ignore_0usec_errors and name not in ("SYNC", "DROPCACHES")):
            print(f"ERROR: phase {display} completed in less than a microsecond — "
                  "the configuration likely measures nothing "
                  "(--no0usecerr to ignore)", file=sys.stderr)
            return False

        interrupted_only = all(e.endswith("interrupted") for e in results.errors)
        if results.errors and not (self.interrupted and interrupted_only):
            return False
        return True
