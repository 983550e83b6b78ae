"""RCCL-over-xGMI phase synchronization for multi-GPU lockstep runs.

This replaces the reference's master-polls-services statistics loop for
intra-node GPU workers: a torch.distributed barrier
gives lockstep phase starts across the node's 8 MI355X GPUs, and the
LiveOps counters + latency histogram buckets are aggregated with a single
all-reduce per phase end. The payloads are tiny (a few KB), so latency —
not xGMI link bandwidth — dominates; we batch everything into one SUM
all-reduce plus one MIN/MAX pair.

Backend: "nccl" (= RCCL on ROCm) with device tensors on GPU ranks, "gloo"
with CPU tensors in CPU tests. Collectives run only at phase boundaries,
never inside the measured I/O loop (SURVEY.md §7 hard part (f)).
"""

from __future__ import annotations

import datetime
import os
import sys
import time
from typing import Optional

import torch
import torch.distributed as dist

from elbencho_amd.dataprofile import HLL_M, DataProfile
from elbencho_amd.stats import PhaseResults


def init_from_env(device: Optional[torch.device] = None) -> "PhaseSync | None":
    """Initialize torch.distributed from torchrun env vars; None if absent.

    Hardened for the first real multi-GPU run:
    - the resolved backend is always printed to stderr (a gloo fallback on a
      GPU box is visible, never silent);
    - NCCL/RCCL collectives abort-and-raise on the process-group timeout
      instead of hanging (TORCH_NCCL_ASYNC_ERROR_HANDLING);
    - EADDRINUSE on the rendezvous port (TIME_WAIT from a previous run) is
      retried — all ranks retry the SAME port so agreement is preserved.
    """
    if "RANK" not in os.environ or "WORLD_SIZE" not in os.environ:
        return None
    if not dist.is_initialized():
        # RCCL refuses two ranks on one device ("Duplicate GPU detected"):
        # when the job is oversubscribed (more ranks than GPUs), coordinate
        # over gloo instead — the I/O staging itself still uses the GPUs
        world = int(os.environ.get("WORLD_SIZE", "1"))
        n_gpus = torch.cuda.device_count() if torch.cuda.is_available() else 0
        usable_nccl = n_gpus > 0 and world <= n_gpus
        backend = os.environ.get("EB_DIST_BACKEND",
                                 "nccl" if usable_nccl else "gloo")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        # watchdog aborts + raises instead of silent hang (1 = TearDown)
        os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "1")
        timeout = datetime.timedelta(
            seconds=int(os.environ.get("EB_DIST_TIMEOUT", "600")))
        last_err: Exception | None = None
        for attempt in range(int(os.environ.get("EB_DIST_INIT_RETRIES", "4"))):
            try:
                dist.init_process_group(backend=backend, timeout=timeout)
                last_err = None
                break
            except (RuntimeError, OSError) as e:  # EADDRINUSE / stale store
                last_err = e
                if "EADDRINUSE" not in str(e) and "address already in use" \
                        not in str(e).lower():
                    raise
                import time as _time
                _time.sleep(3.0 * (attempt + 1))
        if last_err is not None:
            raise last_err
        if backend == "gloo" and n_gpus > 0 and "EB_DIST_BACKEND" not in os.environ:
            print(f"[elbencho_amd] dist backend: gloo FALLBACK "
                  f"({world} ranks > {n_gpus} visible GPUs)",
                  file=sys.stderr, flush=True)
        else:
            print(f"[elbencho_amd] dist backend: {backend} "
                  f"(rank {dist.get_rank()}/{world}, {n_gpus} visible GPUs)",
                  file=sys.stderr, flush=True)
    if device is None and torch.cuda.is_available() and dist.get_backend() == "nccl":
        local_rank = int(os.environ.get("LOCAL_RANK", dist.get_rank()))
        local_rank %= max(torch.cuda.device_count(), 1)
        torch.cuda.set_device(local_rank)
        device = torch.device("cuda", local_rank)
    return PhaseSync(device)


class PhaseSync:
    """Barrier + stats aggregation over an initialized process group."""

    def __init__(self, device: Optional[torch.device] = None):
        if not dist.is_initialized():
            raise RuntimeError("torch.distributed is not initialized")
        self.rank = dist.get_rank()
        self.world_size = dist.get_world_size()
        if device is None:
            device = (torch.device("cuda", torch.cuda.current_device())
                      if dist.get_backend() == "nccl" else torch.device("cpu"))
        self.device = device

    # ------------------------------------------------------------------
    def preflight(self, timeout_s: int = 60) -> dict:
        """Collective self-test before any timed region.

        Runs a barrier + tiny all-reduce + all-gather of the device mapping
        on a SHORT-TIMEOUT subgroup so a broken RCCL setup fails loudly
        within timeout_s instead of stalling the scale bench. Returns a
        record for the bench JSON: backend, per-rank device, elapsed ms.
        """
        t0 = time.perf_counter()
        pg = dist.new_group(ranks=list(range(self.world_size)),
                            timeout=datetime.timedelta(seconds=timeout_s))
        try:
            if dist.get_backend() == "nccl":
                dist.barrier(group=pg, device_ids=[self.device.index])
            else:
                dist.barrier(group=pg)
            t = torch.ones(8, dtype=torch.float64, device=self.device)
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=pg)
            got = t[0].item()
            if got != float(self.world_size):
                raise RuntimeError(
                    f"preflight all-reduce mismatch: got {got}, "
                    f"expected {self.world_size}")
            dev_name = str(self.device)
            if self.device.type == "cuda":
                dev_name += f":{torch.cuda.get_device_name(self.device.index)}"
            devices = [None] * self.world_size
            dist.all_gather_object(devices, dev_name, group=pg)
        finally:
            dist.destroy_process_group(pg)
        elapsed_ms = (time.perf_counter() - t0) * 1000.0
        rec = {
            "backend": dist.get_backend(),
            "world_size": self.world_size,
            "devices": devices,
            "preflight_ms": round(elapsed_ms, 1),
        }
        if self.rank == 0:
            print(f"[elbencho_amd] preflight OK: backend={rec['backend']} "
                  f"world={self.world_size} {elapsed_ms:.0f} ms",
                  file=sys.stderr, flush=True)
        return rec

    # ------------------------------------------------------------------
    def barrier(self) -> None:
        """Lockstep phase start across ranks (replaces /startphase round-trip)."""
        if dist.get_backend() == "nccl":
            dist.barrier(device_ids=[self.device.index])
        else:
            dist.barrier()

    # ------------------------------------------------------------------
    def allreduce_results(self, r: PhaseResults, with_profile: bool = False) -> PhaseResults:
        """Aggregate a per-rank PhaseResults into the whole-job result.

        with_profile (--dataprofile READ phases; the same on every rank): the
        profile's counters and byte histogram ride the SUM tensor and its
        sketch registers the MAX tensor. Otherwise the tensors keep their
        plain length.

        One SUM all-reduce carries counters + both histograms' buckets; one
        MIN and one MAX carry the time/min/max fields — 3 small collectives
        per phase end, off the measured I/O path.
        """
        hist_len = len(r.io_lat.vec)

        # --- SUM: counters + histogram counts/sums + bucket arrays ---
        sum_vals = [
            r.entries, r.bytes, r.iops,
            r.sw_entries, r.sw_bytes, r.sw_iops,
            r.io_lat.vec[0], r.io_lat.vec[1],
            r.entry_lat.vec[0], r.entry_lat.vec[1],
        ]
        sum_vals += r.io_lat.vec[4:]
        sum_vals += r.entry_lat.vec[4:]
        if with_profile:  # a rank without a profile (worker error) adds an empty one
            prof = r.data_profile or DataProfile()
            sum_vals += [1 if r.data_profile else 0, prof.chunks, prof.bytes,
                         prof.zero_chunks]
            sum_vals += prof.hist
        t_sum = torch.tensor(sum_vals, dtype=torch.float64, device=self.device)
        dist.all_reduce(t_sum, op=dist.ReduceOp.SUM)

        # --- MIN: first-finish elapsed + histogram mins ---
        t_min = torch.tensor(
            [r.first_finish_usec if r.first_finish_usec else 2**53,
             r.io_lat.vec[2], r.entry_lat.vec[2]],
            dtype=torch.float64, device=self.device)
        dist.all_reduce(t_min, op=dist.ReduceOp.MIN)

        # --- MAX: last-finish elapsed + histogram maxes ---
        max_vals = [r.last_finish_usec, r.io_lat.vec[3], r.entry_lat.vec[3]]
        if with_profile:
            max_vals += list(prof.regs)
        t_max = torch.tensor(max_vals, dtype=torch.float64, device=self.device)
        dist.all_reduce(t_max, op=dist.ReduceOp.MAX)

        s = [int(x) for x in t_sum.tolist()]
        mn = [int(x) for x in t_min.tolist()]
        mx = [int(x) for x in t_max.tolist()]

        out = PhaseResults(phase_name=r.phase_name, phase_id=r.phase_id,
                           start_time=r.start_time)
        out.entries, out.bytes, out.iops = s[0], s[1], s[2]
        out.sw_entries, out.sw_bytes, out.sw_iops = s[3], s[4], s[5]
        out.first_finish_usec = mn[0] if mn[0] < 2**53 else 0
        out.last_finish_usec = mx[0]
        out.cpu_first, out.cpu_last = r.cpu_first, r.cpu_last

        nb = hist_len - 4
        out.io_lat.vec = [s[6], s[7], mn[1], mx[1]] + s[10:10 + nb]
        out.entry_lat.vec = [s[8], s[9], mn[2], mx[2]] + s[10 + nb:10 + 2 * nb]
        out.errors = list(r.errors)
        out.worker_elapsed_usec = list(r.worker_elapsed_usec)
        if with_profile:
            p0 = 10 + 2 * nb
            if s[p0] == self.world_size:  # every rank finished its part
                out.data_profile = DataProfile(
                    chunks=s[p0 + 1], bytes=s[p0 + 2], zero_chunks=s[p0 + 3],
                    hist=s[p0 + 4:p0 + 4 + 256], regs=bytes(mx[3:3 + HLL_M]))
        return out

    # ------------------------------------------------------------------
    def allreduce_sum(self, values: list[float]) -> list[float]:
        t = torch.tensor(values, dtype=torch.float64, device=self.device)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return t.tolist()

    def allreduce_max(self, values: list[float]) -> list[float]:
        t = torch.tensor(values, dtype=torch.float64, device=self.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return t.tolist()

    def broadcast_obj(self, obj, src: int = 0):
        lst = [obj]
        dist.broadcast_object_list(lst, src=src)
        return lst[0]
