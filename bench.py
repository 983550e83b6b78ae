#!/usr/bin/env python3
"""Flagship benchmark step for the driver contract.

Measures the headline metric of BASELINE.json: sequential-read GiB/s into
GPU HBM (config: "Large-file seq read, 16 threads, 4 MiB blocks, --gpuids N
hipMemcpyAsync into HBM on MI355X") on synthetic files on tmpfs.

One "step" = one full sequential READ pass of this rank's dataset into the
rank's GPU HBM through the native engine (16 C++ I/O threads, pinned host
buffers, hipMemcpyAsync staging on per-thread streams). Multi-GPU runs are
launched by the driver as one rank per GPU via torch.distributed.run; ranks
sync with RCCL barriers around the timed region and the slowest rank's time
is used (MAX all-reduce).

A plain run does only what the headline figure needs: setup, warmup, the
timed steps, the optional --dump-outputs files and the result line.
Anything measured beyond that belongs behind --full (off by default; at
present every figure in the result line comes out of the timed steps
themselves, so --full adds nothing yet).

Usage: python bench.py [--gpus N] [--steps K] [--warmup W]
                       [--dump-outputs DIR] [--full]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BASELINE_GIBS = 11.0  # reference's best recorded seq write: 94.46 Gbps ~= 11.0 GiB/s
                      # (BASELINE.md, 8x NVMe RAID-0 testbed, other hardware)


def node_cores(node: int, cpulist_path: str | None = None) -> list[int]:
    """CPUs of a NUMA node, parsed from kernel cpulist syntax ("0-3,8")."""
    path = cpulist_path or f"/sys/devices/system/node/node{node}/cpulist"
    try:
        with open(path) as f:
            spec = f.read().strip()
    except OSError:
        return []
    out: list[int] = []
    for part in spec.split(","):
        if "-" in part:
            lo, hi = part.split("-")
            out.extend(range(int(lo), int(hi) + 1))
        elif part:
            out.append(int(part))
    return out


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--threads", type=int, default=int(os.environ.get("EB_BENCH_THREADS", "16")))
    p.add_argument("--block", type=int,
                   default=int(os.environ.get("EB_BENCH_BLOCK", str(4 * 1024 * 1024))))
    p.add_argument("--filesize", type=int,
                   default=int(os.environ.get("EB_BENCH_FILESIZE", str(8 * 1024 ** 3))))
    p.add_argument("--dir", default=os.environ.get("EB_BENCH_DIR", "/dev/shm/elbencho_amd_bench"))
    p.add_argument("--workload", default="seqread", choices=["seqread", "seqwrite", "randread"])
    p.add_argument("--iodepth", type=int, default=int(os.environ.get("EB_BENCH_IODEPTH", "1")))
    # p99 into-HBM latency from hipEvent pairs on the zero-copy fast path
    # (part of the BASELINE metric); EB_BENCH_LAT=0 disables
    p.add_argument("--lat", type=int, default=int(os.environ.get("EB_BENCH_LAT", "1")))
    # on-GPU data verification in the timed path: the setup write lays down
    # the checksum pattern (gfx950 fill kernel) and every measured read is
    # verified in HBM (gfx950 verify kernel, 64-block batched). Costs ~0 at
    # staging rates (verify kernel runs at multi-TB/s; see profiles/).
    p.add_argument("--verify", type=int,
                   default=int(os.environ.get("EB_BENCH_VERIFY", "1")))
    # what the last timed step delivered, as DIR/<name>.npy (see dump_outputs)
    p.add_argument("--dump-outputs", metavar="DIR", default=None)
    # measurements beyond the headline figure (none yet: latency percentiles
    # and on-GPU verify are taken inside the timed steps, not in extra runs)
    p.add_argument("--full", action="store_true")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be >= 1")
    if args.warmup < 0:
        p.error("--warmup must be >= 0")
    return args


DUMP_SAMPLE_CHUNKS = 256     # x DUMP_SAMPLE_CHUNK bytes = 1 MiB of data,
DUMP_SAMPLE_CHUNK = 4096     # 4 MiB as float32 (well under the 64 MB cap)
DUMP_SAMPLE_SEED = 20240607


def dump_outputs(out_dir: str, path: str, file_size: int, last_res) -> None:
    """Write what the last timed step delivered, one float .npy per array.

    pass_totals.npy  float64 [entries, bytes, iops, workers_with_error]:
                     the per-worker results finish_phase() returned for the
                     last timed pass, summed over this rank's workers (the
                     split between workers varies with dynamic slicing, the
                     sums do not; latencies are timing, so they stay out).
    data_sample.npy  float32 [chunks, chunk_bytes]: the dataset bytes the
                     pass moved (for reads: what it read and verified in
                     HBM; for seqwrite: what it wrote), taken at fixed,
                     seeded 4 KiB-aligned offsets. The first and the last
                     chunk of the file are always included.
    sample_offsets.npy float64 [chunks]: file offset of each sampled chunk.
    """
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    totals = np.array([
        sum(r["entries"] for r in last_res),
        sum(r["bytes"] for r in last_res),
        sum(r["iops"] for r in last_res),
        sum(1 for r in last_res if r["error"]),
    ], dtype=np.float64)
    np.save(os.path.join(out_dir, "pass_totals.npy"), totals)

    n_chunks = max(file_size // DUMP_SAMPLE_CHUNK, 1)
    rng = np.random.default_rng(DUMP_SAMPLE_SEED)
    picks = rng.integers(0, n_chunks, size=DUMP_SAMPLE_CHUNKS, dtype=np.int64)
    picks[0], picks[-1] = 0, n_chunks - 1
    offsets = np.sort(picks) * DUMP_SAMPLE_CHUNK
    sample = np.zeros((len(offsets), DUMP_SAMPLE_CHUNK), dtype=np.float32)
    fd = os.open(path, os.O_RDONLY)
    try:
        for i, off in enumerate(offsets):
            buf = os.pread(fd, DUMP_SAMPLE_CHUNK, int(off))
            sample[i, :len(buf)] = np.frombuffer(buf, dtype=np.uint8)
    finally:
        os.close(fd)
    np.save(os.path.join(out_dir, "data_sample.npy"), sample)
    np.save(os.path.join(out_dir, "sample_offsets.npy"),
            offsets.astype(np.float64))


def main() -> int:
    args = parse_args()

    # Stream-pool sizing (must be set before the first GpuCtx): with
    # --dynslice both directions peak at a 4-stream staging pool
    # (reads 51.7/51.1 vs 50.2/49.3 at 8, two leases; writes 50.2 vs 49.6
    # at 3 and 47.5 at 2 — r02_streams_*.json + write sweep). Slot-ring
    # depth stays at the default 2 (52.0 vs 51.7/51.6 at 4/8).
    if args.workload in ("seqwrite", "seqread"):
        os.environ.setdefault("EB_GPU_SHARED_STREAMS", "4")

    import torch

    from elbencho_amd import load_core

    core = load_core()

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))

    use_gpu = torch.cuda.is_available()
    if use_gpu and core.gpu_device_count() < 1:
        raise RuntimeError("torch sees a GPU but the HIP engine does not — broken build")

    sync = None
    dist_rec = None
    if world > 1:
        import torch.distributed as dist

        from elbencho_amd import parallel

        pf_timeout = int(os.environ.get("EB_PREFLIGHT_TIMEOUT", "60"))
        try:
            sync = parallel.init_from_env()
            # fail fast + loud on a broken RCCL setup BEFORE any timed work:
            # barrier + all-reduce + device-map gather on a 60s-timeout group
            dist_rec = sync.preflight(timeout_s=pf_timeout)
        except Exception as e:  # noqa: BLE001 — scale data > backend choice
            # A broken RCCL must not zero the whole scale run: the sync only
            # runs OUTSIDE the timed region (barrier + tiny all-reduces), so
            # gloo over TCP measures the same thing. Rebuild the group on a
            # deterministically bumped port and record the fallback loudly.
            print(f"[bench] WARNING: {type(e).__name__} during dist init/"
                  f"preflight ({e}); retrying with gloo", file=sys.stderr,
                  flush=True)
            try:
                if dist.is_initialized():
                    dist.destroy_process_group()
            except Exception:  # noqa: BLE001
                pass
            os.environ["EB_DIST_BACKEND"] = "gloo"
            os.environ["MASTER_PORT"] = str(
                int(os.environ.get("MASTER_PORT", "29511")) + 37)
            sync = parallel.init_from_env()
            dist_rec = sync.preflight(timeout_s=pf_timeout)
            dist_rec["fallback_from_nccl"] = str(e)[:200]

    device = None
    if use_gpu:
        import torch

        dev_idx = local_rank % max(torch.cuda.device_count(), 1)
        torch.cuda.set_device(dev_idx)
        device = torch.device("cuda", dev_idx)

    # --- per-rank dataset on tmpfs ---
    os.makedirs(args.dir, exist_ok=True)
    path = os.path.join(args.dir, f"bench_r{rank}.bin")

    # clamp the per-rank file so world ranks never fill the shared tmpfs
    # (8 GiB/rank default; a small box degrades gracefully, config records
    # the actual size)
    import shutil

    free = shutil.disk_usage(args.dir).free
    budget = int(free * 0.6) // max(world, 1)
    if args.filesize > budget:
        args.filesize = max(1 << 30, budget & ~((1 << 22) - 1))
        if rank == 0:
            print(f"[bench] filesize clamped to {args.filesize} "
                  f"({free / 2**30:.1f} GiB free on {args.dir}, world {world})",
                  file=sys.stderr, flush=True)

    # NUMA placement: bind workers (and so their page-cache pages) to the
    # rank's GPU's node — keeps the H2D DMA on-socket, which matters most
    # at 8 GPUs where unbound traffic saturates the inter-socket fabric.
    # EB_BENCH_ZONES overrides ("" empty value = unbound).
    if "EB_BENCH_ZONES" in os.environ:
        zones = [int(z) for z in os.environ["EB_BENCH_ZONES"].split(",")
                 if z.strip()]
    else:
        zones = []
        if use_gpu:
            node = core.gpu_numa_node(local_rank % max(core.gpu_device_count(), 1))
            if node >= 0:
                zones = [node]

    # EB_BENCH_BIND pins each rank's workers to distinct physical cores.
    # Round 1 used a global even-index list and found it bimodal across
    # boxes (it sometimes landed on the far socket); the list is now drawn
    # from the GPU's own NUMA node cpulist (even stride skips SMT siblings).
    # Default ON for randread (+5-10% measured), OFF for seq (indifferent).
    cores: list[int] = []
    ncpu = os.cpu_count() or 0
    # default ON for randread (node-aware bind measures +5-10%: 11.0-11.4M
    # vs 10.1-10.5M IOPS zones-only, two leases); seq workloads stay
    # zone-bound only (DMA-bound, scheduler placement is fine there)
    bind_default = "1" if args.workload == "randread" else ""
    if os.environ.get("EB_BENCH_BIND", bind_default) not in ("", "0"):
        pool = node_cores(zones[0]) if zones else []
        if not pool:
            pool = list(range(0, ncpu, 2))
        # even stride over the node's cores; offset per local rank so ranks
        # sharing a node don't collide
        pool = pool[::2] or pool
        first = (local_rank * args.threads) % max(len(pool), 1)
        cores = [(pool[(first + i) % len(pool)]) for i in range(args.threads)] \
            if pool else []

    # --verify: dataset carries the checksum pattern (gfx950 fill kernel at
    # setup), measured reads are verified in HBM (gfx950 verify kernel).
    # randread keeps verify off: it forces the per-block checked path off
    # the batched half-ring staging (9.9M -> ~5M IOPS).
    verify_salt = 7 if (args.verify and args.workload != "randread") else -1


    base_cfg = dict(
        path_type="file",
        threads=args.threads,
        num_dataset_threads=args.threads,  # each rank owns its file entirely
        rank_offset=0,
        file_size=args.filesize,
        block_size=args.block,
        iodepth=args.iodepth,
        lat=False,
        verify_salt=verify_salt,
        blockvar_pct=0,  # setup fill is random already; steps measure I/O, not RNG
        bench_seed=0x9E3779B97F4A7C15 ^ rank,
        cores=cores,
        zones=zones,
    )

    # setup: create the synthetic file (not timed)
    wcfg = dict(base_cfg, paths=[path])
    weng = core.Engine(wcfg)
    weng.prepare()

    last_res = []  # per-worker results of the most recent pass

    def run_pass(eng, phase, lat_hist=None):
        eng.start_phase(core.PHASES[phase])
        eng.wait_phase_done(-1)
        res = eng.finish_phase()
        last_res[:] = res
        errs = [r["error"] for r in res if r["error"]]
        if errs:
            raise RuntimeError(f"bench phase failed: {errs}")
        if lat_hist is not None:
            for r in res:
                lat_hist.merge(r["io_lat"])
        return sum(r["bytes"] for r in res)

    run_pass(weng, "WRITE")
    assert os.path.getsize(path) == args.filesize

    # measured engine: GPU-staged when a GPU is present. dynamic_slice pulls
    # blocks from one shared cursor so the pass ends when the work is gone,
    # not when the slowest static slice finishes (EB_BENCH_DYN=0 for A/B)
    measure_lat = bool(args.lat)
    use_dyn = os.environ.get("EB_BENCH_DYN", "1") != "0"
    mcfg = dict(base_cfg, paths=[path], lat=measure_lat, dynamic_slice=use_dyn)
    use_mmap = os.environ.get("EB_BENCH_MMAP", "1") != "0"
    if use_gpu:
        mcfg["gpu_ids"] = [local_rank % max(core.gpu_device_count(), 1)]
        # zero-copy: file pages pinned, each block is one hipMemcpyAsync
        # between the page cache and HBM (fastest seq path; see profiles/)
        if use_mmap and args.workload in ("seqread", "seqwrite"):
            mcfg["mmap"] = True
    if args.workload == "randread":
        mcfg["random"] = True
        mcfg["block_size"] = 4096
        args.block = 4096
    meng = core.Engine(mcfg)
    meng.prepare()

    phase = "WRITE" if args.workload == "seqwrite" else "READ"

    # --- warmup ---
    for _ in range(args.warmup):
        run_pass(meng, phase)

    # --- timed steps, barrier + device sync on both sides ---
    if sync:
        sync.barrier()
    if use_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()

    from elbencho_amd.histogram import Histogram

    lat_hist = Histogram() if measure_lat else None
    bytes_done = 0
    for _ in range(args.steps):
        bytes_done += run_pass(meng, phase, lat_hist)

    if use_gpu:
        torch.cuda.synchronize()
    if sync:
        sync.barrier()
    t1 = time.perf_counter()

    elapsed = t1 - t0
    if sync:  # slowest rank defines the job time
        elapsed = sync.allreduce_max([elapsed])[0]
        total_bytes = sync.allreduce_sum([float(bytes_done)])[0]
        if lat_hist is not None:  # merge histograms across ranks
            s = sync.allreduce_sum(
                [float(lat_hist.vec[0]), float(lat_hist.vec[1])] +
                [float(x) for x in lat_hist.vec[4:]])
            mn = -sync.allreduce_max([float(-lat_hist.vec[2])])[0]
            mx = sync.allreduce_max([float(lat_hist.vec[3])])[0]
            lat_hist.vec = ([int(s[0]), int(s[1]), int(mn), int(mx)] +
                            [int(x) for x in s[2:]])
    else:
        total_bytes = float(bytes_done)

    value = total_bytes / elapsed / (1024 ** 3)  # whole-job GiB/s
    ms_per_step = elapsed * 1000.0 / args.steps

    if rank == 0:
        metric_by_workload = {
            "seqread": "seq-read GiB/s into GPU HBM",
            "seqwrite": "seq-write GiB/s from GPU HBM",
            "randread": "4K-random-read GiB/s into GPU HBM",
        }
        doc = {
            "metric": metric_by_workload[args.workload],
            "value": round(value, 3),
            "unit": "GiB/s",
            "n_gpus": world if use_gpu else 0,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": round(value / BASELINE_GIBS, 3),
            "dtype": "raw-bytes",
            "data": "synthetic (tmpfs files, random fill)",
            "config": {
                "model": "storage-benchmark seq-read into HBM",
                "workload": args.workload,
                "threads_per_gpu": args.threads,
                "block_size": args.block,
                "file_size_per_rank": args.filesize,
                "iodepth": args.iodepth,
                "bench_dir": args.dir,
                "gpu_staged": use_gpu,
                "mmap_zero_copy": bool(use_gpu and use_mmap
                                       and args.workload != "randread"),
                "dynamic_slice": bool(use_dyn and use_gpu and use_mmap
                                      and args.workload != "randread"),
                "verify_on_gpu": bool(verify_salt >= 0 and use_gpu),
                "verify_salt": verify_salt if verify_salt >= 0 else None,
                "parallelism": f"dp{world}" if world > 1 else "single",
            },
        }
        if use_gpu:  # provenance: helps interpret box-to-box variance
            dev0 = local_rank % max(core.gpu_device_count(), 1)
            doc["config"]["device"] = core.gpu_device_name(dev0)
            doc["config"]["device_numa_node"] = core.gpu_numa_node(dev0)
        if dist_rec:
            doc["config"]["dist"] = dist_rec
        if lat_hist is not None and lat_hist.num_values:
            # per-block into-HBM latency (hipEvent pairs around each staging
            # copy on the zero-copy path; wall time per op elsewhere)
            doc["config"]["block_lat_usec"] = {
                "p50": lat_hist.percentile(50),
                "p99": lat_hist.percentile(99),
                "p999": lat_hist.percentile(99.9),
                "avg": round(lat_hist.avg_us, 1),
                "min": lat_hist.min_us,
                "max": lat_hist.max_us,
                "n_blocks": lat_hist.num_values,
            }
        if args.workload == "randread":
            doc["config"]["iops_4k"] = int(total_bytes / 4096 / elapsed)
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, path, args.filesize, last_res)
        print(json.dumps(doc), flush=True)

    # cleanup (tmpfs is shared RAM — do not leak multi-GiB files)
    try:
        os.unlink(path)
    except OSError:
        pass

    if sync:
        import torch.distributed as dist

        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
