#!/usr/bin/env python3
"""S3 data-plane throughput proof.

Starts the native threaded S3 bench endpoint (csrc/s3srv.h — synthetic
object bodies, no Python in the data path) and drives the full S3 engine
through the CLI: multipart PUT then ranged GET, optionally with the GPU
verify path on. Prints one summary line per phase.

Usage: s3_dataplane_bench.py [--threads N] [--objsize S] [--block B]
                             [--objects K] [--gpu] [--verify SALT]
                             [--chksumalgo ALGO]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from elbencho_amd import load_core  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--objsize", default="64m")
    ap.add_argument("--block", default="8m")
    ap.add_argument("--objects", type=int, default=4)  # per thread
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--verify", type=int, default=-1)
    ap.add_argument("--iodepth", type=int, default=1)
    ap.add_argument("--chksumalgo", default="",
                    help="--s3chksumalgo for the run (CRC32/CRC32C/CRC64NVME keep "
                         "the native plane; SHA1/SHA256 take the Python path)")
    args = ap.parse_args()

    core = load_core()
    srv = core.S3BenchServer(0, args.verify)
    port = srv.port()

    from elbencho_amd.cli import main as cli_main

    base = ["--s3endpoints", f"http://127.0.0.1:{port}", "--s3key", "k",
            "--s3secret", "s", "--nolive",
            "-t", str(args.threads), "-N", str(args.objects),
            "-s", args.objsize, "-b", args.block,
            "--iodepth", str(args.iodepth)]
    if args.gpu:
        base += ["--gpuids", "0"]
    if args.verify >= 0:
        base += ["--verify", str(args.verify)]
    if args.chksumalgo:
        base += ["--s3chksumalgo", args.chksumalgo]

    with tempfile.TemporaryDirectory() as td:
        jsonf = os.path.join(td, "res.json")
        rc = cli_main(base + ["-w", "-r", "--jsonfile", jsonf, "s3://dpbench"])
        if rc != 0:
            print("CLI failed", file=sys.stderr)
            return rc
        with open(jsonf) as f:
            for ln in f:
                d = json.loads(ln)
                bytes_total = d["last_done"]["bytes"]
                el_ms = d["last_done"]["elapsed_time_ms"] or 1
                gibs = bytes_total / (el_ms / 1e3) / 1024**3
                print(f"S3 {d['phase_type']}: {gibs:.2f} GiB/s "
                      f"({bytes_total / 1024**2:.0f} MiB in {el_ms:.0f} ms, "
                      f"t={args.threads} obj={args.objsize} blk={args.block} "
                      f"qd={args.iodepth} gpu={args.gpu} "
                      f"verify={args.verify} "
                      f"chksum={args.chksumalgo or '-'})", flush=True)
    srv.stop()
    return 0


if __name__ == "__main__":
    sys.exit(main())
