"""Runs a few cases of tests/shared_streams_cases.py in a process of its own:
`python -m tests.shared_streams_child` with EB_GPU_SHARED_STREAMS set by the
caller (tests/test_gpu_shared_streams.py). The pool size is read once per
process, so other sizes than the default cannot be reached from the process
that runs the suite.

Prints one JSON line: {"pool": the variable's value, "seconds": ..., "cases":
{name: {"verdict": "ok" or the failure, "streams": the case's
Engine.gpu_streams()}}}. Exit status 0 when every verdict is "ok", 1 when not,
2 without a HIP device (it does not fall back to the CPU paths).

Not a test module: nothing here is collected.
"""

import json
import os
import pathlib
import sys
import tempfile
import time

CASES = ["write_pipelined_checksum", "write_pipelined_bv37strong", "read_sync_batched_4k",
         "read_mmap", "verify_pipelined_one_slice"]


def run_case(core, name, tmp, pool):
    from tests import shared_streams_cases as c
    from tests.test_gpu_engine_exact import FILLS

    if name == "write_pipelined_checksum":
        return c.check_write(core, tmp, None, None, "pipelined", FILLS[0], c.BS256K, 5,
                             c.WORKERS, pool=pool)
    if name == "write_pipelined_bv37strong":
        return c.check_write(core, tmp, None, None, "pipelined", FILLS[4], c.BS256K, 5,
                             c.WORKERS, pool=pool)
    if name == "read_sync_batched_4k":
        return c.check_read(core, tmp, None, None, "sync_batched_4k", pool=pool)
    if name == "read_mmap":
        return c.check_read(core, tmp, None, None, "mmap", pool=pool)
    if name == "verify_pipelined_one_slice":
        return c.check_verify(core, tmp, None, None, "pipelined", False, pool=pool)
    raise AssertionError(name)


def main() -> int:
    from elbencho_amd import load_core

    core = load_core()
    if core.gpu_device_count() < 1:
        print("shared_streams_child: no HIP device available (" + core.gpu_probe_error() +
              "); the cases need a GPU and do not fall back to the CPU", file=sys.stderr)
        return 2

    value = os.environ.get("EB_GPU_SHARED_STREAMS", "")
    pool = int(value) if value else 8
    out = {"pool": value, "cases": {}}
    t0 = time.monotonic()
    with tempfile.TemporaryDirectory() as top:
        for name in CASES:
            tmp = pathlib.Path(top) / name
            tmp.mkdir()
            try:
                streams = run_case(core, name, tmp, pool)
                out["cases"][name] = {"verdict": "ok", "streams": streams}
            except BaseException as e:  # pytest.fail raises outside Exception
                if isinstance(e, (KeyboardInterrupt, SystemExit)):
                    raise
                out["cases"][name] = {"verdict": f"{type(e).__name__}: {e}", "streams": []}
    out["seconds"] = round(time.monotonic() - t0, 2)
    print(json.dumps(out), flush=True)
    return 0 if all(v["verdict"] == "ok" for v in out["cases"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
