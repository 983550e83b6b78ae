"""Benchmark configuration — the ProgArgs equivalent.

Holds the full option surface (CLI names match the reference elbencho,
/root/reference/docs/usage/help-all.md), performs unit parsing, bracket
expansion of paths, path-type inference, cross-option validation, and
serializes to/from a JSON-able dict for master->service transfer (the
config system IS the wire schema, like reference ProgArgs.cpp:3921/:3754).
Independent implementation.
"""

from __future__ import annotations

import dataclasses
import os
import re
import stat as statmod
from dataclasses import dataclass, field
from typing import Any

from elbencho_amd.units import parse_size

# benchmark path type
PATH_DIR = "dir"
PATH_FILE = "file"
PATH_BDEV = "bdev"

S3_PATH_PREFIX = "s3://"


class ConfigError(ValueError):
    pass


def expand_path_brackets(path: str) -> list[str]:
    """Expand "name[1-4]" / "name[3,5]" style patterns (one bracket pair),
    mirroring the reference's path expansion (ProgArgs.cpp:1805)."""
    m = re.search(r"\[([0-9,\-]+)\]", path)
    if not m:
        return [path]
    nums: list[int] = []
    for part in m.group(1).split(","):
        if "-" in part:
            lo, hi = part.split("-", 1)
            nums.extend(range(int(lo), int(hi) + 1))
        else:
            nums.append(int(part))
    pre, post = path[: m.start()], path[m.end() :]
    out = []
    for n in nums:
        out.extend(expand_path_brackets(f"{pre}{n}{post}"))
    return out


def expand_hosts(hosts: list[str]) -> list[str]:
    """Expand host lists with port ranges: "localhost:[1711-1712]"."""
    out = []
    for h in hosts:
        out.extend(expand_path_brackets(h))
    return out


@dataclass
class BenchConfig:
    # --- paths & mode ---
    paths: list[str] = field(default_factory=list)
    path_type: str = PATH_FILE  # dir|file|bdev (auto-inferred)
    bench_mode: str = "posix"  # posix|s3|hdfs|netbench
    hdfs: bool = False             # --hdfs (WebHDFS REST engine)

    # --- phases ---
    run_mkdirs: bool = False       # -d/--mkdirs
    run_write: bool = False        # -w/--write
    run_read: bool = False         # -r/--read
    run_stat: bool = False         # --stat
    run_delfiles: bool = False     # -F/--delfiles
    run_deldirs: bool = False      # -D/--deldirs
    run_sync: bool = False         # --sync
    run_dropcaches: bool = False   # --dropcache
    run_statdirs: bool = False     # --statdirs (s3)

    # --- workload shape ---
    threads: int = 1               # -t
    dirs: int = 0                  # -n (per thread)
    files: int = 0                 # -N (per dir per thread)
    file_size: int = 0             # -s
    block_size: int = 1 << 20      # -b
    iodepth: int = 1               # --iodepth
    iterations: int = 1            # -i
    inf_loop: bool = False         # --infloop
    dyn_slice: bool = False        # --dynslice (MI355X extension)

    # --- access pattern ---
    direct: bool = False           # --direct
    random: bool = False           # --rand
    rand_aligned: bool = True      # (--norandalign clears)
    rand_amount: int = 0           # --randamount (total across workers; 0=dataset)
    rand_algo: str = "balanced_single"  # --randalgo
    strided: bool = False          # --strided
    backward: bool = False         # --backward
    truncate: bool = False         # --trunc
    trunc_to_size: bool = False    # --trunctosize
    prealloc: bool = False         # --preallocfile
    sharesize: int = 0             # --sharesize (custom tree)

    # --- integrity / variance ---
    verify: int = -1               # --verify SALT (-1 off)
    verify_mix_pct: int = -1       # --verifymixpct (-1 = plain --verify pattern)
    verify_diag: bool = False      # --verifydiag (classify verify mismatches)
    verify_direct: bool = False    # --verifydirect
    read_inline: bool = False      # --readinline
    stat_inline: bool = False      # --statinline
    mmap: bool = False             # --mmap
    fadv: str = ""                 # --fadv (csv: seq,rand,willneed,dontneed,noreuse)
    madv: str = ""                 # --madv (csv: seq,rand,willneed,dontneed,hugepage)
    flock_mode: str = ""           # --flock ("range"|"full")
    blockvar_pct: int = 100        # --blockvarpct
    blockvar_algo: str = "fast"    # --blockvaralgo
    dedupe_pct: int = 0            # --dedupepct (percent of chunks from the shared pool)
    compress_pct: int = 0          # --compresspct (percent of each chunk that is zero)
    dedupe_chunk: int = 4096       # --dedupechunk (chunk size of the two above)
    dedupe_verify: int = -1        # --dedupeverify SALT (position-keyed, checked on read)
    data_profile: bool = False     # --dataprofile (dedupe/entropy profile of read data)

    # --- GPU ---
    gpu_ids: list[int] = field(default_factory=list)  # --gpuids
    gpu_per_service: bool = False  # --gpuperservice
    gpu_direct: bool = False       # --gds analogue: O_DIRECT + pinned staging
    gpu_pinned: bool = True        # (--cuhostbufreg analogue; pinned host bufs)

    # --- latency / stats / output ---
    lat: bool = False              # --lat
    lat_histo: bool = False        # --lathisto
    lat_percent: bool = False      # --latpercent
    lat_percent_9s: int = 0        # --latpercent9s
    all_elapsed: bool = False      # --allelapsed
    cpu_util: bool = False         # --cpu
    live_int_ms: int = 2000        # --liveint
    no_live: bool = False          # --nolive
    live1: bool = False            # --live1
    live1n: bool = False           # --live1n
    live_csv: str = ""             # --livecsv
    live_csv_ex: bool = False      # --livecsvex
    csv_file: str = ""             # --csvfile
    json_file: str = ""            # --jsonfile
    res_file: str = ""             # --resfile
    no_csv_labels: bool = False    # --nocsvlabels
    label: str = ""                # --label
    show_dir_stats: bool = False   # --dirstats
    show_base10: bool = False      # --base10 (MB/s instead of MiB/s in output)
    log_level: int = 0             # --log
    ops_log_path: str = ""         # --opslog
    ops_log_lock: bool = False     # --opsloglock

    # --- limits / timing ---
    timelimit: int = 0             # --timelimit (secs per phase)
    limit_read: int = 0            # --limitread (bytes/s per thread)
    limit_write: int = 0           # --limitwrite
    phase_delay_secs: int = 0      # --phasedelay
    start_time: int = 0            # --start (epoch secs)

    # --- error handling / checks ---
    ignore_del_errors: bool = False  # --nodelerr
    ignore_0usec_errors: bool = False  # --no0usecerr
    no_dio_check: bool = False     # --nodiocheck
    no_path_expansion: bool = False  # --nopathexp
    dryrun: bool = False           # --dryrun

    # --- placement ---
    numa_zones: str = ""           # --zones
    cpu_cores: str = ""            # --cores

    # --- distributed ---
    hosts: list[str] = field(default_factory=list)  # --hosts
    service_mode: bool = False     # --service
    service_port: int = 1611       # --port
    foreground: bool = False       # --foreground / --nodetach
    alt_http_svc: bool = False     # --althttpsvc (single-threaded HTTP server)
    no_svc_share: bool = False     # --nosvcshare
    num_hosts: int = -1            # --numhosts
    rotate_hosts: int = 0          # --rotatehosts
    svc_update_int_ms: int = 500   # --svcupint
    svc_elapsed: bool = False      # --svcelapsed
    svc_pw_file: str = ""          # --svcpwfile
    svc_wait: bool = False         # --svcwait
    svc_ping: bool = False         # --svcping (service RTT in the dashboard)
    interrupt_services: bool = False  # --interrupt
    quit_services: bool = False    # --quit
    rank_offset: int = 0           # --rankoffset
    dir_sharing: bool = False      # --dirsharing
    # --nofdsharing: accepted for CLI compatibility; this engine always opens
    # per-thread fds (the reference's non-shared mode) — pread/pwrite carry
    # the offset, so fd sharing is only an open()-count optimization there
    no_fd_sharing: bool = False

    # --- custom tree ---
    treefile: str = ""             # --treefile
    tree_round_up: int = 0         # --treeroundup
    tree_scan: str = ""            # --treescan
    tree_rand: bool = False        # --treerand
    tree_round_robin: bool = False  # --treeroundrob (shared blocks round-robin)

    # --- rwmix ---
    rwmix_pct: int = 0             # --rwmixpct
    rwmix_threads: int = 0         # --rwmixthr
    rwmix_thread_pct: int = 0      # --rwmixthrpct

    # --- netbench ---
    netbench: bool = False         # --netbench
    servers: list[str] = field(default_factory=list)  # --servers
    num_servers: int = 0           # --numservers (limit servers list; 0 = all)
    resp_size: int = 1             # --respsize
    send_buf: int = 0              # --sendbuf
    recv_buf: int = 0              # --recvbuf
    netdevs: list[str] = field(default_factory=list)  # --netdevs

    # --- S3 ---
    s3_endpoints: list[str] = field(default_factory=list)  # --s3endpoints
    s3_key: str = ""               # --s3key
    s3_secret: str = ""            # --s3secret
    s3_region: str = ""            # --s3region
    s3_no_compress: bool = False
    s3_fastget: bool = False
    s3_fastput: bool = False
    s3_list_obj: int = 0           # --s3listobj
    s3_list_verify: bool = False   # --s3listverify
    s3_multi_del: int = 0          # --s3multidel
    s3_rand_obj: bool = False      # --s3randobj
    s3_obj_prefix: str = ""        # --s3objprefix
    s3_sign_policy: int = 0        # --s3sign
    s3_max_conns: int = 0          # --s3maxconns
    s3_ignore_errors: bool = False
    s3_acl_put: bool = False       # --s3aclput
    s3_acl_get: bool = False       # --s3aclget
    s3_acl_verify: bool = False    # --s3aclverify
    s3_acl_grants: str = ""        # --s3aclgrants (canned ACL string)
    s3_bacl_put: bool = False      # --s3baclput
    s3_bacl_get: bool = False      # --s3baclget
    s3_otag: bool = False          # --s3otag
    s3_otag_verify: bool = False   # --s3otagverify
    s3_btag: bool = False          # --s3btag
    s3_btag_verify: bool = False   # --s3btagverify
    s3_cred_file: str = ""         # --s3credfile (lines "key:secret")
    s3_cred_list: str = ""         # --s3credlist ("key:secret,key:secret")
    s3_no_mpu_compl: bool = False  # --s3nompucompl (leave multipart uploads open)
    s3_mpu_complete: bool = False  # run the S3MPUCOMPLETE phase
    s3_bversion: bool = False      # --s3bversion
    s3_bversion_verify: bool = False  # --s3bversionverify
    s3_olock: bool = False         # --s3olockcfg
    s3_olock_verify: bool = False  # --s3olockcfgverify
    s3_list_par: bool = False      # --s3listobjpar
    s3_sse: bool = False           # --s3sse (SSE-S3 AES256 header)
    s3_sse_c_key: str = ""         # --s3sseckey (SSE-C base64 key)
    s3_sse_kms_key: str = ""       # --s3ssekmskey (SSE-KMS key id)
    s3_session_token: str = ""     # --s3sessiontoken (x-amz-security-token)
    s3_chksum_algo: str = ""       # --s3chksumalgo (CRC32|CRC32C|CRC64NVME|SHA1|SHA256)
    s3_acl_grantee: str = ""       # --s3aclgrantee (canned ACL or grantee name)
    s3_acl_gtype: str = ""         # --s3aclgtype (id|emailAddress|uri|group)
    s3_acl_put_inline: bool = False  # --s3aclputinl (ACL headers on object PUT)
    s3_mpu_sharing: bool = False   # --s3mpusharing (workers share one MPU/object)
    s3_mpu_size_var: int = 0       # --s3mpusizevar (max bytes subtracted per part)
    s3_mpu_split: int = 0          # --s3mpusplit (part size override)
    s3_no_mp_check: bool = False   # --s3nompcheck (skip 10k part-count check)
    s3_single: bool = False        # --s3single (one shared client for all workers)
    s3_target_gbps: int = 0        # --s3targetgbps (per-client throughput target)
    s3_virt_addr: bool = False     # --s3virtaddr (virtual-hosted addressing)
    s3_log: int = 0                # --s3log (client trace level, 0=off)
    s3_log_prefix: str = ""        # --s3logprefix (trace file prefix)
    # master-precreated shared-MPU uploadIds ("bucket/key" -> id), sent on
    # the wire so every service adds parts to the same upload (internal)
    s3_mpu_upload_ids: dict = field(default_factory=dict)

    # --- misc ---
    config_file: str = ""          # -c/--configfile
    bench_seed: int = 0            # internal; derived per run

    # internal derived values (not user options)
    num_dataset_threads: int = 0
    netbench_is_server: bool = False   # set per host by the master
    netbench_num_conns: int = 0        # server: expected client connections
    tree_dirs_resolved: list = field(default_factory=list)
    tree_files_resolved: list = field(default_factory=list)  # [(relpath, size)]

    # ------------------------------------------------------------------
    def finalize(self) -> None:
        """Expand paths, infer mode/path type, derive values, validate."""
        if not self.no_path_expansion:
            expanded: list[str] = []
            for p in self.paths:
                expanded.extend(expand_path_brackets(p))
            self.paths = expanded
        self.hosts = expand_hosts(self.hosts)

        if self.paths and self.paths[0].startswith(S3_PATH_PREFIX):
            self.bench_mode = "s3"
        elif self.s3_endpoints:
            self.bench_mode = "s3"
        elif self.hdfs or (self.paths and self.paths[0].startswith("hdfs://")):
            self.bench_mode = "hdfs"
        elif self.netbench:
            self.bench_mode = "netbench"

        if self.bench_mode == "posix" and self.paths:
            self.path_type = self._infer_path_type()

        # --numservers: use only the first N hosts of the netbench servers list
        if self.num_servers and self.servers:
            self.servers = self.servers[:self.num_servers]

        if self.treefile and not self.tree_scan:
            from elbencho_amd.pathstore import parse_treefile
            tree = parse_treefile(self.treefile)
            if self.tree_round_up:
                tree.round_up(self.tree_round_up)
            self.tree_dirs_resolved = tree.dirs
            self.tree_files_resolved = tree.files
            if self.path_type != PATH_DIR and self.paths:
                raise ConfigError("--treefile requires directory bench paths")

        # derived: total dataset threads across hosts sharing the dataset
        num_hosts = len(self.hosts) if self.hosts else 1
        if self.num_hosts >= 0:
            num_hosts = min(num_hosts, self.num_hosts)
        share = not self.no_svc_share or self.path_type == PATH_DIR
        if self.hosts and not self.no_svc_share and self.path_type != PATH_DIR:
            self.num_dataset_threads = self.threads * num_hosts
        elif not self.hosts:
            self.num_dataset_threads = self.threads
        else:
            self.num_dataset_threads = self.threads  # per-host private dataset
        _ = share

        self.validate()

    def _infer_path_type(self) -> str:
        types = set()
        for p in self.paths:
            try:
                st = os.stat(p)
            except FileNotFoundError:
                types.add(PATH_FILE)  # will be created
                continue
            if statmod.S_ISDIR(st.st_mode):
                types.add(PATH_DIR)
            elif statmod.S_ISBLK(st.st_mode):
                types.add(PATH_BDEV)
            else:
                types.add(PATH_FILE)
        if len(types) > 1:
            raise ConfigError(f"mixed path types are not supported: {sorted(types)}")
        return types.pop() if types else PATH_FILE

    def validate(self) -> None:
        if self.service_mode:
            return  # service gets its config from the master

        needs_paths = any([self.run_mkdirs, self.run_write, self.run_read, self.run_stat,
                           self.run_delfiles, self.run_deldirs])
        if needs_paths and not self.paths and self.bench_mode != "netbench":
            raise ConfigError("benchmark paths are required")
        if self.bench_mode == "netbench":
            if not self.hosts:
                raise ConfigError("--netbench requires service mode (--hosts)")
            if not self.servers:
                raise ConfigError("--netbench requires --servers")
        if self.bench_mode == "hdfs":
            if not self.paths or not self.paths[0].startswith("hdfs://"):
                raise ConfigError("HDFS mode requires an hdfs://namenode:port/base "
                                  "bench path (WebHDFS)")
            if (self.run_write or self.run_read) and self.files < 1:
                raise ConfigError("HDFS read/write requires -N/--files >= 1")
        if self.bench_mode == "s3":
            if not self.s3_endpoints:
                raise ConfigError("S3 mode requires --s3endpoints")
            if (self.run_write or self.run_read) and self.files < 1 \
                    and not self.s3_mpu_sharing:
                raise ConfigError("S3 object read/write requires -N/--files >= 1")
            # reference ProgArgs.cpp:1505-1515: refuse MPUs above the S3
            # 10,000-part limit unless --s3nompcheck
            part_size = self.s3_mpu_split or self.block_size
            if (self.run_write and not self.s3_no_mp_check and part_size
                    and self.file_size > part_size
                    and self.file_size / part_size > 10000):
                raise ConfigError(
                    "object size and part block size would result in a multipart "
                    "upload exceeding the S3 limit of 10,000 parts. "
                    "(--s3nompcheck disables this check.)")
            if self.s3_chksum_algo and self.s3_chksum_algo.upper() not in (
                    "CRC32", "CRC32C", "CRC64NVME", "SHA1", "SHA256"):
                raise ConfigError("--s3chksumalgo must be one of "
                                  "CRC32, CRC32C, CRC64NVME, SHA1, SHA256")

        if self.threads < 1:
            raise ConfigError("number of threads must be >= 1")
        if self.block_size < 1 and (self.run_write or self.run_read):
            raise ConfigError("block size must be >= 1")
        if self.path_type == PATH_DIR and (self.run_write or self.run_read):
            if not self.treefile and self.files < 1:
                raise ConfigError("dir mode read/write requires -N/--files >= 1")
            if self.file_size and self.block_size > self.file_size:
                self.block_size = self.file_size
        if self.path_type != PATH_DIR and (self.run_write or self.run_read):
            if not self.file_size and self.path_type == PATH_FILE and self.run_write:
                raise ConfigError("file mode write requires -s/--size")
        if self.iodepth < 1:
            raise ConfigError("iodepth must be >= 1")
        if not (0 <= self.blockvar_pct <= 100):
            raise ConfigError("blockvarpct must be in 0..100")
        if self.rwmix_pct and not (0 <= self.rwmix_pct <= 100):
            raise ConfigError("rwmixpct must be in 0..100")
        if self.direct and not self.no_dio_check and (self.run_write or self.run_read):
            if self.block_size % 512:
                raise ConfigError("direct IO requires block size aligned to 512 bytes "
                                  "(--nodiocheck to skip this check)")
            if self.file_size and self.path_type != PATH_DIR and self.file_size % 512:
                raise ConfigError("direct IO requires file size aligned to 512 bytes in "
                                  "file/bdev mode (--nodiocheck to skip this check)")
        if self.verify >= 0 and self.random and not self.rand_aligned:
            raise ConfigError("--verify cannot be used with unaligned random offsets")
        if self.dedupe_verify < -1:
            raise ConfigError("--dedupeverify needs a salt >= 0")
        if self.dedupe_verify >= 0:
            if not (self.dedupe_pct or self.compress_pct):
                raise ConfigError("--dedupeverify requires a non-zero --dedupepct or "
                                  "--compresspct")
            for other, on in (("--verify", self.verify >= 0),
                              ("--verifymixpct", self.verify_mix_pct != -1),
                              ("--verifydiag", self.verify_diag)):
                if on:
                    raise ConfigError("--dedupeverify cannot be used together with " + other)
            if self.random and not self.rand_aligned:
                raise ConfigError("--dedupeverify cannot be used with unaligned random "
                                  "offsets")
            if self.bench_mode in ("s3", "hdfs", "netbench"):
                raise ConfigError("--dedupeverify supports file, block device and "
                                  "directory paths only")
            if (self.run_write or self.run_read) and self.block_size % self.dedupe_chunk:
                raise ConfigError("--dedupeverify requires a block size that is a multiple "
                                  "of --dedupechunk")
        if self.data_profile:
            if not self.run_read:
                raise ConfigError("--dataprofile requires a read phase (-r)")
            if self.bench_mode in ("s3", "hdfs", "netbench"):
                raise ConfigError("--dataprofile supports file, block device and "
                                  "directory paths only")
            if not self.rand_aligned:
                raise ConfigError("--dataprofile cannot be used with unaligned random "
                                  "offsets (--norandalign)")
            c = self.dedupe_chunk
            if not (512 <= c <= 16 << 20) or c & (c - 1):
                raise ConfigError("--dedupechunk must be a power of two in 512..16M")
            if self.block_size % c:
                raise ConfigError("--dataprofile requires a block size that is a multiple "
                                  "of --dedupechunk")
        if self.verify_mix_pct != -1:
            if not (0 <= self.verify_mix_pct <= 100):
                raise ConfigError("verifymixpct must be in 0..100")
            if self.verify < 0:
                raise ConfigError("--verifymixpct requires --verify")
            if self.bench_mode in ("s3", "hdfs", "netbench"):
                raise ConfigError("--verifymixpct supports file, block device and "
                                  "directory paths only")
            if self.block_size % 8:
                raise ConfigError("--verifymixpct requires a block size that is a "
                                  "multiple of 8")
        if self.verify_diag:
            if self.verify < 0:
                raise ConfigError("--verifydiag requires --verify")
            if self.bench_mode in ("s3", "hdfs", "netbench"):
                raise ConfigError("--verifydiag supports file, block device and "
                                  "directory paths only")
        if not (0 <= self.dedupe_pct <= 100):
            raise ConfigError("dedupepct must be in 0..100")
        if not (0 <= self.compress_pct <= 100):
            raise ConfigError("compresspct must be in 0..100")
        if self.dedupe_pct or self.compress_pct:
            c = self.dedupe_chunk
            if not (512 <= c <= 16 << 20) or c & (c - 1):
                raise ConfigError("--dedupechunk must be a power of two in 512..16M")
            if self.verify >= 0:
                raise ConfigError("--dedupepct/--compresspct cannot be used together with "
                                  "--verify")
            if self.blockvar_pct != 100:
                raise ConfigError("--dedupepct/--compresspct cannot be used together with "
                                  "--blockvarpct")
            if self.bench_mode in ("s3", "hdfs", "netbench"):
                raise ConfigError("--dedupepct/--compresspct supports file, block device "
                                  "and directory paths only")
        # reference ProgArgs.cpp:1548-1556: readback verification and inline
        # reads are sync-engine features
        if self.verify_direct and (self.verify < 0 or not self.run_write):
            raise ConfigError("--verifydirect requires --verify and -w/--write")
        if self.verify_direct and self.iodepth > 1:
            raise ConfigError("--verifydirect cannot be used together with --iodepth")
        if self.read_inline and self.iodepth > 1:
            raise ConfigError("--readinline cannot be used together with --iodepth")
        # reference ProgArgs.cpp:1486: mmap is a sync-engine feature
        if self.mmap and self.iodepth > 1:
            raise ConfigError("--mmap does not support --iodepth larger than 1")
        if self.verify >= 0 and self.blockvar_pct and False:
            pass  # verify overrides block variance; no error

    def _rwmix_threads_effective(self) -> int:
        if self.rwmix_threads:
            return self.rwmix_threads
        if self.rwmix_thread_pct:
            return max(1, self.threads * self.rwmix_thread_pct // 100)
        return 0

    # ------------------------------------------------------------------
    def phase_list(self) -> list[str]:
        """Ordered phase names for one iteration (reference order,
        Coordinator.cpp:311-334)."""
        if self.bench_mode == "netbench":
            return ["NETBENCH"] if self.run_write else []
        if self.bench_mode == "s3":
            # reference phase order, Coordinator.cpp:311-334
            order = [
                ("MKDIRS", self.run_mkdirs),       # MKBUCKETS
                ("BVERSION", self.s3_bversion),
                ("OLOCKCFG", self.s3_olock),
                ("PUTBACL", self.s3_bacl_put),
                ("PUTBTAG", self.s3_btag),
                ("GETBTAG", self.s3_btag and self.s3_btag_verify),
                ("WRITE", self.run_write),         # PUT objects
                ("S3MPUCOMPLETE", self.s3_mpu_complete),
                ("PUTOBJACL", self.s3_acl_put),
                ("PUTOTAG", self.s3_otag),
                ("STAT", self.run_stat),           # HEAD objects
                ("GETOTAG", self.s3_otag and self.s3_otag_verify),
                ("GETOBJACL", self.s3_acl_get),
                ("STATDIRS", self.run_statdirs),
                ("LISTOBJ", bool(self.s3_list_obj)),
                ("LISTOBJPAR", self.s3_list_par),
                ("READ", self.run_read),           # GET objects
                ("DELOTAG", self.s3_otag and self.run_delfiles),
                ("RMFILES", self.run_delfiles),    # delete objects
                ("GETBACL", self.s3_bacl_get),
                ("RMDIRS", self.run_deldirs),      # RMBUCKETS
            ]
            return [name for name, enabled in order if enabled]
        order = [
            ("MKDIRS", self.run_mkdirs),
            ("WRITE", self.run_write),
            ("STAT", self.run_stat),
            ("READ", self.run_read),
            ("RMFILES", self.run_delfiles),
            ("RMDIRS", self.run_deldirs),
        ]
        return [name for name, enabled in order if enabled]

    # ------------------------------------------------------------------
    def to_wire(self) -> dict[str, Any]:
        """Serialize for master->service transfer (JSON-able)."""
        d = dataclasses.asdict(self)
        # master-only options never sent to services
        for k in ("hosts", "service_mode", "quit_services", "interrupt_services",
                  "csv_file", "json_file", "res_file", "live_csv", "config_file"):
            d.pop(k, None)
        return d

    @classmethod
    def from_wire(cls, d: dict[str, Any]) -> "BenchConfig":
        cfg = cls()
        for k, v in d.items():
            if hasattr(cfg, k):
                setattr(cfg, k, v)
        return cfg

    # ------------------------------------------------------------------
    def engine_dict(self) -> dict[str, Any]:
        """Config dict for the native engine (_core.Engine)."""
        return dict(
            paths=self.paths,
            path_type=self.path_type,
            threads=self.threads,
            rank_offset=self.rank_offset,
            num_dataset_threads=self.num_dataset_threads or self.threads,
            dirs=self.dirs,
            files=self.files,
            file_size=self.file_size,
            block_size=self.block_size,
            iodepth=self.iodepth,
            direct=self.direct,
            random=self.random,
            rand_aligned=self.rand_aligned,
            rand_amount=self.rand_amount,
            strided=self.strided,
            backward=self.backward,
            truncate=self.truncate,
            trunc_to_size=self.file_size if self.trunc_to_size else None,
            prealloc=self.prealloc,
            verify_salt=self.verify,
            verify_mix_pct=self.verify_mix_pct,
            verify_diag=self.verify_diag,
            verify_direct=self.verify_direct,
            blockvar_pct=self.blockvar_pct,
            blockvar_algo=self.blockvar_algo,
            dedupe_pct=self.dedupe_pct,
            compress_pct=self.compress_pct,
            dedupe_chunk=self.dedupe_chunk,
            reduce_verify_salt=self.dedupe_verify,
            data_profile=self.data_profile,
            rand_algo=self.rand_algo,
            gpu_ids=self.gpu_ids,
            gpu_pinned=self.gpu_pinned,
            lat=self.lat,
            rwmix_pct=self.rwmix_pct,
            rwmix_threads=self._rwmix_threads_effective(),
            mmap=self.mmap,
            fadv_flags=_fadv_to_bits(self.fadv),
            madv_flags=_madv_to_flags(self.madv),
            flock_mode={"": 0, "range": 1, "full": 2}[self.flock_mode],
            read_inline=self.read_inline,
            stat_inline=self.stat_inline,
            ops_log=self.ops_log_path,
            ops_log_lock=self.ops_log_lock,
            cores=_parse_int_list(self.cpu_cores),
            zones=_parse_int_list(self.numa_zones),
            netbench_is_server=self.netbench_is_server,
            netbench_servers=self.servers,
            netbench_port=self.service_port + 1000,
            netbench_num_conns=self.netbench_num_conns,
            resp_size=self.resp_size,
            send_buf=self.send_buf,
            recv_buf=self.recv_buf,
            netdevs=self.netdevs,
            tree_dirs=self.tree_dirs_resolved,
            tree_files=self.tree_files_resolved,
            sharesize=self.sharesize,
            tree_round_robin=self.tree_round_robin,
            tree_rand=self.tree_rand,
            limit_read_bps=self.limit_read,
            limit_write_bps=self.limit_write,
            ignore_del_errors=self.ignore_del_errors,
            dir_sharing=self.dir_sharing,
            inf_loop=self.inf_loop,
            dynamic_slice=self.dyn_slice,
            bench_seed=self.bench_seed or 0x243F6A8885A308D3,
        )


# --fadv bit values must match csrc/engine.cpp FadvBits
_FADV_BITS = {"seq": 1, "sequential": 1, "rand": 2, "random": 2, "willneed": 4,
              "dontneed": 8, "noreuse": 16}

# madvise flag values from <sys/mman.h>
_MADV_FLAGS = {"seq": 2, "sequential": 2, "rand": 1, "random": 1, "willneed": 3,
               "dontneed": 4, "hugepage": 14, "nohugepage": 15}


def _fadv_to_bits(csv_str: str) -> int:
    bits = 0
    for tok in csv_str.split(","):
        tok = tok.strip().lower()
        if not tok:
            continue
        if tok not in _FADV_BITS:
            raise ConfigError(f"unknown fadvise flag: {tok}")
        bits |= _FADV_BITS[tok]
    return bits


def _madv_to_flags(csv_str: str) -> int:
    # madvise advices are not bitmask-combinable; take the last one given
    flags = 0
    for tok in csv_str.split(","):
        tok = tok.strip().lower()
        if not tok:
            continue
        if tok not in _MADV_FLAGS:
            raise ConfigError(f"unknown madvise flag: {tok}")
        flags = _MADV_FLAGS[tok]
    return flags


def _parse_int_list(s: str) -> list[int]:
    if not s:
        return []
    return [int(x) for x in s.replace(",", " ").split()]


def parse_gpu_ids(s: str) -> list[int]:
    if not s:
        return []
    return [int(x) for x in s.replace(",", " ").split()]
