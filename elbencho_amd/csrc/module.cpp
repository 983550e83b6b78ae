// pybind11 bindings for the elbencho_amd core engine (_core).

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <execinfo.h>
#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <optional>
#include <unistd.h>

#include <fcntl.h>

#include "crc.h"
#include "crc64.h"
#include "engine.h"
#include "httpdata.h"
#include "s3srv.h"
#include "gpu.h"
#include "histogram.h"

namespace py = pybind11;
using namespace eb;

namespace {

// geometry the CPU mix loops take for granted (the engine checks it once, in
// its constructor; the GPU wrappers check it per call)
void requireMixArgs(const char* what, uint64_t blockSize, uint64_t mixLen)
{
    if (!blockSize || blockSize % 8 || mixLen % 8 || mixLen > blockSize)
        throw std::invalid_argument(std::string(what) +
                                    ": block_size must be a positive multiple of 8 and "
                                    "mix_len a multiple of 8 not above it");
}

// geometry fillReduceCPU takes for granted (the engine checks it once, in its
// constructor; GpuCtx::fillReduceDev checks it per call)
void requireReduceArgs(const char* what, uint64_t chunk, uint64_t randBytes, int dedupePct,
                       uint64_t pool)
{
    if (chunk < 16 || (chunk & (chunk - 1)) || randBytes % 16 || randBytes > chunk ||
        dedupePct < 0 || dedupePct > 100 || !pool)
        throw std::invalid_argument(std::string(what) +
                                    ": chunk must be a power of two >= 16, rand_bytes a "
                                    "multiple of 16 not above it, dedupe_pct in 0..100 and "
                                    "pool >= 1");
}

// a GpuVerifyDiag as a dict keyed by the record's field names
py::dict diagToDict(const GpuVerifyDiag& r)
{
    py::dict d;
    d["nbad"] = r.numMismatches;
    d["first"] = r.firstBadFileOffset;
    d["last"] = r.lastBadFileOffset;
    d["runs"] = r.runs;
    d["zero"] = r.zero;
    d["pattern"] = r.pattern;
    d["bitflip"] = r.bitflip;
    d["other"] = r.other;
    d["delta_min"] = r.deltaMin;
    d["delta_max"] = r.deltaMax;
    d["flip_or"] = r.flipOr;
    return d;
}

// a DataProfileAcc as it crosses the binding
py::dict profileToDict(const DataProfileAcc& a)
{
    py::dict d;
    d["chunks"] = a.chunks;
    d["bytes"] = a.bytes;
    d["zero_chunks"] = a.zeroChunks;
    py::list hist;
    for (uint64_t v : a.hist) hist.append(v);
    d["hist"] = hist;
    d["regs"] = py::bytes((const char*)a.regs, DP_HLL_M);
    return d;
}

void requireProfileChunk(const char* what, uint64_t chunk)
{
    if (!dataProfileChunkOk(chunk))
        throw std::invalid_argument(std::string(what) +
                                    ": chunk must be a power of two in 512..16M");
}

EngineConfig configFromDict(const py::dict& d)
{
    EngineConfig c;

    auto getU64 = [&](const char* k, uint64_t def) -> uint64_t {
        return d.contains(k) ? d[k].cast<uint64_t>() : def;
    };
    auto getI = [&](const char* k, int64_t def) -> int64_t {
        return d.contains(k) ? d[k].cast<int64_t>() : def;
    };
    auto getB = [&](const char* k, bool def) -> bool {
        return d.contains(k) ? d[k].cast<bool>() : def;
    };
    auto getS = [&](const char* k, std::string def) -> std::string {
        return d.contains(k) ? d[k].cast<std::string>() : def;
    };

    if (d.contains("paths")) c.paths = d["paths"].cast<std::vector<std::string>>();
    std::string pt = getS("path_type", "file");
    c.pathType = (pt == "dir") ? PathType::DIR : (pt == "bdev") ? PathType::BLOCKDEV
                                                                : PathType::FILE;

    c.numThreads = (int)getI("threads", 1);
    c.rankOffset = (int)getI("rank_offset", 0);
    c.numDataSetThreads = (int)getI("num_dataset_threads", c.numThreads);
    c.numDirs = getU64("dirs", 0);
    c.numFiles = getU64("files", 0);
    c.fileSize = getU64("file_size", 0);
    c.blockSize = getU64("block_size", 1ULL << 20);
    c.ioDepth = (int)getI("iodepth", 1);
    c.directIO = getB("direct", false);
    c.random = getB("random", false);
    c.randAligned = getB("rand_aligned", true);
    c.randAmount = getU64("rand_amount", 0);
    c.strided = getB("strided", false);
    c.backward = getB("backward", false);
    c.truncate = getB("truncate", false);
    c.truncToSize = d.contains("trunc_to_size") && !d["trunc_to_size"].is_none()
                        ? d["trunc_to_size"].cast<uint64_t>()
                        : UINT64_MAX;
    c.preallocFile = getB("prealloc", false);
    c.fsyncPerFile = getB("fsync", false);
    c.verifySalt = getI("verify_salt", -1);
    c.verifyMixPct = (int)getI("verify_mix_pct", -1);
    c.verifyDiag = getB("verify_diag", false);
    c.verifyDirect = getB("verify_direct", false);
    c.readInline = getB("read_inline", false);
    c.statInline = getB("stat_inline", false);
    c.rwMixPct = (int)getI("rwmix_pct", 0);
    c.rwMixThreads = (int)getI("rwmix_threads", 0);
    c.useMmap = getB("mmap", false);
    c.fadviseFlags = (int)getI("fadv_flags", 0);
    c.madviseFlags = (int)getI("madv_flags", 0);
    c.flockMode = (int)getI("flock_mode", 0);
    c.opsLogPath = getS("ops_log", "");
    c.opsLogLock = getB("ops_log_lock", false);
    if (d.contains("cores")) c.cpuCores = d["cores"].cast<std::vector<int>>();
    if (d.contains("zones")) c.numaZones = d["zones"].cast<std::vector<int>>();
    if (d.contains("tree_dirs"))
        c.treeDirs = d["tree_dirs"].cast<std::vector<std::string>>();
    if (d.contains("tree_files"))
        c.treeFiles = d["tree_files"].cast<std::vector<std::pair<std::string, uint64_t>>>();
    c.shareSize = getU64("sharesize", 0);
    c.treeRoundRobin = getB("tree_round_robin", false);
    c.treeRandomize = getB("tree_rand", false);
    c.netbenchIsServer = getB("netbench_is_server", false);
    if (d.contains("netbench_servers"))
        c.netbenchServers = d["netbench_servers"].cast<std::vector<std::string>>();
    c.netbenchPort = (int)getI("netbench_port", 2611);
    c.netbenchNumConns = (int)getI("netbench_num_conns", 0);
    c.respSize = getU64("resp_size", 1);
    c.sendBufSize = (int)getI("send_buf", 0);
    c.recvBufSize = (int)getI("recv_buf", 0);
    if (d.contains("netdevs"))
        c.netDevs = d["netdevs"].cast<std::vector<std::string>>();
    c.blockVarPct = (int)getI("blockvar_pct", 100);
    c.blockVarAlgo = getS("blockvar_algo", "fast");
    c.dedupePct = (int)getI("dedupe_pct", 0);
    c.compressPct = (int)getI("compress_pct", 0);
    c.dedupeChunk = getU64("dedupe_chunk", 4096);
    c.reduceVerifySalt = getI("reduce_verify_salt", -1);
    c.dataProfile = getB("data_profile", false);
    c.randAlgo = getS("rand_algo", "balanced_single");
    if (d.contains("gpu_ids")) c.gpuIDs = d["gpu_ids"].cast<std::vector<int>>();
    c.gpuPinnedHostBufs = getB("gpu_pinned", true);
    c.measureLat = getB("lat", false);
    c.limitReadBps = getU64("limit_read_bps", 0);
    c.limitWriteBps = getU64("limit_write_bps", 0);
    c.ignoreDelErrors = getB("ignore_del_errors", false);
    c.dirSharing = getB("dir_sharing", false);
    c.infiniteLoop = getB("inf_loop", false);
    c.dynamicSlice = getB("dynamic_slice", false);
    c.benchSeed = getU64("bench_seed", 0x243F6A8885A308D3ULL);

    return c;
}

py::dict resultToDict(const WorkerResult& r)
{
    py::dict d;
    d["rank"] = r.rank;
    d["elapsed_usec"] = r.elapsedUSec;
    d["entries"] = r.total.entries;
    d["bytes"] = r.total.bytes;
    d["iops"] = r.total.iops;
    d["stonewall_entries"] = r.stonewall.entries;
    d["stonewall_bytes"] = r.stonewall.bytes;
    d["stonewall_iops"] = r.stonewall.iops;
    d["stonewall_elapsed_usec"] = r.stonewallElapsedUSec;
    d["rm_entries"] = r.totalReadMix.entries;
    d["rm_bytes"] = r.totalReadMix.bytes;
    d["rm_iops"] = r.totalReadMix.iops;
    d["rm_stonewall_entries"] = r.stonewallReadMix.entries;
    d["rm_stonewall_bytes"] = r.stonewallReadMix.bytes;
    d["rm_stonewall_iops"] = r.stonewallReadMix.iops;
    d["io_lat"] = r.ioLatVec;
    d["entry_lat"] = r.entryLatVec;
    d["io_lat_rm"] = r.ioLatReadMixVec;
    d["entry_lat_rm"] = r.entryLatReadMixVec;
    d["error"] = r.error;
    if (r.profile) d["data_profile"] = profileToDict(*r.profile);
    return d;
}

// Fault signal handlers: dump a native backtrace to stderr and a trace file
// on SIGSEGV/FPE/BUS/ILL/ABRT (reference analogue: toolkits/SignalTk.cpp:29-53,
// which uses boost::stacktrace; this uses glibc backtrace).
extern "C" void ebFaultHandler(int sig)
{
    void* frames[64];
    int n = backtrace(frames, 64);

    const char* name = (sig == SIGSEGV)   ? "SIGSEGV (segmentation fault)"
                       : (sig == SIGFPE)  ? "SIGFPE (floating point exception)"
                       : (sig == SIGBUS)  ? "SIGBUS (bus error; can be caused by a "
                                            "truncated mmap'ed file)"
                       : (sig == SIGILL)  ? "SIGILL (illegal instruction)"
                       : (sig == SIGABRT) ? "SIGABRT (abort)"
                                          : "fatal signal";
    dprintf(STDERR_FILENO, "\nelbencho-amd: caught %s — native backtrace:\n", name);
    backtrace_symbols_fd(frames, n, STDERR_FILENO);

    const char* tmpdir = getenv("TMPDIR");
    char path[256];
    snprintf(path, sizeof(path), "%s/elbencho_amd_fault_trace.txt",
             tmpdir ? tmpdir : "/tmp");
    int fd = open(path, O_WRONLY | O_CREAT | O_APPEND, 0644);
    if (fd >= 0) {
        dprintf(fd, "caught %s — native backtrace:\n", name);
        backtrace_symbols_fd(frames, n, fd);
        close(fd);
        dprintf(STDERR_FILENO, "(trace also appended to %s)\n", path);
    }

    signal(sig, SIG_DFL);
    raise(sig);
}

static void registerFaultHandlers()
{
    for (int sig : {SIGSEGV, SIGFPE, SIGBUS, SIGILL, SIGABRT}) signal(sig, ebFaultHandler);
}

} // namespace

PYBIND11_MODULE(_core, m)
{
    m.def("register_fault_handlers", &registerFaultHandlers,
          "Install SIGSEGV/FPE/BUS/ILL/ABRT handlers that dump a native backtrace");
    m.doc() = "elbencho_amd native I/O engine (MI355X / gfx950)";

    m.def("gpu_device_count", &gpuDeviceCount);
    m.def("gpu_probe_error", &gpuProbeError);
    m.def("gpu_device_name", &gpuDeviceName);
    m.def("gpu_numa_node", &gpuNumaNode);

    m.def("hist_bucket_lower_bound", &LatencyHistogram::bucketLowerBound);
    m.def("hist_num_buckets", [] { return (int)LatencyHistogram::NUM_BUCKETS; });

    // CPU checksum helpers exposed for tests (numerics parity with the GPU
    // kernels is tested by comparing against these)
    m.def("fill_checksum", [](uint64_t len, uint64_t fileOff, uint64_t salt) {
        std::string buf(len, '\0');
        fillChecksumCPU(buf.data(), len, fileOff, salt);
        return py::bytes(buf);
    });
    m.def("verify_checksum", [](py::bytes data, uint64_t fileOff, uint64_t salt) {
        std::string buf = data;
        return verifyChecksumCPU(buf.data(), buf.size(), fileOff, salt);
    });

    // --verifymixpct pattern on the CPU (tests tie these to the numpy model)
    m.def("fill_checksum_mix", [](uint64_t len, uint64_t fileOff, uint64_t salt,
                                  uint64_t blockSize, uint64_t mixLen) {
        requireMixArgs("fill_checksum_mix", blockSize, mixLen);
        std::string buf(len, '\0');
        fillChecksumMixCPU(buf.data(), len, fileOff, salt, blockSize, mixLen);
        return py::bytes(buf);
    }, py::arg("len"), py::arg("file_off"), py::arg("salt"), py::arg("block_size"),
       py::arg("mix_len"));
    m.def("verify_checksum_mix", [](py::bytes data, uint64_t fileOff, uint64_t salt,
                                    uint64_t blockSize, uint64_t mixLen) {
        requireMixArgs("verify_checksum_mix", blockSize, mixLen);
        std::string buf = data;
        return verifyChecksumMixCPU(buf.data(), buf.size(), fileOff, salt, blockSize, mixLen);
    }, py::arg("data"), py::arg("file_off"), py::arg("salt"), py::arg("block_size"),
       py::arg("mix_len"));

    // --dedupepct / --compresspct pattern on the CPU (tests tie it to the
    // numpy model) and the seeds the engine derives for a worker and phase
    m.def("fill_reduce", [](uint64_t len, uint64_t firstChunk, uint64_t chunk,
                            uint64_t randBytes, int dedupePct, uint64_t pool,
                            uint64_t uniqSeed, uint64_t poolSeed) {
        requireReduceArgs("fill_reduce", chunk, randBytes, dedupePct, pool);
        std::string buf(len, '\xA5');
        fillReduceCPU(buf.data(), len, firstChunk, chunk, randBytes, dedupePct, pool, uniqSeed,
                      poolSeed);
        return py::bytes(buf);
    }, py::arg("len"), py::arg("first_chunk"), py::arg("chunk"), py::arg("rand_bytes"),
       py::arg("dedupe_pct"), py::arg("pool"), py::arg("uniq_seed"), py::arg("pool_seed"));
    m.def("reduce_seeds", [](uint64_t benchSeed, int phaseSeq, int rank) {
        ReduceSeeds s = reduceSeeds(benchSeed, phaseSeq, rank);
        return py::make_tuple(s.uniq, s.pool);
    }, py::arg("bench_seed"), py::arg("phase_seq"), py::arg("rank"));
    m.attr("REDUCE_POOL_CHUNKS") = REDUCE_POOL_CHUNKS;

    // --dedupeverify on the CPU: (mismatching 8-byte words, first bad file
    // offset or 2^64-1) of data, which lies at file_off, against the pattern
    // from chunk first_chunk on; the seeds of a file; the key of a dir-mode file
    m.def("verify_reduce", [](py::bytes data, uint64_t fileOff, uint64_t firstChunk,
                              uint64_t chunk, uint64_t randBytes, int dedupePct, uint64_t pool,
                              uint64_t uniqSeed, uint64_t poolSeed) {
        requireReduceArgs("verify_reduce", chunk, randBytes, dedupePct, pool);
        std::string buf = data;
        GpuVerifyResult r = verifyReduceCPU(buf.data(), buf.size(), fileOff, firstChunk, chunk,
                                            randBytes, dedupePct, pool, uniqSeed, poolSeed);
        return py::make_tuple(r.numMismatches, r.firstBadFileOffset);
    }, py::arg("data"), py::arg("file_off"), py::arg("first_chunk"), py::arg("chunk"),
       py::arg("rand_bytes"), py::arg("dedupe_pct"), py::arg("pool"), py::arg("uniq_seed"),
       py::arg("pool_seed"));
    m.def("reduce_verify_seeds", [](uint64_t salt, uint64_t fileKey) {
        ReduceSeeds s = reduceVerifySeeds(salt, fileKey);
        return py::make_tuple(s.uniq, s.pool);
    }, py::arg("salt"), py::arg("file_key"));
    m.def("reduce_dir_file_key", &reduceDirFileKey, py::arg("rank"), py::arg("dir"),
          py::arg("file"));

    // --verifydiag on the CPU; block_size 0 selects the plain pattern
    // --dataprofile: the CPU twin over one block
    m.def("data_profile", [](py::bytes data, uint64_t chunk) {
        requireProfileChunk("data_profile", chunk);
        std::string buf = data;
        auto acc = std::make_unique<DataProfileAcc>();
        dataProfileCPU(buf.data(), buf.size(), chunk, *acc);
        return profileToDict(*acc);
    }, py::arg("data"), py::arg("chunk") = 4096);

    m.def("verify_diag", [](py::bytes data, uint64_t fileOff, uint64_t salt,
                            uint64_t blockSize, uint64_t mixLen) {
        std::string buf = data;
        GpuVerifyDiag r;
        if (blockSize) {
            requireMixArgs("verify_diag", blockSize, mixLen);
            verifyDiagMixCPU(buf.data(), buf.size(), fileOff, salt, blockSize, mixLen, r);
        } else {
            verifyDiagCPU(buf.data(), buf.size(), fileOff, salt, r);
        }
        return diagToDict(r);
    }, py::arg("data"), py::arg("file_off"), py::arg("salt"), py::arg("block_size") = 0,
       py::arg("mix_len") = 0);
    m.def("verify_diag_text", [](const py::dict& d) {
        GpuVerifyDiag r;
        r.numMismatches = d["nbad"].cast<uint64_t>();
        r.firstBadFileOffset = d["first"].cast<uint64_t>();
        r.lastBadFileOffset = d["last"].cast<uint64_t>();
        r.runs = d["runs"].cast<uint64_t>();
        r.zero = d["zero"].cast<uint64_t>();
        r.pattern = d["pattern"].cast<uint64_t>();
        r.bitflip = d["bitflip"].cast<uint64_t>();
        r.other = d["other"].cast<uint64_t>();
        r.deltaMin = d["delta_min"].cast<int64_t>();
        r.deltaMax = d["delta_max"].cast<int64_t>();
        r.flipOr = d["flip_or"].cast<uint64_t>();
        return verifyDiagText(r);
    }, py::arg("record"));

    // CRC32C (Castagnoli, slice-by-8) for the S3 client's
    // x-amz-checksum-crc32c header (--s3chksumalgo CRC32C)
    m.def("crc32c", [](py::bytes data) {
        std::string buf = data;
        return crcUpdate(CrcAlgo::CRC32C, 0, buf.data(), buf.size());
    });

    // CRC host libraries (csrc/crc.h, csrc/crc64.h): algo is "CRC32",
    // "CRC32C" or "CRC64NVME"; the last returns an int of up to 64 bits
    m.def("crc", [](py::bytes data, const std::string& algo) -> uint64_t {
        std::string buf = data;
        if (algo == CRC64_NVME_NAME) {
            py::gil_scoped_release rel;
            return crc64Update(0, buf.data(), buf.size());
        }
        CrcAlgo a = crcAlgoFromName(algo);
        py::gil_scoped_release rel;
        return crcUpdate(a, 0, buf.data(), buf.size());
    }, py::arg("data"), py::arg("algo"));
    // CRC of A||B from the CRCs of A and B (zlib crc32_combine semantics)
    m.def("crc_combine", [](const std::string& algo, uint64_t crcA, uint64_t crcB,
                            uint64_t lenB) -> uint64_t {
        if (algo == CRC64_NVME_NAME) return crc64Combine(crcA, crcB, lenB);
        CrcAlgo a = crcAlgoFromName(algo);
        if ((crcA | crcB) >> 32) throw py::type_error(algo + " values are 32 bits wide");
        return crcCombine(a, (uint32_t)crcA, (uint32_t)crcB, lenB);
    }, py::arg("algo"), py::arg("crc_a"), py::arg("crc_b"), py::arg("len_b"));
    // Finished CRC from the host emulation of the device tile kernel
    // (crc64TilesHost + the host fold): the kernel's tables, weights and
    // geometry checked without a GPU. len(data) % 16 must be 0.
    m.def("crc_tiles_host", [](py::bytes data, const std::string& algo) -> uint64_t {
        if (algo != CRC64_NVME_NAME)
            throw std::invalid_argument("crc_tiles_host: unknown algorithm '" + algo +
                                        "' (CRC64NVME)");
        std::string buf = data;
        if (buf.size() % 16)
            throw std::invalid_argument("crc_tiles_host: length must be a multiple of 16");
        py::gil_scoped_release rel;
        std::vector<uint64_t> part = crc64TilesHost(buf.data(), buf.size());
        Crc64Shift tileShift(CRC64_TILE_BYTES);
        return crc64FinishRaw(crc64FoldTiles(tileShift, 0, part.data(), buf.size()),
                              buf.size());
    }, py::arg("data"), py::arg("algo") = CRC64_NVME_NAME);

    // --- offset generator test hook ---
    m.def("gen_offsets",
          [](const std::string& kind, uint64_t blockSize, uint64_t rangeStart,
             uint64_t rangeLen, uint64_t seed, uint64_t rank, uint64_t nranks,
             uint64_t amount, uint64_t maxCount) {
              RandAlgoXoshiro256ss rng(seed);
              std::unique_ptr<OffsetGen> gen;
              if (kind == "seq")
                  gen = std::make_unique<OffsetGenSequential>(blockSize);
              else if (kind == "reverse")
                  gen = std::make_unique<OffsetGenReverseSeq>(blockSize);
              else if (kind == "random")
                  gen = std::make_unique<OffsetGenRandom>(blockSize, rng, amount);
              else if (kind == "random_aligned")
                  gen = std::make_unique<OffsetGenRandomAligned>(blockSize, rng, amount);
              else if (kind == "full_coverage")
                  gen = std::make_unique<OffsetGenRandomAlignedFullCoverage>(blockSize, seed);
              else if (kind == "strided")
                  gen = std::make_unique<OffsetGenStrided>(blockSize, rank, nranks);
              else
                  throw std::runtime_error("unknown offset generator: " + kind);
              gen->reset(rangeStart, rangeLen);
              std::vector<std::pair<uint64_t, uint64_t>> out;
              BlockSpec spec;
              while (gen->next(spec) && out.size() < maxCount)
                  out.emplace_back(spec.offset, spec.len);
              return py::make_tuple(out, gen->totalBytes());
          },
          py::arg("kind"), py::arg("block_size"), py::arg("range_start"),
          py::arg("range_len"), py::arg("seed") = 1, py::arg("rank") = 0,
          py::arg("nranks") = 1, py::arg("amount") = 0,
          py::arg("max_count") = 1u << 22);

    // Like gen_offsets but resets ONE generator over several ranges (the way
    // the engine reuses a generator across files in dir/custom-tree mode) and
    // returns the per-range offset lists. Guards the reset() contract.
    m.def("gen_offsets_ranges",
          [](const std::string& kind, uint64_t blockSize,
             const std::vector<std::pair<uint64_t, uint64_t>>& ranges,
             uint64_t seed, uint64_t maxCount) {
              RandAlgoXoshiro256ss rng(seed);
              std::unique_ptr<OffsetGen> gen;
              if (kind == "seq")
                  gen = std::make_unique<OffsetGenSequential>(blockSize);
              else if (kind == "reverse")
                  gen = std::make_unique<OffsetGenReverseSeq>(blockSize);
              else if (kind == "random")
                  gen = std::make_unique<OffsetGenRandom>(blockSize, rng, 0);
              else if (kind == "random_aligned")
                  gen = std::make_unique<OffsetGenRandomAligned>(blockSize, rng, 0);
              else if (kind == "full_coverage")
                  gen = std::make_unique<OffsetGenRandomAlignedFullCoverage>(blockSize, seed);
              else
                  throw std::runtime_error("unknown offset generator: " + kind);
              std::vector<std::vector<std::pair<uint64_t, uint64_t>>> out;
              for (const auto& r : ranges) {
                  gen->reset(r.first, r.second);
                  std::vector<std::pair<uint64_t, uint64_t>> pass;
                  BlockSpec spec;
                  while (gen->next(spec) && pass.size() < maxCount)
                      pass.emplace_back(spec.offset, spec.len);
                  out.push_back(std::move(pass));
              }
              return out;
          },
          py::arg("kind"), py::arg("block_size"), py::arg("ranges"),
          py::arg("seed") = 1, py::arg("max_count") = 1u << 22);

    // --- GPU kernel test helpers (numerics parity vs the CPU reference) ---
    m.def("gpu_fill_checksum", [](uint64_t len, uint64_t fileOff, uint64_t salt, int dev) {
        GpuCtx ctx(dev, 1, len, true);
        ctx.fillChecksumDev(0, len, fileOff, salt);
        ctx.copyD2HAsync(0, len);
        ctx.syncStream();
        return py::bytes(ctx.hostBuf(0), len);
    }, py::arg("len"), py::arg("file_off"), py::arg("salt"), py::arg("dev") = 0);

    // lds=true runs the LDS-tiled A/B kernel instead of the production one
    m.def("gpu_verify_checksum", [](py::bytes data, uint64_t fileOff, uint64_t salt, int dev,
                                    bool lds) {
        std::string buf = data;
        GpuCtx ctx(dev, 1, buf.size(), true);
        std::memcpy(ctx.hostBuf(0), buf.data(), buf.size());
        ctx.copyH2DAsync(0, buf.size());
        ctx.syncStream();
        GpuVerifyResult r = ctx.verifyChecksumDev(0, buf.size(), fileOff, salt, lds);
        return py::make_tuple(r.numMismatches, r.firstBadFileOffset);
    }, py::arg("data"), py::arg("file_off"), py::arg("salt"), py::arg("dev") = 0,
       py::arg("lds") = false);

    // --- test-only helpers for the bit-exact kernel tests (not for the engine) ---

    // One xoshiro256++ stream of the CPU "balanced" fill (seeded with the
    // same four splitmix64 outputs as the device Xoshiro256pp::seed), as n
    // little-endian u64 — ties the tests' numpy model to rand.h.
    m.def("xoshiro256pp_stream", [](uint64_t seed, uint64_t n) {
        RandAlgoXoshiro256ppSIMD<1> rng(seed);
        std::string out(n * 8, '\0');
        for (uint64_t i = 0; i < n; i++) {
            uint64_t v = rng.next();
            std::memcpy(&out[i * 8], &v, 8);
        }
        return py::bytes(out);
    }, py::arg("seed"), py::arg("n"));

    // Guarded fill: preset len+guard device bytes to `sentinel`, run `calls`
    // fills of `len` bytes on a fresh context, return all len+guard bytes so
    // a test can compare [0,len) exactly and see any write past len.
    // op: "checksum" (a=file_off, b=salt), "rand" (a=seed),
    //     "blockvar" (a=seed, b=refill_len).
    m.def("gpu_fill_guarded", [](const std::string& op, uint64_t len, uint64_t guard,
                                 uint64_t a, uint64_t b, bool fast, int sentinel, int calls,
                                 int dev) {
        if (op != "checksum" && op != "rand" && op != "blockvar")
            throw std::invalid_argument("gpu_fill_guarded: unknown op " + op);
        const uint64_t total = len + guard;
        GpuCtx ctx(dev, 1, total, true);
        std::memset(ctx.hostBuf(0), sentinel, total);
        ctx.copyH2DAsync(0, total);
        ctx.syncStream();
        for (int i = 0; i < calls; i++) {
            if (op == "checksum")
                ctx.fillChecksumDev(0, len, a, b);
            else if (op == "rand")
                ctx.fillRandDev(0, len, a, fast);
            else
                ctx.blockVarRefillDev(0, len, b, a, fast);
        }
        std::memset(ctx.hostBuf(0), ~sentinel, total); // D2H must overwrite all of it
        ctx.copyD2HAsync(0, total);
        ctx.syncStream();
        return py::bytes(ctx.hostBuf(0), total);
    }, py::arg("op"), py::arg("len"), py::arg("guard"), py::arg("a") = 0, py::arg("b") = 0,
       py::arg("fast") = false, py::arg("sentinel") = 0xA5, py::arg("calls") = 1,
       py::arg("dev") = 0);

    // Batched verify: one context, one slot per (data, file_off) item, one
    // verifyChecksumDevAsync launch each with no fetch in between; then two
    // fetchVerifyResult calls, then (optionally) a synchronous verify of
    // `then` on the same context. Returns the results in that order.
    m.def("gpu_verify_batch", [](const std::vector<std::pair<py::bytes, uint64_t>>& items,
                                 uint64_t salt, bool lds,
                                 std::optional<std::pair<py::bytes, uint64_t>> then, int dev) {
        std::vector<std::string> bufs;
        uint64_t maxLen = 16;
        for (const auto& it : items) {
            bufs.emplace_back(it.first);
            maxLen = std::max<uint64_t>(maxLen, bufs.back().size());
        }
        std::string thenBuf;
        if (then) {
            thenBuf = then->first;
            maxLen = std::max<uint64_t>(maxLen, thenBuf.size());
        }
        if (bufs.empty()) throw std::invalid_argument("gpu_verify_batch: no items");
        GpuCtx ctx(dev, (int)bufs.size(), maxLen, true);
        for (size_t i = 0; i < bufs.size(); i++) {
            std::memcpy(ctx.hostBuf((int)i), bufs[i].data(), bufs[i].size());
            ctx.copyH2DAsync((int)i, bufs[i].size());
            ctx.verifyChecksumDevAsync((int)i, bufs[i].size(), items[i].second, salt, lds);
        }
        py::list out;
        auto push = [&](const GpuVerifyResult& r) {
            out.append(py::make_tuple(r.numMismatches, r.firstBadFileOffset));
        };
        push(ctx.fetchVerifyResult());
        push(ctx.fetchVerifyResult());
        if (then) {
            std::memcpy(ctx.hostBuf(0), thenBuf.data(), thenBuf.size());
            ctx.copyH2DAsync(0, thenBuf.size());
            ctx.syncStream();
            push(ctx.verifyChecksumDev(0, thenBuf.size(), then->second, salt, lds));
        }
        return out;
    }, py::arg("items"), py::arg("salt"), py::arg("lds") = false,
       py::arg("then") = py::none(), py::arg("dev") = 0);

    // --- test-only helpers for the --verifymixpct kernels ---

    // Guarded mix fill: len+guard device bytes preset to `sentinel`, one
    // fillChecksumMixDev of len bytes, all len+guard bytes returned.
    m.def("gpu_fill_checksum_mix", [](uint64_t len, uint64_t guard, uint64_t fileOff,
                                      uint64_t salt, uint64_t blockSize, uint64_t mixLen,
                                      int sentinel, int dev) {
        const uint64_t total = len + guard;
        GpuCtx ctx(dev, 1, std::max<uint64_t>(total, 16), true);
        std::memset(ctx.hostBuf(0), sentinel, total);
        if (total) ctx.copyH2DAsync(0, total);
        ctx.syncStream();
        ctx.fillChecksumMixDev(0, len, fileOff, salt, blockSize, mixLen);
        std::memset(ctx.hostBuf(0), ~sentinel, total); // D2H must overwrite all of it
        if (total) ctx.copyD2HAsync(0, total);
        ctx.syncStream();
        return py::bytes(ctx.hostBuf(0), total);
    }, py::arg("len"), py::arg("guard"), py::arg("file_off"), py::arg("salt"),
       py::arg("block_size"), py::arg("mix_len"), py::arg("sentinel") = 0xA5,
       py::arg("dev") = 0);

    m.def("gpu_verify_checksum_mix", [](py::bytes data, uint64_t fileOff, uint64_t salt,
                                        uint64_t blockSize, uint64_t mixLen, int dev) {
        std::string buf = data;
        GpuCtx ctx(dev, 1, std::max<uint64_t>(buf.size(), 16), true);
        std::memcpy(ctx.hostBuf(0), buf.data(), buf.size());
        if (!buf.empty()) ctx.copyH2DAsync(0, buf.size());
        ctx.syncStream();
        GpuVerifyResult r =
            ctx.verifyChecksumMixDev(0, buf.size(), fileOff, salt, blockSize, mixLen);
        return py::make_tuple(r.numMismatches, r.firstBadFileOffset);
    }, py::arg("data"), py::arg("file_off"), py::arg("salt"), py::arg("block_size"),
       py::arg("mix_len"), py::arg("dev") = 0);

    // Like gpu_verify_batch for the mix kernel: one slot and one async launch
    // per (data, file_off) item with no fetch in between; plain_items are
    // verified with the plain kernel on the same context, interleaved after
    // the mix item of the same index (the rest after the last mix item).
    // Returns the results of two fetchVerifyResult calls.
    m.def("gpu_verify_mix_batch", [](const std::vector<std::pair<py::bytes, uint64_t>>& items,
                                     uint64_t salt, uint64_t blockSize, uint64_t mixLen,
                                     const std::vector<std::pair<py::bytes, uint64_t>>& plainItems,
                                     int dev) {
        if (items.empty()) throw std::invalid_argument("gpu_verify_mix_batch: no items");
        std::vector<std::string> bufs, plainBufs;
        uint64_t maxLen = 16;
        for (const auto& it : items) bufs.emplace_back(it.first);
        for (const auto& it : plainItems) plainBufs.emplace_back(it.first);
        for (const auto& b : bufs) maxLen = std::max<uint64_t>(maxLen, b.size());
        for (const auto& b : plainBufs) maxLen = std::max<uint64_t>(maxLen, b.size());
        GpuCtx ctx(dev, (int)(bufs.size() + plainBufs.size()), maxLen, true);
        int slot = 0;
        auto stage = [&](const std::string& b) {
            std::memcpy(ctx.hostBuf(slot), b.data(), b.size());
            if (!b.empty()) ctx.copyH2DAsync(slot, b.size());
        };
        auto plainAt = [&](size_t i) {
            stage(plainBufs[i]);
            ctx.verifyChecksumDevAsync(slot++, plainBufs[i].size(), plainItems[i].second, salt);
        };
        for (size_t i = 0; i < bufs.size(); i++) {
            stage(bufs[i]);
            ctx.verifyChecksumMixDevAsync(slot++, bufs[i].size(), items[i].second, salt,
                                          blockSize, mixLen);
            if (i < plainBufs.size()) plainAt(i);
        }
        for (size_t i = bufs.size(); i < plainBufs.size(); i++) plainAt(i);
        py::list out;
        for (int k = 0; k < 2; k++) {
            GpuVerifyResult r = ctx.fetchVerifyResult();
            out.append(py::make_tuple(r.numMismatches, r.firstBadFileOffset));
        }
        return out;
    }, py::arg("items"), py::arg("salt"), py::arg("block_size"), py::arg("mix_len"),
       py::arg("plain_items") = std::vector<std::pair<py::bytes, uint64_t>>{},
       py::arg("dev") = 0);

    // --- --dataprofile kernel ---

    // One block through ebDataProfileKernel. The whole slot is filled with
    // 0xA5 before data is copied in, on the host and on the device, so a
    // kernel that counts or hashes anything at or past len shows up.
    m.def("gpu_data_profile", [](py::bytes data, uint64_t chunk, int dev) {
        requireProfileChunk("gpu_data_profile", chunk);
        std::string buf = data;
        GpuCtx ctx(dev, 1, std::max<uint64_t>(buf.size(), 16), true);
        std::memset(ctx.hostBuf(0), 0xA5, ctx.slotStride());
        std::memcpy(ctx.hostBuf(0), buf.data(), buf.size());
        ctx.copyH2DAsync(0, ctx.slotStride());
        ctx.dataProfileReset();
        ctx.dataProfileDevAsync(0, buf.size(), chunk);
        auto acc = std::make_unique<DataProfileAcc>();
        ctx.dataProfileFetch(*acc);
        return profileToDict(*acc);
    }, py::arg("data"), py::arg("chunk") = 4096, py::arg("dev") = 0);

    // Several blocks with no fetch in between. contexts = 1: all of them into
    // one context, one slot each. contexts = 2: two contexts on one stream of
    // the shared pool, block i into context i % 2. Returns one profile per
    // context.
    m.def("gpu_data_profile_batch", [](const std::vector<py::bytes>& items, uint64_t chunk,
                                       int dev, int contexts) {
        requireProfileChunk("gpu_data_profile_batch", chunk);
        if (items.empty()) throw std::invalid_argument("gpu_data_profile_batch: no items");
        if (contexts != 1 && contexts != 2)
            throw std::invalid_argument("gpu_data_profile_batch: contexts must be 1 or 2");
        std::vector<std::string> bufs;
        uint64_t maxLen = 16;
        for (const auto& it : items) {
            bufs.emplace_back(it);
            maxLen = std::max<uint64_t>(maxLen, bufs.back().size());
        }
        std::vector<std::unique_ptr<GpuCtx>> ctxs;
        ctxs.push_back(std::make_unique<GpuCtx>(dev, (int)bufs.size(), maxLen, true));
        // the pool hands its streams out in turn: make contexts until one gets
        // the first one's stream again (at most 64 streams per device)
        for (int tries = 0; contexts == 2 && ctxs.size() < 2; tries++) {
            if (!ctxs[0]->streamShared() || tries > 64)
                throw std::runtime_error("gpu_data_profile_batch: no shared stream pool "
                                         "(EB_GPU_SHARED_STREAMS=0?)");
            auto c = std::make_unique<GpuCtx>(dev, (int)bufs.size(), maxLen, true);
            if (c->streamId() == ctxs[0]->streamId()) ctxs.push_back(std::move(c));
        }
        for (auto& c : ctxs) c->dataProfileReset();
        for (size_t i = 0; i < bufs.size(); i++) {
            GpuCtx& c = *ctxs[i % contexts];
            std::memset(c.hostBuf((int)i), 0xA5, c.slotStride());
            std::memcpy(c.hostBuf((int)i), bufs[i].data(), bufs[i].size());
            c.copyH2DAsync((int)i, c.slotStride());
            c.dataProfileDevAsync((int)i, bufs[i].size(), chunk);
        }
        py::list out;
        for (auto& c : ctxs) {
            auto acc = std::make_unique<DataProfileAcc>();
            c->dataProfileFetch(*acc);
            out.append(profileToDict(*acc));
        }
        return out;
    }, py::arg("items"), py::arg("chunk") = 4096, py::arg("dev") = 0,
       py::arg("contexts") = 1);

    // GB/s of ebDataProfileKernel on one len-byte buffer
    m.def("gpu_data_profile_bench_gbs",
          [](uint64_t len, int iters, int dev, const std::string& kind, uint64_t chunk) {
              const int k = kind == "random" ? 0 : kind == "zero-heavy" ? 1
                            : kind == "all-zero" ? 2 : -1;
              if (k < 0)
                  throw std::invalid_argument("gpu_data_profile_bench_gbs: kind must be "
                                              "random, zero-heavy or all-zero");
              py::gil_scoped_release rel;
              return gpuDataProfileBenchGBs(len, iters, dev, chunk, k);
          },
          py::arg("len"), py::arg("iters") = 50, py::arg("dev") = 0,
          py::arg("kind") = "random", py::arg("chunk") = 4096);

    // --- --verifydiag kernels; block_size 0 selects the plain kernel ---

    m.def("gpu_verify_diag", [](py::bytes data, uint64_t fileOff, uint64_t salt, int dev,
                                uint64_t blockSize, uint64_t mixLen) {
        std::string buf = data;
        GpuCtx ctx(dev, 1, std::max<uint64_t>(buf.size(), 16), true);
        std::memcpy(ctx.hostBuf(0), buf.data(), buf.size());
        if (!buf.empty()) ctx.copyH2DAsync(0, buf.size());
        ctx.syncStream();
        return diagToDict(blockSize ? ctx.verifyDiagMixDev(0, buf.size(), fileOff, salt,
                                                           blockSize, mixLen)
                                    : ctx.verifyDiagDev(0, buf.size(), fileOff, salt));
    }, py::arg("data"), py::arg("file_off"), py::arg("salt"), py::arg("dev") = 0,
       py::arg("block_size") = 0, py::arg("mix_len") = 0);

    // Like gpu_verify_batch: one slot and one async diag launch per
    // (data, file_off) item with no fetch in between, then two
    // fetchVerifyDiag calls, then (optionally) a synchronous diag of `then`
    // on the same context. Returns the records in that order. fetch_each
    // fetches after every item instead and returns one record per item (many
    // one-shot diagnoses on one context).
    m.def("gpu_verify_diag_batch", [](const std::vector<std::pair<py::bytes, uint64_t>>& items,
                                      uint64_t salt, int dev, uint64_t blockSize,
                                      uint64_t mixLen,
                                      std::optional<std::pair<py::bytes, uint64_t>> then,
                                      bool fetchEach) {
        if (items.empty()) throw std::invalid_argument("gpu_verify_diag_batch: no items");
        std::vector<std::string> bufs;
        uint64_t maxLen = 16;
        for (const auto& it : items) {
            bufs.emplace_back(it.first);
            maxLen = std::max<uint64_t>(maxLen, bufs.back().size());
        }
        std::string thenBuf;
        if (then) {
            thenBuf = then->first;
            maxLen = std::max<uint64_t>(maxLen, thenBuf.size());
        }
        GpuCtx ctx(dev, (int)bufs.size(), maxLen, true);
        auto launch = [&](int slot, const std::string& b, uint64_t fileOff) {
            std::memcpy(ctx.hostBuf(slot), b.data(), b.size());
            if (!b.empty()) ctx.copyH2DAsync(slot, b.size());
            if (blockSize)
                ctx.verifyDiagMixDevAsync(slot, b.size(), fileOff, salt, blockSize, mixLen);
            else
                ctx.verifyDiagDevAsync(slot, b.size(), fileOff, salt);
        };
        py::list out;
        for (size_t i = 0; i < bufs.size(); i++) {
            launch((int)i, bufs[i], items[i].second);
            if (fetchEach) out.append(diagToDict(ctx.fetchVerifyDiag()));
        }
        if (!fetchEach) {
            out.append(diagToDict(ctx.fetchVerifyDiag()));
            out.append(diagToDict(ctx.fetchVerifyDiag()));
        }
        if (then) {
            launch(0, thenBuf, then->second);
            out.append(diagToDict(ctx.fetchVerifyDiag()));
        }
        return out;
    }, py::arg("items"), py::arg("salt"), py::arg("dev") = 0, py::arg("block_size") = 0,
       py::arg("mix_len") = 0, py::arg("then") = py::none(), py::arg("fetch_each") = false);

    // like gpu_verify_bench (clean data, GB/s) for ebVerifyDiagKernel
    m.def("gpu_verify_diag_bench",
          [](uint64_t len, int iters, int dev) {
              py::gil_scoped_release rel;
              return gpuVerifyDiagBenchGBs(len, iters, dev);
          },
          py::arg("len"), py::arg("iters") = 50, py::arg("dev") = 0);

    // block_size 0 stands for len (one launch never exceeds a block)
    m.def("gpu_verify_mix_bench",
          [](uint64_t len, int iters, int dev, uint64_t blockSize, uint64_t mixLen) {
              py::gil_scoped_release rel;
              return gpuMixBenchGBs(len, iters, dev, blockSize ? blockSize : len, mixLen,
                                    false, false);
          },
          py::arg("len"), py::arg("iters") = 50, py::arg("dev") = 0,
          py::arg("block_size") = 0, py::arg("mix_len") = 0);
    // plain=true times ebFillChecksumKernel the same way, for comparison
    m.def("gpu_fill_mix_bench",
          [](uint64_t len, int iters, int dev, uint64_t blockSize, uint64_t mixLen,
             bool plain) {
              py::gil_scoped_release rel;
              return gpuMixBenchGBs(len, iters, dev, blockSize ? blockSize : len, mixLen,
                                    true, plain);
          },
          py::arg("len"), py::arg("iters") = 50, py::arg("dev") = 0,
          py::arg("block_size") = 0, py::arg("mix_len") = 0, py::arg("plain") = false);

    // Device CRC test helper: data plus `guard` sentinel bytes go into one
    // slot; returns the CRC the tile kernel + host fold give for len(data).
    m.def("gpu_crc", [](py::bytes data, const std::string& algo, int dev, uint64_t guard,
                        int sentinel) -> uint64_t {
        const bool is64 = algo == CRC64_NVME_NAME;
        CrcAlgo a = is64 ? CrcAlgo::CRC32C : crcAlgoFromName(algo);
        std::string buf = data;
        py::gil_scoped_release rel;
        const uint64_t total = buf.size() + guard;
        GpuCtx ctx(dev, 1, std::max<uint64_t>(total, 16), true);
        std::memcpy(ctx.hostBuf(0), buf.data(), buf.size());
        std::memset(ctx.hostBuf(0) + buf.size(), sentinel, guard);
        if (total) ctx.copyH2DAsync(0, total);
        ctx.syncStream();
        if (is64) return ctx.crc64Dev(0, buf.size());
        return ctx.crcDev(0, buf.size(), a);
    }, py::arg("data"), py::arg("algo"), py::arg("dev") = 0, py::arg("guard") = 0,
       py::arg("sentinel") = 0);
    // One context, CRC32C and CRC64NVME of the same buffer alternating
    // `rounds` times: [(crc32c, crc64nvme), ...]. The two trios keep separate
    // state on the context; this shows that neither disturbs the other.
    m.def("gpu_crc_interleaved", [](py::bytes data, int rounds, int dev) {
        std::string buf = data;
        std::vector<std::pair<uint32_t, uint64_t>> out;
        {
            py::gil_scoped_release rel;
            GpuCtx ctx(dev, 1, std::max<uint64_t>(buf.size(), 16), true);
            std::memcpy(ctx.hostBuf(0), buf.data(), buf.size());
            if (buf.size()) ctx.copyH2DAsync(0, buf.size());
            ctx.syncStream();
            for (int i = 0; i < rounds; i++) {
                uint32_t c32 = ctx.crcDev(0, buf.size(), CrcAlgo::CRC32C);
                out.emplace_back(c32, ctx.crc64Dev(0, buf.size()));
            }
        }
        return out;
    }, py::arg("data"), py::arg("rounds") = 2, py::arg("dev") = 0);
    // geometry of the device CRC kernel that serves `algo`
    m.def("gpu_crc_tile_bytes", [](const std::string& algo) {
        if (algo == CRC64_NVME_NAME) return gpuCrc64TileBytes();
        (void)crcAlgoFromName(algo);
        return gpuCrcTileBytes();
    }, py::arg("algo") = "CRC32C");
    m.def("gpu_crc_wave_bytes", [](const std::string& algo) {
        if (algo == CRC64_NVME_NAME) return gpuCrc64WaveBytes();
        (void)crcAlgoFromName(algo);
        return gpuCrcWaveBytes();
    }, py::arg("algo") = "CRC32C");

    m.def("gpu_verify_bench",
          [](uint64_t len, int iters, bool lds, int dev) {
              py::gil_scoped_release rel;
              return gpuVerifyBenchGBs(len, iters, lds, dev);
          },
          py::arg("len"), py::arg("iters") = 50, py::arg("lds") = false,
          py::arg("dev") = 0);

    m.def("gpu_fill_rand", [](uint64_t len, uint64_t seed, int dev, bool fast) {
        GpuCtx ctx(dev, 1, len, true);
        ctx.fillRandDev(0, len, seed, fast);
        ctx.copyD2HAsync(0, len);
        ctx.syncStream();
        return py::bytes(ctx.hostBuf(0), len);
    }, py::arg("len"), py::arg("seed"), py::arg("dev") = 0, py::arg("fast") = false);

    m.def("gpu_blockvar_refill", [](uint64_t len, uint64_t refillLen, uint64_t seed,
                                    int dev, bool fast) {
        GpuCtx ctx(dev, 1, len, true);
        std::memset(ctx.hostBuf(0), 0, len);
        ctx.copyH2DAsync(0, len);
        ctx.syncStream();
        ctx.blockVarRefillDev(0, len, refillLen, seed, fast);
        ctx.copyD2HAsync(0, len);
        ctx.syncStream();
        return py::bytes(ctx.hostBuf(0), len);
    }, py::arg("len"), py::arg("refill_len"), py::arg("seed"), py::arg("dev") = 0,
       py::arg("fast") = false);

    // Guarded --dedupepct / --compresspct fill: len+pad device bytes preset to
    // `sentinel`, one fillReduceDev of len bytes, all len+pad bytes returned.
    // then_blockvar_seed: a fast block-variance refill of the same len bytes
    // (half random) follows on the same context and is what comes back; it is
    // that context's fill call 1 iff fillReduceDev took no fill-call number.
    m.def("gpu_fill_reduce", [](uint64_t len, uint64_t firstChunk, uint64_t chunk,
                                uint64_t randBytes, int dedupePct, uint64_t pool,
                                uint64_t uniqSeed, uint64_t poolSeed, int dev, uint64_t pad,
                                int sentinel, std::optional<uint64_t> thenBlockVarSeed) {
        const uint64_t total = len + pad;
        GpuCtx ctx(dev, 1, std::max<uint64_t>(total, 16), true);
        std::memset(ctx.hostBuf(0), sentinel, total);
        if (total) ctx.copyH2DAsync(0, total);
        ctx.syncStream();
        ctx.fillReduceDev(0, len, firstChunk, chunk, randBytes, dedupePct, pool, uniqSeed,
                          poolSeed);
        if (thenBlockVarSeed) ctx.blockVarRefillDev(0, len, len / 2, *thenBlockVarSeed, true);
        std::memset(ctx.hostBuf(0), ~sentinel, total); // D2H must overwrite all of it
        if (total) ctx.copyD2HAsync(0, total);
        ctx.syncStream();
        return py::bytes(ctx.hostBuf(0), total);
    }, py::arg("len"), py::arg("first_chunk"), py::arg("chunk"), py::arg("rand_bytes"),
       py::arg("dedupe_pct"), py::arg("pool"), py::arg("uniq_seed"), py::arg("pool_seed"),
       py::arg("dev") = 0, py::arg("pad") = 0, py::arg("sentinel") = 0xA5,
       py::arg("then_blockvar_seed") = py::none());

    // --dedupeverify kernel: data goes into a one-slot context and its first
    // verify_len bytes (default: all of it) are verified in HBM, so bytes
    // behind verify_len lie directly behind the verified range in the slot.
    m.def("gpu_verify_reduce", [](py::bytes data, uint64_t fileOff, uint64_t firstChunk,
                                  uint64_t chunk, uint64_t randBytes, int dedupePct,
                                  uint64_t pool, uint64_t uniqSeed, uint64_t poolSeed, int dev,
                                  std::optional<uint64_t> verifyLen) {
        std::string buf = data;
        const uint64_t len = verifyLen ? *verifyLen : buf.size();
        if (len > buf.size())
            throw std::invalid_argument("gpu_verify_reduce: verify_len exceeds the data");
        GpuCtx ctx(dev, 1, std::max<uint64_t>(buf.size(), 16), true);
        std::memcpy(ctx.hostBuf(0), buf.data(), buf.size());
        if (!buf.empty()) ctx.copyH2DAsync(0, buf.size());
        ctx.syncStream();
        GpuVerifyResult r = ctx.verifyReduceDev(0, len, fileOff, firstChunk, chunk, randBytes,
                                                dedupePct, pool, uniqSeed, poolSeed);
        return py::make_tuple(r.numMismatches, r.firstBadFileOffset);
    }, py::arg("data"), py::arg("file_off"), py::arg("first_chunk"), py::arg("chunk"),
       py::arg("rand_bytes"), py::arg("dedupe_pct"), py::arg("pool"), py::arg("uniq_seed"),
       py::arg("pool_seed"), py::arg("dev") = 0, py::arg("verify_len") = py::none());

    // One slot and one async launch per (data, file_off, first_chunk) item with
    // no fetch in between; returns the results of two fetchVerifyResult calls.
    m.def("gpu_verify_reduce_batch",
          [](const std::vector<std::tuple<py::bytes, uint64_t, uint64_t>>& items, uint64_t chunk,
             uint64_t randBytes, int dedupePct, uint64_t pool, uint64_t uniqSeed,
             uint64_t poolSeed, int dev) {
        if (items.empty()) throw std::invalid_argument("gpu_verify_reduce_batch: no items");
        std::vector<std::string> bufs;
        uint64_t maxLen = 16;
        for (const auto& it : items) {
            bufs.emplace_back(std::get<0>(it));
            maxLen = std::max<uint64_t>(maxLen, bufs.back().size());
        }
        GpuCtx ctx(dev, (int)bufs.size(), maxLen, true);
        for (size_t i = 0; i < bufs.size(); i++) {
            std::memcpy(ctx.hostBuf((int)i), bufs[i].data(), bufs[i].size());
            if (!bufs[i].empty()) ctx.copyH2DAsync((int)i, bufs[i].size());
            ctx.verifyReduceDevAsync((int)i, bufs[i].size(), std::get<1>(items[i]),
                                     std::get<2>(items[i]), chunk, randBytes, dedupePct, pool,
                                     uniqSeed, poolSeed);
        }
        py::list out;
        for (int k = 0; k < 2; k++) {
            GpuVerifyResult r = ctx.fetchVerifyResult();
            out.append(py::make_tuple(r.numMismatches, r.firstBadFileOffset));
        }
        return out;
    }, py::arg("items"), py::arg("chunk"), py::arg("rand_bytes"), py::arg("dedupe_pct"),
       py::arg("pool"), py::arg("uniq_seed"), py::arg("pool_seed"), py::arg("dev") = 0);

    // like gpu_verify_mix_bench (clean data, GB/s) for ebVerifyReduceKernel
    m.def("gpu_reduce_verify_bench_gbs",
          [](uint64_t len, int iters, int dev, uint64_t chunk, uint64_t randBytes,
             int dedupePct) {
              py::gil_scoped_release rel;
              return gpuReduceVerifyBenchGBs(len, iters, dev, chunk, randBytes, dedupePct);
          },
          py::arg("len"), py::arg("iters") = 50, py::arg("dev") = 0, py::arg("chunk") = 4096,
          py::arg("rand_bytes") = 2048, py::arg("dedupe_pct") = 50);

    // Kernel micro-benchmark: bandwidth of the gfx950 fill/verify kernels and
    // the staging copies on one device buffer (GB/s, stream-synchronized).
    m.def("gpu_kernel_bench", [](uint64_t len, int iters, int dev) {
        GpuCtx ctx(dev, 1, len, true);
        auto timeIt = [&](auto&& fn) {
            fn(); // warmup
            ctx.syncStream();
            auto t0 = std::chrono::steady_clock::now();
            for (int i = 0; i < iters; i++) fn();
            ctx.syncStream();
            auto dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0)
                          .count();
            return (double)len * iters / dt / 1e9; // GB/s
        };
        py::dict d;
        d["fill_rand_gbps"] = timeIt([&] { ctx.fillRandDev(0, len, 42); });
        d["fill_fast_gbps"] = timeIt([&] { ctx.fillRandDev(0, len, 42, true); });
        d["blockvar_fast_gbps"] =
            timeIt([&] { ctx.blockVarRefillDev(0, len, len / 2, 9, true); });
        if (len % 16 == 0) { // --dedupepct 50 --compresspct 50 at the default chunk size
            uint64_t chunks = 0;
            d["fill_reduce_gbps"] = timeIt([&] {
                ctx.fillReduceDev(0, len, chunks, 4096, 2048, 50, REDUCE_POOL_CHUNKS, 42, 43);
                chunks += (len + 4095) / 4096;
            });
        }
        d["fill_checksum_gbps"] = timeIt([&] { ctx.fillChecksumDev(0, len, 0, 7); });
        d["blockvar_gbps"] = timeIt([&] { ctx.blockVarRefillDev(0, len, len / 2, 9); });
        ctx.fillChecksumDev(0, len, 0, 7);
        d["verify_gbps"] = timeIt([&] { (void)ctx.verifyChecksumDev(0, len, 0, 7); });
        if (len % 16 == 0) {
            d["crc32c_gbps"] = timeIt([&] { (void)ctx.crcDev(0, len, CrcAlgo::CRC32C); });
            d["crc64nvme_gbps"] = timeIt([&] { (void)ctx.crc64Dev(0, len); });
        }
        d["d2h_gbps"] = timeIt([&] { ctx.copyD2HAsync(0, len); ctx.syncStream(); });
        d["h2d_gbps"] = timeIt([&] { ctx.copyH2DAsync(0, len); ctx.syncStream(); });
        return d;
    }, py::arg("len") = (uint64_t)256 << 20, py::arg("iters") = 10, py::arg("dev") = 0);

    // Persistent GPU buffer ops for Python-side engines (S3): keeps one
    // GpuCtx alive so per-object verify/fill costs one H2D + kernel, not a
    // context setup. Used for the "on-GPU verify" S3 path (BASELINE config 5).
    py::class_<GpuCtx>(m, "GpuBufferOps")
        .def(py::init([](int dev, uint64_t bufSize) {
                 return std::make_unique<GpuCtx>(dev, 1, bufSize, true);
             }),
             py::arg("dev") = 0, py::arg("buf_size") = (uint64_t)64 << 20)
        .def("verify",
             [](GpuCtx& ctx, py::bytes data, uint64_t fileOff, uint64_t salt) {
                 std::string buf = data;
                 if (buf.size() > ctx.bufSize())
                     throw std::runtime_error("GpuBufferOps: data larger than buffer");
                 {
                     py::gil_scoped_release rel;
                     std::memcpy(ctx.hostBuf(0), buf.data(), buf.size());
                     ctx.copyH2DAsync(0, buf.size());
                     ctx.syncStream();
                 }
                 GpuVerifyResult r = ctx.verifyChecksumDev(0, buf.size(), fileOff, salt);
                 return py::make_tuple(r.numMismatches, r.firstBadFileOffset);
             },
             py::arg("data"), py::arg("file_off"), py::arg("salt"))
        .def("fill_checksum",
             [](GpuCtx& ctx, uint64_t len, uint64_t fileOff, uint64_t salt) {
                 if (len > ctx.bufSize())
                     throw std::runtime_error("GpuBufferOps: len larger than buffer");
                 py::gil_scoped_release rel;
                 ctx.fillChecksumDev(0, len, fileOff, salt);
                 ctx.copyD2HAsync(0, len);
                 ctx.syncStream();
                 py::gil_scoped_acquire acq;
                 return py::bytes(ctx.hostBuf(0), len);
             },
             py::arg("len"), py::arg("file_off"), py::arg("salt"))
        .def("fill_rand",
             [](GpuCtx& ctx, uint64_t len, uint64_t seed) {
                 if (len > ctx.bufSize())
                     throw std::runtime_error("GpuBufferOps: len larger than buffer");
                 py::gil_scoped_release rel;
                 ctx.fillRandDev(0, len, seed);
                 ctx.copyD2HAsync(0, len);
                 ctx.syncStream();
                 py::gil_scoped_acquire acq;
                 return py::bytes(ctx.hostBuf(0), len);
             },
             py::arg("len"), py::arg("seed"));

    // native S3/HTTP data plane: block transfers in C++ (SigV4 in Python)
    py::class_<HttpDataPlane>(m, "HttpDataPlane")
        .def(py::init<std::string, int, int, uint64_t, uint64_t>(),
             py::arg("host"), py::arg("port"), py::arg("dev") = -1,
             py::arg("max_block") = 1ULL << 23, py::arg("seed") = 0x243F6A88ULL)
        .def("get",
             [](HttpDataPlane& h, py::bytes req, uint64_t expect_len,
                uint64_t pattern_off, int64_t salt) {
                 std::string r = req;
                 std::tuple<int, uint64_t, uint64_t, uint64_t> out;
                 {
                     py::gil_scoped_release rel;
                     out = h.get(r, expect_len, pattern_off, salt);
                 }
                 return out;
             },
             py::arg("request"), py::arg("expect_len"),
             py::arg("pattern_off") = 0, py::arg("salt") = -1)
        .def("get_data",
             [](HttpDataPlane& h, py::bytes req, uint64_t max_len) {
                 std::string r = req;
                 std::pair<int, std::string> out;
                 {
                     py::gil_scoped_release rel;
                     out = h.getData(r, max_len);
                 }
                 return py::make_tuple(out.first, py::bytes(out.second));
             },
             py::arg("request"), py::arg("max_len") = 1ULL << 26)
        .def("put",
             [](HttpDataPlane& h, py::bytes reqHdrs, uint64_t len,
                uint64_t pattern_off, int64_t salt) {
                 std::string r = reqHdrs;
                 std::pair<int, std::string> out;
                 {
                     py::gil_scoped_release rel;
                     out = h.put(r, len, pattern_off, salt);
                 }
                 return py::make_tuple(out.first, out.second);
             },
             py::arg("request_headers"), py::arg("len"),
             py::arg("pattern_off") = 0, py::arg("salt") = -1)
        .def("body_crc",
             [](HttpDataPlane& h, uint64_t len, uint64_t pattern_off, int64_t salt,
                const std::string& algo) -> uint64_t {
                 if (algo == CRC64_NVME_NAME) {
                     py::gil_scoped_release rel;
                     return h.bodyCrc64(len, pattern_off, salt);
                 }
                 CrcAlgo a = crcAlgoFromName(algo);
                 py::gil_scoped_release rel;
                 return h.bodyCrc(len, pattern_off, salt, a);
             },
             py::arg("len"), py::arg("pattern_off") = 0, py::arg("salt") = -1,
             py::arg("algo") = "CRC32C")
        .def("close", &HttpDataPlane::close);
    m.def("http_dataplane_live", [] { return HttpDataPlane::liveCount().load(); });

    // native threaded S3 bench endpoint (data-plane throughput fixture)
    py::class_<S3BenchServer>(m, "S3BenchServer")
        .def(py::init<int, int64_t>(), py::arg("port") = 0, py::arg("salt") = -1)
        .def("port", &S3BenchServer::port)
        .def("stop", &S3BenchServer::stop,
             py::call_guard<py::gil_scoped_release>());

    py::class_<Engine>(m, "Engine")
        .def(py::init([](const py::dict& cfg) {
            return std::make_unique<Engine>(configFromDict(cfg));
        }))
        .def("prepare", &Engine::prepare, py::call_guard<py::gil_scoped_release>())
        .def("start_phase",
             [](Engine& e, int phaseCode) { e.startPhase((Phase)phaseCode); })
        .def("wait_phase_done", &Engine::waitPhaseDone,
             py::call_guard<py::gil_scoped_release>())
        .def("interrupt", &Engine::interrupt)
        .def("trigger_stonewall", &Engine::triggerStonewall)
        .def("poll",
             [](Engine& e) {
                 Engine::LivePoll lp = e.poll();
                 py::dict d;
                 d["entries"] = lp.entries;
                 d["bytes"] = lp.bytes;
                 d["iops"] = lp.iops;
                 d["workers_done"] = lp.workersDone;
                 d["workers_total"] = lp.workersTotal;
                 d["workers_with_error"] = lp.workersWithError;
                 d["elapsed_usec"] = lp.elapsedUSec;
                 d["stonewall_triggered"] = lp.stonewallTriggered;
                 d["lat_num_ios"] = lp.latNumIOs;
                 d["lat_sum_ios"] = lp.latSumIOs;
                 d["lat_num_entries"] = lp.latNumEntries;
                 d["lat_sum_entries"] = lp.latSumEntries;
                 return d;
             })
        .def("poll_workers",
             [](Engine& e) {
                 py::list out;
                 for (auto& w : e.workers) {
                     py::dict d;
                     d["rank"] = w->globalRank;
                     d["entries"] = w->liveOps.entries.load();
                     d["bytes"] = w->liveOps.bytes.load() + w->liveOpsReadMix.bytes.load();
                     d["iops"] = w->liveOps.iops.load() + w->liveOpsReadMix.iops.load();
                     out.append(d);
                 }
                 return out;
             })
        .def("finish_phase",
             [](Engine& e) {
                 std::vector<WorkerResult> rs;
                 {
                     py::gil_scoped_release rel;
                     rs = e.finishPhase();
                 }
                 py::list out;
                 for (auto& r : rs) out.append(resultToDict(r));
                 return out;
             })
        // read-only copy of worker local_rank's device slot ring:
        // (num_slots, slot_stride, bytes); raises while a phase is running
        .def("gpu_slots",
             [](Engine& e, int localRank) {
                 Engine::GpuSlotsSnapshot snap;
                 {
                     py::gil_scoped_release rel;
                     snap = e.gpuSlots(localRank);
                 }
                 return py::make_tuple(snap.numSlots, snap.slotStride,
                                       py::bytes(snap.bytes.data(), snap.bytes.size()));
             },
             py::arg("local_rank") = 0)
        // [(stream_id, shared)] per local worker rank: which HIP stream each
        // worker's context enqueues into; raises while a phase is running
        .def("gpu_streams",
             [](Engine& e) {
                 py::list out;
                 for (auto& s : e.gpuStreams()) out.append(py::make_tuple(s.first, s.second));
                 return out;
             })
        // sequence number of the current (or last) phase: 0 before the first
        // start_phase, +1 per start_phase; the per-phase seeds derive from it
        .def_property_readonly("phase_seq", [](Engine& e) { return e.phaseSeq; })
        .def("planned_work", [](Engine& e, int phaseCode) {
            auto pw = e.plannedWork((Phase)phaseCode);
            return py::make_tuple(pw.first, pw.second);
        });

    // phase code constants (wire-stable)
    py::dict phases;
    phases["IDLE"] = (int)Phase::IDLE;
    phases["TERMINATE"] = (int)Phase::TERMINATE;
    phases["MKDIRS"] = (int)Phase::MKDIRS;
    phases["WRITE"] = (int)Phase::WRITE;
    phases["READ"] = (int)Phase::READ;
    phases["STAT"] = (int)Phase::STAT;
    phases["RMFILES"] = (int)Phase::RMFILES;
    phases["RMDIRS"] = (int)Phase::RMDIRS;
    phases["SYNC"] = (int)Phase::SYNC;
    phases["DROPCACHES"] = (int)Phase::DROPCACHES;
    phases["NETBENCH"] = (int)Phase::NETBENCH;
    m.attr("PHASES") = phases;
}
