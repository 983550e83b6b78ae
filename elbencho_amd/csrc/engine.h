// The elbencho_amd I/O engine: multithreaded block/file/dir benchmark core.
//
// MI355X-native counterpart of the reference's LocalWorker/WorkerManager
// machinery (/root/reference/source/workers/LocalWorker.{h,cpp},
// WorkerManager.{h,cpp}) — independent design:
//   - phase lifecycle driven from Python (start/poll/wait/finish), worker
//     threads spawned per phase behind a start gate,
//   - io_uring (raw syscalls) instead of libaio for async depth,
//   - GPU staging through GpuCtx (HIP streams + gfx950 kernels, see gpu.h),
//   - stonewall ("first done") snapshots taken by the first finisher reading
//     peers' relaxed atomics.

#pragma once

#include <chrono>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "common.h"
#include "dataprofile.h"
#include "gpu.h"
#include "histogram.h"
#include "offsetgen.h"
#include "opslog.h"
#include "rand.h"
#include "rate.h"

namespace eb {

struct EngineConfig {
    std::vector<std::string> paths;
    PathType pathType = PathType::FILE;

    int numThreads = 1;
    int rankOffset = 0;        // global rank of this instance's worker 0
    int numDataSetThreads = 1; // total workers across all instances sharing the dataset

    uint64_t numDirs = 0;  // dir mode: dirs per thread
    uint64_t numFiles = 0; // dir mode: files per dir (per thread)
    uint64_t fileSize = 0;
    uint64_t blockSize = 1ULL << 20;
    int ioDepth = 1;

    bool directIO = false;
    bool random = false;
    bool randAligned = true;
    uint64_t randAmount = 0; // bytes per instance; 0 = dataset size
    bool strided = false;
    bool backward = false;

    bool truncate = false;
    uint64_t truncToSize = UINT64_MAX; // UINT64_MAX = off
    bool preallocFile = false;
    bool fsyncPerFile = false;

    int64_t verifySalt = -1; // -1 = off
    int verifyMixPct = -1;   // --verifymixpct: -1 = plain --verify pattern
    bool verifyDiag = false; // --verifydiag: classify what a verify failure found
    bool verifyDirect = false;
    bool readInline = false;  // read each file back right after writing it
    bool statInline = false;  // fstat right after open in dir mode
    int blockVarPct = 100;
    // --dedupepct / --compresspct: write payloads with set reduction ratios
    // (on iff either percentage is > 0; see fillReduceCPU)
    int dedupePct = 0;
    int compressPct = 0;
    uint64_t dedupeChunk = 4096;
    // --dedupeverify SALT: reduce pattern keyed by (SALT, file, file offset)
    // and checked on read; < 0 off. Needs dedupePct / compressPct > 0.
    int64_t reduceVerifySalt = -1;
    // --dataprofile: READ phases profile what they read (dataprofile.h), in
    // chunks of dedupeChunk bytes
    bool dataProfile = false;
    std::string blockVarAlgo = "fast";
    std::string randAlgo = "fast";

    int rwMixPct = 0;     // % of blocks read instead of written in a write phase
    int rwMixThreads = 0; // first N threads of a write phase only read

    bool useMmap = false;
    int fadviseFlags = 0;  // POSIX_FADV_* bitmask-ish (applied in order)
    int madviseFlags = 0;  // MADV_* combined
    int flockMode = 0;     // 0 none, 1 range, 2 full file

    std::string opsLogPath;
    bool opsLogLock = false;

    std::vector<int> cpuCores;  // round-robin thread->core binding
    std::vector<int> numaZones; // round-robin thread->NUMA-zone binding

    // netbench (service-only TCP request/response benchmark)
    bool netbenchIsServer = false;
    std::vector<std::string> netbenchServers; // "host" or "host:port"
    int netbenchPort = 2611;   // service port + 1000 convention
    int netbenchNumConns = 0;  // server: total client connections to expect
    uint64_t respSize = 1;
    int sendBufSize = 0, recvBufSize = 0;
    std::vector<std::string> netDevs; // --netdevs round-robin client binding

    // custom tree mode (reference PathStore / --treefile):
    // dirs + (relpath, size) files under paths[0]; files >= shareSize are
    // range-sliced across ranks, smaller ones distributed round-robin.
    std::vector<std::string> treeDirs;
    std::vector<std::pair<std::string, uint64_t>> treeFiles;
    uint64_t shareSize = 0;
    // assign shared-file blocks round-robin to ranks instead of consecutive
    // ranges (reference --treeroundrob, PathStore getWorkerSublistSharedRoundRobin)
    bool treeRoundRobin = false;
    // randomize each worker's custom-tree processing order (reference
    // --treerand, PathStore randomShuffle)
    bool treeRandomize = false;

    std::vector<int> gpuIDs; // empty = CPU buffers only
    bool gpuPinnedHostBufs = true;

    bool measureLat = false;
    uint64_t limitReadBps = 0;
    uint64_t limitWriteBps = 0;

    bool ignoreDelErrors = false;
    bool dirSharing = false;
    bool infiniteLoop = false;

    // MI355X extension (--dynslice): workers pull blocks from one shared
    // atomic cursor instead of static fair-share slices — removes straggler
    // skew at phase end (the slowest of N static slices defines the phase
    // time). Single-instance sequential workloads only; aggregate coverage
    // is identical, per-worker attribution becomes work actually done.
    bool dynamicSlice = false;

    uint64_t benchSeed = 0x243F6A8885A308D3ULL; // per-run; Python sets per iteration
};

// --dedupepct / --compresspct seeds: uniq differs per worker and phase, pool
// depends on the run's seed alone (shared by all workers, files and services)
struct ReduceSeeds {
    uint64_t uniq = 0, pool = 0;
};

struct WorkerResult {
    int rank = 0; // global rank
    uint64_t elapsedUSec = 0;
    LiveOpsSnapshot total;
    LiveOpsSnapshot stonewall;
    LiveOpsSnapshot totalReadMix;     // reads done within a write phase
    LiveOpsSnapshot stonewallReadMix;
    uint64_t stonewallElapsedUSec = 0;
    std::vector<uint64_t> ioLatVec;
    std::vector<uint64_t> entryLatVec;
    std::vector<uint64_t> ioLatReadMixVec;
    std::vector<uint64_t> entryLatReadMixVec;
    std::string error;
    // --dataprofile: what this worker read in a READ phase; null when the
    // option is off, in other phases and when the worker ended in an error
    std::shared_ptr<DataProfileAcc> profile;
};

class Engine;

// One benchmark worker = one OS thread (+ its GPU stream when GPU mode).
class Worker {
public:
    Worker(Engine& engine, int localRank);
    ~Worker();

    void threadMain();

    AtomicLiveOps liveOps;
    AtomicLiveOps liveOpsReadMix; // rwmix reads within a write phase
    LiveOpsSnapshot stonewallOps;
    LiveOpsSnapshot stonewallOpsReadMix;
    uint64_t stonewallElapsedUSec = 0;

    // histograms are worker-private until the thread is joined; the live
    // stats poller reads only these running-average atomics
    std::atomic<uint64_t> liveIoLatNum{0}, liveIoLatSum{0};
    std::atomic<uint64_t> liveEntryLatNum{0}, liveEntryLatSum{0};

    LatencyHistogram ioLat;
    LatencyHistogram entryLat;
    LatencyHistogram ioLatReadMix;
    LatencyHistogram entryLatReadMix;

    uint64_t elapsedUSec = 0;
    std::string error;
    int localRank;
    int globalRank;
    bool dedicatedReader = false; // rwmix role (read by Engine::onWorkerDone)

    // Clear all per-phase counters/histograms before the next phase reuses
    // this (persistent) worker. Called from the engine thread while the
    // worker is parked at the phase gate.
    void resetPhaseStats();

    // --dataprofile: the finished phase's profile (set by the worker thread
    // before it reports done, read by Engine::finishPhase)
    std::shared_ptr<DataProfileAcc> profileResult;

    // this worker's GPU context (nullptr without --gpuids or before its first
    // data phase); only for use while the worker is parked at the phase gate
    GpuCtx* gpuCtx() const { return gpu.get(); }

private:
    using Clock = std::chrono::steady_clock;

    void runPhase();
    void checkInterrupt();

    // phase bodies
    void fileModeBlocks(bool isWrite);
    void fileModeBlocksGpuMmap(bool isWrite);
    void fileModeBlocksUring(bool isWrite);
    void fileModeDelete();
    void fileModeStat();
    void dirModeMkdirs();
    void dirModeRmdirs();
    void dirModeFiles(Phase phase);
    void customTreeDirs(Phase phase);
    void customTreeFiles(Phase phase);
    void netbenchServer();
    void netbenchClient();
    void anyModeSync();
    void anyModeDropCaches();

    // dir/custom-tree async engine (reference parity: aioBlockSized applies
    // in every rw mode, LocalWorker.cpp:1210-1379): one io_uring context per
    // phase, reused across files; processes one file's offset stream at
    // cfg.ioDepth. Defined in engine.cpp.
    struct FileUring;
    void uringFileBlocks(FileUring& u, int fd, const std::string& path,
                         OffsetGen& gen, bool phaseIsWrite, bool rwMixActive,
                         bool allMixRead, bool checkMixReads);

    // Small-file metadata pipeline (--iodepth, dir mode, fileSize <=
    // blockSize): open -> write/read -> close as LINKED io_uring chains on
    // direct descriptors, `iodepth` whole files in flight per thread.
    // Returns false if the kernel lacks the required ops (caller falls
    // back to the per-file engine).
    bool dirModeSmallFileUring(bool isWrite);

    // STAT/RMFILES phases at --iodepth: statx/unlinkat pipelined through
    // the ring (reference aio covers data ops only).
    void dirModeMetaUring(Phase phase);

    // per-block helpers (sync path)
    void addIoLat(uint64_t us, bool readMix = false)
    {
        (readMix ? ioLatReadMix : ioLat).add(us);
        liveIoLatNum.fetch_add(1, std::memory_order_relaxed);
        liveIoLatSum.fetch_add(us, std::memory_order_relaxed);
    }
    // rwmix decision: keep reads/total at rwMixPct (write phase only)
    bool rwMixDecideRead(); // defined in engine.cpp (needs Engine)
    void applyBinding();
    bool rwBalancerActive() const;
    void rwBalanceWait(bool isRead, uint64_t nextLen); // throttle to the byte ratio
    void rwBalanceAccount(bool isRead, uint64_t len);
    void addEntryLat(uint64_t us)
    {
        entryLat.add(us);
        liveEntryLatNum.fetch_add(1, std::memory_order_relaxed);
        liveEntryLatSum.fetch_add(us, std::memory_order_relaxed);
    }
    void preWriteFill(int slot, uint64_t len, uint64_t fileOff);
    void postReadCheck(int slot, uint64_t len, uint64_t fileOff);
    // verify steps shared by the read paths (plain, --verifymixpct, --verifydiag)
    void gpuVerifyAsync(int slot, uint64_t len, uint64_t fileOff);
    void gpuVerifyFetch();     // throws WorkerError on a mismatch
    void gpuVerifyDropStale(); // forget what a failed phase left unfetched
    // slot: the I/O slot the block belongs to (--dedupeverify takes the file
    // key from it); buf need not be that slot's host buffer
    void cpuVerify(int slot, const char* buf, uint64_t len, uint64_t fileOff);
    // --dedupeverify: the seeds of the file that the slot's block belongs to
    void setSlotFileKey(int slot, uint64_t fileKey);
    void setAllSlotFileKeys(uint64_t fileKey);
    // --dataprofile steps of the read paths; no-ops unless `profiling`
    void profileGpuAsync(int slot, uint64_t len);
    void profileCpu(const char* buf, uint64_t len);
    ssize_t blockIO(bool isWrite, int fd, int slot, uint64_t len, uint64_t fileOff,
                    char* mmapBase = nullptr, const std::string* path = nullptr);
    void verifyDirectReadback(int fd, int slot, uint64_t len, uint64_t fileOff);

    // setup
    void allocBuffers();
    void setupGpu();
    std::unique_ptr<OffsetGen> makeOffsetGen(uint64_t myRangeStart, uint64_t myRangeLen);
    void fairShareSlice(uint64_t totalLen, uint64_t& myStart, uint64_t& myLen) const;

    Engine& eng;
    std::vector<char*> hostBufs; // CPU-owned unless GPU mode (then GpuCtx owns)
    bool ownHostBufs = false;
    char* scratchBuf = nullptr;  // verify-direct readback buffer
    uint64_t rwMixOps = 0, rwMixReads = 0;
    bool isDedicatedReader = false; // rwMixThreads role
    std::unique_ptr<GpuCtx> gpu;
    std::unique_ptr<RandAlgo> rng;        // offsets
    std::unique_ptr<RandAlgo> fillRng;    // block variance fill
    // --dedupepct / --compresspct: number of the next chunk this worker
    // generates (0 at the start of a phase and of every --infloop pass)
    uint64_t reduceNextChunk = 0;
    ReduceSeeds reduceSeed;
    // --dedupeverify: per I/O slot, the seeds of the file whose block the slot
    // holds (several files are in flight per worker on the io_uring paths)
    std::vector<ReduceSeeds> slotReduceSeed;
    // --dataprofile: on in this phase; host accumulator (CPU-profiled blocks,
    // and the device state after the phase's one fetch)
    bool profiling = false;
    std::unique_ptr<DataProfileAcc> profileAcc;
    RateLimiter rateLimiter;
};

// Shared per-phase state + the engine facade exposed to Python.
class Engine {
public:
    explicit Engine(EngineConfig cfg);
    ~Engine();

    // Resolve path type specifics (bdev sizes, existing file sizes).
    void prepare();

    void startPhase(Phase phase);
    bool waitPhaseDone(int64_t timeoutMs); // true when all workers finished
    void interrupt();
    void triggerStonewall(); // remote stonewall propagation (master RPC)

    struct LivePoll {
        uint64_t entries, bytes, iops;
        int workersDone, workersTotal, workersWithError;
        uint64_t elapsedUSec;
        bool stonewallTriggered;
        uint64_t latNumIOs, latSumIOs, latNumEntries, latSumEntries;
    };
    LivePoll poll();

    std::vector<WorkerResult> finishPhase(); // joins threads, returns results

    // planned work for dryrun/progress: {entries, bytes} for this instance
    std::pair<uint64_t, uint64_t> plannedWork(Phase phase) const;

    const EngineConfig& config() const { return cfg; }

    // Read-only snapshot of one worker's device slot ring (test/diagnostic
    // hook): looks at the persistent worker's context first, then at a
    // context parked in gpuCtxCache. Throws while a phase is running (never
    // blocks) and when that worker has no GPU context.
    struct GpuSlotsSnapshot {
        int numSlots = 0;
        uint64_t slotStride = 0;
        std::vector<char> bytes; // numSlots * slotStride
    };
    GpuSlotsSnapshot gpuSlots(int localRank);

    // Which HIP stream each local worker's context enqueues into (test/
    // diagnostic hook): {GpuCtx::streamId(), GpuCtx::streamShared()} per local
    // rank, contexts looked up as gpuSlots does. No device work. Throws while
    // a phase is running and when a worker has no GPU context.
    std::vector<std::pair<uint64_t, bool>> gpuStreams();

    // ---- shared state visible to workers ----
    EngineConfig cfg;
    Phase currentPhase = Phase::IDLE;
    std::atomic<bool> interruptFlag{false};
    std::atomic<int> workersDone{0};
    std::atomic<int> workersWithError{0};
    std::atomic<bool> stonewallTriggered{false};
    std::chrono::steady_clock::time_point phaseStart;

    // Phase gate for PERSISTENT worker threads (reference analogue:
    // WorkerManager condvar barrier + Worker::waitForNextPhase): threads are
    // spawned once on the first startPhase and then park here between
    // phases — no per-pass thread spawn/join, buffer alloc or RNG prefill
    // (this was ~9% of the measured headline pass in round 1).
    std::mutex gateMtx;
    std::condition_variable gateCv;
    uint64_t phaseGen = 0;       // bumped per startPhase (guarded by gateMtx)
    bool terminateRequested = false;

    std::mutex doneMtx;
    std::condition_variable doneCv;

    std::vector<std::unique_ptr<Worker>> workers;

    // rwmix byte-ratio balancer state (reference RateLimiterRWMixThreads):
    // active when both --rwmixthr and --rwmixpct are set; holds read bytes at
    // rwMixPct% of the combined volume with blockSize*peerThreads headroom
    std::atomic<uint64_t> rwBalBytesRead{0};
    std::atomic<uint64_t> rwBalBytesWrite{0};
    std::atomic<int> rwReadersDone{0};
    std::atomic<int> rwWritersDone{0};
    int phaseSeq = 0; // bumped per startPhase; decorrelates iteration streams

    // --dynslice shared block cursor (reset every startPhase)
    std::atomic<uint64_t> dynCursor{0};

    // resolved at prepare()
    std::vector<uint64_t> resolvedFileSizes; // per path (file/bdev mode)
    uint64_t effFileSize = 0;                // uniform stripe unit

    // --verifymixpct, fixed at construction: the first verifyMixLen bytes of
    // every block hold hashed words (floor(blockSize * pct / 100), rounded
    // down to a multiple of 8)
    bool verifyMix = false;
    uint64_t verifyMixLen = 0;

    // --dedupepct / --compresspct, fixed at construction: on iff either
    // percentage is > 0; the first reduceRandBytes bytes of every chunk are
    // random, the rest zero
    bool reduce = false;
    uint64_t reduceRandBytes = 0;
    // --dedupeverify on (then reduce is on too); dataVerify: reads are checked,
    // by --verify or by --dedupeverify
    bool reduceVerify = false;
    bool dataVerify = false;
    // --dataprofile on (fixed at construction)
    bool dataProfile = false;

    // GPU contexts cached across phases (hipMalloc + pinned allocs are
    // expensive; reusing them keeps phase setup off the measured path)
    std::mutex gpuCacheMtx;
    std::vector<std::unique_ptr<GpuCtx>> gpuCtxCache;

    OpsLogger opsLog;

    // mmap+GPU zero-copy path: per-path registered file mappings, cached
    // across phases (hipHostRegister of multi-GiB regions is expensive)
    struct MappedReg {
        char* base = nullptr;
        uint64_t len = 0;
        bool registered = false;
        bool writable = false;
    };
    std::mutex mmapRegMtx;
    std::map<std::string, MappedReg> mmapRegCache;
    MappedReg& getMappedReg(const std::string& path, uint64_t len, bool writable);
    void dropMappedRegs();

    // netbench server: worker 0 accepts all connections, peers take a subset
    std::mutex nbMtx;
    std::condition_variable nbCv;
    std::vector<int> nbConns;
    bool nbAcceptDone = false;

    void onWorkerDone(Worker& w, bool hadError);

private:
    std::vector<std::thread> threads;
    bool phaseRunning = false;
};

// CPU-side integrity checksum helpers (pattern: u64 at 8-aligned file offset
// o has value o + salt, little-endian; arbitrary alignment handled bytewise).
void fillChecksumCPU(char* buf, uint64_t len, uint64_t fileOff, uint64_t salt);
// returns UINT64_MAX when ok, else file offset of first mismatching byte
uint64_t verifyChecksumCPU(const char* buf, uint64_t len, uint64_t fileOff, uint64_t salt);

// --verifymixpct variants: the u64 at 8-aligned file offset o has value
// splitmix64(o + salt) if (o % blockSize) < mixLen, else o + salt. blockSize
// (> 0) and mixLen are multiples of 8.
void fillChecksumMixCPU(char* buf, uint64_t len, uint64_t fileOff, uint64_t salt,
                        uint64_t blockSize, uint64_t mixLen);
uint64_t verifyChecksumMixCPU(const char* buf, uint64_t len, uint64_t fileOff, uint64_t salt,
                              uint64_t blockSize, uint64_t mixLen);

// --dedupepct / --compresspct pattern. A worker numbers the chunks (chunkBytes
// each, a power of two >= 16) it generates in a phase n = 0, 1, 2, ...; with
// mix = splitmix64 of a value and GOLD = 0x9E3779B97F4A7C15, all mod 2^64:
//   dup(n) = ((n+1) * dedupePct) / 100 > (n * dedupePct) / 100
//   key(n) = dup(n) ? mix(poolSeed + (mix(uniqSeed ^ n) % pool))
//                   : mix(uniqSeed ^ mix(n))
//   8-byte word i of chunk n = (8*i < randBytes) ? mix(key(n) + i * GOLD) : 0
// Pool chunks (one of `pool` contents, the same for every worker of a run)
// deduplicate; the zero tail compresses. fillReduceCPU writes chunks
// firstChunk, firstChunk+1, ... into buf and cuts the last one at len (any
// len); randBytes is a multiple of 16 and <= chunkBytes, pool >= 1.
constexpr uint64_t REDUCE_POOL_CHUNKS = 256;
void fillReduceCPU(char* buf, uint64_t len, uint64_t firstChunk, uint64_t chunkBytes,
                   uint64_t randBytes, int dedupePct, uint64_t pool, uint64_t uniqSeed,
                   uint64_t poolSeed);
// the seeds a worker uses in the phase with sequence number phaseSeq
ReduceSeeds reduceSeeds(uint64_t benchSeed, int phaseSeq, int globalRank);

// --dedupeverify: the content of a file is a function of (salt, file key, file
// offset) alone. The block at file offset o (a multiple of chunkBytes) holds
// chunks o / chunkBytes, o / chunkBytes + 1, ... of the pattern above with
//   poolSeed = mix(salt ^ REDUCE_VERIFY_POOL_XOR)            (the same for every file)
//   uniqSeed = mix(mix(salt ^ REDUCE_VERIFY_UNIQ_XOR) + fileKey * GOLD)
// The file key is the path's index in file/bdev mode, the file's index in the
// tree file list in custom-tree mode and reduceDirFileKey in directory mode.
constexpr uint64_t REDUCE_VERIFY_POOL_XOR = 0xA0761D6478BD642FULL;
constexpr uint64_t REDUCE_VERIFY_UNIQ_XOR = 0xE7037ED1A0B428DBULL;
ReduceSeeds reduceVerifySeeds(uint64_t salt, uint64_t fileKey);
// key of r{rank}/d{dir}/r{rank}-f{file}: mix(mix(mix(rank + 1) ^ dir) ^ file)
uint64_t reduceDirFileKey(uint64_t rank, uint64_t dir, uint64_t file);
// Compares buf, which lies at file offset fileOff, with what fillReduceCPU
// writes for the same arguments (any len; a cut last word is compared over
// the bytes it has). Returns the number of mismatching 8-byte words and the
// file offset of the first one (fileOff + 8 * word index), UINT64_MAX if none:
// the result of GpuCtx::verifyReduceDev.
GpuVerifyResult verifyReduceCPU(const char* buf, uint64_t len, uint64_t fileOff,
                                uint64_t firstChunk, uint64_t chunkBytes, uint64_t randBytes,
                                int dedupePct, uint64_t pool, uint64_t uniqSeed,
                                uint64_t poolSeed);

// --verifydiag on a host buffer: the contract of GpuVerifyDiag (gpu.h), added
// into `acc` (a default-constructed record is empty). Any alignment; a word
// the range holds only in part is compared on those bytes and counts as OTHER.
void verifyDiagCPU(const char* buf, uint64_t len, uint64_t fileOff, uint64_t salt,
                   GpuVerifyDiag& acc);
void verifyDiagMixCPU(const char* buf, uint64_t len, uint64_t fileOff, uint64_t salt,
                      uint64_t blockSize, uint64_t mixLen, GpuVerifyDiag& acc);
// what a failed verify appends to its message: "; diagnosis: ..."
std::string verifyDiagText(const GpuVerifyDiag& d);

} // namespace eb
