// elbencho_amd engine implementation.
//
// Independent MI355X-native implementation of the behavior of the reference's
// LocalWorker I/O engine (/root/reference/source/workers/LocalWorker.cpp):
// same work partitioning and directory layout contract (fair-share block
// split: fileModeIterateFilesSeq :3597; per-worker random subrange :3511;
// dir layout "r{rank}/d{dir}/r{rank}-f{file}" :3097; bench path round-robin
// (rank+dirIdx)%numPaths :3111), re-designed around io_uring + HIP streams.

#include "engine.h"

#include <fcntl.h>
#include <linux/fs.h>
#include <pthread.h>
#include <sched.h>
#include <sys/ioctl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <unistd.h>

#include <algorithm>
#include <random>
#include <cerrno>
#include <cstdio>
#include <cstring>

#include "netbench.h"
#include "uring.h"

namespace eb {

static constexpr uint64_t INTERRUPT_CHECK_INTERVAL = 128;

// ---------------------------------------------------------------------------
// integrity checksum pattern (CPU side)
// u64 at 8-aligned file offset o has little-endian value (o + salt).
// ---------------------------------------------------------------------------

static inline uint64_t checksumValueAt(uint64_t alignedOff, uint64_t salt)
{
    return alignedOff + salt;
}

void fillChecksumCPU(char* buf, uint64_t len, uint64_t fileOff, uint64_t salt)
{
    // pos/end are compared by difference only, so a range that ends at (or
    // wraps past) 2^64 is handled like any other
    uint64_t pos = fileOff;
    uint64_t end = fileOff + len;

    // unaligned head: bytes of the u64 containing fileOff
    while (pos != end && (pos & 7)) {
        uint64_t v = checksumValueAt(pos & ~7ULL, salt);
        buf[pos - fileOff] = (char)((v >> (8 * (pos & 7))) & 0xff);
        pos++;
    }
    // aligned middle
    while (end - pos >= 8) {
        uint64_t v = checksumValueAt(pos, salt);
        std::memcpy(buf + (pos - fileOff), &v, 8);
        pos += 8;
    }
    // tail
    while (pos != end) {
        uint64_t v = checksumValueAt(pos & ~7ULL, salt);
        buf[pos - fileOff] = (char)((v >> (8 * (pos & 7))) & 0xff);
        pos++;
    }
}

uint64_t verifyChecksumCPU(const char* buf, uint64_t len, uint64_t fileOff, uint64_t salt)
{
    uint64_t pos = fileOff;
    uint64_t end = fileOff + len;

    while (pos != end && (pos & 7)) {
        uint64_t v = checksumValueAt(pos & ~7ULL, salt);
        if (buf[pos - fileOff] != (char)((v >> (8 * (pos & 7))) & 0xff)) return pos;
        pos++;
    }
    while (end - pos >= 8) {
        uint64_t v = checksumValueAt(pos, salt);
        uint64_t got;
        std::memcpy(&got, buf + (pos - fileOff), 8);
        if (got != v) { // find exact byte
            for (int b = 0; b < 8; b++)
                if (((got >> (8 * b)) & 0xff) != ((v >> (8 * b)) & 0xff)) return pos + b;
        }
        pos += 8;
    }
    while (pos != end) {
        uint64_t v = checksumValueAt(pos & ~7ULL, salt);
        if (buf[pos - fileOff] != (char)((v >> (8 * (pos & 7))) & 0xff)) return pos;
        pos++;
    }
    return UINT64_MAX;
}

// ---------------------------------------------------------------------------
// --verifymixpct pattern (CPU side)
// u64 at 8-aligned file offset o holds splitmix64(o + salt) if
// (o % blockSize) < mixLen, else the plain (o + salt). blockSize and mixLen are
// multiples of 8, so a word is never split between the two kinds.
// ---------------------------------------------------------------------------

static inline uint64_t splitmix64Of(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

static inline uint64_t mixValueAt(uint64_t alignedOff, uint64_t salt, uint64_t rel,
                                  uint64_t mixLen)
{
    uint64_t x = alignedOff + salt;
    return (rel < mixLen) ? splitmix64Of(x) : x;
}

// --dedupepct / --compresspct pattern (CPU side; stated at engine.h)
static inline uint64_t reduceKeyCPU(uint64_t n, uint64_t d, uint64_t pool, uint64_t uniqSeed,
                                    uint64_t poolSeed)
{
    const bool dup = ((n + 1) * d) / 100 > (n * d) / 100;
    return dup ? splitmix64Of(poolSeed + (splitmix64Of(uniqSeed ^ n) % pool))
               : splitmix64Of(uniqSeed ^ splitmix64Of(n));
}

void fillReduceCPU(char* buf, uint64_t len, uint64_t firstChunk, uint64_t chunkBytes,
                   uint64_t randBytes, int dedupePct, uint64_t pool, uint64_t uniqSeed,
                   uint64_t poolSeed)
{
    constexpr uint64_t GOLD = 0x9E3779B97F4A7C15ULL;
    const uint64_t d = (uint64_t)dedupePct;
    uint64_t n = firstChunk;
    for (uint64_t pos = 0; pos < len; pos += chunkBytes, n++) {
        const uint64_t chunkLen = std::min(chunkBytes, len - pos);
        const uint64_t randLen = std::min(randBytes, chunkLen);
        const uint64_t key = reduceKeyCPU(n, d, pool, uniqSeed, poolSeed);
        for (uint64_t o = 0; o < randLen; o += 8) {
            const uint64_t v = splitmix64Of(key + (o / 8) * GOLD);
            std::memcpy(buf + pos + o, &v, std::min<uint64_t>(8, randLen - o));
        }
        std::memset(buf + pos + randLen, 0, chunkLen - randLen);
    }
}

ReduceSeeds reduceSeeds(uint64_t benchSeed, int phaseSeq, int globalRank)
{
    const uint64_t phaseSeed = benchSeed + 0x9E3779B97F4A7C15ULL * (uint64_t)phaseSeq;
    ReduceSeeds s;
    s.uniq = splitmix64Of(phaseSeed ^ (0xD1B54A32D192ED03ULL * (uint64_t)(globalRank + 1)));
    s.pool = splitmix64Of(benchSeed ^ 0x5DED0C0DE5EED001ULL);
    return s;
}

GpuVerifyResult verifyReduceCPU(const char* buf, uint64_t len, uint64_t fileOff,
                                uint64_t firstChunk, uint64_t chunkBytes, uint64_t randBytes,
                                int dedupePct, uint64_t pool, uint64_t uniqSeed,
                                uint64_t poolSeed)
{
    constexpr uint64_t GOLD = 0x9E3779B97F4A7C15ULL;
    GpuVerifyResult r{0, UINT64_MAX};
    uint64_t n = firstChunk;
    for (uint64_t pos = 0; pos < len; pos += chunkBytes, n++) {
        const uint64_t chunkLen = std::min(chunkBytes, len - pos);
        const uint64_t key = reduceKeyCPU(n, (uint64_t)dedupePct, pool, uniqSeed, poolSeed);
        for (uint64_t o = 0; o < chunkLen; o += 8) {
            const uint64_t want = (o < randBytes) ? splitmix64Of(key + (o / 8) * GOLD) : 0;
            if (std::memcmp(buf + pos + o, &want, std::min<uint64_t>(8, chunkLen - o))) {
                r.numMismatches++;
                if (r.firstBadFileOffset == UINT64_MAX) r.firstBadFileOffset = fileOff + pos + o;
            }
        }
    }
    return r;
}

ReduceSeeds reduceVerifySeeds(uint64_t salt, uint64_t fileKey)
{
    ReduceSeeds s;
    s.uniq = splitmix64Of(splitmix64Of(salt ^ REDUCE_VERIFY_UNIQ_XOR) +
                          fileKey * 0x9E3779B97F4A7C15ULL);
    s.pool = splitmix64Of(salt ^ REDUCE_VERIFY_POOL_XOR);
    return s;
}

uint64_t reduceDirFileKey(uint64_t rank, uint64_t dir, uint64_t file)
{
    return splitmix64Of(splitmix64Of(splitmix64Of(rank + 1) ^ dir) ^ file);
}

void fillChecksumMixCPU(char* buf, uint64_t len, uint64_t fileOff, uint64_t salt,
                        uint64_t blockSize, uint64_t mixLen)
{
    // pos/end are compared by difference only (see fillChecksumCPU); rel
    // follows pos inside the block so the aligned loop needs no division
    uint64_t pos = fileOff;
    uint64_t end = fileOff + len;

    while (pos != end && (pos & 7)) {
        uint64_t a = pos & ~7ULL;
        uint64_t v = mixValueAt(a, salt, a % blockSize, mixLen);
        buf[pos - fileOff] = (char)((v >> (8 * (pos & 7))) & 0xff);
        pos++;
    }
    uint64_t rel = pos % blockSize;
    while (end - pos >= 8) {
        uint64_t v = mixValueAt(pos, salt, rel, mixLen);
        std::memcpy(buf + (pos - fileOff), &v, 8);
        pos += 8;
        rel += 8;
        if (rel >= blockSize) rel = 0;
    }
    while (pos != end) {
        uint64_t v = mixValueAt(pos & ~7ULL, salt, rel, mixLen);
        buf[pos - fileOff] = (char)((v >> (8 * (pos & 7))) & 0xff);
        pos++;
    }
}

uint64_t verifyChecksumMixCPU(const char* buf, uint64_t len, uint64_t fileOff, uint64_t salt,
                              uint64_t blockSize, uint64_t mixLen)
{
    uint64_t pos = fileOff;
    uint64_t end = fileOff + len;

    while (pos != end && (pos & 7)) {
        uint64_t a = pos & ~7ULL;
        uint64_t v = mixValueAt(a, salt, a % blockSize, mixLen);
        if (buf[pos - fileOff] != (char)((v >> (8 * (pos & 7))) & 0xff)) return pos;
        pos++;
    }
    uint64_t rel = pos % blockSize;
    while (end - pos >= 8) {
        uint64_t v = mixValueAt(pos, salt, rel, mixLen);
        uint64_t got;
        std::memcpy(&got, buf + (pos - fileOff), 8);
        if (got != v) { // find exact byte
            for (int b = 0; b < 8; b++)
                if (((got >> (8 * b)) & 0xff) != ((v >> (8 * b)) & 0xff)) return pos + b;
        }
        pos += 8;
        rel += 8;
        if (rel >= blockSize) rel = 0;
    }
    while (pos != end) {
        uint64_t v = mixValueAt(pos & ~7ULL, salt, rel, mixLen);
        if (buf[pos - fileOff] != (char)((v >> (8 * (pos & 7))) & 0xff)) return pos;
        pos++;
    }
    return UINT64_MAX;
}

// ---------------------------------------------------------------------------
// --verifydiag (CPU side): the classification of GpuVerifyDiag (gpu.h), word
// for word what ebVerifyDiagKernel / ebVerifyDiagMixKernel compute for an
// 8-aligned range. Unaligned ranges exist only here: the bytes of a word that
// the range holds in part are compared as the plain verify compares them, and
// such a word, when bad, counts as OTHER at the file offset of its first byte
// inside the range (its value cannot be decoded); pairs are counted from the
// first whole word.
// ---------------------------------------------------------------------------

static inline uint64_t unmix64(uint64_t z) // inverse of splitmix64Of's finalizer
{
    z ^= (z >> 31) ^ (z >> 62);
    z *= 0x319642B2D24D8EC3ULL;
    z ^= (z >> 27) ^ (z >> 54);
    z *= 0x96DE1B173F119089ULL;
    z ^= (z >> 30) ^ (z >> 60);
    return z;
}

static inline void diagCount(GpuVerifyDiag& a, uint64_t v, uint64_t exp, uint64_t off,
                             bool pairPattern, int64_t d, bool runStart)
{
    a.numMismatches++;
    if (off < a.firstBadFileOffset) a.firstBadFileOffset = off;
    if (off > a.lastBadFileOffset) a.lastBadFileOffset = off;
    if (runStart) a.runs++;
    if (v == 0) {
        a.zero++;
    } else if (pairPattern) {
        a.pattern++;
        if (d < a.deltaMin) a.deltaMin = d;
        if (d > a.deltaMax) a.deltaMax = d;
    } else if (__builtin_popcountll(v ^ exp) <= 2) {
        a.bitflip++;
        a.flipOr |= v ^ exp;
    } else {
        a.other++;
    }
}

// blockSize == 0 selects the plain pattern
static void verifyDiagRange(const char* buf, uint64_t len, uint64_t fileOff, uint64_t salt,
                            uint64_t blockSize, uint64_t mixLen, GpuVerifyDiag& acc)
{
    const bool mix = blockSize != 0;
    uint64_t pos = fileOff; // wraps past 2^64 like the fill and verify loops
    uint64_t left = len;
    bool prevBad = false; // the word before pos is bad (false at the range start)

    // bytes [pos, pos+n) of the word at (pos & ~7): a part of one word
    auto partialWord = [&](uint64_t n) {
        const uint64_t a = pos & ~7ULL;
        const uint64_t exp = mix ? mixValueAt(a, salt, a % blockSize, mixLen) : a + salt;
        bool bad = false;
        for (uint64_t k = 0; k < n; k++) {
            const uint64_t p = pos + k;
            if (buf[p - fileOff] != (char)((exp >> (8 * (p & 7))) & 0xff)) bad = true;
        }
        if (bad) {
            acc.numMismatches++;
            if (pos < acc.firstBadFileOffset) acc.firstBadFileOffset = pos;
            if (pos > acc.lastBadFileOffset) acc.lastBadFileOffset = pos;
            if (!prevBad) acc.runs++;
            acc.other++;
        }
        prevBad = bad;
        pos += n;
        left -= n;
    };

    if (left && (pos & 7)) partialWord(std::min<uint64_t>(8 - (pos & 7), left));

    uint64_t rel = mix ? pos % blockSize : 0;
    auto nextRel = [&](uint64_t r) { return (r + 8 >= blockSize) ? r + 8 - blockSize : r + 8; };

    while (left >= 8) {
        const bool have1 = left >= 16;
        const uint64_t rel1 = mix ? nextRel(rel) : 0;
        const uint64_t x0 = pos + salt, x1 = pos + 8 + salt;
        const bool hashed0 = mix && rel < mixLen, hashed1 = mix && rel1 < mixLen;
        const uint64_t exp0 = hashed0 ? splitmix64Of(x0) : x0;
        const uint64_t exp1 = hashed1 ? splitmix64Of(x1) : x1;
        uint64_t v0, v1 = exp1;
        std::memcpy(&v0, buf + (pos - fileOff), 8);
        if (have1) std::memcpy(&v1, buf + (pos - fileOff) + 8, 8);
        const bool bad0 = v0 != exp0, bad1 = v1 != exp1;

        if (bad0 || bad1) {
            int64_t d0 = 0, d1 = 0;
            bool pairPattern = false;
            if (bad0 && bad1 && v0 && v1) {
                d0 = (int64_t)((hashed0 ? unmix64(v0) - 0x9E3779B97F4A7C15ULL : v0) - x0);
                d1 = (int64_t)((hashed1 ? unmix64(v1) - 0x9E3779B97F4A7C15ULL : v1) - x1);
                pairPattern = d0 == d1;
            }
            if (bad0) diagCount(acc, v0, exp0, pos, pairPattern, d0, !prevBad);
            if (bad1) diagCount(acc, v1, exp1, pos + 8, pairPattern, d1, !bad0);
        }

        if (have1) {
            prevBad = bad1;
            pos += 16;
            left -= 16;
            if (mix) rel = nextRel(rel1);
        } else {
            prevBad = bad0;
            pos += 8;
            left -= 8;
        }
    }

    if (left) partialWord(left);
}

void verifyDiagCPU(const char* buf, uint64_t len, uint64_t fileOff, uint64_t salt,
                   GpuVerifyDiag& acc)
{
    verifyDiagRange(buf, len, fileOff, salt, 0, 0, acc);
}

void verifyDiagMixCPU(const char* buf, uint64_t len, uint64_t fileOff, uint64_t salt,
                      uint64_t blockSize, uint64_t mixLen, GpuVerifyDiag& acc)
{
    if (!blockSize || blockSize % 8 || mixLen % 8)
        throw std::invalid_argument("verifyDiagMixCPU: block size and mix length must be "
                                    "multiples of 8, the block size positive");
    verifyDiagRange(buf, len, fileOff, salt, blockSize, mixLen, acc);
}

std::string verifyDiagText(const GpuVerifyDiag& d)
{
    std::string s = "; diagnosis: last bad file offset: " + std::to_string(d.lastBadFileOffset) +
                    "; runs: " + std::to_string(d.runs) + "; zero: " + std::to_string(d.zero) +
                    "; pattern: " + std::to_string(d.pattern) +
                    "; bitflip: " + std::to_string(d.bitflip) +
                    "; other: " + std::to_string(d.other);
    if (d.pattern) {
        s += "; pattern delta: " + std::to_string(d.deltaMin);
        if (d.deltaMin != d.deltaMax) s += ".." + std::to_string(d.deltaMax);
    }
    if (d.bitflip) {
        char hex[32];
        snprintf(hex, sizeof(hex), "0x%llx", (unsigned long long)d.flipOr);
        s += std::string("; flipped bits: ") + hex;
    }
    return s;
}

// ---------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------

static uint64_t nowUSecSince(std::chrono::steady_clock::time_point t0)
{
    return (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(
               std::chrono::steady_clock::now() - t0)
        .count();
}

static void throwErrno(const std::string& what, const std::string& path)
{
    throw WorkerError(what + " failed. Path: " + path + "; SysErr: " + strerror(errno));
}

// mkdir -p for one level chain (benchPath/r{rank}) — parents must exist.
static void mkdirIgnoreExists(const std::string& path)
{
    if (mkdir(path.c_str(), 0777) && errno != EEXIST) throwErrno("mkdir", path);
}

// Staging geometry for GPU mode. Reads batch `batch` consecutive slots into
// ONE ranged H2D (pinned and device slots are contiguous): 4 MiB copies only
// reach ~30 GB/s on the SDMA path, ~16 MiB spans run near the 57 GB/s peak.
// The ring holds two batches so pread-fill overlaps the copy.
static uint64_t gpuBatchBytes()
{
    static const uint64_t v = [] {
        const char* e = getenv("EB_GPU_BATCH_BYTES");
        // swept on MI355X (gpurun_out/batch_sweep2.log): 4K random read hits
        // 9.4M IOPS with 1 MiB half-rings (256 slots) vs 5.3M at 256 KiB
        return e ? (uint64_t)atoll(e) : (1ULL << 20);
    }();
    return v;
}

static int gpuBatchSlots(uint64_t blockSize)
{
    uint64_t bb = gpuBatchBytes();
    if (!bb) return 1; // batching disabled
    // measured: batching only pays for small blocks (many tiny copies
    // amortized into one); at >=256 KiB blocks the fine-grained per-block
    // pipeline interleaves better across workers (-25% when batched)
    if (blockSize >= (256ULL << 10)) return 1;
    uint64_t batch = bb / std::max<uint64_t>(blockSize, 1);
    // cap the ring (2 batches) at 64 MiB per worker
    uint64_t maxBatch = (32ULL << 20) / std::max<uint64_t>(blockSize, 1);
    batch = std::min(batch, std::max<uint64_t>(maxBatch, 1));
    return (int)std::min<uint64_t>(std::max<uint64_t>(batch, 1), 512);
}

static int gpuSlotCount(int ioDepth, uint64_t blockSize)
{
    static const int def = [] {
        const char* v = getenv("EB_GPU_SLOTS");
        int n = v ? atoi(v) : 2;
        return (n >= 1 && n <= 128) ? n : 2;
    }();
    int slots = std::max(def, 2 * gpuBatchSlots(blockSize));
    return std::max(slots, ioDepth);
}

// ---------------------------------------------------------------------------
// Worker
// ---------------------------------------------------------------------------

Worker::Worker(Engine& engine, int localRank)
    : localRank(localRank), globalRank(engine.cfg.rankOffset + localRank), eng(engine)
{
}

Worker::~Worker()
{
    if (ownHostBufs)
        for (auto p : hostBufs) free(p);
    free(scratchBuf);

    if (gpu) { // return the GPU context for reuse by the next phase
        std::lock_guard<std::mutex> lk(eng.gpuCacheMtx);
        if ((size_t)localRank >= eng.gpuCtxCache.size())
            eng.gpuCtxCache.resize(localRank + 1);
        eng.gpuCtxCache[localRank] = std::move(gpu);
    }
}

// --- rwmix byte-ratio balancer (reference toolkits/RateLimiterRWMixThreads:
// readers and writers mutually throttle so read bytes stay at rwMixPct% of
// the combined volume; headroom = blockSize * peer threads; 600s watchdog) ---

bool Worker::rwBalancerActive() const
{
    const auto& cfg = eng.cfg;
    return cfg.rwMixThreads > 0 && cfg.rwMixPct > 0 && cfg.rwMixPct < 100 &&
           eng.currentPhase == Phase::WRITE;
}

void Worker::rwBalanceWait(bool isRead, uint64_t nextLen)
{
    const auto& cfg = eng.cfg;
    const uint64_t pct = (uint64_t)cfg.rwMixPct;
    const unsigned peers = isRead ? (cfg.numThreads - cfg.rwMixThreads) : cfg.rwMixThreads;
    const uint64_t headroom = cfg.blockSize * std::max(1u, peers);
    auto waitStart = Clock::now();

    for (;;) {
        uint64_t rd = eng.rwBalBytesRead.load(std::memory_order_relaxed);
        uint64_t wr = eng.rwBalBytesWrite.load(std::memory_order_relaxed);
        uint64_t allowed;
        if (isRead) // read <= (write + headroom) * pct / (100 - pct)
            allowed = (wr + headroom) * pct / (100 - pct);
        else // write <= (read + headroom) * (100 - pct) / pct
            allowed = (rd + headroom) * (100 - pct) / pct;

        uint64_t mine = isRead ? rd : wr;
        if (mine + nextLen <= allowed) return;

        // the peer GROUP is done? then no more balancing possible — proceed
        int peersDone = (isRead ? eng.rwWritersDone : eng.rwReadersDone)
                            .load(std::memory_order_relaxed);
        if (peers > 0 && peersDone >= (int)peers) return;

        checkInterrupt();
        if (std::chrono::duration_cast<std::chrono::seconds>(Clock::now() - waitStart)
                .count() > 600)
            throw WorkerError("rwmix balancer: stalled >600s waiting for " +
                              std::string(isRead ? "writer" : "reader") + " progress");
        std::this_thread::sleep_for(std::chrono::milliseconds(2));
    }
}

void Worker::rwBalanceAccount(bool isRead, uint64_t len)
{
    (isRead ? eng.rwBalBytesRead : eng.rwBalBytesWrite)
        .fetch_add(len, std::memory_order_relaxed);
}

bool Worker::rwMixDecideRead()
{
    bool doRead = (rwMixReads * 100) < (rwMixOps * (uint64_t)eng.cfg.rwMixPct);
    rwMixOps++;
    if (doRead) rwMixReads++;
    return doRead;
}

void Worker::checkInterrupt()
{
    if (eng.interruptFlag.load(std::memory_order_relaxed)) throw InterruptedError();
}

void Worker::allocBuffers()
{
    if (!hostBufs.empty()) { // persistent worker: buffers survive phases
        if (gpu) {
            gpu->bindThread();
            // a --lat phase that threw before its drain (verify failure, I/O
            // error, interrupt) left timed pairs uncollected in this
            // persistent context: they are not this phase's samples
            gpu->dropTimedPairs();
        }
        return;
    }

    const auto& cfg = eng.cfg;
    int slots = std::max(1, cfg.ioDepth);
    if (!cfg.gpuIDs.empty()) slots = gpuSlotCount(cfg.ioDepth, cfg.blockSize);

    if (!cfg.gpuIDs.empty()) {
        setupGpu();
        for (int i = 0; i < slots; i++) hostBufs.push_back(gpu->hostBuf(i));
        ownHostBufs = false;
    } else {
        for (int i = 0; i < slots; i++) {
            char* p = nullptr;
            if (posix_memalign((void**)&p, 4096, cfg.blockSize))
                throw WorkerError("host I/O buffer allocation failed");
            hostBufs.push_back(p);
        }
        ownHostBufs = true;
    }

    // pre-fill host buffers with random data (defeats compression; same
    // contract as reference LocalWorker.cpp:1386-1420)
    RandAlgoXoshiro256ppSIMD<8> bufFillRng(cfg.benchSeed ^ (0x517cc1b7ULL * (globalRank + 1)));
    for (auto p : hostBufs) bufFillRng.fillBuf(p, cfg.blockSize);

    if (gpu) { // seed device buffers so a pct<100 refill mixes defined data
        for (int i = 0; i < slots; i++) gpu->copyH2DAsync(i, cfg.blockSize);
        gpu->syncStream();
    }

    if (cfg.verifyDirect && posix_memalign((void**)&scratchBuf, 4096, cfg.blockSize))
        throw WorkerError("scratch buffer allocation failed");
}

// CPU core / NUMA zone binding (reference analogue: Worker.cpp:102-146 +
// NumaTk). Zones bind to all CPUs listed in /sys/devices/system/node.
void Worker::applyBinding()
{
    const auto& cfg = eng.cfg;

    cpu_set_t set;
    CPU_ZERO(&set);
    bool haveSet = false;

    if (!cfg.cpuCores.empty()) {
        int core = cfg.cpuCores[globalRank % cfg.cpuCores.size()];
        CPU_SET(core, &set);
        haveSet = true;
    } else if (!cfg.numaZones.empty()) {
        int zone = cfg.numaZones[globalRank % cfg.numaZones.size()];
        std::string path = "/sys/devices/system/node/node" + std::to_string(zone) + "/cpulist";
        FILE* f = fopen(path.c_str(), "r");
        if (!f) throw WorkerError("unknown NUMA zone " + std::to_string(zone));
        char buf[512] = {0};
        if (fgets(buf, sizeof(buf), f)) {
            // parse "0-15,32-47" style lists
            char* save = nullptr;
            for (char* tok = strtok_r(buf, ",\n", &save); tok;
                 tok = strtok_r(nullptr, ",\n", &save)) {
                int lo, hi;
                if (sscanf(tok, "%d-%d", &lo, &hi) == 2)
                    for (int i = lo; i <= hi; i++) CPU_SET(i, &set);
                else if (sscanf(tok, "%d", &lo) == 1)
                    CPU_SET(lo, &set);
            }
            haveSet = true;
        }
        fclose(f);
    }

    if (haveSet && pthread_setaffinity_np(pthread_self(), sizeof(set), &set))
        throw WorkerError("CPU affinity binding failed");
}

void Worker::setupGpu()
{
    const auto& cfg = eng.cfg;
    int devId = cfg.gpuIDs[globalRank % cfg.gpuIDs.size()];
    int slots = gpuSlotCount(cfg.ioDepth, cfg.blockSize);

    if (gpuDeviceCount() <= 0)
        throw WorkerError("GPU requested (gpuids) but no HIP device is available — "
                          "refusing silent CPU fallback");

    { // reuse a cached context from a previous phase when shapes match
        std::lock_guard<std::mutex> lk(eng.gpuCacheMtx);
        if ((size_t)localRank < eng.gpuCtxCache.size() && eng.gpuCtxCache[localRank] &&
            eng.gpuCtxCache[localRank]->deviceId() == devId &&
            eng.gpuCtxCache[localRank]->numSlots() >= slots &&
            eng.gpuCtxCache[localRank]->bufSize() >= cfg.blockSize)
            gpu = std::move(eng.gpuCtxCache[localRank]);
    }

    if (gpu)
        gpu->bindThread();
    else
        gpu = std::make_unique<GpuCtx>(devId, slots, cfg.blockSize, cfg.gpuPinnedHostBufs);
}

void Worker::fairShareSlice(uint64_t totalLen, uint64_t& myStart, uint64_t& myLen) const
{
    // contiguous per-rank block slice; last rank takes remainder blocks+tail
    // (same contract as reference fileModeIterateFilesSeq :3597)
    const auto& cfg = eng.cfg;
    uint64_t bs = cfg.blockSize;
    uint64_t numRanks = cfg.numDataSetThreads;
    uint64_t numBlocksTotal = (totalLen + bs - 1) / bs;
    uint64_t perRank = numBlocksTotal / numRanks;
    uint64_t startBlock = (uint64_t)globalRank * perRank;
    uint64_t myBlocks = perRank;
    if ((uint64_t)globalRank == numRanks - 1) myBlocks = numBlocksTotal - startBlock;

    myStart = startBlock * bs;
    uint64_t endByte = std::min(totalLen, (startBlock + myBlocks) * bs);
    myLen = (myStart >= endByte) ? 0 : endByte - myStart;
}

std::unique_ptr<OffsetGen> Worker::makeOffsetGen(uint64_t rangeStart, uint64_t rangeLen)
{
    const auto& cfg = eng.cfg;
    bool isWrite = (eng.currentPhase == Phase::WRITE);
    uint64_t perWorkerRandAmount =
        cfg.randAmount ? cfg.randAmount / cfg.numDataSetThreads : rangeLen;

    std::unique_ptr<OffsetGen> gen;

    if (cfg.backward) {
        gen = std::make_unique<OffsetGenReverseSeq>(cfg.blockSize);
    } else if (cfg.strided) {
        gen = std::make_unique<OffsetGenStrided>(cfg.blockSize, globalRank,
                                                 cfg.numDataSetThreads);
    } else if (!cfg.random) {
        gen = std::make_unique<OffsetGenSequential>(cfg.blockSize);
    } else if (!cfg.randAligned) {
        gen = std::make_unique<OffsetGenRandom>(cfg.blockSize, *rng, perWorkerRandAmount);
    } else if (isWrite) {
        // random aligned writes: full coverage so the resulting file is fully
        // allocated (reference behavior, LocalWorker.cpp:1177-1185)
        gen = std::make_unique<OffsetGenRandomAlignedFullCoverage>(
            cfg.blockSize, cfg.benchSeed + 0x9E3779B97F4A7C15ULL * (uint64_t)eng.phaseSeq +
                               0x94D049BB133111EBULL * (uint64_t)(globalRank + 1));
    } else {
        gen = std::make_unique<OffsetGenRandomAligned>(cfg.blockSize, *rng, perWorkerRandAmount);
    }

    gen->reset(rangeStart, rangeLen);
    return gen;
}

namespace {

// fcntl advisory lock guard (reference analogue: FileTk::flock range/full)
struct FlockGuard {
    int fd = -1;
    struct flock fl{};

    FlockGuard(int fd_, int mode, bool isWrite, uint64_t off, uint64_t len) : fd(fd_)
    {
        if (!mode) { fd = -1; return; }
        fl.l_type = isWrite ? F_WRLCK : F_RDLCK;
        fl.l_whence = SEEK_SET;
        fl.l_start = (mode == 2) ? 0 : (off_t)off;
        fl.l_len = (mode == 2) ? 0 : (off_t)len;
        if (fcntl(fd, F_SETLKW, &fl)) throw WorkerError("flock (fcntl F_SETLKW) failed");
    }

    ~FlockGuard()
    {
        if (fd < 0) return;
        fl.l_type = F_UNLCK;
        fcntl(fd, F_SETLK, &fl);
    }
};

} // namespace

// single synchronous block I/O incl. GPU staging, verify hooks, mmap path,
// flock and ops logging
ssize_t Worker::blockIO(bool isWrite, int fd, int slot, uint64_t len, uint64_t fileOff,
                        char* mmapBase, const std::string* path)
{
    const auto& cfg = eng.cfg;
    char* buf = hostBufs[slot];
    const bool logOps = eng.opsLog.isEnabled();
    static const std::string emptyPath;
    const std::string& target = path ? *path : emptyPath;

    if (isWrite) {
        rateLimiter.wait(len);
        preWriteFill(slot, len, fileOff);

        if (gpu) { // stage GPU->host on this worker's stream
            gpu->copyD2HAsync(slot, len);
            gpu->syncStream();
        }

        FlockGuard lock(fd, cfg.flockMode, true, fileOff, len);

        ssize_t res;
        if (mmapBase) {
            if (logOps) eng.opsLog.log(globalRank, "memcpy_w", target, fileOff, len, true, false);
            std::memcpy(mmapBase + fileOff, buf, len);
            res = (ssize_t)len;
            if (logOps) eng.opsLog.log(globalRank, "memcpy_w", target, fileOff, len, false, false);
        } else {
            if (logOps) eng.opsLog.log(globalRank, "pwrite", target, fileOff, len, true, false);
            res = pwrite(fd, buf, len, fileOff);
            if (logOps) eng.opsLog.log(globalRank, "pwrite", target, fileOff, len, false, res < 0);
        }

        if (res == (ssize_t)len && cfg.verifyDirect) verifyDirectReadback(fd, slot, len, fileOff);
        return res;
    } else {
        rateLimiter.wait(len);

        FlockGuard lock(fd, cfg.flockMode, false, fileOff, len);

        ssize_t res;
        if (mmapBase) {
            if (logOps) eng.opsLog.log(globalRank, "memcpy_r", target, fileOff, len, true, false);
            std::memcpy(buf, mmapBase + fileOff, len);
            res = (ssize_t)len;
            if (logOps) eng.opsLog.log(globalRank, "memcpy_r", target, fileOff, len, false, false);
        } else {
            if (logOps) eng.opsLog.log(globalRank, "pread", target, fileOff, len, true, false);
            res = pread(fd, buf, len, fileOff);
            if (logOps) eng.opsLog.log(globalRank, "pread", target, fileOff, len, false, res < 0);
        }
        if (res < 0) return res;

        if (gpu) { // stage host->GPU (HBM3E resident buffers)
            gpu->copyH2DAsync(slot, len);
            gpu->syncStream();
        }

        postReadCheck(slot, (uint64_t)res, fileOff);
        return res;
    }
}

// --verifydirect: read each block back right after writing and compare
void Worker::verifyDirectReadback(int fd, int slot, uint64_t len, uint64_t fileOff)
{
    ssize_t res = pread(fd, scratchBuf, len, fileOff);
    if (res != (ssize_t)len)
        throw WorkerError("verify-direct readback failed at offset " +
                          std::to_string(fileOff));
    if (std::memcmp(scratchBuf, hostBufs[slot], len))
        throw WorkerError("verify-direct mismatch: block at offset " +
                          std::to_string(fileOff) + " differs after readback");
}

void Worker::preWriteFill(int slot, uint64_t len, uint64_t fileOff)
{
    const auto& cfg = eng.cfg;
    char* buf = hostBufs[slot];

    if (cfg.verifySalt >= 0) {
        // integrity fill
        if (gpu && (fileOff % 8 == 0) && (len % 8 == 0)) {
            if (eng.verifyMix)
                gpu->fillChecksumMixDev(slot, len, fileOff, (uint64_t)cfg.verifySalt,
                                        cfg.blockSize, eng.verifyMixLen);
            else
                gpu->fillChecksumDev(slot, len, fileOff, (uint64_t)cfg.verifySalt);
            return; // D2H staging copies it to host buf
        }
        if (eng.verifyMix)
            fillChecksumMixCPU(buf, len, fileOff, (uint64_t)cfg.verifySalt, cfg.blockSize,
                               eng.verifyMixLen);
        else
            fillChecksumCPU(buf, len, fileOff, (uint64_t)cfg.verifySalt);
        if (gpu) { // keep device buffer coherent for the D2H staging copy
            gpu->copyH2DAsync(slot, len);
            gpu->syncStream();
        }
        return;
    }

    if (eng.reduceVerify) {
        // --dedupeverify: the chunks that the file offset names, with the
        // seeds of the slot's file; no worker state
        const ReduceSeeds& seed = slotReduceSeed[slot];
        const uint64_t first = fileOff / cfg.dedupeChunk;
        if (gpu && (len % 16 == 0)) {
            gpu->fillReduceDev(slot, len, first, cfg.dedupeChunk, eng.reduceRandBytes,
                               cfg.dedupePct, REDUCE_POOL_CHUNKS, seed.uniq, seed.pool);
            return;
        }
        fillReduceCPU(buf, len, first, cfg.dedupeChunk, eng.reduceRandBytes, cfg.dedupePct,
                      REDUCE_POOL_CHUNKS, seed.uniq, seed.pool);
        if (gpu) {
            gpu->copyH2DAsync(slot, len);
            gpu->syncStream();
        }
        return;
    }

    if (eng.reduce) {
        // --dedupepct / --compresspct: the next ceil(len / chunk) chunks of
        // this worker's sequence, whatever the file offset
        const uint64_t first = reduceNextChunk;
        reduceNextChunk += (len + cfg.dedupeChunk - 1) / cfg.dedupeChunk;
        if (gpu && (len % 16 == 0)) {
            gpu->fillReduceDev(slot, len, first, cfg.dedupeChunk, eng.reduceRandBytes,
                               cfg.dedupePct, REDUCE_POOL_CHUNKS, reduceSeed.uniq,
                               reduceSeed.pool);
            return;
        }
        fillReduceCPU(buf, len, first, cfg.dedupeChunk, eng.reduceRandBytes, cfg.dedupePct,
                      REDUCE_POOL_CHUNKS, reduceSeed.uniq, reduceSeed.pool);
        if (gpu) {
            gpu->copyH2DAsync(slot, len);
            gpu->syncStream();
        }
        return;
    }

    if (cfg.blockVarPct > 0) {
        uint64_t refillLen = (len * cfg.blockVarPct) / 100;
        if (gpu && (len % 16 == 0)) {
            gpu->blockVarRefillDev(slot, len, refillLen,
                                   cfg.benchSeed ^ (0xD1B54A32D192ED03ULL * (globalRank + 1)),
                                   cfg.blockVarAlgo == "fast");
            return;
        }
        // CPU refill: refillLen random bytes, rest a fresh constant u64
        fillRng->fillBuf(buf, refillLen);
        if (refillLen < len) {
            uint64_t c = fillRng->next();
            uint64_t pos = refillLen;
            while (pos < len) {
                uint64_t n = std::min<uint64_t>(8, len - pos);
                std::memcpy(buf + pos, &c, n);
                pos += n;
            }
        }
        if (gpu) {
            gpu->copyH2DAsync(slot, len);
            gpu->syncStream();
        }
    }
    // blockVarPct == 0: keep the pre-filled random buffer as is
}

void Worker::postReadCheck(int slot, uint64_t len, uint64_t fileOff)
{
    if (!eng.dataVerify && !profiling) return;

    if (gpu && (fileOff % 8 == 0) && (len % 16 == 0)) {
        if (eng.dataVerify) gpuVerifyAsync(slot, len, fileOff);
        profileGpuAsync(slot, len);
        if (eng.dataVerify) gpuVerifyFetch();
        return;
    }

    if (eng.dataVerify) cpuVerify(slot, hostBufs[slot], len, fileOff);
    profileCpu(hostBufs[slot], len);
}

// --dataprofile: the two steps that go with every verify step of a READ
// phase. profileGpuAsync enqueues one block's profile kernel on the worker's
// stream, behind the block's H2D copy; nothing is fetched before the phase
// ends. profileCpu profiles a host buffer at once (no --gpuids, and the odd
// tails that the read paths hand to cpuVerify).
void Worker::profileGpuAsync(int slot, uint64_t len)
{
    if (profiling) gpu->dataProfileDevAsync(slot, len, eng.cfg.dedupeChunk);
}

void Worker::profileCpu(const char* buf, uint64_t len)
{
    if (profiling) dataProfileCPU(buf, len, eng.cfg.dedupeChunk, *profileAcc);
}

void Worker::setSlotFileKey(int slot, uint64_t fileKey)
{
    if (!eng.reduceVerify) return;
    if (slotReduceSeed.size() < hostBufs.size()) slotReduceSeed.resize(hostBufs.size());
    slotReduceSeed[slot] = reduceVerifySeeds((uint64_t)eng.cfg.reduceVerifySalt, fileKey);
}

void Worker::setAllSlotFileKeys(uint64_t fileKey)
{
    if (!eng.reduceVerify) return;
    slotReduceSeed.assign(hostBufs.size(),
                          reduceVerifySeeds((uint64_t)eng.cfg.reduceVerifySalt, fileKey));
}

// The three verify steps of every read path, in their plain, --verifymixpct
// and --verifydiag forms. gpuVerifyAsync enqueues one block's verify on the
// worker's stream; gpuVerifyFetch collects what accumulated since the last
// fetch and throws on a mismatch; cpuVerify checks a host buffer at once.

void Worker::gpuVerifyAsync(int slot, uint64_t len, uint64_t fileOff)
{
    const auto& cfg = eng.cfg;
    if (eng.reduceVerify) {
        const ReduceSeeds& seed = slotReduceSeed[slot];
        gpu->verifyReduceDevAsync(slot, len, fileOff, fileOff / cfg.dedupeChunk,
                                  cfg.dedupeChunk, eng.reduceRandBytes, cfg.dedupePct,
                                  REDUCE_POOL_CHUNKS, seed.uniq, seed.pool);
        return;
    }
    const uint64_t salt = (uint64_t)cfg.verifySalt;
    if (cfg.verifyDiag) {
        if (eng.verifyMix)
            gpu->verifyDiagMixDevAsync(slot, len, fileOff, salt, cfg.blockSize,
                                       eng.verifyMixLen);
        else
            gpu->verifyDiagDevAsync(slot, len, fileOff, salt);
    } else if (eng.verifyMix) {
        gpu->verifyChecksumMixDevAsync(slot, len, fileOff, salt, cfg.blockSize,
                                       eng.verifyMixLen);
    } else {
        gpu->verifyChecksumDevAsync(slot, len, fileOff, salt);
    }
}

void Worker::gpuVerifyFetch()
{
    uint64_t numBad, firstBad;
    std::string diagnosis;
    if (eng.cfg.verifyDiag) {
        GpuVerifyDiag d = gpu->fetchVerifyDiag();
        numBad = d.numMismatches;
        firstBad = d.firstBadFileOffset;
        if (numBad) diagnosis = verifyDiagText(d);
    } else {
        GpuVerifyResult r = gpu->fetchVerifyResult();
        numBad = r.numMismatches;
        firstBad = r.firstBadFileOffset;
    }
    if (numBad)
        throw WorkerError("Data verification failed (GPU). First bad file offset: " +
                          std::to_string(firstBad) + "; mismatching 8-byte words: " +
                          std::to_string(numBad) + diagnosis);
}

// drop what a READ that threw mid-window left unfetched in this persistent
// context's counters, so it is not reported by the next phase
void Worker::gpuVerifyDropStale()
{
    (void)gpu->fetchVerifyResult();
    if (eng.cfg.verifyDiag) (void)gpu->fetchVerifyDiag();
}

void Worker::cpuVerify(int slot, const char* buf, uint64_t len, uint64_t fileOff)
{
    const auto& cfg = eng.cfg;
    if (eng.reduceVerify) {
        const ReduceSeeds& seed = slotReduceSeed[slot];
        GpuVerifyResult r = verifyReduceCPU(buf, len, fileOff, fileOff / cfg.dedupeChunk,
                                            cfg.dedupeChunk, eng.reduceRandBytes, cfg.dedupePct,
                                            REDUCE_POOL_CHUNKS, seed.uniq, seed.pool);
        if (r.numMismatches)
            throw WorkerError("Data verification failed. First bad file offset: " +
                              std::to_string(r.firstBadFileOffset) +
                              "; mismatching 8-byte words: " + std::to_string(r.numMismatches));
        return;
    }
    const uint64_t salt = (uint64_t)cfg.verifySalt;
    std::string diagnosis;
    if (cfg.verifyDiag) {
        GpuVerifyDiag d;
        if (eng.verifyMix)
            verifyDiagMixCPU(buf, len, fileOff, salt, cfg.blockSize, eng.verifyMixLen, d);
        else
            verifyDiagCPU(buf, len, fileOff, salt, d);
        if (!d.numMismatches) return;
        // the failure path: the plain verify below finds the exact first bad
        // byte, so the text up to the diagnosis is what a run without
        // --verifydiag prints
        diagnosis = "; mismatching 8-byte words: " + std::to_string(d.numMismatches) +
                    verifyDiagText(d);
    }
    uint64_t bad = eng.verifyMix
                       ? verifyChecksumMixCPU(buf, len, fileOff, salt, cfg.blockSize,
                                              eng.verifyMixLen)
                       : verifyChecksumCPU(buf, len, fileOff, salt);
    if (bad != UINT64_MAX)
        throw WorkerError("Data verification failed. First bad file offset: " +
                          std::to_string(bad) + diagnosis);
}

// ---------------------------------------------------------------------------
// file/bdev mode
// ---------------------------------------------------------------------------

namespace {

struct FdGuard {
    std::vector<int> fds;
    ~FdGuard()
    {
        for (int fd : fds)
            if (fd >= 0) close(fd);
    }
};

// per-file mmap guard (reference analogue: FileTk::mmapAndMadvise)
struct MmapGuard {
    std::vector<std::pair<char*, uint64_t>> maps;

    void map(int fd, uint64_t len, bool writable, int madvFlags, const std::string& path)
    {
        int prot = writable ? (PROT_READ | PROT_WRITE) : PROT_READ;
        void* p = mmap(nullptr, len, prot, MAP_SHARED, fd, 0);
        if (p == MAP_FAILED)
            throw WorkerError("mmap failed. Path: " + path + "; SysErr: " + strerror(errno));
        if (madvFlags && madvise(p, len, madvFlags))
            throw WorkerError("madvise failed. Path: " + path);
        maps.emplace_back((char*)p, len);
    }

    char* base(uint64_t idx) const
    {
        return idx < maps.size() ? maps[idx].first : nullptr;
    }

    ~MmapGuard()
    {
        for (auto& [p, len] : maps) munmap(p, len);
    }
};

// --fadv: bitmask encodes the POSIX_FADV_* advices to apply in order
enum FadvBits {
    FADV_BIT_SEQ = 1,
    FADV_BIT_RAND = 2,
    FADV_BIT_WILLNEED = 4,
    FADV_BIT_DONTNEED = 8,
    FADV_BIT_NOREUSE = 16,
};

inline void applyFadvise(int fd, int bits, const std::string& path)
{
    if (!bits) return;
    struct { int bit; int advice; } table[] = {
        {FADV_BIT_SEQ, POSIX_FADV_SEQUENTIAL},   {FADV_BIT_RAND, POSIX_FADV_RANDOM},
        {FADV_BIT_WILLNEED, POSIX_FADV_WILLNEED}, {FADV_BIT_DONTNEED, POSIX_FADV_DONTNEED},
        {FADV_BIT_NOREUSE, POSIX_FADV_NOREUSE},
    };
    for (auto& e : table)
        if ((bits & e.bit) && posix_fadvise(fd, 0, 0, e.advice))
            throw WorkerError("posix_fadvise failed. Path: " + path);
}

} // namespace

void Worker::fileModeBlocks(bool isWrite)
{
    const auto& cfg = eng.cfg;
    if (cfg.ioDepth > 1) return fileModeBlocksUring(isWrite);
    // --lat stays ON the zero-copy fast path: per-block timing comes from
    // hipEvent pairs around each staging copy
    if (cfg.useMmap && !cfg.gpuIDs.empty() && cfg.flockMode == 0 &&
        !(isWrite && (cfg.rwMixPct > 0 || cfg.rwMixThreads > 0)) && !cfg.verifyDirect &&
        cfg.pathType == PathType::FILE && !eng.opsLog.isEnabled())
        return fileModeBlocksGpuMmap(isWrite);

    const uint64_t fileSize = eng.effFileSize;
    const uint64_t bs = cfg.blockSize;
    const size_t numFiles = cfg.paths.size();
    const uint64_t numBlocksPerFile = (fileSize + bs - 1) / bs;
    const bool rwMixActive = isWrite && (cfg.rwMixPct > 0 || isDedicatedReader);

    // open all files
    FdGuard fg;
    MmapGuard mg;
    int rwFlags = isWrite
                      ? ((cfg.verifyDirect || rwMixActive || cfg.useMmap) ? O_RDWR : O_WRONLY)
                      : O_RDONLY;
    int openFlags = rwFlags | (cfg.directIO ? O_DIRECT : 0);
    if (isWrite && cfg.pathType == PathType::FILE) openFlags |= O_CREAT;
    for (const auto& p : cfg.paths) {
        int fd = open(p.c_str(), openFlags, 0644);
        if (fd < 0) throwErrno("open", p);
        fg.fds.push_back(fd);
        if (isWrite && cfg.pathType == PathType::FILE) {
            if (cfg.truncate && ftruncate(fd, 0)) throwErrno("truncate", p);
            if ((cfg.truncToSize != UINT64_MAX || cfg.useMmap) && ftruncate(fd, fileSize))
                throwErrno("truncate-to-size", p);
            if (cfg.preallocFile && fallocate(fd, 0, 0, fileSize)) throwErrno("fallocate", p);
        }
        applyFadvise(fd, cfg.fadviseFlags, p);
        if (cfg.useMmap) mg.map(fd, fileSize, isWrite, cfg.madviseFlags, p);
    }

    // Virtual concatenated range: sequential uses ceil blocks per file (the
    // tail block is trimmed at I/O time); random/strided use floor blocks per
    // file (reference fileModeIterateFilesSeq :3597 / ...Rand :3511).
    const uint64_t mapBPF = (cfg.random || cfg.strided) ? (fileSize / bs) : numBlocksPerFile;
    const uint64_t virtFileLen = mapBPF * bs;

    auto mapBlock = [&](const BlockSpec& s, uint64_t& fileIdx, uint64_t& inFileOff,
                        uint64_t& ioLen) -> bool {
        if (!virtFileLen) return false;
        fileIdx = s.offset / virtFileLen;
        if (fileIdx >= numFiles) return false;
        inFileOff = s.offset - fileIdx * virtFileLen;
        if (inFileOff >= fileSize) return false;
        ioLen = std::min(s.len, fileSize - inFileOff);
        return true;
    };

    std::unique_ptr<OffsetGen> gen;
    if (cfg.random || cfg.strided) {
        // per-worker contiguous subrange of the virtual concatenated range
        // (whole-block granularity; reference fileModeIterateFilesRand :3511)
        uint64_t numBlocksTotal = mapBPF * numFiles;
        uint64_t rangeLen = bs * (numBlocksTotal / cfg.numDataSetThreads);
        uint64_t rangeOff = (uint64_t)globalRank * rangeLen;
        if (cfg.strided) {
            gen = std::make_unique<OffsetGenStrided>(bs, globalRank, cfg.numDataSetThreads);
            gen->reset(0, bs * numBlocksTotal);
        } else {
            gen = makeOffsetGen(rangeOff, rangeLen);
        }
    } else {
        uint64_t myStart, myLen;
        fairShareSlice(virtFileLen * numFiles, myStart, myLen);
        if (!myLen) return; // no work this round
        gen = makeOffsetGen(myStart, myLen);
    }

    // GPU staging pipeline: with two slots and per-slot events, storage I/O
    // of block i overlaps the PCIe copy of block i-1 and GPU verify batches
    // 64 blocks per stream sync. --lat stays on this path: per-block
    // latency = syscall wall time + the staging copy's hipEvent-pair time
    // (batched reads amortize the ranged copy over its blocks).
    // Plain per-block path when mmap, flock or rwmix are requested.
    static const bool pipelineDisabled = [] {
        const char* v = getenv("EB_GPU_PIPELINE");
        return v && v[0] == '0';
    }();
    const bool gpuPipelined = gpu && !pipelineDisabled && cfg.ioDepth == 1 &&
                              !cfg.useMmap && cfg.flockMode == 0 &&
                              !rwMixActive && !cfg.verifyDirect && hostBufs.size() >= 2 &&
                              !eng.opsLog.isEnabled(); // tracing needs per-op hooks
    if (gpuPipelined) {
        constexpr uint64_t VERIFY_FETCH_INTERVAL = 64;
        const bool doVerify = eng.dataVerify;
        const bool doCheck = doVerify || profiling; // per-block path, as --verify takes
        const bool lat = cfg.measureLat;
        const int nSlots = (int)hostBufs.size();
        std::vector<char> slotBusy(nSlots, 0);
        uint64_t sinceFetch = 0;
        BlockSpec spec;
        uint64_t opCount = 0;

        auto fetchVerify = [&]() { gpuVerifyFetch(); };

        if (isWrite) {
            // one-block lookahead: prepare (fill + D2H) next while pwriting cur
            int slot = 0;
            bool havePrev = false;
            int prevSlot = 0;
            uint64_t prevFileIdx = 0, prevInFileOff = 0, prevIoLen = 0;

            for (;;) {
                bool haveCur = false;
                uint64_t fileIdx = 0, inFileOff = 0, ioLen = 0;
                while (gen->next(spec)) {
                    if (mapBlock(spec, fileIdx, inFileOff, ioLen)) {
                        haveCur = true;
                        break;
                    }
                }

                if (haveCur) {
                    if ((opCount++ % INTERRUPT_CHECK_INTERVAL) == 0) checkInterrupt();
                    rateLimiter.wait(ioLen);
                    if (slotBusy[slot]) gpu->waitSlotEvent(slot);
                    setSlotFileKey(slot, fileIdx);
                    preWriteFill(slot, ioLen, inFileOff);
                    if (lat) gpu->recordTimedStart(slot);
                    gpu->copyD2HAsync(slot, ioLen);
                    if (lat) gpu->recordTimedEnd(slot);
                    gpu->recordSlotEvent(slot);
                    slotBusy[slot] = 1;
                }

                if (havePrev) { // write the previously prepared block
                    gpu->waitSlotEvent(prevSlot);
                    // --lat: D2H copy exec time + pwrite wall time
                    uint64_t copyUs = (lat && gpu->timedPairActive(prevSlot))
                                          ? gpu->timedElapsedUSec(prevSlot) : 0;
                    auto t0 = lat ? Clock::now() : Clock::time_point();
                    ssize_t res = pwrite(fg.fds[prevFileIdx], hostBufs[prevSlot],
                                         prevIoLen, prevInFileOff);
                    if (res != (ssize_t)prevIoLen) throwErrno("write", cfg.paths[prevFileIdx]);
                    if (lat)
                        addIoLat(copyUs + (uint64_t)std::chrono::duration_cast<
                            std::chrono::microseconds>(Clock::now() - t0).count());
                    liveOps.bytes.fetch_add(prevIoLen, std::memory_order_relaxed);
                    liveOps.iops.fetch_add(1, std::memory_order_relaxed);
                }

                if (!haveCur) break;
                havePrev = true;
                prevSlot = slot;
                prevFileIdx = fileIdx;
                prevInFileOff = inFileOff;
                prevIoLen = ioLen;
                slot = (slot + 1) % nSlots;
            }
            if (cfg.fsyncPerFile)
                for (size_t i = 0; i < fg.fds.size(); i++)
                    if (fsync(fg.fds[i])) throwErrno("fsync", cfg.paths[i]);
        } else if (!doCheck && gpuBatchSlots(cfg.blockSize) >= 2 && nSlots >= 4) {
            // batched read: fill half the ring with preads, then one ranged
            // H2D covers all of them (slots are contiguous); the other half
            // stages while this half reads. --lat: per block = its pread
            // wall time + an equal share of its batch's ranged-copy time.
            const int batch = gpuBatchSlots(cfg.blockSize);
            int half = 0; // 0 -> slots [0, batch), 1 -> [batch, 2*batch)
            bool halfBusy[2] = {false, false};
            std::vector<uint64_t> blkUs[2];
            int halfCount[2] = {0, 0};
            if (lat) {
                blkUs[0].resize(batch);
                blkUs[1].resize(batch);
            }

            auto collectHalfLat = [&](int h) { // after the half's copy is done
                if (!lat || !halfCount[h]) return;
                int b = h * batch;
                if (!gpu->timedPairActive(b)) return;
                uint64_t share = gpu->timedElapsedUSec(b) / (uint64_t)halfCount[h];
                for (int i = 0; i < halfCount[h]; i++)
                    addIoLat(blkUs[h][i] + share);
                halfCount[h] = 0;
            };

            int filled = 0;
            int base = 0;
            while (gen->next(spec)) {
                uint64_t fileIdx, inFileOff, ioLen;
                if (!mapBlock(spec, fileIdx, inFileOff, ioLen)) continue;

                if (filled == 0) {
                    if ((opCount++ % 4) == 0) checkInterrupt();
                    base = half * batch;
                    if (halfBusy[half]) {
                        gpu->waitSlotEvent(base); // ring reuse
                        collectHalfLat(half);
                    }
                }

                rateLimiter.wait(ioLen);
                auto t0 = lat ? Clock::now() : Clock::time_point();
                ssize_t res = pread(fg.fds[fileIdx], hostBufs[base + filled], ioLen,
                                    inFileOff);
                if (res != (ssize_t)ioLen) throwErrno("read", cfg.paths[fileIdx]);
                if (lat)
                    blkUs[half][filled] = (uint64_t)std::chrono::duration_cast<
                        std::chrono::microseconds>(Clock::now() - t0).count();
                liveOps.bytes.fetch_add(ioLen, std::memory_order_relaxed);
                liveOps.iops.fetch_add(1, std::memory_order_relaxed);
                filled++;

                if (filled == batch) {
                    if (lat) {
                        halfCount[half] = batch;
                        gpu->recordTimedStart(base);
                    }
                    gpu->copyH2DRangeAsync(base, batch);
                    if (lat) gpu->recordTimedEnd(base);
                    gpu->recordSlotEvent(base); // event indexed by ring base
                    halfBusy[half] = true;
                    half ^= 1;
                    filled = 0;
                }
            }
            if (filled) { // tail batch
                int b = half * batch;
                if (lat) {
                    halfCount[half] = filled;
                    gpu->recordTimedStart(b);
                }
                gpu->copyH2DRangeAsync(b, filled);
                if (lat) gpu->recordTimedEnd(b);
            }
            if (lat) { // drain both halves' pending samples
                gpu->syncStream();
                collectHalfLat(0);
                collectHalfLat(1);
            }
        } else {
            // a READ that threw mid-window (CPU tail check, I/O error,
            // interrupt) leaves its unfetched mismatches in this persistent
            // context's counters: drop them so they are not reported now
            if (doVerify) gpuVerifyDropStale();
            int slot = 0;
            std::vector<uint64_t> preadUs(lat ? nSlots : 0, 0);
            while (gen->next(spec)) {
                if ((opCount++ % INTERRUPT_CHECK_INTERVAL) == 0) checkInterrupt();

                uint64_t fileIdx, inFileOff, ioLen;
                if (!mapBlock(spec, fileIdx, inFileOff, ioLen)) continue;

                rateLimiter.wait(ioLen);
                if (slotBusy[slot]) gpu->waitSlotEvent(slot); // host buf reuse
                if (lat && gpu->timedPairActive(slot)) // prior block's sample
                    addIoLat(preadUs[slot] + gpu->timedElapsedUSec(slot));

                auto t0 = lat ? Clock::now() : Clock::time_point();
                ssize_t res = pread(fg.fds[fileIdx], hostBufs[slot], ioLen, inFileOff);
                if (res != (ssize_t)ioLen) throwErrno("read", cfg.paths[fileIdx]);
                if (lat) {
                    preadUs[slot] = (uint64_t)std::chrono::duration_cast<
                        std::chrono::microseconds>(Clock::now() - t0).count();
                    gpu->recordTimedStart(slot);
                }

                gpu->copyH2DAsync(slot, ioLen);
                if (lat) gpu->recordTimedEnd(slot);
                if (doCheck) {
                    setSlotFileKey(slot, fileIdx);
                    if ((inFileOff % 8 == 0) && (ioLen % 16 == 0)) {
                        if (doVerify) gpuVerifyAsync(slot, ioLen, inFileOff);
                        profileGpuAsync(slot, ioLen);
                        if (doVerify && ++sinceFetch >= VERIFY_FETCH_INTERVAL) {
                            fetchVerify();
                            sinceFetch = 0;
                        }
                    } else { // odd tail: CPU check of the host copy
                        if (doVerify) cpuVerify(slot, hostBufs[slot], ioLen, inFileOff);
                        profileCpu(hostBufs[slot], ioLen);
                    }
                }
                gpu->recordSlotEvent(slot);
                slotBusy[slot] = 1;

                liveOps.bytes.fetch_add(ioLen, std::memory_order_relaxed);
                liveOps.iops.fetch_add(1, std::memory_order_relaxed);
                slot = (slot + 1) % nSlots;
            }
            if (doVerify) fetchVerify();
            if (lat) { // drain remaining per-slot samples
                gpu->syncStream();
                for (int s = 0; s < nSlots; s++)
                    if (gpu->timedPairActive(s))
                        addIoLat(preadUs[s] + gpu->timedElapsedUSec(s));
            }
        }

        gpu->syncStream(); // drain outstanding staging copies before finishing
        return;
    }

    const bool lat = cfg.measureLat;
    BlockSpec spec;
    uint64_t opCount = 0;

    while (gen->next(spec)) {
        if ((opCount++ % INTERRUPT_CHECK_INTERVAL) == 0) checkInterrupt();

        uint64_t fileIdx, inFileOff, ioLen;
        if (!mapBlock(spec, fileIdx, inFileOff, ioLen)) continue;

        // rwmix: dedicated readers always read; otherwise hold reads/total
        // at rwMixPct (reference --rwmixpct / --rwmixthr semantics)
        // with dedicated reader threads (--rwmixthr) the pct is a BYTE ratio
        // held by the balancer; without them it is a per-block read probability
        bool mixRead = rwMixActive &&
                       (isDedicatedReader ||
                        (cfg.rwMixThreads == 0 && rwMixDecideRead()));
        bool blockWrite = isWrite && !mixRead;

        if (rwMixActive && rwBalancerActive()) rwBalanceWait(mixRead, ioLen);

        auto t0 = lat ? Clock::now() : Clock::time_point();

        setSlotFileKey(0, fileIdx);
        ssize_t res = blockIO(blockWrite, fg.fds[fileIdx], 0, ioLen, inFileOff,
                              mg.base(fileIdx), &cfg.paths[fileIdx]);
        if (res < 0)
            throwErrno(blockWrite ? "write" : "read", cfg.paths[fileIdx]);
        if ((uint64_t)res != ioLen)
            throw WorkerError(std::string("unexpected short ") + (blockWrite ? "write" : "read") +
                              ". Path: " + cfg.paths[fileIdx] +
                              "; expected: " + std::to_string(ioLen) +
                              "; got: " + std::to_string(res) +
                              (mixRead ? "; Hint: rwmix reads need a pre-written file." : ""));

        if (lat)
            addIoLat((uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(
                Clock::now() - t0).count(), mixRead);

        AtomicLiveOps& ops = mixRead ? liveOpsReadMix : liveOps;
        ops.bytes.fetch_add(ioLen, std::memory_order_relaxed);
        ops.iops.fetch_add(1, std::memory_order_relaxed);
        if (rwMixActive && rwBalancerActive()) rwBalanceAccount(mixRead, ioLen);
    }

    if (isWrite && cfg.fsyncPerFile)
        for (size_t i = 0; i < fg.fds.size(); i++)
            if (fsync(fg.fds[i])) throwErrno("fsync", cfg.paths[i]);
}

// mmap + GPU zero-copy: every block is ONE hipMemcpyAsync between pinned
// page-cache pages and the worker's HBM slot ring — no pread/pwrite, no host
// bounce buffer. The MI355X-native answer to cuFile for cache-resident data.
void Worker::fileModeBlocksGpuMmap(bool isWrite)
{
    const auto& cfg = eng.cfg;
    const uint64_t fileSize = eng.effFileSize;
    const uint64_t bs = cfg.blockSize;
    const size_t numFiles = cfg.paths.size();
    const uint64_t numBlocksPerFile = (fileSize + bs - 1) / bs;
    const bool doVerify = eng.dataVerify;
    const bool lat = cfg.measureLat;

    // registered mappings (cached in the engine across phases)
    std::vector<char*> bases(numFiles);
    for (size_t i = 0; i < numFiles; i++)
        bases[i] = eng.getMappedReg(cfg.paths[i], fileSize, isWrite).base;

    const uint64_t mapBPF = (cfg.random || cfg.strided) ? (fileSize / bs) : numBlocksPerFile;
    const uint64_t virtFileLen = mapBPF * bs;

    // --dynslice: all workers of this instance pull blocks from one shared
    // atomic cursor — no static slices, no straggler tail (the phase ends
    // when the work is gone, not when the slowest fixed slice finishes)
    const bool dynamic = cfg.dynamicSlice && !cfg.random && !cfg.strided &&
                         !cfg.backward && cfg.numThreads == cfg.numDataSetThreads;

    std::unique_ptr<OffsetGen> gen;
    if (dynamic) {
        // driver loop below pulls from eng.dynCursor
    } else if (cfg.random || cfg.strided) {
        uint64_t numBlocksTotal = mapBPF * numFiles;
        uint64_t rangeLen = bs * (numBlocksTotal / cfg.numDataSetThreads);
        uint64_t rangeOff = (uint64_t)globalRank * rangeLen;
        if (cfg.strided) {
            gen = std::make_unique<OffsetGenStrided>(bs, globalRank, cfg.numDataSetThreads);
            gen->reset(0, bs * numBlocksTotal);
        } else {
            gen = makeOffsetGen(rangeOff, rangeLen);
        }
    } else {
        uint64_t myStart, myLen;
        fairShareSlice(virtFileLen * numFiles, myStart, myLen);
        if (!myLen) return;
        gen = makeOffsetGen(myStart, myLen);
    }

    const int nSlots = (int)hostBufs.size();
    constexpr uint64_t VERIFY_FETCH_INTERVAL = 64;
    uint64_t sinceFetch = 0;
    BlockSpec spec;
    uint64_t opCount = 0;
    int slot = 0;

    auto fetchVerify = [&]() { gpuVerifyFetch(); };

    // drop mismatches that a READ which threw mid-window left unfetched in
    // this persistent context's counters (see fileModeBlocks)
    if (doVerify && !isWrite) gpuVerifyDropStale();

    const uint64_t totalBlocks = numBlocksPerFile * numFiles;

    auto nextBlock = [&](uint64_t& fileIdx, uint64_t& inFileOff,
                         uint64_t& ioLen) -> bool {
        if (dynamic) {
            for (;;) {
                uint64_t b = eng.dynCursor.fetch_add(1, std::memory_order_relaxed);
                if (b >= totalBlocks) return false;
                fileIdx = b / numBlocksPerFile;
                inFileOff = (b % numBlocksPerFile) * bs;
                if (inFileOff >= fileSize) continue;
                ioLen = std::min(bs, fileSize - inFileOff);
                return true;
            }
        }
        while (gen->next(spec)) {
            if (!virtFileLen) return false;
            fileIdx = spec.offset / virtFileLen;
            if (fileIdx >= numFiles) continue;
            inFileOff = spec.offset - fileIdx * virtFileLen;
            if (inFileOff >= fileSize) continue;
            ioLen = std::min(spec.len, fileSize - inFileOff);
            return true;
        }
        return false;
    };

    uint64_t fileIdx, inFileOff, ioLen;
    while (nextBlock(fileIdx, inFileOff, ioLen)) {
        if ((opCount++ % INTERRUPT_CHECK_INTERVAL) == 0) checkInterrupt();

        rateLimiter.wait(ioLen);

        // --lat: collect the slot's previous timed copy before reusing it;
        // the hipEvent pair brackets ONLY the staging memcpy on the stream,
        // so p99 into-HBM latency is measured at full pipelining
        if (lat && gpu->timedPairActive(slot))
            addIoLat(gpu->timedElapsedUSec(slot));

        setSlotFileKey(slot, fileIdx);
        if (isWrite) {
            // fill the HBM slot, then DMA into the mapped file pages
            preWriteFill(slot, ioLen, inFileOff);
            if (lat) gpu->recordTimedStart(slot);
            gpu->copyToHostAsync(slot, bases[fileIdx] + inFileOff, ioLen);
            if (lat) gpu->recordTimedEnd(slot);
        } else {
            if (lat) gpu->recordTimedStart(slot);
            gpu->copyFromHostAsync(slot, bases[fileIdx] + inFileOff, ioLen);
            if (lat) gpu->recordTimedEnd(slot);
            if ((doVerify || profiling) && (inFileOff % 8 == 0) && (ioLen % 16 == 0)) {
                if (doVerify) gpuVerifyAsync(slot, ioLen, inFileOff);
                profileGpuAsync(slot, ioLen);
                if (doVerify && ++sinceFetch >= VERIFY_FETCH_INTERVAL) {
                    fetchVerify();
                    sinceFetch = 0;
                }
            } else if (doVerify || profiling) { // odd tail: check the mapped pages directly
                if (doVerify) cpuVerify(slot, bases[fileIdx] + inFileOff, ioLen, inFileOff);
                profileCpu(bases[fileIdx] + inFileOff, ioLen);
            }
        }

        liveOps.bytes.fetch_add(ioLen, std::memory_order_relaxed);
        liveOps.iops.fetch_add(1, std::memory_order_relaxed);
        slot = (slot + 1) % nSlots;

        if ((opCount & 127) == 0) gpu->syncStream(); // bound the async queue
    }

    gpu->syncStream();
    if (lat) // drain the remaining timed pairs
        for (int s = 0; s < nSlots; s++)
            if (gpu->timedPairActive(s)) addIoLat(gpu->timedElapsedUSec(s));
    if (doVerify && !isWrite) fetchVerify();
}

void Worker::fileModeBlocksUring(bool isWrite)
{
    const auto& cfg = eng.cfg;
    const uint64_t fileSize = eng.effFileSize;
    const uint64_t bs = cfg.blockSize;
    const size_t numFiles = cfg.paths.size();
    const uint64_t numBlocksPerFile = (fileSize + bs - 1) / bs;
    const int depth = cfg.ioDepth;
    const bool lat = cfg.measureLat;

    const bool rwMixActive = isWrite && (cfg.rwMixPct > 0 || isDedicatedReader);

    FdGuard fg;
    int rwFlags = isWrite ? ((cfg.verifyDirect || rwMixActive) ? O_RDWR : O_WRONLY) : O_RDONLY;
    int openFlags = rwFlags | (cfg.directIO ? O_DIRECT : 0);
    if (isWrite && cfg.pathType == PathType::FILE) openFlags |= O_CREAT;
    for (const auto& p : cfg.paths) {
        int fd = open(p.c_str(), openFlags, 0644);
        if (fd < 0) throwErrno("open", p);
        fg.fds.push_back(fd);
        if (isWrite && cfg.pathType == PathType::FILE) {
            if (cfg.truncate && ftruncate(fd, 0)) throwErrno("truncate", p);
            if (cfg.truncToSize != UINT64_MAX && ftruncate(fd, fileSize))
                throwErrno("truncate-to-size", p);
            if (cfg.preallocFile && fallocate(fd, 0, 0, fileSize)) throwErrno("fallocate", p);
        }
        applyFadvise(fd, cfg.fadviseFlags, p);
    }

    const uint64_t mapBPF = (cfg.random || cfg.strided) ? (fileSize / bs) : numBlocksPerFile;
    const uint64_t virtFileLen = mapBPF * bs;

    auto mapBlock = [&](const BlockSpec& s, uint64_t& fileIdx, uint64_t& inFileOff,
                        uint64_t& ioLen) -> bool {
        if (!virtFileLen) return false;
        fileIdx = s.offset / virtFileLen;
        if (fileIdx >= numFiles) return false;
        inFileOff = s.offset - fileIdx * virtFileLen;
        if (inFileOff >= fileSize) return false;
        ioLen = std::min(s.len, fileSize - inFileOff);
        return true;
    };

    std::unique_ptr<OffsetGen> gen;
    if (cfg.random || cfg.strided) {
        uint64_t numBlocksTotal = mapBPF * numFiles;
        uint64_t rangeLen = bs * (numBlocksTotal / cfg.numDataSetThreads);
        uint64_t rangeOff = (uint64_t)globalRank * rangeLen;
        if (cfg.strided) {
            gen = std::make_unique<OffsetGenStrided>(bs, globalRank, cfg.numDataSetThreads);
            gen->reset(0, bs * numBlocksTotal);
        } else {
            gen = makeOffsetGen(rangeOff, rangeLen);
        }
    } else {
        uint64_t myStart, myLen;
        fairShareSlice(virtFileLen * numFiles, myStart, myLen);
        if (!myLen) return;
        gen = makeOffsetGen(myStart, myLen);
    }

    IoUring ring;
    ring.init(depth);

    // fixed buffers + registered files: one-time page pin / fd ref instead of
    // per-op (EB_URING_NOFIXED=1 disables; silent fallback if the kernel
    // refuses, e.g. RLIMIT_MEMLOCK without CAP_IPC_LOCK)
    if (!getenv("EB_URING_NOFIXED")) {
        std::vector<struct iovec> iovs(depth);
        for (int s = 0; s < depth; s++)
            iovs[s] = {hostBufs[s], (size_t)bs};
        ring.registerBuffers(iovs.data(), depth);
        ring.registerFiles(fg.fds.data(), (unsigned)fg.fds.size());
    }

    // Batched GPU staging for small-block async reads (BASELINE config 3:
    // 4K random read, io_uring QD128, buffers in HBM): per-block 4K
    // hipMemcpyAsync caps at ~150K IOPS (launch-bound); instead the ring is
    // split into two halves — when every read of a half has completed, ONE
    // ranged H2D covers all its contiguous slots while the other half's
    // storage reads stay in flight (same geometry as the sync path's
    // half-ring batching above).
    // measured (profiles/r01_uring_iops.md): at QD>=32 the per-block
    // event-pipelined staging below overlaps storage and PCIe better than
    // half-ring batching (5.1M vs 3.4M IOPS warm), so batching here is
    // opt-in (EB_GPU_URING_BATCH=1) — unlike the sync path where it wins
    const int gpuBatch = gpu ? gpuBatchSlots(bs) : 1;
    const bool batchedRead = gpu && !isWrite && !eng.dataVerify && !profiling &&
                             gpuBatch >= 2 && depth >= 4 &&
                             getenv("EB_GPU_URING_BATCH");
    if (getenv("EB_DEBUG_PATH"))
        fprintf(stderr, "[eb] uring path: gpu=%d batchedRead=%d batch=%d depth=%d\n",
                gpu ? 1 : 0, (int)batchedRead, gpuBatch, depth);
    if (batchedRead) {
        const int halfSize = std::min(depth / 2, 64);
        struct Op {
            uint64_t off = 0, len = 0;
            Clock::time_point start;
            int fileIdx = 0;
        };
        std::vector<Op> ops(2 * halfSize);
        std::vector<IoUring::Completion> bcomps(depth);
        int submitted[2] = {0, 0}, done[2] = {0, 0};
        bool exhausted2 = false;
        BlockSpec bspec;

        auto fillHalf = [&](int h) -> int {
            int base = h * halfSize;
            int n = 0;
            while (n < halfSize && !exhausted2) {
                uint64_t fileIdx = 0, inFileOff = 0, ioLen = 0;
                for (;;) {
                    if (!gen->next(bspec)) { exhausted2 = true; break; }
                    if (mapBlock(bspec, fileIdx, inFileOff, ioLen)) break;
                }
                if (exhausted2) break;
                rateLimiter.wait(ioLen);
                int slot = base + n;
                ops[slot] = {inFileOff, ioLen,
                             lat ? Clock::now() : Clock::time_point(), (int)fileIdx};
                if (eng.opsLog.isEnabled())
                    eng.opsLog.log(globalRank, "uring_read", cfg.paths[fileIdx],
                                   inFileOff, ioLen, true, false);
                int rfd = ring.hasFixedFiles() ? (int)fileIdx : fg.fds[fileIdx];
                while (!ring.prep(false, rfd, hostBufs[slot], ioLen, inFileOff,
                                  (uint64_t)slot,
                                  ring.hasFixedBuffers() ? slot : -1,
                                  ring.hasFixedFiles())) {
                    // SQPOLL: the kernel thread may lag behind — kick it
                    ring.submitAndWait(0);
                    checkInterrupt();
                }
                n++;
            }
            submitted[h] = n;
            done[h] = 0;
            return n;
        };

        int inFlightB = fillHalf(0) + fillHalf(1);
        uint64_t opCountB = 0;
        while (inFlightB > 0) {
            checkInterrupt();
            ring.submitAndWait(1, 250);
            unsigned n = ring.reap(bcomps.data(), depth);
            for (unsigned i = 0; i < n; i++) {
                int slot = (int)bcomps[i].userData;
                const Op& op = ops[slot];
                if (eng.opsLog.isEnabled())
                    eng.opsLog.log(globalRank, "uring_read", cfg.paths[op.fileIdx],
                                   op.off, op.len, false, bcomps[i].res < 0);
                if (bcomps[i].res < 0)
                    throw WorkerError(std::string("async read failed. Path: ") +
                                      cfg.paths[op.fileIdx] + "; SysErr: " +
                                      strerror(-bcomps[i].res));
                if ((uint64_t)bcomps[i].res != op.len)
                    throw WorkerError("unexpected short async read. Path: " +
                                      cfg.paths[op.fileIdx]);
                if (lat)
                    addIoLat((uint64_t)std::chrono::duration_cast<
                        std::chrono::microseconds>(Clock::now() - op.start).count());
                liveOps.bytes.fetch_add(op.len, std::memory_order_relaxed);
                liveOps.iops.fetch_add(1, std::memory_order_relaxed);
                done[slot / halfSize]++;
                inFlightB--;
                if ((opCountB++ % INTERRUPT_CHECK_INTERVAL) == 0) checkInterrupt();
            }
            for (int h = 0; h < 2; h++) {
                if (submitted[h] && done[h] == submitted[h]) {
                    int base = h * halfSize;
                    gpu->copyH2DRangeAsync(base, submitted[h]);
                    gpu->recordSlotEvent(base);
                    if (!exhausted2) {
                        // short PCIe wait before the slots' host bufs are
                        // reused; the other half's reads stay in flight
                        gpu->waitSlotEvent(base);
                        inFlightB += fillHalf(h);
                    } else {
                        submitted[h] = 0; // drained
                    }
                }
            }
        }
        gpu->syncStream();
        return;
    }

    struct SlotState {
        uint64_t inFileOff = 0;
        uint64_t len = 0;
        Clock::time_point start;
        int fileIdx = 0;
        bool isWriteOp = true;
    };
    std::vector<SlotState> slots(depth);
    std::vector<char> slotHasCopy(depth, 0);

    BlockSpec spec;
    int inFlight = 0;
    bool exhausted = false;
    std::vector<IoUring::Completion> comps(depth);

    auto prepSlot = [&](int slot) -> bool {
        if (!gen->next(spec)) return false;
        uint64_t fileIdx, inFileOff, ioLen;
        if (!mapBlock(spec, fileIdx, inFileOff, ioLen)) return true; // skip this block

        bool mixRead = rwMixActive &&
                       (isDedicatedReader ||
                        (cfg.rwMixThreads == 0 && rwMixDecideRead()));
        bool blockWrite = isWrite && !mixRead;

        rateLimiter.wait(ioLen);
        if (gpu && slotHasCopy[slot]) { // prior async staging of this slot
            gpu->waitSlotEvent(slot);
            slotHasCopy[slot] = false;
        }
        setSlotFileKey(slot, fileIdx);
        if (blockWrite) {
            preWriteFill(slot, ioLen, inFileOff);
            if (gpu) {
                gpu->copyD2HAsync(slot, ioLen);
                gpu->syncStream();
            }
        }

        slots[slot] = {inFileOff, ioLen, lat ? Clock::now() : Clock::time_point(),
                       (int)fileIdx, blockWrite};
        if (eng.opsLog.isEnabled())
            eng.opsLog.log(globalRank, blockWrite ? "uring_write" : "uring_read",
                           cfg.paths[fileIdx], inFileOff, ioLen, true, false);
        int ringFd = ring.hasFixedFiles() ? (int)fileIdx : fg.fds[fileIdx];
        while (!ring.prep(blockWrite, ringFd, hostBufs[slot], ioLen, inFileOff,
                          (uint64_t)slot, ring.hasFixedBuffers() ? slot : -1,
                          ring.hasFixedFiles())) {
            ring.submitAndWait(0); // SQPOLL: kernel thread may lag
            checkInterrupt();
        }
        inFlight++;
        return true;
    };

    // seed the queue
    for (int s = 0; s < depth && !exhausted; s++)
        if (!prepSlot(s)) exhausted = true;

    uint64_t opCount = 0;

    while (inFlight > 0) {
        checkInterrupt();
        ring.submitAndWait(1, 250); // bounded: interrupt checks keep running
        unsigned n = ring.reap(comps.data(), depth);
        for (unsigned i = 0; i < n; i++) {
            int slot = (int)comps[i].userData;
            SlotState& st = slots[slot];
            inFlight--;

            const bool wasWrite = st.isWriteOp;
            if (eng.opsLog.isEnabled())
                eng.opsLog.log(globalRank, wasWrite ? "uring_write" : "uring_read",
                               cfg.paths[st.fileIdx], st.inFileOff, st.len, false,
                               comps[i].res < 0);
            if (comps[i].res < 0)
                throw WorkerError(std::string("async ") + (wasWrite ? "write" : "read") +
                                  " failed. Path: " + cfg.paths[st.fileIdx] +
                                  "; SysErr: " + strerror(-comps[i].res));
            if ((uint64_t)comps[i].res != st.len)
                throw WorkerError(std::string("unexpected short async ") +
                                  (wasWrite ? "write" : "read") +
                                  ". Path: " + cfg.paths[st.fileIdx]);

            if (!wasWrite) {
                if (gpu) {
                    gpu->copyH2DAsync(slot, st.len);
                    if ((eng.dataVerify || profiling) && !isWrite) {
                        gpu->syncStream();
                        postReadCheck(slot, st.len, st.inFileOff);
                    } else { // pipelined: wait only when the slot is reused
                        gpu->recordSlotEvent(slot);
                        slotHasCopy[slot] = 1;
                    }
                } else if (!isWrite) {
                    postReadCheck(slot, st.len, st.inFileOff);
                }
            }

            const bool mixRead = isWrite && !wasWrite;
            if (lat)
                addIoLat((uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(
                    Clock::now() - st.start).count(), mixRead);

            AtomicLiveOps& ops = mixRead ? liveOpsReadMix : liveOps;
            ops.bytes.fetch_add(st.len, std::memory_order_relaxed);
            ops.iops.fetch_add(1, std::memory_order_relaxed);

            if ((opCount++ % INTERRUPT_CHECK_INTERVAL) == 0) checkInterrupt();

            if (!exhausted && !prepSlot(slot)) exhausted = true;
        }
    }

    if (gpu) gpu->syncStream(); // drain async staging copies
}

void Worker::fileModeDelete()
{
    const auto& cfg = eng.cfg;
    for (size_t i = 0; i < cfg.paths.size(); i++) {
        if ((int)(i % cfg.numDataSetThreads) != globalRank) continue;
        checkInterrupt();
        if (unlink(cfg.paths[i].c_str())) {
            if (!cfg.ignoreDelErrors) throwErrno("unlink", cfg.paths[i]);
        }
        liveOps.entries.fetch_add(1, std::memory_order_relaxed);
    }
}

void Worker::fileModeStat()
{
    const auto& cfg = eng.cfg;
    struct stat st;
    for (size_t i = 0; i < cfg.paths.size(); i++) {
        if ((int)(i % cfg.numDataSetThreads) != globalRank) continue;
        checkInterrupt();
        if (stat(cfg.paths[i].c_str(), &st)) throwErrno("stat", cfg.paths[i]);
        liveOps.entries.fetch_add(1, std::memory_order_relaxed);
    }
}

// ---------------------------------------------------------------------------
// dir mode
// ---------------------------------------------------------------------------

void Worker::dirModeMkdirs()
{
    const auto& cfg = eng.cfg;
    const bool lat = cfg.measureLat;
    const int dirRank = cfg.dirSharing ? 0 : globalRank; // --dirsharing
    char rel[64];

    // rank root dir under every bench path that this worker will use
    snprintf(rel, sizeof(rel), "r%d", dirRank);
    for (const auto& p : cfg.paths) mkdirIgnoreExists(p + "/" + rel);

    for (uint64_t d = 0; d < cfg.numDirs; d++) {
        if ((d % INTERRUPT_CHECK_INTERVAL) == 0) checkInterrupt();
        size_t pathIdx = (dirRank + d) % cfg.paths.size();
        snprintf(rel, sizeof(rel), "r%d/d%lu", dirRank, (unsigned long)d);
        std::string full = cfg.paths[pathIdx] + "/" + rel;

        auto t0 = lat ? Clock::now() : Clock::time_point();
        if (mkdir(full.c_str(), 0777) && errno != EEXIST) throwErrno("mkdir", full);
        if (lat)
            addEntryLat((uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(
                Clock::now() - t0).count());
        liveOps.entries.fetch_add(1, std::memory_order_relaxed);
    }
}

void Worker::dirModeRmdirs()
{
    const auto& cfg = eng.cfg;
    const bool lat = cfg.measureLat;
    const int dirRank = cfg.dirSharing ? 0 : globalRank;
    char rel[64];

    // with --dirsharing only one worker removes the shared dirs
    if (cfg.dirSharing && globalRank != cfg.rankOffset) return;

    for (uint64_t d = 0; d < cfg.numDirs; d++) {
        if ((d % INTERRUPT_CHECK_INTERVAL) == 0) checkInterrupt();
        size_t pathIdx = (dirRank + d) % cfg.paths.size();
        snprintf(rel, sizeof(rel), "r%d/d%lu", dirRank, (unsigned long)d);
        std::string full = cfg.paths[pathIdx] + "/" + rel;

        auto t0 = lat ? Clock::now() : Clock::time_point();
        if (rmdir(full.c_str())) {
            if (!cfg.ignoreDelErrors) throwErrno("rmdir", full);
        }
        if (lat)
            addEntryLat((uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(
                Clock::now() - t0).count());
        liveOps.entries.fetch_add(1, std::memory_order_relaxed);
    }

    // rank root dirs (not counted as entries)
    snprintf(rel, sizeof(rel), "r%d", dirRank);
    for (const auto& p : cfg.paths) {
        std::string full = p + "/" + rel;
        if (rmdir(full.c_str()) && errno != ENOENT && errno != ENOTEMPTY) {
            if (!cfg.ignoreDelErrors) throwErrno("rmdir", full);
        }
    }
}

// ---------------------------------------------------------------------------
// dir/custom-tree async block engine (--iodepth in dir + tree modes).
// Reference parity: the function-pointer pipeline applies aioBlockSized in
// EVERY rw mode (LocalWorker.cpp:1210-1379, :1828-2070), per file. Here one
// io_uring ring (+ fixed buffers) lives for the whole phase and each file's
// offset stream runs through it at cfg.ioDepth.
// ---------------------------------------------------------------------------

struct Worker::FileUring {
    IoUring ring;
    std::vector<IoUring::Completion> comps;
    struct Slot {
        uint64_t off = 0, len = 0;
        Worker::Clock::time_point start;
        bool isWriteOp = true;
    };
    std::vector<Slot> slots;
    std::vector<char> slotHasCopy;
    int depth;

    FileUring(int d, const std::vector<char*>& bufs, uint64_t blockSize) : depth(d)
    {
        ring.init(depth);
        comps.resize(depth);
        slots.resize(depth);
        slotHasCopy.assign(depth, 0);
        if (!getenv("EB_URING_NOFIXED")) {
            std::vector<struct iovec> iovs(depth);
            for (int s = 0; s < depth; s++)
                iovs[s] = {bufs[s], (size_t)blockSize};
            ring.registerBuffers(iovs.data(), depth);
        }
    }
};

void Worker::uringFileBlocks(FileUring& u, int fd, const std::string& path,
                             OffsetGen& gen, bool phaseIsWrite, bool rwMixActive,
                             bool allMixRead, bool checkMixReads)
{
    const auto& cfg = eng.cfg;
    const bool lat = cfg.measureLat;
    const int depth = u.depth;
    const bool logOps = eng.opsLog.isEnabled();

    BlockSpec spec;
    int inFlight = 0;
    bool exhausted = false;

    auto prepSlot = [&](int slot) -> bool {
        if (!gen.next(spec)) return false;
        bool mixRead = allMixRead ||
                       (rwMixActive && cfg.rwMixThreads == 0 && rwMixDecideRead());
        bool blockWrite = phaseIsWrite && !mixRead;
        rateLimiter.wait(spec.len);
        if (gpu && u.slotHasCopy[slot]) { // prior async staging of this slot
            gpu->waitSlotEvent(slot);
            u.slotHasCopy[slot] = 0;
        }
        if (blockWrite) {
            preWriteFill(slot, spec.len, spec.offset);
            if (gpu) {
                gpu->copyD2HAsync(slot, spec.len);
                gpu->syncStream();
            }
        }
        u.slots[slot] = {spec.offset, spec.len,
                         lat ? Clock::now() : Clock::time_point(), blockWrite};
        if (logOps)
            eng.opsLog.log(globalRank, blockWrite ? "uring_write" : "uring_read",
                           path, spec.offset, spec.len, true, false);
        while (!u.ring.prep(blockWrite, fd, hostBufs[slot], spec.len, spec.offset,
                            (uint64_t)slot,
                            u.ring.hasFixedBuffers() ? slot : -1, false)) {
            u.ring.submitAndWait(0); // SQPOLL: kernel thread may lag
            checkInterrupt();
        }
        inFlight++;
        return true;
    };

    for (int s = 0; s < depth && !exhausted; s++)
        if (!prepSlot(s)) exhausted = true;

    uint64_t opCount = 0;
    while (inFlight > 0) {
        checkInterrupt();
        u.ring.submitAndWait(1, 250); // bounded: interrupt checks keep running
        unsigned n = u.ring.reap(u.comps.data(), depth);
        for (unsigned i = 0; i < n; i++) {
            int slot = (int)u.comps[i].userData;
            FileUring::Slot& st = u.slots[slot];
            inFlight--;

            const bool wasWrite = st.isWriteOp;
            if (logOps)
                eng.opsLog.log(globalRank, wasWrite ? "uring_write" : "uring_read",
                               path, st.off, st.len, false, u.comps[i].res < 0);
            if (u.comps[i].res < 0)
                throw WorkerError(std::string("async ") + (wasWrite ? "write" : "read") +
                                  " failed. Path: " + path + "; SysErr: " +
                                  strerror(-u.comps[i].res));
            if ((uint64_t)u.comps[i].res != st.len)
                throw WorkerError(std::string("unexpected short async ") +
                                  (wasWrite ? "write" : "read") + ". Path: " + path);

            if (!wasWrite) {
                const bool check = !phaseIsWrite || checkMixReads;
                if (gpu) {
                    gpu->copyH2DAsync(slot, st.len);
                    if ((eng.dataVerify && check) || profiling) {
                        gpu->syncStream();
                        postReadCheck(slot, st.len, st.off);
                    } else { // pipelined: wait only when the slot is reused
                        gpu->recordSlotEvent(slot);
                        u.slotHasCopy[slot] = 1;
                    }
                } else if (check) {
                    postReadCheck(slot, st.len, st.off);
                }
            }

            const bool mixRead = phaseIsWrite && !wasWrite;
            if (lat)
                addIoLat((uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(
                    Clock::now() - st.start).count(), mixRead);
            AtomicLiveOps& ops = mixRead ? liveOpsReadMix : liveOps;
            ops.bytes.fetch_add(st.len, std::memory_order_relaxed);
            ops.iops.fetch_add(1, std::memory_order_relaxed);

            if ((opCount++ % INTERRUPT_CHECK_INTERVAL) == 0) checkInterrupt();

            if (!exhausted && !prepSlot(slot)) exhausted = true;
        }
    }
}

// Small-file metadata pipeline: open -> write/read -> close per file as a
// LINKED io_uring chain on direct descriptors (fds live only in the ring's
// fixed file table), `iodepth` whole files in flight per thread. The
// reference's libaio engine cannot overlap metadata ops at all
// (aio covers data only); this is the io_uring-first payoff for the
// mdtest-style small-file configs (BASELINE config 4).
bool Worker::dirModeSmallFileUring(bool isWrite)
{
    const auto& cfg = eng.cfg;
    const bool lat = cfg.measureLat;
    const uint64_t fileSize = cfg.fileSize;
    const bool haveSubdirs = (cfg.numDirs > 0);
    const uint64_t numDirs = haveSubdirs ? cfg.numDirs : 1;
    const int dirRank = cfg.dirSharing ? 0 : globalRank;
    const int depth = std::min<int>(cfg.ioDepth, (int)hostBufs.size());
    const bool doVerify = eng.dataVerify || profiling; // per-file check after the copy

    int openFlags = isWrite ? (O_CREAT | O_WRONLY) : O_RDONLY;
    if (cfg.directIO) openFlags |= O_DIRECT;
    if (isWrite && cfg.truncate) openFlags |= O_TRUNC;

    IoUring ring;
    ring.init(3u * depth); // one chain = up to 3 SQEs per in-flight file
    if (!ring.registerFilesSparse(depth)) return false; // old kernel
    { // cap io-wq workers: punted opens/closes thrash otherwise
        static const unsigned iowq = [] {
            const char* v = getenv("EB_SF_IOWQ");
            return v ? (unsigned)atoi(v) : 2u;
        }();
        if (iowq) ring.limitWorkers(iowq, iowq);
    }
    {
        std::vector<struct iovec> iovs(depth);
        for (int s = 0; s < depth; s++)
            iovs[s] = {hostBufs[s], (size_t)cfg.blockSize};
        ring.registerBuffers(iovs.data(), depth);
    }

    struct SlotSt {
        std::string path;
        Clock::time_point entryStart, rwStart;
        bool failed = false;
    };
    std::vector<SlotSt> slots(depth);
    std::vector<char> slotHasCopy(depth, 0);
    // userData = slot | stage << 16 (stage: 0 open, 1 rw, 2 close)
    auto ud = [](int slot, int stage) {
        return (uint64_t)slot | ((uint64_t)stage << 16);
    };

    uint64_t nextFile = 0;
    const uint64_t totalFiles = numDirs * cfg.numFiles;
    char rel[128];

    auto startChain = [&](int s) -> bool {
        if (nextFile >= totalFiles) return false;
        uint64_t d = nextFile / cfg.numFiles;
        uint64_t f = nextFile % cfg.numFiles;
        nextFile++;

        size_t pathIdx = (dirRank + d) % cfg.paths.size();
        if (haveSubdirs)
            snprintf(rel, sizeof(rel), "r%d/d%lu/r%d-f%lu", dirRank,
                     (unsigned long)d, globalRank, (unsigned long)f);
        else
            snprintf(rel, sizeof(rel), "r%d-f%lu", globalRank, (unsigned long)f);

        SlotSt& st = slots[s];
        st.path = cfg.paths[pathIdx] + "/" + rel;
        st.failed = false;
        if (lat) st.entryStart = Clock::now();
        setSlotFileKey(s, reduceDirFileKey((uint64_t)globalRank, d, f));

        if (isWrite && fileSize) {
            if (gpu && slotHasCopy[s]) { // prior read staged from this buf
                gpu->waitSlotEvent(s);
                slotHasCopy[s] = 0;
            }
            preWriteFill(s, fileSize, 0);
            if (gpu) {
                gpu->copyD2HAsync(s, fileSize);
                gpu->syncStream();
            }
        } else if (!isWrite && gpu && slotHasCopy[s]) {
            gpu->waitSlotEvent(s); // host buf reuse by the next read
            slotHasCopy[s] = 0;
        }

        bool haveRW = fileSize > 0;
        while (!ring.prepOpenAt(st.path.c_str(), openFlags, 0644, (unsigned)s,
                                ud(s, 0), /*link*/ true)) {
            ring.submitAndWait(0);
            checkInterrupt();
        }
        if (haveRW)
            while (!ring.prep(isWrite, s, hostBufs[s], fileSize, 0, ud(s, 1),
                              ring.hasFixedBuffers() ? s : -1,
                              /*fixedFile*/ true, /*link*/ true)) {
                ring.submitAndWait(0);
                checkInterrupt();
            }
        while (!ring.prepCloseDirect((unsigned)s, ud(s, 2))) {
            ring.submitAndWait(0);
            checkInterrupt();
        }
        return true;
    };

    int inFlight = 0; // chains in flight
    for (int s = 0; s < depth; s++)
        if (startChain(s))
            inFlight++;
        else
            break;

    std::vector<IoUring::Completion> comps(3u * depth);
    uint64_t opCount = 0;

    while (inFlight > 0) {
        checkInterrupt();
        ring.submitAndWait(1, 250); // bounded: interrupt checks keep running
        unsigned n = ring.reap(comps.data(), (unsigned)comps.size());
        for (unsigned i = 0; i < n; i++) {
            int s = (int)(comps[i].userData & 0xFFFF);
            int stage = (int)(comps[i].userData >> 16);
            SlotSt& st = slots[s];
            int32_t res = comps[i].res;

            if (res < 0 && res != -ECANCELED) {
                throw WorkerError(std::string(stage == 0   ? "async open"
                                              : stage == 1 ? (isWrite ? "async write"
                                                                      : "async read")
                                                           : "async close") +
                                  " failed. Path: " + st.path +
                                  "; SysErr: " + strerror(-res));
            }
            if (res == -ECANCELED) st.failed = true; // link broken upstream

            if (stage == 0) {
                if (lat) st.rwStart = Clock::now();
            } else if (stage == 1 && !st.failed) {
                if ((uint64_t)res != fileSize)
                    throw WorkerError("unexpected short async " +
                                      std::string(isWrite ? "write" : "read") +
                                      ". Path: " + st.path);
                if (lat)
                    addIoLat((uint64_t)std::chrono::duration_cast<
                        std::chrono::microseconds>(Clock::now() - st.rwStart)
                        .count());
                if (!isWrite) {
                    if (gpu) {
                        gpu->copyH2DAsync(s, fileSize);
                        if (doVerify) {
                            gpu->syncStream();
                            postReadCheck(s, fileSize, 0);
                        } else {
                            gpu->recordSlotEvent(s);
                            slotHasCopy[s] = 1;
                        }
                    } else {
                        postReadCheck(s, fileSize, 0);
                    }
                }
                liveOps.bytes.fetch_add(fileSize, std::memory_order_relaxed);
                liveOps.iops.fetch_add(1, std::memory_order_relaxed);
            } else if (stage == 2) {
                if (st.failed)
                    throw WorkerError("file chain canceled (open failed?). "
                                      "Path: " + st.path);
                if (lat)
                    addEntryLat((uint64_t)std::chrono::duration_cast<
                        std::chrono::microseconds>(Clock::now() - st.entryStart)
                        .count());
                liveOps.entries.fetch_add(1, std::memory_order_relaxed);
                inFlight--;
                if ((opCount++ % INTERRUPT_CHECK_INTERVAL) == 0) checkInterrupt();
                if (startChain(s)) inFlight++;
            }
        }
    }

    if (gpu) gpu->syncStream();
    return true;
}

// STAT/RMFILES at --iodepth: keep `iodepth` statx/unlinkat ops in flight
// per thread. The reference's libaio engine cannot pipeline metadata ops.
void Worker::dirModeMetaUring(Phase phase)
{
    const auto& cfg = eng.cfg;
    const bool lat = cfg.measureLat;
    const bool haveSubdirs = (cfg.numDirs > 0);
    const uint64_t numDirs = haveSubdirs ? cfg.numDirs : 1;
    const int dirRank = cfg.dirSharing ? 0 : globalRank;
    const int depth = cfg.ioDepth;
    const bool isStat = (phase == Phase::STAT);

    IoUring ring;
    ring.init(depth);
    {
        static const unsigned iowq = [] {
            const char* v = getenv("EB_SF_IOWQ");
            return v ? (unsigned)atoi(v) : 2u;
        }();
        if (iowq) ring.limitWorkers(iowq, iowq);
    }

    struct SlotSt {
        std::string path;
        struct statx stx;
        Clock::time_point start;
    };
    std::vector<SlotSt> slots(depth);

    uint64_t nextFile = 0;
    const uint64_t totalFiles = numDirs * cfg.numFiles;
    char rel[128];

    auto startOp = [&](int s) -> bool {
        if (nextFile >= totalFiles) return false;
        uint64_t d = nextFile / cfg.numFiles;
        uint64_t f = nextFile % cfg.numFiles;
        nextFile++;
        size_t pathIdx = (dirRank + d) % cfg.paths.size();
        if (haveSubdirs)
            snprintf(rel, sizeof(rel), "r%d/d%lu/r%d-f%lu", dirRank,
                     (unsigned long)d, globalRank, (unsigned long)f);
        else
            snprintf(rel, sizeof(rel), "r%d-f%lu", globalRank, (unsigned long)f);
        SlotSt& st = slots[s];
        st.path = cfg.paths[pathIdx] + "/" + rel;
        if (lat) st.start = Clock::now();
        bool ok = isStat ? ring.prepStatx(st.path.c_str(), &st.stx,
                                          STATX_BASIC_STATS, (uint64_t)s)
                         : ring.prepUnlink(st.path.c_str(), (uint64_t)s);
        while (!ok) {
            ring.submitAndWait(0);
            checkInterrupt();
            ok = isStat ? ring.prepStatx(st.path.c_str(), &st.stx,
                                         STATX_BASIC_STATS, (uint64_t)s)
                        : ring.prepUnlink(st.path.c_str(), (uint64_t)s);
        }
        return true;
    };

    int inFlight = 0;
    for (int s = 0; s < depth; s++)
        if (startOp(s))
            inFlight++;
        else
            break;

    std::vector<IoUring::Completion> comps(depth);
    uint64_t opCount = 0;
    while (inFlight > 0) {
        checkInterrupt();
        ring.submitAndWait(1, 250); // bounded: interrupt checks keep running
        unsigned n = ring.reap(comps.data(), depth);
        for (unsigned i = 0; i < n; i++) {
            int s = (int)comps[i].userData;
            SlotSt& st = slots[s];
            int32_t res = comps[i].res;
            if (res < 0 && !(!isStat && cfg.ignoreDelErrors))
                throw WorkerError(std::string(isStat ? "async stat" : "async unlink") +
                                  " failed. Path: " + st.path +
                                  "; SysErr: " + strerror(-res));
            if (lat)
                addEntryLat((uint64_t)std::chrono::duration_cast<
                    std::chrono::microseconds>(Clock::now() - st.start).count());
            liveOps.entries.fetch_add(1, std::memory_order_relaxed);
            inFlight--;
            if ((opCount++ % INTERRUPT_CHECK_INTERVAL) == 0) checkInterrupt();
            if (startOp(s)) inFlight++;
        }
    }
}

void Worker::dirModeFiles(Phase phase)
{
    const auto& cfg = eng.cfg;
    const bool lat = cfg.measureLat;
    const bool isWrite = (phase == Phase::WRITE);
    const bool isRead = (phase == Phase::READ);
    const bool haveSubdirs = (cfg.numDirs > 0);
    const uint64_t numDirs = haveSubdirs ? cfg.numDirs : 1;
    const uint64_t fileSize = cfg.fileSize;
    char rel[128];

    const bool rwMixActive = isWrite && (cfg.rwMixPct > 0 || isDedicatedReader);

    // Dedicated rwmix readers (--rwmixthr) run READ-phase semantics inside the
    // write phase: O_RDONLY, no create/truncate/prealloc — they must never
    // modify the pre-written dataset they read (reference flips them to
    // benchPhase=READFILES entirely, LocalWorker.cpp:1059-1060).
    const bool readerSemantics = isRead || (isWrite && isDedicatedReader);

    int openFlags = 0;
    if (isWrite && !readerSemantics)
        openFlags = O_CREAT | ((cfg.verifyDirect || cfg.readInline || rwMixActive ||
                                cfg.useMmap) ? O_RDWR : O_WRONLY);
    if (readerSemantics) openFlags = O_RDONLY;
    if (cfg.directIO) openFlags |= O_DIRECT;

    // --dirsharing: all threads work in the dirs of rank 0 (file names keep
    // the per-rank prefix, so files stay unique; reference workerDirRank)
    const int dirRank = cfg.dirSharing ? 0 : globalRank;

    // offsets within one file
    std::unique_ptr<OffsetGen> gen;

    // --iodepth in dir mode: per-file async engine, ring shared across files
    // (reference applies aio in every rw mode, LocalWorker.cpp:1210-1379)
    const bool useUring = cfg.ioDepth > 1 && !cfg.useMmap &&
                          (phase == Phase::WRITE || phase == Phase::READ);

    // small files (<= one block): whole open->rw->close chains pipeline
    // through the ring instead (metadata + data overlap)
    // plain sequential access only: --rand with --randamount re-reads
    // blocks (bytes != one pass of the file), which a one-shot whole-file
    // chain cannot express — those shapes use the per-file engine below
    if (useUring && fileSize <= cfg.blockSize && !cfg.statInline &&
        !cfg.readInline && !cfg.fsyncPerFile && !rwMixActive &&
        !cfg.random && !cfg.strided && !cfg.backward &&
        cfg.flockMode == 0 && !eng.opsLog.isEnabled() &&
        !cfg.preallocFile && cfg.truncToSize == UINT64_MAX &&
        !cfg.verifyDirect && !getenv("EB_NO_SF_URING")) { // env = A/B hatch
        if (dirModeSmallFileUring(isWrite)) return;
    }

    // STAT/RMFILES at --iodepth: pipelined statx/unlinkat
    if (cfg.ioDepth > 1 && (phase == Phase::STAT || phase == Phase::RMFILES) &&
        !cfg.statInline && !eng.opsLog.isEnabled() && !getenv("EB_NO_SF_URING"))
        return dirModeMetaUring(phase);

    std::unique_ptr<FileUring> fu;
    if (useUring)
        fu = std::make_unique<FileUring>(cfg.ioDepth, hostBufs, cfg.blockSize);

    for (uint64_t d = 0; d < numDirs; d++) {
        for (uint64_t f = 0; f < cfg.numFiles; f++) {
            if ((f % INTERRUPT_CHECK_INTERVAL) == 0) checkInterrupt();

            size_t pathIdx = (dirRank + d) % cfg.paths.size();
            if (haveSubdirs)
                snprintf(rel, sizeof(rel), "r%d/d%lu/r%d-f%lu", dirRank, (unsigned long)d,
                         globalRank, (unsigned long)f);
            else
                snprintf(rel, sizeof(rel), "r%d-f%lu", globalRank, (unsigned long)f);

            std::string full = cfg.paths[pathIdx] + "/" + rel;

            auto tEntry0 = lat ? Clock::now() : Clock::time_point();

            switch (phase) {
                case Phase::WRITE:
                case Phase::READ: {
                    if (eng.opsLog.isEnabled())
                        eng.opsLog.log(globalRank, "open", full, 0, 0, true, false);
                    int fd = open(full.c_str(), openFlags, 0644);
                    if (fd < 0) throwErrno("open", full);
                    if (eng.opsLog.isEnabled())
                        eng.opsLog.log(globalRank, "open", full, 0, 0, false, false);

                    MmapGuard mg;
                    try {
                        if (cfg.statInline) { // --statinline: fstat right after open
                            struct stat st;
                            if (fstat(fd, &st)) throwErrno("fstat", full);
                        }

                        if (isWrite && !readerSemantics) {
                            if (cfg.truncate && ftruncate(fd, 0)) throwErrno("truncate", full);
                            if ((cfg.truncToSize != UINT64_MAX || cfg.useMmap) &&
                                ftruncate(fd, fileSize))
                                throwErrno("truncate-to-size", full);
                            if (cfg.preallocFile && fallocate(fd, 0, 0, fileSize))
                                throwErrno("fallocate", full);
                        }

                        applyFadvise(fd, cfg.fadviseFlags, full);
                        if (cfg.useMmap)
                            mg.map(fd, fileSize, isWrite && !readerSemantics,
                                   cfg.madviseFlags, full);

                        if (!gen) gen = makeOffsetGen(0, fileSize);
                        else gen->reset(0, fileSize);

                        setAllSlotFileKeys(reduceDirFileKey((uint64_t)globalRank, d, f));
                        if (useUring) {
                            uringFileBlocks(*fu, fd, full, *gen, isWrite,
                                            rwMixActive,
                                            /*allMixRead=*/isWrite && readerSemantics,
                                            /*checkMixReads=*/true);
                            if (isWrite && !readerSemantics && cfg.readInline) {
                                gen->reset(0, fileSize);
                                uringFileBlocks(*fu, fd, full, *gen,
                                                /*phaseIsWrite=*/true,
                                                /*rwMixActive=*/false,
                                                /*allMixRead=*/true,
                                                /*checkMixReads=*/true);
                            }
                        } else {
                        BlockSpec spec;
                        while (gen->next(spec)) {
                            bool mixRead = rwMixActive &&
                                (isDedicatedReader ||
                                 (cfg.rwMixThreads == 0 && rwMixDecideRead()));
                            bool blockWrite = isWrite && !mixRead;
                            auto t0 = lat ? Clock::now() : Clock::time_point();
                            ssize_t res = blockIO(blockWrite, fd, 0, spec.len, spec.offset,
                                                  mg.base(0), &full);
                            if (res < 0) throwErrno(blockWrite ? "write" : "read", full);
                            if ((uint64_t)res != spec.len)
                                throw WorkerError("unexpected short I/O on " + full);
                            if (lat)
                                addIoLat((uint64_t)std::chrono::duration_cast<
                                    std::chrono::microseconds>(Clock::now() - t0).count(),
                                    mixRead);
                            AtomicLiveOps& ops = mixRead ? liveOpsReadMix : liveOps;
                            ops.bytes.fetch_add(spec.len, std::memory_order_relaxed);
                            ops.iops.fetch_add(1, std::memory_order_relaxed);
                        }

                        if (isWrite && !readerSemantics && cfg.readInline) {
                            // --readinline: read the file back within the write
                            // phase; bytes accounted as rwmix reads
                            gen->reset(0, fileSize);
                            while (gen->next(spec)) {
                                auto t0 = lat ? Clock::now() : Clock::time_point();
                                ssize_t res = blockIO(false, fd, 0, spec.len, spec.offset,
                                                      mg.base(0), &full);
                                if (res != (ssize_t)spec.len)
                                    throwErrno("inline readback", full);
                                if (lat)
                                    addIoLat((uint64_t)std::chrono::duration_cast<
                                        std::chrono::microseconds>(Clock::now() - t0).count(),
                                        true);
                                liveOpsReadMix.bytes.fetch_add(spec.len,
                                                               std::memory_order_relaxed);
                                liveOpsReadMix.iops.fetch_add(1, std::memory_order_relaxed);
                            }
                        }
                        } // !useUring

                        if (isWrite && !readerSemantics && cfg.fsyncPerFile && fsync(fd))
                            throwErrno("fsync", full);
                    } catch (...) {
                        close(fd);
                        throw;
                    }
                    close(fd);
                    break;
                }
                case Phase::STAT: {
                    struct stat st;
                    if (stat(full.c_str(), &st)) throwErrno("stat", full);
                    break;
                }
                case Phase::RMFILES: {
                    if (unlink(full.c_str())) {
                        if (!cfg.ignoreDelErrors) throwErrno("unlink", full);
                    }
                    break;
                }
                default:
                    throw WorkerError("bad dir mode phase");
            }

            if (lat)
                addEntryLat((uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(
                    Clock::now() - tEntry0).count());
            liveOps.entries.fetch_add(1, std::memory_order_relaxed);
        }
    }

    if (useUring && gpu) gpu->syncStream(); // drain pipelined staging copies
}

// ---------------------------------------------------------------------------
// custom tree mode (reference analogue: PathStore::getWorkerSublist* +
// LocalWorker custom-tree iterate, LocalWorker.cpp:2960/:3294)
// ---------------------------------------------------------------------------

// mkdir -p: create every missing parent of a relative path under base.
static void mkdirBottomUp(const std::string& base, const std::string& rel)
{
    std::string cur = base;
    size_t pos = 0;
    while (pos != std::string::npos) {
        size_t next = rel.find('/', pos);
        std::string part = rel.substr(pos, next == std::string::npos ? next : next - pos);
        if (!part.empty()) {
            cur += "/" + part;
            if (mkdir(cur.c_str(), 0777) && errno != EEXIST) throwErrno("mkdir", cur);
        }
        pos = (next == std::string::npos) ? next : next + 1;
    }
}

void Worker::customTreeDirs(Phase phase)
{
    const auto& cfg = eng.cfg;
    const bool lat = cfg.measureLat;
    const std::string& base = cfg.paths[globalRank % cfg.paths.size()];
    const uint64_t numRanks = cfg.numDataSetThreads;

    if (phase == Phase::MKDIRS) {
        for (size_t i = 0; i < cfg.treeDirs.size(); i++) {
            if ((int)(i % numRanks) != globalRank) continue;
            if ((i % INTERRUPT_CHECK_INTERVAL) == 0) checkInterrupt();
            auto t0 = lat ? Clock::now() : Clock::time_point();
            mkdirBottomUp(base, cfg.treeDirs[i]);
            if (lat)
                addEntryLat((uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(
                    Clock::now() - t0).count());
            liveOps.entries.fetch_add(1, std::memory_order_relaxed);
        }
    } else { // RMDIRS: deepest dirs first; a dir whose child belongs to a
             // peer rank may still be non-empty, so retry until it drains
        std::vector<size_t> mine;
        for (size_t i = 0; i < cfg.treeDirs.size(); i++)
            if ((int)(i % numRanks) == globalRank) mine.push_back(i);
        std::sort(mine.begin(), mine.end(), [&](size_t a, size_t b) {
            return std::count(cfg.treeDirs[a].begin(), cfg.treeDirs[a].end(), '/') >
                   std::count(cfg.treeDirs[b].begin(), cfg.treeDirs[b].end(), '/');
        });

        std::vector<size_t> pending = mine;
        for (int attempt = 0; !pending.empty() && attempt < 5000; attempt++) {
            checkInterrupt();
            std::vector<size_t> still;
            for (size_t i : pending) {
                std::string full = base + "/" + cfg.treeDirs[i];
                auto t0 = lat ? Clock::now() : Clock::time_point();
                int rc = rmdir(full.c_str());
                if (rc && errno == ENOTEMPTY) { // peer's child not gone yet
                    still.push_back(i);
                    continue;
                }
                if (rc && errno != ENOENT && !cfg.ignoreDelErrors) throwErrno("rmdir", full);
                if (lat)
                    addEntryLat((uint64_t)std::chrono::duration_cast<
                        std::chrono::microseconds>(Clock::now() - t0).count());
                liveOps.entries.fetch_add(1, std::memory_order_relaxed);
            }
            if (still.size() == pending.size())
                std::this_thread::sleep_for(std::chrono::milliseconds(1));
            pending.swap(still);
        }
        if (!pending.empty() && !cfg.ignoreDelErrors)
            throw WorkerError("rmdir: directories stayed non-empty: " +
                              cfg.treeDirs[pending[0]]);
    }
}

void Worker::customTreeFiles(Phase phase)
{
    const auto& cfg = eng.cfg;
    const bool lat = cfg.measureLat;
    const bool isWrite = (phase == Phase::WRITE);
    const bool isRead = (phase == Phase::READ);
    const std::string& base = cfg.paths[globalRank % cfg.paths.size()];
    const uint64_t numRanks = cfg.numDataSetThreads;

    int openFlags = 0;
    if (isWrite) openFlags = O_CREAT | O_WRONLY;
    if (isRead) openFlags = O_RDONLY;
    if (cfg.directIO) openFlags |= O_DIRECT;

    std::unique_ptr<OffsetGen> gen;
    std::unique_ptr<OffsetGen> rrGen; // --treeroundrob strided generator
    size_t nonSharedIdx = 0; // running index over the non-shared sublist

    // --iodepth in custom-tree mode (reference parity: aio in every rw mode)
    const bool useUring = cfg.ioDepth > 1 &&
                          (phase == Phase::WRITE || phase == Phase::READ);
    std::unique_ptr<FileUring> fu;
    if (useUring)
        fu = std::make_unique<FileUring>(cfg.ioDepth, hostBufs, cfg.blockSize);

    // pass 1: ownership/partitioning in treefile order (must be identical on
    // every rank), collecting this rank's work items
    struct TreeWorkItem {
        size_t idx;
        uint64_t rangeStart, rangeLen;
        bool roundRobin;
    };
    std::vector<TreeWorkItem> work;
    for (size_t i = 0; i < cfg.treeFiles.size(); i++) {
        const uint64_t size = cfg.treeFiles[i].second;
        const bool shared = cfg.shareSize && size >= cfg.shareSize;
        // round-robin block interleaving of shared files across ranks
        // (reference --treeroundrob) instead of consecutive range slices
        const bool roundRobin = shared && cfg.treeRoundRobin &&
                                (phase == Phase::WRITE || phase == Phase::READ);

        uint64_t rangeStart = 0, rangeLen = size;
        if (!shared) {
            // whole files round-robin across ranks
            bool mine = (int)(nonSharedIdx % numRanks) == globalRank;
            nonSharedIdx++;
            if (!mine) continue;
        } else if (roundRobin) {
            // strided interleave over the whole file; skip files where this
            // rank's first stride position is already past the end
            if (!rrGen)
                rrGen = std::make_unique<OffsetGenStrided>(cfg.blockSize, globalRank,
                                                           numRanks);
            rrGen->reset(0, size);
            if (!rrGen->totalBytes()) continue;
        } else if (phase == Phase::WRITE || phase == Phase::READ) {
            // blockwise range slice of each shared file per rank
            fairShareSlice(size, rangeStart, rangeLen);
            if (!rangeLen) continue;
        } else {
            // stat/unlink of shared files: one rank per file
            if ((int)(i % numRanks) != globalRank) continue;
        }
        work.push_back({i, rangeStart, rangeLen, roundRobin});
    }

    // --treerand: randomize this worker's processing order (reference
    // PathStore randomShuffle, LocalWorker.cpp:1591); partitioning above is
    // untouched, so coverage stays exact
    if (cfg.treeRandomize) {
        std::mt19937_64 shuffleRng(cfg.benchSeed ^ (0x7EEF11EULL + globalRank));
        std::shuffle(work.begin(), work.end(), shuffleRng);
    }

    for (size_t w = 0; w < work.size(); w++) {
        const size_t i = work[w].idx;
        const auto& [rel, size] = cfg.treeFiles[i];
        const uint64_t rangeStart = work[w].rangeStart;
        const uint64_t rangeLen = work[w].rangeLen;
        const bool roundRobin = work[w].roundRobin;
        if (roundRobin) rrGen->reset(0, size); // re-arm for this file

        if ((w % INTERRUPT_CHECK_INTERVAL) == 0) checkInterrupt();
        std::string full = base + "/" + rel;
        auto tEntry0 = lat ? Clock::now() : Clock::time_point();

        switch (phase) {
            case Phase::WRITE:
            case Phase::READ: {
                int fd = open(full.c_str(), openFlags, 0644);
                if (fd < 0 && isWrite && errno == ENOENT) {
                    // parent dirs may be missing when no MKDIRS phase ran
                    size_t slash = rel.rfind('/');
                    if (slash != std::string::npos) mkdirBottomUp(base, rel.substr(0, slash));
                    fd = open(full.c_str(), openFlags, 0644);
                }
                if (fd < 0) throwErrno("open", full);
                try {
                    OffsetGen* og;
                    if (roundRobin) {
                        og = rrGen.get(); // reset above during the skip check
                    } else {
                        if (!gen) gen = makeOffsetGen(rangeStart, rangeLen);
                        else gen->reset(rangeStart, rangeLen);
                        og = gen.get();
                    }
                    setAllSlotFileKeys(i); // the file's index in the tree file list
                    if (useUring) {
                        uringFileBlocks(*fu, fd, full, *og, isWrite,
                                        /*rwMixActive=*/false,
                                        /*allMixRead=*/false,
                                        /*checkMixReads=*/true);
                        close(fd);
                        if (lat)
                            addEntryLat((uint64_t)std::chrono::duration_cast<
                                std::chrono::microseconds>(Clock::now() - tEntry0)
                                .count());
                        liveOps.entries.fetch_add(1, std::memory_order_relaxed);
                        continue;
                    }
                    BlockSpec spec;
                    while (og->next(spec)) {
                        uint64_t ioLen = std::min(spec.len, size - spec.offset);
                        auto t0 = lat ? Clock::now() : Clock::time_point();
                        ssize_t res = blockIO(isWrite, fd, 0, ioLen, spec.offset,
                                              nullptr, &full);
                        if (res != (ssize_t)ioLen)
                            throwErrno(isWrite ? "write" : "read", full);
                        if (lat)
                            addIoLat((uint64_t)std::chrono::duration_cast<
                                std::chrono::microseconds>(Clock::now() - t0).count());
                        liveOps.bytes.fetch_add(ioLen, std::memory_order_relaxed);
                        liveOps.iops.fetch_add(1, std::memory_order_relaxed);
                    }
                } catch (...) {
                    close(fd);
                    throw;
                }
                close(fd);
                break;
            }
            case Phase::STAT: {
                struct stat st;
                if (stat(full.c_str(), &st)) throwErrno("stat", full);
                break;
            }
            case Phase::RMFILES: {
                if (unlink(full.c_str()) && errno != ENOENT) {
                    if (!cfg.ignoreDelErrors) throwErrno("unlink", full);
                }
                break;
            }
            default:
                throw WorkerError("bad custom tree phase");
        }

        if (lat)
            addEntryLat((uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(
                Clock::now() - tEntry0).count());
        liveOps.entries.fetch_add(1, std::memory_order_relaxed);
    }

    if (useUring && gpu) gpu->syncStream(); // drain pipelined staging copies
}

// ---------------------------------------------------------------------------
// netbench (reference LocalWorker.cpp:7789-8064)
// ---------------------------------------------------------------------------

void Worker::netbenchServer()
{
    const auto& cfg = eng.cfg;

    // worker 0 accepts all expected client connections, then distributes
    // them round-robin (reference: first worker of each server host accepts,
    // LocalWorker.cpp:646-728)
    if (localRank == 0) {
        int listenFd = netListen(cfg.netbenchPort, 128);
        try {
            int expected = cfg.netbenchNumConns > 0 ? cfg.netbenchNumConns : 1;
            std::vector<int> conns;
            for (int i = 0; i < expected; i++) {
                struct pollfd pfd = {listenFd, POLLIN, 0};
                for (;;) {
                    checkInterrupt();
                    int pr = poll(&pfd, 1, 250);
                    if (pr > 0) break;
                }
                int cfd = accept(listenFd, nullptr, nullptr);
                if (cfd < 0) throwErrno("accept", "netbench");
                setSockBufs(cfd, cfg.sendBufSize, cfg.recvBufSize);
                conns.push_back(cfd);
            }
            {
                std::lock_guard<std::mutex> lk(eng.nbMtx);
                eng.nbConns = std::move(conns);
                eng.nbAcceptDone = true;
            }
            eng.nbCv.notify_all();
        } catch (...) {
            close(listenFd);
            {
                std::lock_guard<std::mutex> lk(eng.nbMtx);
                eng.nbAcceptDone = true; // release waiting peers
            }
            eng.nbCv.notify_all();
            throw;
        }
        close(listenFd);
    } else {
        std::unique_lock<std::mutex> lk(eng.nbMtx);
        eng.nbCv.wait(lk, [&] { return eng.nbAcceptDone; });
    }

    // take my round-robin subset of the connections
    std::vector<int> mine;
    {
        std::lock_guard<std::mutex> lk(eng.nbMtx);
        for (size_t i = 0; i < eng.nbConns.size(); i++)
            if ((int)(i % cfg.numThreads) == localRank) mine.push_back(eng.nbConns[i]);
    }
    if (mine.empty()) return;

    const uint64_t bs = cfg.blockSize;
    std::vector<char> block(bs);
    std::vector<char> resp(cfg.respSize, 'R');
    std::vector<struct pollfd> pfds;
    for (int fd : mine) pfds.push_back({fd, POLLIN, 0});

    size_t openConns = mine.size();
    while (openConns) {
        checkInterrupt();
        int pr = poll(pfds.data(), pfds.size(), 250);
        if (pr <= 0) continue;
        for (auto& pfd : pfds) {
            if (!(pfd.revents & (POLLIN | POLLHUP | POLLERR)) || pfd.fd < 0) continue;
            if (!recvExact(pfd.fd, block.data(), bs)) { // EOF: client finished
                close(pfd.fd);
                pfd.fd = -1;
                openConns--;
                continue;
            }
            if (!sendExact(pfd.fd, resp.data(), cfg.respSize))
                throw WorkerError("netbench: response send failed");
            // transfer stats are accounted on the CLIENT side only, so the
            // master's aggregate equals the payload bytes sent once
        }
    }
}

void Worker::netbenchClient()
{
    const auto& cfg = eng.cfg;
    if (cfg.netbenchServers.empty())
        throw WorkerError("netbench client without --servers");

    const bool lat = cfg.measureLat;
    const uint64_t bs = cfg.blockSize;
    const uint64_t total = cfg.fileSize; // bytes per client thread

    // round-robin client->server assignment (reference LocalWorker.cpp:735)
    const std::string& srv = cfg.netbenchServers[globalRank % cfg.netbenchServers.size()];
    std::string host = srv;
    int port = cfg.netbenchPort;
    if (auto pos = srv.rfind(':'); pos != std::string::npos) {
        host = srv.substr(0, pos);
        port = std::stoi(srv.substr(pos + 1)) + 1000; // service port + 1000
    }

    const std::string bindDev =
        cfg.netDevs.empty() ? "" : cfg.netDevs[globalRank % cfg.netDevs.size()];
    int fd = netConnect(host, port, bindDev, 30, eng.interruptFlag);
    setSockBufs(fd, cfg.sendBufSize, cfg.recvBufSize);
    setRecvTimeout(fd, 5); // a dead server can't hang the client worker

    std::vector<char> resp(cfg.respSize);
    uint64_t sent = 0;
    uint64_t opCount = 0;

    try {
        while (sent < total) {
            if ((opCount++ % INTERRUPT_CHECK_INTERVAL) == 0) checkInterrupt();
            rateLimiter.wait(bs);
            auto t0 = lat ? Clock::now() : Clock::time_point();
            if (!sendExact(fd, hostBufs[0], bs))
                throw WorkerError("netbench: block send failed");
            if (!recvExactInterruptible(fd, resp.data(), cfg.respSize,
                                        eng.interruptFlag))
                throw WorkerError("netbench: response recv failed");
            if (lat)
                addIoLat((uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(
                    Clock::now() - t0).count());
            sent += bs;
            liveOps.bytes.fetch_add(bs, std::memory_order_relaxed);
            liveOps.iops.fetch_add(1, std::memory_order_relaxed);
        }
    } catch (...) {
        close(fd);
        throw;
    }
    close(fd);
}

// ---------------------------------------------------------------------------
// sync / dropcaches
// ---------------------------------------------------------------------------

void Worker::anyModeSync()
{
    if (localRank != 0) return; // once per instance
    sync();
}

void Worker::anyModeDropCaches()
{
    if (localRank != 0) return;
    int fd = open("/proc/sys/vm/drop_caches", O_WRONLY);
    if (fd < 0) throwErrno("open", "/proc/sys/vm/drop_caches");
    if (write(fd, "3\n", 2) != 2) {
        close(fd);
        throwErrno("write", "/proc/sys/vm/drop_caches");
    }
    close(fd);
}

// ---------------------------------------------------------------------------
// thread main / phase dispatch
// ---------------------------------------------------------------------------

void Worker::runPhase()
{
    const auto& cfg = eng.cfg;

    const bool customTree = !cfg.treeFiles.empty() || !cfg.treeDirs.empty();

    switch (eng.currentPhase) {
        case Phase::MKDIRS:
            if (customTree)
                customTreeDirs(Phase::MKDIRS);
            else
                dirModeMkdirs();
            break;
        case Phase::RMDIRS:
            if (customTree)
                customTreeDirs(Phase::RMDIRS);
            else
                dirModeRmdirs();
            break;
        case Phase::WRITE:
            if (customTree)
                customTreeFiles(Phase::WRITE);
            else if (cfg.pathType == PathType::DIR)
                dirModeFiles(Phase::WRITE);
            else
                fileModeBlocks(true);
            break;
        case Phase::READ:
            if (customTree)
                customTreeFiles(Phase::READ);
            else if (cfg.pathType == PathType::DIR)
                dirModeFiles(Phase::READ);
            else
                fileModeBlocks(false);
            break;
        case Phase::STAT:
            if (customTree)
                customTreeFiles(Phase::STAT);
            else if (cfg.pathType == PathType::DIR)
                dirModeFiles(Phase::STAT);
            else
                fileModeStat();
            break;
        case Phase::RMFILES:
            if (customTree)
                customTreeFiles(Phase::RMFILES);
            else if (cfg.pathType == PathType::DIR)
                dirModeFiles(Phase::RMFILES);
            else
                fileModeDelete();
            break;
        case Phase::NETBENCH:
            if (cfg.netbenchIsServer)
                netbenchServer();
            else
                netbenchClient();
            break;
        case Phase::SYNC:
            anyModeSync();
            break;
        case Phase::DROPCACHES:
            anyModeDropCaches();
            break;
        default:
            throw WorkerError(std::string("engine phase not implemented: ") +
                              phaseName(eng.currentPhase));
    }
}

void Worker::resetPhaseStats()
{
    liveOps.reset();
    liveOpsReadMix.reset();
    stonewallOps = LiveOpsSnapshot{};
    stonewallOpsReadMix = LiveOpsSnapshot{};
    stonewallElapsedUSec = 0;
    liveIoLatNum.store(0, std::memory_order_relaxed);
    liveIoLatSum.store(0, std::memory_order_relaxed);
    liveEntryLatNum.store(0, std::memory_order_relaxed);
    liveEntryLatSum.store(0, std::memory_order_relaxed);
    ioLat = LatencyHistogram{};
    entryLat = LatencyHistogram{};
    ioLatReadMix = LatencyHistogram{};
    entryLatReadMix = LatencyHistogram{};
    elapsedUSec = 0;
    error.clear();
    rwMixOps = rwMixReads = 0;
    isDedicatedReader = false;
    dedicatedReader = false;
}

void Worker::threadMain()
{
    applyBinding();

    uint64_t seenGen = 0;
    for (;;) {
        { // park at the phase gate until the next phase (or termination)
            std::unique_lock<std::mutex> lk(eng.gateMtx);
            eng.gateCv.wait(lk, [&] {
                return eng.terminateRequested || eng.phaseGen != seenGen;
            });
            if (eng.terminateRequested) return;
            seenGen = eng.phaseGen;
        }

        bool hadError = false;
        try {
            const auto& cfg = eng.cfg;

            const uint64_t phaseSeed =
                cfg.benchSeed + 0x9E3779B97F4A7C15ULL * (uint64_t)eng.phaseSeq;
            rng.reset(makeRandAlgo(cfg.randAlgo,
                                   phaseSeed ^ (0xBF58476D1CE4E5B9ULL * (globalRank + 1))));
            fillRng.reset(makeRandAlgo(cfg.blockVarAlgo,
                                       phaseSeed ^ (0x94D049BB133111EBULL * (globalRank + 1))));
            reduceSeed = reduceSeeds(cfg.benchSeed, eng.phaseSeq, globalRank);

            // --rwmixthr: first N threads of a write phase only read
            isDedicatedReader =
                (eng.currentPhase == Phase::WRITE) && (localRank < cfg.rwMixThreads);
            dedicatedReader = isDedicatedReader;

            // buffers only needed for data phases; allocation + random
            // prefill happen once, later phases reuse them
            if (eng.currentPhase == Phase::WRITE || eng.currentPhase == Phase::READ ||
                eng.currentPhase == Phase::NETBENCH)
                allocBuffers();
            if (eng.reduceVerify) slotReduceSeed.resize(hostBufs.size());

            // --dataprofile: READ phases only (not the reads of an rwmix
            // write phase); accumulators start empty in every phase
            profiling = eng.dataProfile && eng.currentPhase == Phase::READ;
            profileResult.reset();
            if (profiling) {
                profileAcc = std::make_unique<DataProfileAcc>();
                if (gpu) gpu->dataProfileReset();
            }

            rateLimiter.init((eng.currentPhase == Phase::WRITE && !isDedicatedReader)
                                 ? eng.cfg.limitWriteBps
                                 : eng.cfg.limitReadBps);

            const bool loopingPhase =
                cfg.infiniteLoop && (eng.currentPhase == Phase::WRITE ||
                                     eng.currentPhase == Phase::READ ||
                                     eng.currentPhase == Phase::STAT);
            do {
                reduceNextChunk = 0;
                runPhase();
            } while (loopingPhase && !eng.interruptFlag.load(std::memory_order_relaxed));

            if (profiling) { // the one fetch of the phase; an error reports none
                if (gpu) gpu->dataProfileFetch(*profileAcc);
                profileResult = std::move(profileAcc);
            }
        } catch (const InterruptedError&) {
            error = "interrupted";
            hadError = true;
        } catch (const std::exception& e) {
            error = e.what();
            hadError = true;
        }

        elapsedUSec = nowUSecSince(eng.phaseStart);
        eng.onWorkerDone(*this, hadError);
    }
}

// ---------------------------------------------------------------------------
// Engine
// ---------------------------------------------------------------------------

Engine::Engine(EngineConfig cfgIn) : cfg(std::move(cfgIn))
{
    if (cfg.verifyMixPct < -1 || cfg.verifyMixPct > 100)
        throw std::invalid_argument("verify_mix_pct must be in 0..100 (or -1 for unset)");
    if (cfg.verifyMixPct >= 0) {
        if (cfg.verifySalt < 0)
            throw std::invalid_argument("verify_mix_pct requires verify_salt");
        if (!cfg.blockSize || cfg.blockSize % 8)
            throw std::invalid_argument(
                "verify_mix_pct requires a block size that is a multiple of 8");
        verifyMix = true;
        // blockSize / 100 * pct would lose the remainder; the product can
        // overflow only for block sizes beyond 2^57
        verifyMixLen = (uint64_t)((unsigned __int128)cfg.blockSize * cfg.verifyMixPct / 100)
                       & ~7ULL;
    }

    if (cfg.dedupePct < 0 || cfg.dedupePct > 100)
        throw std::invalid_argument("dedupe_pct must be in 0..100");
    if (cfg.compressPct < 0 || cfg.compressPct > 100)
        throw std::invalid_argument("compress_pct must be in 0..100");
    if (cfg.dedupePct > 0 || cfg.compressPct > 0) {
        if (cfg.verifySalt >= 0)
            throw std::invalid_argument(
                "dedupe_pct / compress_pct cannot be used together with verify_salt");
        if (cfg.dedupeChunk < 16 || (cfg.dedupeChunk & (cfg.dedupeChunk - 1)) ||
            cfg.dedupeChunk > (1ULL << 40))
            throw std::invalid_argument(
                "dedupe_chunk must be a power of two in 16..2^40");
        reduce = true;
        reduceRandBytes = (cfg.dedupeChunk * (uint64_t)(100 - cfg.compressPct) / 100) & ~15ULL;
    }

    if (cfg.reduceVerifySalt < -1)
        throw std::invalid_argument("reduce_verify_salt must be >= 0 (or -1 for unset)");
    if (cfg.reduceVerifySalt >= 0) {
        if (!reduce)
            throw std::invalid_argument(
                "reduce_verify_salt requires a non-zero dedupe_pct or compress_pct");
        if (cfg.verifyMixPct >= 0)
            throw std::invalid_argument(
                "reduce_verify_salt cannot be used together with verify_mix_pct");
        if (cfg.verifyDiag)
            throw std::invalid_argument(
                "reduce_verify_salt cannot be used together with verify_diag");
        if (cfg.random && !cfg.randAligned)
            throw std::invalid_argument(
                "reduce_verify_salt cannot be used with unaligned random offsets");
        if (!cfg.blockSize || cfg.blockSize % cfg.dedupeChunk)
            throw std::invalid_argument(
                "reduce_verify_salt requires a block size that is a multiple of dedupe_chunk");
        reduceVerify = true;
    }
    dataVerify = cfg.verifySalt >= 0 || reduceVerify;

    if (cfg.dataProfile) {
        if (!dataProfileChunkOk(cfg.dedupeChunk))
            throw std::invalid_argument(
                "data_profile requires a dedupe_chunk that is a power of two in 512..16M");
        if (cfg.random && !cfg.randAligned)
            throw std::invalid_argument(
                "data_profile cannot be used with unaligned random offsets");
        if (!cfg.blockSize || cfg.blockSize % cfg.dedupeChunk)
            throw std::invalid_argument(
                "data_profile requires a block size that is a multiple of dedupe_chunk");
        dataProfile = true;
    }
}

Engine::~Engine()
{
    interrupt();
    { // wake parked persistent workers so they can exit
        std::lock_guard<std::mutex> lk(gateMtx);
        terminateRequested = true;
    }
    gateCv.notify_all();
    for (auto& t : threads)
        if (t.joinable()) t.join();
    workers.clear(); // returns GpuCtx instances to the cache before teardown
    dropMappedRegs();
}

void Engine::prepare()
{
    resolvedFileSizes.clear();
    effFileSize = cfg.fileSize;

    if (cfg.pathType == PathType::DIR) return;

    for (const auto& p : cfg.paths) {
        struct stat st;
        if (stat(p.c_str(), &st)) {
            if (cfg.pathType == PathType::FILE && errno == ENOENT) {
                resolvedFileSizes.push_back(cfg.fileSize);
                continue; // will be created by write phase
            }
            throwErrno("stat", p);
        }
        if (S_ISBLK(st.st_mode)) {
            int fd = open(p.c_str(), O_RDONLY);
            if (fd < 0) throwErrno("open", p);
            uint64_t sz = 0;
            if (ioctl(fd, BLKGETSIZE64, &sz)) {
                close(fd);
                throwErrno("BLKGETSIZE64", p);
            }
            close(fd);
            resolvedFileSizes.push_back(sz);
        } else {
            resolvedFileSizes.push_back(st.st_size);
        }
    }

    if (!cfg.fileSize && !resolvedFileSizes.empty()) {
        // no -s given: use detected size (min across paths for uniform stripe)
        uint64_t minSz = UINT64_MAX;
        for (auto s : resolvedFileSizes) minSz = std::min(minSz, s);
        effFileSize = (minSz == UINT64_MAX) ? 0 : minSz;
    }
}

void Engine::startPhase(Phase phase)
{
    if (phaseRunning) throw std::runtime_error("phase already running");

    currentPhase = phase;
    phaseSeq++; // new offset/fill streams every phase (iterations differ)
    rwBalBytesRead.store(0);
    rwBalBytesWrite.store(0);
    rwReadersDone.store(0);
    rwWritersDone.store(0);
    nbAcceptDone = false;
    nbConns.clear();
    if (!cfg.opsLogPath.empty() && !opsLog.isEnabled())
        opsLog.open(cfg.opsLogPath, cfg.opsLogLock);
    interruptFlag.store(false);
    workersDone.store(0);
    workersWithError.store(0);
    stonewallTriggered.store(false);
    dynCursor.store(0);

    if (workers.empty()) { // first phase: spawn the persistent worker pool
        for (int i = 0; i < cfg.numThreads; i++)
            workers.push_back(std::make_unique<Worker>(*this, i));
        for (auto& w : workers) threads.emplace_back(&Worker::threadMain, w.get());
    } else { // reuse parked workers; clear their per-phase stats
        for (auto& w : workers) w->resetPhaseStats();
    }

    { // release the gate; timestamp = phase start
        std::lock_guard<std::mutex> lk(gateMtx);
        phaseStart = std::chrono::steady_clock::now();
        phaseGen++;
    }
    gateCv.notify_all();
    phaseRunning = true;
}

void Engine::onWorkerDone(Worker& w, bool hadError)
{
    std::lock_guard<std::mutex> lk(doneMtx);

    (w.dedicatedReader ? rwReadersDone : rwWritersDone).fetch_add(1);

    if (hadError) {
        workersWithError.fetch_add(1);
        interruptFlag.store(true); // peers stop cooperatively (reference behavior)
    } else if (!stonewallTriggered.load()) {
        // first successful finisher triggers the stonewall: snapshot every
        // worker's live counters ("first done" result)
        bool didWork = w.liveOps.entries.load(std::memory_order_relaxed) ||
                       w.liveOps.bytes.load(std::memory_order_relaxed) ||
                       w.liveOps.iops.load(std::memory_order_relaxed) ||
                       w.liveOpsReadMix.bytes.load(std::memory_order_relaxed) ||
                       w.liveOpsReadMix.iops.load(std::memory_order_relaxed);
        if (didWork) {
            uint64_t elapsed = nowUSecSince(phaseStart);
            for (auto& peer : workers) {
                peer->stonewallOps.takeFrom(peer->liveOps);
                peer->stonewallOpsReadMix.takeFrom(peer->liveOpsReadMix);
                peer->stonewallElapsedUSec = elapsed;
            }
            stonewallTriggered.store(true);
        }
    }

    workersDone.fetch_add(1);
    doneCv.notify_all();
}

bool Engine::waitPhaseDone(int64_t timeoutMs)
{
    std::unique_lock<std::mutex> lk(doneMtx);
    auto pred = [&] { return workersDone.load() >= (int)workers.size(); };
    if (timeoutMs < 0) {
        doneCv.wait(lk, pred);
        return true;
    }
    return doneCv.wait_for(lk, std::chrono::milliseconds(timeoutMs), pred);
}

void Engine::interrupt() { interruptFlag.store(true); }

void Engine::triggerStonewall()
{
    // remote stonewall propagation: another service's first finisher defines
    // the global first-done point; snapshot local workers now (reference
    // RemoteWorker stonewall handling)
    std::lock_guard<std::mutex> lk(doneMtx);
    if (stonewallTriggered.load()) return;
    uint64_t elapsed = nowUSecSince(phaseStart);
    for (auto& peer : workers) {
        peer->stonewallOps.takeFrom(peer->liveOps);
        peer->stonewallOpsReadMix.takeFrom(peer->liveOpsReadMix);
        peer->stonewallElapsedUSec = elapsed;
    }
    stonewallTriggered.store(true);
}

Engine::LivePoll Engine::poll()
{
    LivePoll lp{};
    lp.workersTotal = (int)workers.size();
    lp.workersDone = workersDone.load();
    lp.workersWithError = workersWithError.load();
    lp.stonewallTriggered = stonewallTriggered.load();
    lp.elapsedUSec = phaseRunning ? nowUSecSince(phaseStart) : 0;

    for (auto& w : workers) {
        lp.entries += w->liveOps.entries.load(std::memory_order_relaxed);
        lp.bytes += w->liveOps.bytes.load(std::memory_order_relaxed) +
                    w->liveOpsReadMix.bytes.load(std::memory_order_relaxed);
        lp.iops += w->liveOps.iops.load(std::memory_order_relaxed) +
                   w->liveOpsReadMix.iops.load(std::memory_order_relaxed);
        lp.latNumIOs += w->liveIoLatNum.load(std::memory_order_relaxed);
        lp.latSumIOs += w->liveIoLatSum.load(std::memory_order_relaxed);
        lp.latNumEntries += w->liveEntryLatNum.load(std::memory_order_relaxed);
        lp.latSumEntries += w->liveEntryLatSum.load(std::memory_order_relaxed);
    }
    return lp;
}

Engine::GpuSlotsSnapshot Engine::gpuSlots(int localRank)
{
    if (phaseRunning)
        throw std::runtime_error("gpu_slots: a phase is running (call finish_phase first)");
    if (localRank < 0) throw std::out_of_range("gpu_slots: bad worker rank");

    // parked workers are idle between finishPhase and the next startPhase,
    // so their context is safe to use from the calling thread
    GpuCtx* ctx = nullptr;
    if ((size_t)localRank < workers.size()) ctx = workers[localRank]->gpuCtx();
    std::lock_guard<std::mutex> lk(gpuCacheMtx);
    if (!ctx && (size_t)localRank < gpuCtxCache.size()) ctx = gpuCtxCache[localRank].get();
    if (!ctx)
        throw std::runtime_error("gpu_slots: worker " + std::to_string(localRank) +
                                 " has no GPU context");

    GpuSlotsSnapshot snap;
    ctx->bindThread();
    snap.numSlots = ctx->numSlots();
    snap.slotStride = ctx->slotStride();
    ctx->snapshotSlots(snap.bytes);
    return snap;
}

std::vector<std::pair<uint64_t, bool>> Engine::gpuStreams()
{
    if (phaseRunning)
        throw std::runtime_error("gpu_streams: a phase is running (call finish_phase first)");

    std::vector<std::pair<uint64_t, bool>> out;
    std::lock_guard<std::mutex> lk(gpuCacheMtx);
    for (int r = 0; r < cfg.numThreads; r++) { // same lookup as gpuSlots
        GpuCtx* ctx = nullptr;
        if ((size_t)r < workers.size()) ctx = workers[r]->gpuCtx();
        if (!ctx && (size_t)r < gpuCtxCache.size()) ctx = gpuCtxCache[r].get();
        if (!ctx)
            throw std::runtime_error("gpu_streams: worker " + std::to_string(r) +
                                     " has no GPU context");
        out.emplace_back(ctx->streamId(), ctx->streamShared());
    }
    return out;
}

std::vector<WorkerResult> Engine::finishPhase()
{
    { // workers stay alive (parked at the gate); just wait for phase end
        std::unique_lock<std::mutex> lk(doneMtx);
        doneCv.wait(lk, [&] { return workersDone.load() >= (int)workers.size(); });
    }
    phaseRunning = false;

    std::vector<WorkerResult> results;
    for (auto& w : workers) {
        WorkerResult r;
        r.rank = w->globalRank;
        r.elapsedUSec = w->elapsedUSec;
        r.total.takeFrom(w->liveOps);
        r.totalReadMix.takeFrom(w->liveOpsReadMix);
        r.stonewall = stonewallTriggered.load() ? w->stonewallOps : r.total;
        r.stonewallReadMix =
            stonewallTriggered.load() ? w->stonewallOpsReadMix : r.totalReadMix;
        r.stonewallElapsedUSec =
            stonewallTriggered.load() ? w->stonewallElapsedUSec : w->elapsedUSec;
        r.ioLatVec = w->ioLat.toVec();
        r.entryLatVec = w->entryLat.toVec();
        r.ioLatReadMixVec = w->ioLatReadMix.toVec();
        r.entryLatReadMixVec = w->entryLatReadMix.toVec();
        r.error = w->error;
        if (w->error.empty()) r.profile = w->profileResult;
        results.push_back(std::move(r));
    }

    currentPhase = Phase::IDLE;
    return results;
}

// mmap+GPU zero-copy: map the file and pin its pages so SDMA copies move
// data straight between the page cache and HBM3E (no bounce buffer, no
// read/write syscalls). Mapping+registration cached across phases.
Engine::MappedReg& Engine::getMappedReg(const std::string& path, uint64_t len, bool writable)
{
    std::lock_guard<std::mutex> lk(mmapRegMtx);
    auto& reg = mmapRegCache[path];
    if (reg.base && reg.len >= len && (reg.writable || !writable)) return reg;
    if (reg.base) { // grow or upgrade to writable: drop the old mapping first
        if (reg.registered) gpuHostUnregister(reg.base);
        munmap(reg.base, reg.len);
        reg = MappedReg{};
    }

    int fd = open(path.c_str(), writable ? (O_RDWR | O_CREAT) : O_RDONLY, 0644);
    if (fd < 0) throwErrno("open", path);
    if (writable && ftruncate(fd, len)) {
        close(fd);
        throwErrno("truncate-to-size", path);
    }
    int prot = PROT_READ | (writable ? PROT_WRITE : 0);
    void* p = mmap(nullptr, len, prot, MAP_SHARED | MAP_POPULATE, fd, 0);
    close(fd); // mapping keeps the file alive
    if (p == MAP_FAILED)
        throw WorkerError("mmap failed. Path: " + path + "; SysErr: " + strerror(errno));

    reg.base = (char*)p;
    reg.len = len;
    reg.writable = writable;
    // pin for full-speed DMA; if pinning fails (memlock limits with many
    // ranks x multi-GiB maps), keep the mapping and let the copies run
    // pageable — slower, never fatal
    reg.registered = gpuHostRegisterTry(reg.base, len);
    if (!reg.registered)
        fprintf(stderr, "[eb] WARNING: hipHostRegister of %s (%.1f GiB) "
                "failed — staging copies run unpinned\n",
                path.c_str(), len / 1073741824.0);
    return reg;
}

void Engine::dropMappedRegs()
{
    std::lock_guard<std::mutex> lk(mmapRegMtx);
    for (auto& [path, reg] : mmapRegCache) {
        if (reg.registered) gpuHostUnregister(reg.base);
        if (reg.base) munmap(reg.base, reg.len);
    }
    mmapRegCache.clear();
}

std::pair<uint64_t, uint64_t> Engine::plannedWork(Phase phase) const
{
    uint64_t entries = 0, bytes = 0;

    // custom tree (--treefile): replicate the worker partition math
    // (reference dry-run covers custom trees too, Statistics.cpp:2865)
    if (!cfg.treeFiles.empty() || !cfg.treeDirs.empty()) {
        const uint64_t numRanks = cfg.numDataSetThreads;
        const int firstRank = cfg.rankOffset;
        const int lastRank = cfg.rankOffset + cfg.numThreads; // exclusive
        auto rankIsMine = [&](uint64_t idx) {
            int r = (int)(idx % numRanks);
            return r >= firstRank && r < lastRank;
        };

        switch (phase) {
            case Phase::MKDIRS:
            case Phase::RMDIRS:
                for (size_t i = 0; i < cfg.treeDirs.size(); i++)
                    if (rankIsMine(i)) entries++;
                break;
            case Phase::WRITE:
            case Phase::READ: {
                const uint64_t bs = cfg.blockSize;
                size_t nonSharedIdx = 0;
                for (const auto& [rel, size] : cfg.treeFiles) {
                    (void)rel;
                    const bool shared = cfg.shareSize && size >= cfg.shareSize;
                    if (!shared) {
                        if (rankIsMine(nonSharedIdx)) {
                            entries++;
                            bytes += size;
                        }
                        nonSharedIdx++;
                        continue;
                    }
                    // shared: every rank of this instance with a non-empty
                    // slice counts the file as one entry + its slice bytes
                    uint64_t numBlocksTotal = (size + bs - 1) / bs;
                    uint64_t perRank = numBlocksTotal / numRanks;
                    for (int g = firstRank; g < lastRank; g++) {
                        uint64_t myLen;
                        if (cfg.treeRoundRobin) {
                            // mirrors OffsetGenStrided::reset exactly:
                            // full blocks split round-robin, byte tail goes
                            // to rank (full % numRanks)
                            uint64_t full = size / bs;
                            uint64_t tail = size - full * bs;
                            uint64_t myBlocks =
                                full / numRanks +
                                ((full % numRanks) > (uint64_t)g ? 1 : 0);
                            myLen = myBlocks * bs;
                            if (tail && (full % numRanks) == (uint64_t)g)
                                myLen += tail;
                        } else {
                            uint64_t startBlock = (uint64_t)g * perRank;
                            uint64_t myBlocks = perRank;
                            if ((uint64_t)g == numRanks - 1)
                                myBlocks = numBlocksTotal - startBlock;
                            uint64_t myStart = startBlock * bs;
                            uint64_t endByte =
                                std::min<uint64_t>(size, (startBlock + myBlocks) * bs);
                            myLen = (myStart >= endByte) ? 0 : endByte - myStart;
                        }
                        if (myLen) {
                            entries++;
                            bytes += myLen;
                        }
                    }
                }
                break;
            }
            case Phase::STAT:
            case Phase::RMFILES: {
                // shared files: one rank per file by absolute treefile index;
                // non-shared: round-robin over the non-shared sublist (same
                // split as customTreeFiles pass 1)
                size_t nonSharedIdx = 0;
                for (size_t i = 0; i < cfg.treeFiles.size(); i++) {
                    const uint64_t size = cfg.treeFiles[i].second;
                    const bool shared = cfg.shareSize && size >= cfg.shareSize;
                    if (shared) {
                        if (rankIsMine(i)) entries++;
                    } else {
                        if (rankIsMine(nonSharedIdx)) entries++;
                        nonSharedIdx++;
                    }
                }
                break;
            }
            default:
                break;
        }
        return {entries, bytes};
    }

    if (cfg.pathType == PathType::DIR) {
        uint64_t numDirs = cfg.numDirs ? cfg.numDirs : 1;
        switch (phase) {
            case Phase::MKDIRS:
            case Phase::RMDIRS:
                entries = cfg.numDirs * cfg.numThreads;
                break;
            case Phase::WRITE:
            case Phase::READ:
                entries = numDirs * cfg.numFiles * cfg.numThreads;
                bytes = entries * cfg.fileSize;
                break;
            case Phase::STAT:
            case Phase::RMFILES:
                entries = numDirs * cfg.numFiles * cfg.numThreads;
                break;
            default:
                break;
        }
    } else {
        switch (phase) {
            case Phase::WRITE:
            case Phase::READ: {
                uint64_t totalLen = effFileSize * cfg.paths.size();
                if (cfg.random) {
                    uint64_t amount = cfg.randAmount ? cfg.randAmount : totalLen;
                    bytes = (amount / cfg.numDataSetThreads) * cfg.numThreads;
                } else {
                    // fair-share block slices over the padded virtual range,
                    // minus bytes trimmed off per-file tail blocks
                    uint64_t bs = cfg.blockSize;
                    uint64_t bpf = bs ? (effFileSize + bs - 1) / bs : 0;
                    uint64_t tailTrim = bpf * bs - effFileSize; // per file
                    uint64_t numBlocksTotal = bpf * cfg.paths.size();
                    uint64_t perRank = numBlocksTotal / cfg.numDataSetThreads;
                    auto tailsBelow = [&](uint64_t x) -> uint64_t {
                        return (bpf && x >= bpf) ? ((x - bpf) / bpf + 1) : 0;
                    };
                    for (int i = 0; i < cfg.numThreads; i++) {
                        uint64_t grank = cfg.rankOffset + i;
                        uint64_t startBlock = grank * perRank;
                        uint64_t myBlocks = perRank;
                        if (grank == (uint64_t)cfg.numDataSetThreads - 1)
                            myBlocks = (numBlocksTotal > startBlock)
                                           ? numBlocksTotal - startBlock
                                           : 0;
                        uint64_t endBlock = startBlock + myBlocks;
                        uint64_t tails = tailsBelow(endBlock) - tailsBelow(startBlock);
                        bytes += myBlocks * bs - tails * tailTrim;
                    }
                }
                break;
            }
            case Phase::STAT:
            case Phase::RMFILES:
                for (size_t i = 0; i < cfg.paths.size(); i++)
                    if ((int)(i % cfg.numDataSetThreads) >= cfg.rankOffset &&
                        (int)(i % cfg.numDataSetThreads) < cfg.rankOffset + cfg.numThreads)
                        entries++;
                break;
            default:
                break;
        }
    }
    return {entries, bytes};
}

} // namespace eb
