// GPU buffer management + CDNA4 kernel wrappers — host-facing interface.
//
// MI355X-native replacement of the reference's CUDA/cuFile call sites
// (/root/reference/source/workers/LocalWorker.cpp:1427-1537 allocGPUIOBuffer,
// :2269-2310 curand block-variance refill, :2437-2486 staging memcpys).
// Design differences (deliberate, per BASELINE.json north star):
//   - random fill and integrity fill/verify run as hand-written gfx950 HIP
//     kernels directly in HBM3E (the reference does fill on CPU or curand,
//     verify always on CPU),
//   - staging uses hipMemcpyAsync on a per-worker non-blocking stream with
//     pinned host buffers (the reference uses synchronous cudaMemcpy),
//   - there is no cuFile/GDS on ROCm: the "direct" storage<->HBM path is
//     O_DIRECT into pinned host bounce buffers behind the same seam.
//
// All HIP API usage lives in gpu_kernels.hip; this header keeps the engine
// translation-unit HIP-free.

#pragma once

#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "crc.h"
#include "dataprofile.h"

namespace eb {

struct GpuVerifyResult {
    uint64_t numMismatches;
    uint64_t firstBadFileOffset; // UINT64_MAX if none
};

// --verifydiag record: what a verify pass saw, classified per bad word.
// Accumulates over launches like the two counters above; the defaults are the
// empty record. Classes, first match wins: ZERO (word reads 0), PATTERN (both
// words of a 16-byte pair are bad, non-zero and decode to the same delta from
// the expected offset + salt), BITFLIP (at most two bits differ), OTHER.
// See docs/usage.md (--verifydiag) for the full contract.
struct GpuVerifyDiag {
    uint64_t numMismatches = 0;
    uint64_t firstBadFileOffset = UINT64_MAX;
    uint64_t lastBadFileOffset = 0;
    uint64_t runs = 0; // maximal stretches of consecutive bad words, per launch
    uint64_t zero = 0, pattern = 0, bitflip = 0, other = 0;
    int64_t deltaMin = std::numeric_limits<int64_t>::max(); // over PATTERN words
    int64_t deltaMax = std::numeric_limits<int64_t>::min();
    uint64_t flipOr = 0; // OR of (found ^ expected) over BITFLIP words

    static constexpr int NUM_FIELDS = 11; // device layout: the fields in this order
};

// Pin (hipHostRegister) / unpin an arbitrary host region — used to register
// mmap'ed file pages so storage<->HBM copies DMA straight from/to the page
// cache with no bounce buffer (the MI355X-native --mmap + GPU path).
void gpuHostRegister(void* ptr, uint64_t len);
// non-throwing variant: false when pinning fails (e.g. memlock limits at
// 8 ranks x multi-GiB registrations) — callers degrade to pageable copies
bool gpuHostRegisterTry(void* ptr, uint64_t len);
void gpuHostUnregister(void* ptr);

// Copy between a registered host region and a device slot buffer.
class GpuCtx;

// Returns number of visible HIP devices; 0 when no GPU or no driver.
int gpuDeviceCount();

// A/B micro-bench: verify-kernel effective read bandwidth in GB/s.
// lds=false runs the production LDS-free kernel, lds=true the LDS-tiled
// variant kept only to justify that design choice.
double gpuVerifyBenchGBs(uint64_t len, int iters, bool lds, int dev);

// Micro-bench of the --verifymixpct kernels on one len-byte buffer (GB/s):
// fill=false times ebVerifyChecksumMixKernel, fill=true the fill kernel
// (plainFill: ebFillChecksumKernel instead, timed the same way for comparison).
// Requires len % 16 == 0 and len <= blockSize.
double gpuMixBenchGBs(uint64_t len, int iters, int dev, uint64_t blockSize, uint64_t mixLen,
                      bool fill, bool plainFill);

// Micro-bench of ebVerifyReduceKernel (GB/s) on one len-byte buffer of clean
// pattern data (chunk 0 onwards, pool of 256), timed as gpuMixBenchGBs times
// its verify. Requires len % 16 == 0 and fillReduceDev's geometry.
double gpuReduceVerifyBenchGBs(uint64_t len, int iters, int dev, uint64_t chunkBytes,
                               uint64_t randBytes, int dedupePct);

// gpuVerifyBenchGBs for ebVerifyDiagKernel: same buffer, same clean data.
double gpuVerifyDiagBenchGBs(uint64_t len, int iters, int dev);

// Micro-bench of ebDataProfileKernel (GB/s) on one len-byte buffer cut into
// chunkBytes chunks, timed as gpuMixBenchGBs times its verify. kind selects the
// content: 0 random words, 1 zero-heavy (the second half of every 4 KiB is
// zero, as --compresspct 50 writes it), 2 all zero.
double gpuDataProfileBenchGBs(uint64_t len, int iters, int dev, uint64_t chunkBytes, int kind);

// Geometry of the device CRC kernel: bytes per tile (one raw partial CRC
// each) and bytes covered by one wave within a tile. Tests key their sizes
// off these.
uint64_t gpuCrcTileBytes();
uint64_t gpuCrcWaveBytes();
// The same for the CRC-64/NVME kernel (crc64.h: CRC64_TILE_BYTES, CRC64_WAVE_BYTES).
uint64_t gpuCrc64TileBytes();
uint64_t gpuCrc64WaveBytes();

// Diagnostic: the hipGetDeviceCount error string (or "ok: N device(s)").
std::string gpuProbeError();

// Human-readable device name (empty if unavailable).
std::string gpuDeviceName(int deviceId);

// NUMA node of the GPU's PCIe device (-1 unknown).
int gpuNumaNode(int deviceId);

// Per-worker GPU context: one HIP stream, `numSlots` device buffers of
// `bufSize` bytes (one per io-depth slot) and matching pinned host buffers.
class GpuCtx {
public:
    GpuCtx(int deviceId, int numSlots, uint64_t bufSize, bool pinnedHostBufs);
    ~GpuCtx();
    GpuCtx(const GpuCtx&) = delete;
    GpuCtx& operator=(const GpuCtx&) = delete;

    int deviceId() const { return devId; }
    char* hostBuf(int slot) const;
    uint64_t bufSize() const { return slotSize; }
    int numSlots() const { return slots; }
    // distance between consecutive slots in the device (and host) slab: the
    // 4 KiB-rounded slot size
    uint64_t slotStride() const;

    // Read-only snapshot of the whole device slab (numSlots * slotStride
    // bytes, slot i at i * slotStride) into dst, copied on this context's
    // stream; synchronizes. Diagnostic/test hook: no I/O path calls it and it
    // leaves device memory and the pinned host buffers untouched.
    void snapshotSlots(std::vector<char>& dst);

    // Which stream this context enqueues into: the hipStream_t value as an
    // integer, for identity only (two contexts share a stream iff their ids
    // are equal), and whether it came from the process-wide pool of
    // EB_GPU_SHARED_STREAMS or is this context's own. Diagnostic/test hook:
    // no device work, no I/O path calls it.
    uint64_t streamId() const;
    bool streamShared() const;

    // bind the calling thread to this context's device (hipSetDevice);
    // required when a cached context is reused by a new worker thread
    void bindThread();

    // --- async staging copies on this worker's stream ---
    // direct copies between a registered host region (mmap'ed file) and HBM
    void copyFromHostAsync(int slot, const void* src, uint64_t len);
    void copyToHostAsync(int slot, void* dst, uint64_t len);
    void copyH2DAsync(int slot, uint64_t len);
    // one memcpy covering `count` consecutive slots (slot stride is the
    // 4 KiB-rounded slot size) — batches small-block staging
    void copyH2DRangeAsync(int firstSlot, int count);
    void copyD2HAsync(int slot, uint64_t len);
    void syncStream();

    // per-slot completion events: record after the slot's async op, wait
    // before reusing the slot's buffers (enables storage<->PCIe pipelining)
    void recordSlotEvent(int slot);
    void waitSlotEvent(int slot);

    // --lat on the pipelined fast path: per-slot TIMED
    // hipEvent pairs bracketing one async copy. The elapsed time is the
    // copy's execution time on the stream — the per-block into-HBM latency
    // at full pipelining (the reference can only measure latency in its
    // synchronous loop, LocalWorker.cpp:1702-1814). Events are created on
    // first use so non-lat runs pay nothing.
    void recordTimedStart(int slot);
    void recordTimedEnd(int slot);
    // true if a timed pair was recorded for this slot and not yet collected
    bool timedPairActive(int slot) const;
    // synchronize on the slot's end event, return elapsed microseconds and
    // clear the pair
    uint64_t timedElapsedUSec(int slot);
    // forget pairs that were recorded but never collected (a phase that
    // threw before its drain), so the next phase does not count them
    void dropTimedPairs();

    // async verify accumulating into persistent device counters; results
    // fetched (and reset) by fetchVerifyResult() — lets the caller batch
    // many blocks per stream synchronization
    // Same alignment contract as verifyChecksumDev. ldsVariant selects the
    // LDS-tiled A/B kernel (tests and gpu_verify_bench only).
    void verifyChecksumDevAsync(int slot, uint64_t len, uint64_t fileOff, uint64_t salt,
                                bool ldsVariant = false);
    GpuVerifyResult fetchVerifyResult();

    // --- device-side buffer ops (hand-written gfx950 kernels) ---

    // Fill device buffer with xoshiro256++ random data (replaces curand).
    // Requires len % 16 == 0 (one 16 B store per element); throws
    // std::invalid_argument otherwise.
    void fillRandDev(int slot, uint64_t len, uint64_t seed, bool fastAlgo = false);

    // Integrity-checksum fill: u64 at 8-aligned file offset o gets value
    // o + salt. Requires fileOff % 8 == 0 and len % 8 == 0; throws
    // std::invalid_argument otherwise.
    void fillChecksumDev(int slot, uint64_t len, uint64_t fileOff, uint64_t salt);

    // Verify the checksum pattern on-device (LDS/wave-reduced mismatch count
    // + first bad offset). Requires fileOff % 8 == 0 and len % 8 == 0 (an odd
    // final u64 is checked too); throws std::invalid_argument otherwise.
    // Synchronizes.
    GpuVerifyResult verifyChecksumDev(int slot, uint64_t len, uint64_t fileOff, uint64_t salt,
                                      bool ldsVariant = false);

    // --verifymixpct variants of the three calls above. The u64 at 8-aligned
    // file offset o holds splitmix64(o + salt) if (o % blockSize) < mixLen,
    // else o + salt; mixLen == 0 gives the plain pattern. Same alignment
    // contract as the plain calls; in addition blockSize % 8 == 0,
    // mixLen % 8 == 0, mixLen <= blockSize and len <= blockSize (one launch
    // wraps the block boundary at most once), else std::invalid_argument.
    // The verifies add into the same persistent counters as the plain ones,
    // so fetchVerifyResult() serves both.
    void fillChecksumMixDev(int slot, uint64_t len, uint64_t fileOff, uint64_t salt,
                            uint64_t blockSize, uint64_t mixLen);
    void verifyChecksumMixDevAsync(int slot, uint64_t len, uint64_t fileOff, uint64_t salt,
                                   uint64_t blockSize, uint64_t mixLen);
    GpuVerifyResult verifyChecksumMixDev(int slot, uint64_t len, uint64_t fileOff,
                                         uint64_t salt, uint64_t blockSize, uint64_t mixLen);

    // --verifydiag variants of the verifies: same compare and same alignment
    // contracts (so numMismatches / firstBadFileOffset equal the plain calls'
    // results), plus the per-word classification of GpuVerifyDiag. They
    // accumulate into a device record of their own, allocated on first use;
    // fetchVerifyDiag() returns and resets it (no device work when nothing
    // was launched since the last fetch).
    void verifyDiagDevAsync(int slot, uint64_t len, uint64_t fileOff, uint64_t salt);
    void verifyDiagMixDevAsync(int slot, uint64_t len, uint64_t fileOff, uint64_t salt,
                               uint64_t blockSize, uint64_t mixLen);
    GpuVerifyDiag fetchVerifyDiag();
    GpuVerifyDiag verifyDiagDev(int slot, uint64_t len, uint64_t fileOff, uint64_t salt);
    GpuVerifyDiag verifyDiagMixDev(int slot, uint64_t len, uint64_t fileOff, uint64_t salt,
                                   uint64_t blockSize, uint64_t mixLen);

    // Block-variance refill: first refillLen bytes random, remainder filled
    // with one random u64 constant (defeats dedup). Requires len % 16 == 0
    // (throws std::invalid_argument otherwise); refillLen is floored to a
    // multiple of 16 and capped at len.
    void blockVarRefillDev(int slot, uint64_t len, uint64_t refillLen, uint64_t seed,
                           bool fastAlgo = false);

    // --dedupepct / --compresspct fill (ebFillReduceKernel): the slot's first
    // len bytes become chunks firstChunk, firstChunk+1, ... of the pattern
    // that fillReduceCPU (engine.h) states, the last one cut at len. Requires
    // len % 16 == 0; chunkBytes a power of two >= 16; randBytes a multiple of
    // 16 and <= chunkBytes; dedupePct in 0..100; pool >= 1; firstChunk < 2^56;
    // else std::invalid_argument. A pure function of its arguments: it does
    // not advance the fill counter that fillRandDev and blockVarRefillDev use.
    void fillReduceDev(int slot, uint64_t len, uint64_t firstChunk, uint64_t chunkBytes,
                       uint64_t randBytes, int dedupePct, uint64_t pool, uint64_t uniqSeed,
                       uint64_t poolSeed);

    // --dedupeverify (ebVerifyReduceKernel): compare the slot's first len bytes,
    // which lie at file offset fileOff, with what fillReduceDev writes for the
    // same arguments. fillReduceDev's argument contract, and fileOff % 8 == 0,
    // else std::invalid_argument; len == 0 launches nothing. The mismatching
    // 8-byte words and the lowest bad file offset (fileOff + byte index) add
    // into the counters of verifyChecksumDevAsync, so fetchVerifyResult()
    // serves it; verifyReduceDev fetches at once (synchronizes).
    void verifyReduceDevAsync(int slot, uint64_t len, uint64_t fileOff, uint64_t firstChunk,
                              uint64_t chunkBytes, uint64_t randBytes, int dedupePct,
                              uint64_t pool, uint64_t uniqSeed, uint64_t poolSeed);
    GpuVerifyResult verifyReduceDev(int slot, uint64_t len, uint64_t fileOff,
                                    uint64_t firstChunk, uint64_t chunkBytes,
                                    uint64_t randBytes, int dedupePct, uint64_t pool,
                                    uint64_t uniqSeed, uint64_t poolSeed);

    // --- CRC-32 / CRC-32C of a slot's first len bytes, computed in HBM ---
    // Everything these need (byte tables, the partials array) is allocated
    // on the first call, so runs without a checksum pay nothing.

    // Enqueue the tile kernel on this context's stream: one raw partial CRC
    // per gpuCrcTileBytes() tile lands at partials[partialBase...] in a
    // growable device array. Requires len % 16 == 0 (throws
    // std::invalid_argument otherwise); len == 0 is a no-op. Successive
    // calls before a fetch must use contiguous, ascending partialBase
    // values: the calls' data, in call order, is the message.
    void crcDevAsync(int slot, uint64_t len, CrcAlgo algo, uint64_t partialBase);

    // One D2H of the partials + one stream synchronization, then the host
    // folds them in tile order and applies init/xorout for totalLen. Returns
    // the finished CRC of everything enqueued since the last fetch; throws
    // std::invalid_argument if that is not totalLen bytes in tileCount tiles.
    uint32_t crcFetch(CrcAlgo algo, uint64_t totalLen, uint64_t tileCount);

    // crcDevAsync + crcFetch of one buffer. Synchronizes.
    uint32_t crcDev(int slot, uint64_t len, CrcAlgo algo);

    // --- CRC-64/NVME of a slot's first len bytes (ebCrc64TilesKernel) ---
    // The contracts of the 32-bit trio above, with gpuCrc64TileBytes()
    // tiles: len % 16 == 0 (std::invalid_argument otherwise), len == 0 is a
    // no-op, contiguous ascending partialBase values between fetches. The
    // tables and the partials array are this trio's own and allocated on its
    // first call, so 32-bit and 64-bit calls may interleave on one context.
    void crc64DevAsync(int slot, uint64_t len, uint64_t partialBase);
    uint64_t crc64Fetch(uint64_t totalLen, uint64_t tileCount);
    uint64_t crc64Dev(int slot, uint64_t len);

    // --- --dataprofile (ebDataProfileKernel; contract at dataprofile.h) ---
    // The accumulators (sketch registers, byte histogram, counters) live in
    // device memory of this context's own, allocated on the first call of any
    // of the three; contexts that share a stream do not share them.
    // dataProfileReset zeroes them with one async memset on the stream.
    // dataProfileDevAsync adds the profile of the slot's first len bytes, cut
    // into chunkBytes chunks (dataProfileChunkOk, else std::invalid_argument;
    // any len up to the slot size, len == 0 launches nothing): it reads the
    // slot and writes nothing but the accumulators. dataProfileFetch
    // synchronizes the stream and merges the device state into acc; it does
    // not reset.
    void dataProfileReset();
    void dataProfileDevAsync(int slot, uint64_t len, uint64_t chunkBytes);
    void dataProfileFetch(DataProfileAcc& acc);

private:
    struct Impl;
    Impl* impl;
    unsigned long long* diagRecordDev(); // device record, allocated on first use
    void dataProfileAlloc();             // device accumulators, on first use
    int devId;
    uint64_t slotSize;
    int slots;
};

} // namespace eb
