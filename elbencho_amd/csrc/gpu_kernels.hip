// gfx950 (CDNA4) kernels + HIP host wrappers for the elbencho_amd engine.
//
// Kernels are written for MI355X: 64-wide wavefronts, 16 B/lane vectorized
// HBM3E access, grid-stride loops capped so the launch fills all 8 XCDs
// (>=2048 workgroups for large buffers), LDS-free reductions via wave
// ballot + per-block atomics (memory-bound ops — no MFMA-shaped work here).
// The CRC kernel is the exception on LDS: its byte tables live there.
//
// Replaces the reference's CUDA runtime calls and curand usage
// (LocalWorker.cpp:1427-1537, :2269-2310) with native CDNA4 code.

#include <hip/hip_runtime.h>

#include <cstdio>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "crc.h"
#include "crc64.h"
#include "gpu.h"

namespace eb {

#define HIP_CHECK(cmd)                                                                 \
    do {                                                                               \
        hipError_t e = (cmd);                                                          \
        if (e != hipSuccess)                                                           \
            throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e) \
                                     + " at " __FILE__ ":" + std::to_string(__LINE__)); \
    } while (0)

// ---------------------------------------------------------------------------
// device-side helpers
// ---------------------------------------------------------------------------

__device__ __forceinline__ uint64_t d_splitmix64(uint64_t& state)
{
    uint64_t z = (state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

__device__ __forceinline__ uint64_t d_rotl64(uint64_t x, int k)
{
    return (x << k) | (x >> (64 - k));
}

struct Xoshiro256pp {
    uint64_t s0, s1, s2, s3;

    __device__ void seed(uint64_t seedVal)
    {
        uint64_t sm = seedVal;
        s0 = d_splitmix64(sm);
        s1 = d_splitmix64(sm);
        s2 = d_splitmix64(sm);
        s3 = d_splitmix64(sm);
    }

    __device__ __forceinline__ uint64_t next()
    {
        const uint64_t result = d_rotl64(s0 + s3, 23) + s0;
        const uint64_t t = s1 << 17;
        s2 ^= s0;
        s3 ^= s1;
        s1 ^= s2;
        s0 ^= s3;
        s2 ^= t;
        s3 = d_rotl64(s3, 45);
        return result;
    }
};

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------

// Random fill: each thread owns an independent xoshiro256++ stream and writes
// 16 B per store (ulonglong2). U64S_PER_THREAD amortizes the 4-splitmix seed
// cost over 8 generated values per grid-stride step.
constexpr int FILL_U64S_PER_STEP = 8; // per thread per grid-stride step

__global__ __launch_bounds__(256) void ebFillRandKernel(ulonglong2* __restrict__ buf,
                                                        uint64_t nVec2, // # of 16B elements
                                                        uint64_t seed)
{
    uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;

    // two independent streams per thread: xoshiro's next() is a serial
    // ~8-op dependency chain, so one stream leaves the SIMD starved for
    // ILP; interleaving two doubles the independent work in flight
    Xoshiro256pp rngA, rngB;
    rngA.seed(seed ^ (tid * 0xA24BAED4963EE407ULL));
    rngB.seed(seed ^ (tid * 0xA24BAED4963EE407ULL) ^ 0x9E6D62D06F6A9A9BULL);

    // each step writes FILL_U64S_PER_STEP/2 ulonglong2 elements
    constexpr int VEC_PER_STEP = FILL_U64S_PER_STEP / 2;
    for (uint64_t base = tid * VEC_PER_STEP; base < nVec2; base += stride * VEC_PER_STEP) {
#pragma unroll
        for (int v = 0; v < VEC_PER_STEP; v++) {
            uint64_t idx = base + v;
            if (idx < nVec2) {
                ulonglong2 val;
                val.x = rngA.next();
                val.y = rngB.next();
                buf[idx] = val;
            }
        }
    }
}

// "fast" random fill: value = splitmix64(seed, index) — a pure function of
// the element index (no per-thread RNG state, ~6 ALU ops per u64), the GPU
// analogue of the reference's golden-prime "fast" RandAlgo. Used for
// --blockvaralgo fast; xoshiro256++ above serves balanced/strong.
__global__ __launch_bounds__(256) void ebFillFastKernel(ulonglong2* __restrict__ buf,
                                                        uint64_t nVec2,
                                                        uint64_t seed)
{
    uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t idx = tid; idx < nVec2; idx += stride) {
        uint64_t s0 = seed + idx * 2 * 0x9E3779B97F4A7C15ULL;
        uint64_t s1 = s0 + 0x9E3779B97F4A7C15ULL;
        ulonglong2 val;
        uint64_t z = s0;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        val.x = z ^ (z >> 31);
        z = s1;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        val.y = z ^ (z >> 31);
        buf[idx] = val;
    }
}

// "fast" block-variance refill: splitmix-of-index prefix + constant tail.
__global__ __launch_bounds__(256) void ebBlockVarFastKernel(ulonglong2* __restrict__ buf,
                                                            uint64_t nVec2,
                                                            uint64_t refillVec2,
                                                            uint64_t seed,
                                                            uint64_t fillConst)
{
    uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t idx = tid; idx < nVec2; idx += stride) {
        ulonglong2 val;
        if (idx < refillVec2) {
            uint64_t s0 = seed + idx * 2 * 0x9E3779B97F4A7C15ULL;
            uint64_t z = s0;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
            val.x = z ^ (z >> 31);
            z = s0 + 0x9E3779B97F4A7C15ULL;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
            val.y = z ^ (z >> 31);
        } else {
            val.x = fillConst;
            val.y = fillConst;
        }
        buf[idx] = val;
    }
}

// --dedupepct / --compresspct pattern (docs/usage.md, "Data reduction"): the
// buffer is a run of chunks numbered firstChunk, firstChunk+1, ...; chunk n
// holds randVec2 16 B elements of splitmix64(key(n) + word * GOLD) and zeros
// after them. key(n) is a pool key (one of `pool` contents that depend on
// poolSeed alone) for dedupePct of 100 chunks, else unique to (uniqSeed, n).
__device__ __forceinline__ uint64_t d_mix64(uint64_t x)
{
    return d_splitmix64(x);
}

// n = firstChunk + j is a pool chunk iff floor((n+1)*d/100) > floor(n*d/100),
// i.e. iff (n*d) % 100 + d >= 100. Only n % 100 matters, so the host passes
// firstMod = firstChunk % 100 and the 64-bit product never forms.
__device__ __forceinline__ uint64_t d_reduceKey(uint64_t firstChunk, uint32_t firstMod,
                                                uint64_t j, uint32_t dedupePct, uint64_t pool,
                                                uint64_t uniqSeed, uint64_t poolSeed)
{
    const uint64_t n = firstChunk + j;
    const uint32_t nMod = (firstMod + (uint32_t)(j % 100)) % 100;
    if ((nMod * dedupePct) % 100 + dedupePct >= 100) {
        const uint64_t h = d_mix64(uniqSeed ^ n);
        // the engine's pool size is a power of two: no 64-bit division then
        const uint64_t member = (pool & (pool - 1)) ? h % pool : h & (pool - 1);
        return d_mix64(poolSeed + member);
    }
    return d_mix64(uniqSeed ^ d_mix64(n));
}

// Pins a workgroup-uniform value to scalar registers. Without it the compiler
// merges the last hash of the uniform key with the per-lane one of the small-
// chunk path and runs it once per element on the vector unit.
__device__ __forceinline__ uint64_t d_uniform64(uint64_t v)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// The 16 B element with index idx (in workgroup step `step` = idx / 256) of a
// buffer that starts with chunk firstChunk: what the fill writes and what the
// verify expects. With chunks of 4 KiB and more (vecShift >= 8) the 256
// elements of a step lie in one chunk, so the chunk number and its key depend
// on the step alone: they are uniform over the workgroup and cost one
// computation per chunk and wave, not per element. Smaller chunks compute the
// key per lane. Lanes in the zero tail of a chunk skip the hashing.
__device__ __forceinline__ ulonglong2 d_reduceElem(uint64_t step, uint64_t idx,
                                                   uint64_t firstChunk, uint32_t firstMod,
                                                   uint32_t vecShift, uint64_t randVec2,
                                                   uint32_t dedupePct, uint64_t pool,
                                                   uint64_t uniqSeed, uint64_t poolSeed)
{
    const uint64_t pos = idx & ((1ULL << vecShift) - 1); // element within its chunk
    ulonglong2 val;
    val.x = 0;
    val.y = 0;
    if (pos < randVec2) {
        uint64_t key; // two calls: the first one's arguments are all uniform
        if (vecShift >= 8)
            key = d_uniform64(d_reduceKey(firstChunk, firstMod, step >> (vecShift - 8),
                                          dedupePct, pool, uniqSeed, poolSeed));
        else
            key = d_reduceKey(firstChunk, firstMod, idx >> vecShift, dedupePct, pool,
                              uniqSeed, poolSeed);
        const uint64_t s0 = key + pos * 2 * 0x9E3779B97F4A7C15ULL;
        val.x = d_mix64(s0);
        val.y = d_mix64(s0 + 0x9E3779B97F4A7C15ULL);
    }
    return val;
}

// One workgroup step writes 256 consecutive 16 B elements = 4 KiB, each one
// d_reduceElem of its index. No LDS, no atomics.
__global__ __launch_bounds__(256) void ebFillReduceKernel(
    ulonglong2* __restrict__ buf, uint64_t nVec2, uint64_t firstChunk, uint32_t firstMod,
    uint32_t vecShift,  // log2(16 B elements per chunk)
    uint64_t randVec2,  // random 16 B elements per chunk, <= 1 << vecShift
    uint32_t dedupePct, uint64_t pool, uint64_t uniqSeed, uint64_t poolSeed)
{
    const uint64_t nSteps = (nVec2 + 255) / 256;
    for (uint64_t step = blockIdx.x; step < nSteps; step += gridDim.x) {
        const uint64_t idx = step * 256 + threadIdx.x;
        const ulonglong2 val = d_reduceElem(step, idx, firstChunk, firstMod, vecShift, randVec2,
                                            dedupePct, pool, uniqSeed, poolSeed);
        if (idx < nVec2) buf[idx] = val;
    }
}

// --dedupeverify: the read side of the pattern above. Same geometry as the
// fill (one workgroup step = 256 consecutive 16 B elements, grid-stride over
// steps): one 16 B load per element, compared with d_reduceElem of its index.
// The buffer's byte 0 lies at file offset fileOff. Mismatching 8-byte words
// are counted (.x and .y separately) and the lowest bad file offset is kept;
// one wave64 reduction after the loop, then one atomicAdd / atomicMin per
// wave that saw a bad word, into the counters of ebVerifyChecksumKernel
// (out[0] += count, out[1] = min offset). No LDS; nothing at or past nVec2 is
// read.
__global__ __launch_bounds__(256) void ebVerifyReduceKernel(
    const ulonglong2* __restrict__ buf, uint64_t nVec2, uint64_t fileOff, uint64_t firstChunk,
    uint32_t firstMod, uint32_t vecShift, uint64_t randVec2, uint32_t dedupePct, uint64_t pool,
    uint64_t uniqSeed, uint64_t poolSeed, unsigned long long* __restrict__ out)
{
    const uint64_t nSteps = (nVec2 + 255) / 256;

    unsigned long long localBad = 0;
    unsigned long long localFirst = ~0ULL;

    for (uint64_t step = blockIdx.x; step < nSteps; step += gridDim.x) {
        const uint64_t idx = step * 256 + threadIdx.x;
        if (idx < nVec2) {
            const ulonglong2 v = buf[idx]; // 16 B/lane coalesced read
            const ulonglong2 exp = d_reduceElem(step, idx, firstChunk, firstMod, vecShift,
                                                randVec2, dedupePct, pool, uniqSeed, poolSeed);
            const uint64_t off0 = fileOff + idx * 16;
            if (v.x != exp.x) {
                localBad++;
                if (off0 < localFirst) localFirst = off0;
            }
            if (v.y != exp.y) {
                localBad++;
                if (off0 + 8 < localFirst) localFirst = off0 + 8;
            }
        }
    }

    // wave64 reduction: sum mismatches and min first-bad across lanes
#pragma unroll
    for (int delta = 32; delta > 0; delta >>= 1) {
        localBad += __shfl_down(localBad, delta, 64);
        unsigned long long other = __shfl_down(localFirst, delta, 64);
        if (other < localFirst) localFirst = other;
    }

    if ((threadIdx.x & 63) == 0 && localBad) {
        atomicAdd(&out[0], localBad);
        atomicMin(&out[1], localFirst);
    }
}

// Integrity fill: u64 at file offset (fileOff + i*8) = fileOff + i*8 + salt.
// 16 B/lane vectorized main loop (same idiom as the other fill kernels);
// an odd final u64 is handled by the first thread.
__global__ __launch_bounds__(256) void ebFillChecksumKernel(uint64_t* __restrict__ buf,
                                                            uint64_t n64,
                                                            uint64_t fileOff,
                                                            uint64_t salt)
{
    uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t nVec2 = n64 / 2;
    ulonglong2* __restrict__ v = (ulonglong2*)buf;
    for (uint64_t i = tid; i < nVec2; i += stride) {
        ulonglong2 val;
        val.x = fileOff + i * 16 + salt;
        val.y = fileOff + i * 16 + 8 + salt;
        v[i] = val;
    }
    if (tid == 0 && (n64 & 1))
        buf[n64 - 1] = fileOff + (n64 - 1) * 8 + salt;
}

// Integrity verify: compare against the checksum pattern; one atomicAdd of
// the wave-reduced mismatch count per wave, atomicMin for first bad offset.
// out[0] = mismatch count, out[1] = first bad file offset (init UINT64_MAX).
// n64 counts u64 words; an odd final word is compared by the first thread,
// mirroring ebFillChecksumKernel, and feeds the same reduction.
__global__ __launch_bounds__(256) void ebVerifyChecksumKernel(const ulonglong2* __restrict__ buf,
                                                              uint64_t n64,
                                                              uint64_t fileOff,
                                                              uint64_t salt,
                                                              unsigned long long* __restrict__ out)
{
    uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t nVec2 = n64 / 2;

    unsigned long long localBad = 0;
    unsigned long long localFirst = ~0ULL;

    for (uint64_t i = tid; i < nVec2; i += stride) {
        ulonglong2 v = buf[i]; // 16 B/lane coalesced read
        uint64_t off0 = fileOff + i * 16;
        uint64_t exp0 = off0 + salt;
        uint64_t exp1 = off0 + 8 + salt;
        if (v.x != exp0) {
            localBad++;
            if (off0 < localFirst) localFirst = off0;
        }
        if (v.y != exp1) {
            localBad++;
            if (off0 + 8 < localFirst) localFirst = off0 + 8;
        }
    }

    if (tid == 0 && (n64 & 1)) { // odd final u64
        uint64_t offT = fileOff + (n64 - 1) * 8;
        if (((const uint64_t*)buf)[n64 - 1] != offT + salt) {
            localBad++;
            if (offT < localFirst) localFirst = offT;
        }
    }

    // wave64 reduction: sum mismatches and min first-bad across lanes
#pragma unroll
    for (int delta = 32; delta > 0; delta >>= 1) {
        localBad += __shfl_down(localBad, delta, 64);
        unsigned long long other = __shfl_down(localFirst, delta, 64);
        if (other < localFirst) localFirst = other;
    }

    if ((threadIdx.x & 63) == 0 && localBad) {
        atomicAdd(&out[0], localBad);
        atomicMin(&out[1], localFirst);
    }
}

// --verifymixpct pattern: the word at byte index i of the launch lies at
// rel = (phase + i) mod B inside its block (phase = fileOff % B, len <= B, so
// one conditional subtract replaces the division) and holds
// splitmix64(fileOff + i + salt) if rel < M, else the plain fileOff + i + salt.
__device__ __forceinline__ uint64_t d_mixWordAt(uint64_t byteIdx, uint64_t fileOff,
                                                uint64_t salt, uint64_t phase,
                                                uint64_t blockSize, uint64_t mixLen)
{
    uint64_t rel = phase + byteIdx;
    if (rel >= blockSize) rel -= blockSize;
    uint64_t x = fileOff + byteIdx + salt;
    uint64_t state = x;
    uint64_t hashed = d_splitmix64(state);
    return (rel < mixLen) ? hashed : x;
}

// Integrity fill with a hashed (incompressible) prefix of mixLen bytes per
// block. Same shape as ebFillChecksumKernel; the two words of one 16 B
// element are decided separately because mixLen % 16 may be 8.
__global__ __launch_bounds__(256) void ebFillChecksumMixKernel(uint64_t* __restrict__ buf,
                                                               uint64_t n64,
                                                               uint64_t fileOff,
                                                               uint64_t salt,
                                                               uint64_t phase,
                                                               uint64_t blockSize,
                                                               uint64_t mixLen)
{
    uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t nVec2 = n64 / 2;
    ulonglong2* __restrict__ v = (ulonglong2*)buf;
    for (uint64_t i = tid; i < nVec2; i += stride) {
        ulonglong2 val;
        val.x = d_mixWordAt(i * 16, fileOff, salt, phase, blockSize, mixLen);
        val.y = d_mixWordAt(i * 16 + 8, fileOff, salt, phase, blockSize, mixLen);
        v[i] = val;
    }
    if (tid == 0 && (n64 & 1))
        buf[n64 - 1] = d_mixWordAt((n64 - 1) * 8, fileOff, salt, phase, blockSize, mixLen);
}

// Verify of the --verifymixpct pattern: ebVerifyChecksumKernel's reduction
// and counters (out[0] += mismatches, out[1] = min first bad file offset).
__global__ __launch_bounds__(256) void ebVerifyChecksumMixKernel(
    const ulonglong2* __restrict__ buf, uint64_t n64, uint64_t fileOff, uint64_t salt,
    uint64_t phase, uint64_t blockSize, uint64_t mixLen, unsigned long long* __restrict__ out)
{
    uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t nVec2 = n64 / 2;

    unsigned long long localBad = 0;
    unsigned long long localFirst = ~0ULL;

    for (uint64_t i = tid; i < nVec2; i += stride) {
        ulonglong2 v = buf[i]; // 16 B/lane coalesced read
        uint64_t off0 = fileOff + i * 16;
        uint64_t exp0 = d_mixWordAt(i * 16, fileOff, salt, phase, blockSize, mixLen);
        uint64_t exp1 = d_mixWordAt(i * 16 + 8, fileOff, salt, phase, blockSize, mixLen);
        if (v.x != exp0) {
            localBad++;
            if (off0 < localFirst) localFirst = off0;
        }
        if (v.y != exp1) {
            localBad++;
            if (off0 + 8 < localFirst) localFirst = off0 + 8;
        }
    }

    if (tid == 0 && (n64 & 1)) { // odd final u64
        uint64_t offT = fileOff + (n64 - 1) * 8;
        if (((const uint64_t*)buf)[n64 - 1] !=
            d_mixWordAt((n64 - 1) * 8, fileOff, salt, phase, blockSize, mixLen)) {
            localBad++;
            if (offT < localFirst) localFirst = offT;
        }
    }

    // wave64 reduction: sum mismatches and min first-bad across lanes
#pragma unroll
    for (int delta = 32; delta > 0; delta >>= 1) {
        localBad += __shfl_down(localBad, delta, 64);
        unsigned long long other = __shfl_down(localFirst, delta, 64);
        if (other < localFirst) localFirst = other;
    }

    if ((threadIdx.x & 63) == 0 && localBad) {
        atomicAdd(&out[0], localBad);
        atomicMin(&out[1], localFirst);
    }
}

// ---------------------------------------------------------------------------
// --verifydiag: the verify compare plus a classification of every bad word
// ---------------------------------------------------------------------------

// Inverse of the splitmix64 finalizer used by d_splitmix64: each xor-shift
// z ^= z >> s is undone by z ^= z >> s ^ z >> 2s (3s >= 64 here), each
// multiply by the modular inverse of its odd constant.
__device__ __forceinline__ uint64_t d_unmix64(uint64_t z)
{
    z ^= (z >> 31) ^ (z >> 62);
    z *= 0x319642B2D24D8EC3ULL;
    z ^= (z >> 27) ^ (z >> 54);
    z *= 0x96DE1B173F119089ULL;
    z ^= (z >> 30) ^ (z >> 60);
    return z;
}

// per-thread GpuVerifyDiag accumulators, in the record's field order
struct DiagAcc {
    unsigned long long nbad = 0, first = ~0ULL, last = 0, runs = 0;
    unsigned long long zero = 0, pattern = 0, bitflip = 0, other = 0;
    long long dmin = 0x7FFFFFFFFFFFFFFFLL, dmax = -0x7FFFFFFFFFFFFFFFLL - 1;
    unsigned long long flipOr = 0;
};

// geometry of one diag launch; MIX=false ignores the block fields
struct DiagGeom {
    uint64_t fileOff, salt, phase, blockSize, mixLen;
};

template <bool MIX>
__device__ __forceinline__ bool d_diagHashed(const DiagGeom& g, uint64_t byteIdx)
{
    if (!MIX) return false;
    uint64_t rel = g.phase + byteIdx;
    if (rel >= g.blockSize) rel -= g.blockSize;
    return rel < g.mixLen;
}

template <bool MIX>
__device__ __forceinline__ uint64_t d_diagExp(const DiagGeom& g, uint64_t byteIdx)
{
    if (MIX) return d_mixWordAt(byteIdx, g.fileOff, g.salt, g.phase, g.blockSize, g.mixLen);
    return g.fileOff + byteIdx + g.salt;
}

// delta of a bad word: what the found value decodes to (a hashed position is
// un-hashed first) minus the plain offset + salt expected here
template <bool MIX>
__device__ __forceinline__ long long d_diagDelta(const DiagGeom& g, uint64_t byteIdx,
                                                 uint64_t v)
{
    uint64_t u = d_diagHashed<MIX>(g, byteIdx) ? d_unmix64(v) - 0x9E3779B97F4A7C15ULL : v;
    return (long long)(u - (g.fileOff + byteIdx + g.salt));
}

// one bad word into the accumulators; first matching class wins
__device__ __forceinline__ void d_diagCount(DiagAcc& a, uint64_t v, uint64_t exp,
                                            uint64_t off, bool pairPattern, long long d,
                                            bool runStart)
{
    a.nbad++;
    if (off < a.first) a.first = off;
    if (off > a.last) a.last = off;
    if (runStart) a.runs++;
    if (v == 0) {
        a.zero++;
    } else if (pairPattern) {
        a.pattern++;
        if (d < a.dmin) a.dmin = d;
        if (d > a.dmax) a.dmax = d;
    } else if (__popcll(v ^ exp) <= 2) {
        a.bitflip++;
        a.flipOr |= v ^ exp;
    } else {
        a.other++;
    }
}

// Shape of ebVerifyChecksumKernel: 16 B/lane loads, grid-stride, the odd
// final word on thread 0. A clean element costs the load and two compares
// (the ballot below is the second compare's lane mask); everything else sits
// behind the "this word is bad" branch.
//
// A bad word starts a run iff its predecessor is good. .y follows .x in the
// same lane; .x follows the previous lane's .y, which the ballot carries.
// Lane 0 of a wave has no previous lane and reads word 2i-1 from memory, only
// when its .x is bad. A wave's 64 elements are consecutive (the grid stride
// is a multiple of 256), so the rule holds in every grid-stride pass.
template <bool MIX>
__device__ __forceinline__ void d_verifyDiag(const ulonglong2* __restrict__ buf, uint64_t n64,
                                             const DiagGeom g,
                                             unsigned long long* __restrict__ out)
{
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t nVec2 = n64 / 2;
    const int lane = threadIdx.x & 63;
    const uint64_t* __restrict__ words = (const uint64_t*)buf;

    DiagAcc a;

    for (uint64_t i = tid; i < nVec2; i += stride) {
        ulonglong2 v = buf[i]; // 16 B/lane coalesced read
        const uint64_t exp0 = d_diagExp<MIX>(g, i * 16);
        const uint64_t exp1 = d_diagExp<MIX>(g, i * 16 + 8);
        const bool badX = v.x != exp0;
        const bool badY = v.y != exp1;
        const unsigned long long badYMask = __ballot(badY);
        if (badX || badY) {
            const uint64_t off0 = g.fileOff + i * 16;
            long long d0 = 0, d1 = 0;
            bool pairPattern = false;
            if (badX && badY && v.x && v.y) {
                d0 = d_diagDelta<MIX>(g, i * 16, v.x);
                d1 = d_diagDelta<MIX>(g, i * 16 + 8, v.y);
                pairPattern = d0 == d1;
            }
            if (badX) {
                bool prevBad = false;
                if (lane)
                    prevBad = (badYMask >> (lane - 1)) & 1;
                else if (i)
                    prevBad = words[2 * i - 1] != d_diagExp<MIX>(g, i * 16 - 8);
                d_diagCount(a, v.x, exp0, off0, pairPattern, d0, !prevBad);
            }
            if (badY) d_diagCount(a, v.y, exp1, off0 + 8, pairPattern, d1, !badX);
        }
    }

    if (tid == 0 && (n64 & 1)) { // odd final u64: no partner, predecessor n64-2
        const uint64_t w = n64 - 1;
        const uint64_t vT = words[w];
        const uint64_t expT = d_diagExp<MIX>(g, w * 8);
        if (vT != expT) {
            bool prevBad = w && words[w - 1] != d_diagExp<MIX>(g, w * 8 - 8);
            d_diagCount(a, vT, expT, g.fileOff + w * 8, false, 0, !prevBad);
        }
    }

    // a clean wave is done here: no reduction, no atomics
    if (!__ballot(a.nbad != 0)) return;

#pragma unroll
    for (int delta = 32; delta > 0; delta >>= 1) {
        a.nbad += __shfl_down(a.nbad, delta, 64);
        a.runs += __shfl_down(a.runs, delta, 64);
        a.zero += __shfl_down(a.zero, delta, 64);
        a.pattern += __shfl_down(a.pattern, delta, 64);
        a.bitflip += __shfl_down(a.bitflip, delta, 64);
        a.other += __shfl_down(a.other, delta, 64);
        a.flipOr |= __shfl_down(a.flipOr, delta, 64);
        unsigned long long oFirst = __shfl_down(a.first, delta, 64);
        if (oFirst < a.first) a.first = oFirst;
        unsigned long long oLast = __shfl_down(a.last, delta, 64);
        if (oLast > a.last) a.last = oLast;
        long long oMin = __shfl_down(a.dmin, delta, 64);
        if (oMin < a.dmin) a.dmin = oMin;
        long long oMax = __shfl_down(a.dmax, delta, 64);
        if (oMax > a.dmax) a.dmax = oMax;
    }

    if (lane == 0) {
        atomicAdd(&out[0], a.nbad);
        atomicMin(&out[1], a.first);
        atomicMax(&out[2], a.last);
        atomicAdd(&out[3], a.runs);
        if (a.zero) atomicAdd(&out[4], a.zero);
        if (a.pattern) {
            atomicAdd(&out[5], a.pattern);
            atomicMin((long long*)&out[8], a.dmin);
            atomicMax((long long*)&out[9], a.dmax);
        }
        if (a.bitflip) {
            atomicAdd(&out[6], a.bitflip);
            atomicOr(&out[10], a.flipOr);
        }
        if (a.other) atomicAdd(&out[7], a.other);
    }
}

// out[] is the GpuVerifyDiag record (GpuVerifyDiag::NUM_FIELDS words).
__global__ __launch_bounds__(256) void ebVerifyDiagKernel(const ulonglong2* __restrict__ buf,
                                                          uint64_t n64, uint64_t fileOff,
                                                          uint64_t salt,
                                                          unsigned long long* __restrict__ out)
{
    d_verifyDiag<false>(buf, n64, DiagGeom{fileOff, salt, 0, 0, 0}, out);
}

__global__ __launch_bounds__(256) void ebVerifyDiagMixKernel(
    const ulonglong2* __restrict__ buf, uint64_t n64, uint64_t fileOff, uint64_t salt,
    uint64_t phase, uint64_t blockSize, uint64_t mixLen, unsigned long long* __restrict__ out)
{
    d_verifyDiag<true>(buf, n64, DiagGeom{fileOff, salt, phase, blockSize, mixLen}, out);
}

// LDS-tiled verify variant — kept ONLY for the A/B that justifies the
// LDS-free design above (profiles/r02_lds_ab.md): stages 16 KiB tiles
// through LDS before comparing. For a streaming compare the extra
// LDS round-trip is pure overhead (no reuse), so this is expected to lose;
// ebVerifyChecksumKernel is what the engine runs.
__global__ __launch_bounds__(256) void ebVerifyChecksumLdsKernel(
    const ulonglong2* __restrict__ buf, uint64_t n64, uint64_t fileOff,
    uint64_t salt, unsigned long long* __restrict__ out)
{
    const uint64_t nVec2 = n64 / 2;
    constexpr int VPT = 4; // vec2 per thread per tile: 256*4*16 B = 16 KiB LDS
    __shared__ ulonglong2 lds[256 * VPT];
    __shared__ unsigned long long blkBad, blkFirst;
    if (threadIdx.x == 0) {
        blkBad = 0;
        blkFirst = ~0ULL;
    }
    __syncthreads();

    unsigned long long localBad = 0, localFirst = ~0ULL;
    const uint64_t tileElems = (uint64_t)blockDim.x * VPT;

    for (uint64_t tileBase = (uint64_t)blockIdx.x * tileElems; tileBase < nVec2;
         tileBase += (uint64_t)gridDim.x * tileElems) {
#pragma unroll
        for (int v = 0; v < VPT; v++) { // stage the tile
            uint64_t idx = tileBase + (uint64_t)v * blockDim.x + threadIdx.x;
            if (idx < nVec2) lds[v * blockDim.x + threadIdx.x] = buf[idx];
        }
        __syncthreads();
#pragma unroll
        for (int v = 0; v < VPT; v++) { // compare from LDS
            uint64_t idx = tileBase + (uint64_t)v * blockDim.x + threadIdx.x;
            if (idx >= nVec2) continue;
            ulonglong2 val = lds[v * blockDim.x + threadIdx.x];
            uint64_t off0 = fileOff + idx * 16;
            if (val.x != off0 + salt) {
                localBad++;
                if (off0 < localFirst) localFirst = off0;
            }
            if (val.y != off0 + 8 + salt) {
                localBad++;
                if (off0 + 8 < localFirst) localFirst = off0 + 8;
            }
        }
        __syncthreads();
    }

    if (blockIdx.x == 0 && threadIdx.x == 0 && (n64 & 1)) { // odd final u64
        uint64_t offT = fileOff + (n64 - 1) * 8;
        if (((const uint64_t*)buf)[n64 - 1] != offT + salt) {
            localBad++;
            if (offT < localFirst) localFirst = offT;
        }
    }

#pragma unroll
    for (int delta = 32; delta > 0; delta >>= 1) {
        localBad += __shfl_down(localBad, delta, 64);
        unsigned long long other = __shfl_down(localFirst, delta, 64);
        if (other < localFirst) localFirst = other;
    }
    if ((threadIdx.x & 63) == 0 && localBad) {
        atomicAdd(&blkBad, localBad);
        atomicMin(&blkFirst, localFirst);
    }
    __syncthreads();
    if (threadIdx.x == 0 && blkBad) {
        atomicAdd(&out[0], blkBad);
        atomicMin(&out[1], blkFirst);
    }
}

// Block-variance refill: first refill64 u64s get fresh random data, the rest
// one random constant (changes every call => defeats dedup of the remainder).
__global__ __launch_bounds__(256) void ebBlockVarKernel(ulonglong2* __restrict__ buf,
                                                        uint64_t nVec2,
                                                        uint64_t refillVec2,
                                                        uint64_t seed,
                                                        uint64_t fillConst)
{
    uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;

    Xoshiro256pp rngA, rngB; // dual streams for ILP (see ebFillRandKernel)
    rngA.seed(seed ^ (tid * 0xA24BAED4963EE407ULL));
    rngB.seed(seed ^ (tid * 0xA24BAED4963EE407ULL) ^ 0x9E6D62D06F6A9A9BULL);

    constexpr int VEC_PER_STEP = FILL_U64S_PER_STEP / 2;
    for (uint64_t base = tid * VEC_PER_STEP; base < nVec2; base += stride * VEC_PER_STEP) {
#pragma unroll
        for (int v = 0; v < VEC_PER_STEP; v++) {
            uint64_t idx = base + v;
            if (idx < nVec2) {
                ulonglong2 val;
                if (idx < refillVec2) {
                    val.x = rngA.next();
                    val.y = rngB.next();
                } else {
                    val.x = fillConst;
                    val.y = fillConst;
                }
                buf[idx] = val;
            }
        }
    }
}

// CRC-32 / CRC-32C of a device buffer: one RAW partial (init 0, no xorout)
// per tile, written to partial[tileIdx] — no atomics, so the result does not
// depend on the grid. The host folds the partials in tile order (crcFetch).
//
// Geometry: a workgroup of CRC_WAVES_PER_TILE waves takes one tile per
// grid-stride pass; each wave covers CRC_STEPS_PER_WAVE rows of 64 lanes x
// 16 B, so one wave covers CRC_WAVE_BYTES and a tile CRC_TILE_BYTES.
//
// A CRC is not a commutative reduction: every partial result is weighted by
// x^(8 * distance to the end) mod P. All distances here are fixed, so each
// weight is a constant, and "multiply by a constant mod P" is four byte-table
// lookups (gfx950 has no carry-less multiply). The tables (crc.h,
// crcBuildTileTables; 48 KiB) are copied into LDS once per workgroup:
//   - 16 lookups turn a lane's 16 B element into its raw CRC,
//   - the lane's accumulator is shifted by one row between steps (Horner),
//   - lanes are joined by __shfl_down with the shift doubling each step,
//   - thread 0 joins the waves' results through LDS.
// A short final tile is right-aligned in the tile's frame: the missing
// leading elements count as zeros, which a raw CRC ignores, so the same
// constants serve every tile and nothing past `nVec2` is read.
constexpr int CRC_STEPS_PER_WAVE = 4; // rows of 64 x 16 B per wave and tile
constexpr int CRC_WAVES_PER_TILE = 4; // = 256 threads / 64
constexpr uint64_t CRC_WAVE_BYTES = (uint64_t)CRC_ROW_BYTES * CRC_STEPS_PER_WAVE; // 4 KiB
constexpr uint64_t CRC_TILE_BYTES = CRC_WAVE_BYTES * CRC_WAVES_PER_TILE;          // 16 KiB

__device__ __forceinline__ uint32_t d_crcLut4(const uint32_t* tab, uint32_t v)
{
    return tab[v & 0xFF] ^ tab[256 + ((v >> 8) & 0xFF)] ^ tab[512 + ((v >> 16) & 0xFF)] ^
           tab[768 + (v >> 24)];
}

__global__ __launch_bounds__(256) void ebCrcTilesKernel(const ulonglong2* __restrict__ buf,
                                                        uint64_t nVec2, // # of 16B elements
                                                        const uint32_t* __restrict__ tables,
                                                        uint32_t* __restrict__ partial)
{
    __shared__ uint32_t tab[CRC_TAB_COUNT * 256];
    __shared__ uint32_t wavePart[CRC_WAVES_PER_TILE];

    for (int i = threadIdx.x; i < CRC_TAB_COUNT * 256 / 4; i += 256)
        ((uint4*)tab)[i] = ((const uint4*)tables)[i];
    __syncthreads();

    constexpr uint64_t TILE_VEC2 = CRC_TILE_BYTES / 16;
    const uint64_t nTiles = (nVec2 + TILE_VEC2 - 1) / TILE_VEC2;
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;

    for (uint64_t tile = blockIdx.x; tile < nTiles; tile += gridDim.x) {
        const uint64_t first = tile * TILE_VEC2;
        const uint64_t have = (nVec2 - first < TILE_VEC2) ? nVec2 - first : TILE_VEC2;
        const uint64_t pad = TILE_VEC2 - have; // leading zero elements of a short tile

        ulonglong2 v[CRC_STEPS_PER_WAVE];
#pragma unroll
        for (int j = 0; j < CRC_STEPS_PER_WAVE; j++) { // 16 B/lane coalesced reads
            uint64_t pos = (uint64_t)(wave * CRC_STEPS_PER_WAVE + j) * 64 + lane;
            v[j] = make_ulonglong2(0, 0);
            if (pos >= pad) v[j] = buf[first + pos - pad];
        }

        uint32_t acc = 0;
#pragma unroll
        for (int j = 0; j < CRC_STEPS_PER_WAVE; j++) {
            uint32_t r = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                r ^= tab[(CRC_TAB_ELEM + k) * 256 + ((v[j].x >> (8 * k)) & 0xFF)];
                r ^= tab[(CRC_TAB_ELEM + 8 + k) * 256 + ((v[j].y >> (8 * k)) & 0xFF)];
            }
            acc = d_crcLut4(tab + CRC_TAB_ROW * 256, acc) ^ r;
        }

        // join the 64 lanes: lane l absorbs lane l+d, shifted by the 16*d
        // bytes that follow it; only lane 0's result is used
#pragma unroll
        for (int i = 0; i < 6; i++) {
            uint32_t other = __shfl_down(acc, 1 << i, 64);
            acc = d_crcLut4(tab + (CRC_TAB_LANE + 4 * i) * 256, acc) ^ other;
        }

        if (lane == 0) wavePart[wave] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t t = 0;
#pragma unroll
            for (int w = 0; w < CRC_WAVES_PER_TILE; w++)
                t = d_crcLut4(tab + CRC_TAB_WAVE * 256, t) ^ wavePart[w];
            partial[tile] = t;
        }
        __syncthreads(); // wavePart is rewritten in the next pass
    }
}

// CRC-64/NVME of a device buffer: the contract of ebCrcTilesKernel at 64
// bits — 16 B/lane reads, one RAW partial per tile written to partial[tile],
// no atomics, grid-stride over tiles, a short final tile right-aligned in the
// tile frame, nothing at or past nVec2 read. Geometry and table image come
// from crc64.h (CRC64_*, crc64BuildTileTables), which also emulates this
// kernel on the host.
//
// At 64 bits a multiply by a constant is eight lookups in 2 KiB tables, and
// the 32-bit kernel's eight shift operators plus the element tables would
// fill a CU's 160 KiB of LDS. This kernel keeps only what the inner loop
// needs, 48 KiB, so three workgroups fit per CU:
//   - 16 element tables: a lane's 16 B element -> its raw CRC (32 KiB),
//   - one row-shift operator for the Horner step between rows (16 KiB).
// There are no lane or wave operators. Raw CRCs are linear, so after its
// rows each thread multiplies its accumulator once by its own weight,
// x^(8 * bytes that follow its last-row element in the tile), read from the
// image into a register at kernel start, with a 64-step shift-and-xor
// carry-less multiply in registers (gfx950 has none in hardware). The tile's
// partial is then the plain XOR of the 256 products: wave shuffles, then four
// words through LDS. That multiply is VALU-only work next to an inner loop
// of LDS lookups (24 ds_read_b64 per 16 B), so other waves' lookups can
// overlap it, and CRC64_STEPS_PER_WAVE = 8 rows amortise it
// (profiles/s3_native_crc64.md).
__device__ __forceinline__ uint64_t d_crc64Lut8(const uint64_t* tab, uint64_t v)
{
    uint64_t r = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) r ^= tab[k * 256 + ((v >> (8 * k)) & 0xFF)];
    return r;
}

// a(x) * b(x) mod P, as crc64MulMod
__device__ __forceinline__ uint64_t d_crc64MulMod(uint64_t a, uint64_t b)
{
    uint64_t p = 0;
#pragma unroll 8
    for (int i = 63; i >= 0; i--) {
        p ^= b & (0 - ((a >> i) & 1));
        b = (b >> 1) ^ (CRC64_NVME_POLY & (0 - (b & 1)));
    }
    return p;
}

__global__ __launch_bounds__(256) void ebCrc64TilesKernel(const ulonglong2* __restrict__ buf,
                                                          uint64_t nVec2, // # of 16B elements
                                                          const uint64_t* __restrict__ tables,
                                                          uint64_t* __restrict__ partial)
{
    static_assert(CRC64_WAVES_PER_TILE * CRC64_WAVE_LANES == 256, "one thread per weight");
    __shared__ __align__(16) uint64_t tab[CRC64_TAB_LDS * 256];
    __shared__ uint64_t wavePart[CRC64_WAVES_PER_TILE];

    for (int i = threadIdx.x; i < CRC64_TAB_LDS * 256 / 2; i += 256)
        ((uint4*)tab)[i] = ((const uint4*)tables)[i];
    const uint64_t weight = tables[CRC64_TAB_WEIGHT * 256 + threadIdx.x];
    __syncthreads();

    constexpr uint64_t TILE_VEC2 = CRC64_TILE_BYTES / 16;
    const uint64_t nTiles = (nVec2 + TILE_VEC2 - 1) / TILE_VEC2;
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;

    for (uint64_t tile = blockIdx.x; tile < nTiles; tile += gridDim.x) {
        const uint64_t first = tile * TILE_VEC2;
        const uint64_t have = (nVec2 - first < TILE_VEC2) ? nVec2 - first : TILE_VEC2;
        const uint64_t pad = TILE_VEC2 - have; // leading zero elements of a short tile

        ulonglong2 v[CRC64_STEPS_PER_WAVE];
#pragma unroll
        for (int j = 0; j < CRC64_STEPS_PER_WAVE; j++) { // 16 B/lane coalesced reads
            uint64_t pos = (uint64_t)(wave * CRC64_STEPS_PER_WAVE + j) * 64 + lane;
            v[j] = make_ulonglong2(0, 0);
            if (pos >= pad) v[j] = buf[first + pos - pad];
        }

        uint64_t acc = 0;
#pragma unroll
        for (int j = 0; j < CRC64_STEPS_PER_WAVE; j++)
            acc = d_crc64Lut8(tab + CRC64_TAB_ROW * 256, acc) ^
                  d_crc64Lut8(tab + CRC64_TAB_ELEM * 256, v[j].x) ^
                  d_crc64Lut8(tab + (CRC64_TAB_ELEM + 8) * 256, v[j].y);

        acc = d_crc64MulMod(weight, acc);

        // the weights have placed every value; what is left is an XOR
#pragma unroll
        for (int i = 0; i < 6; i++) acc ^= __shfl_down(acc, 1 << i, 64);

        if (lane == 0) wavePart[wave] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t t = 0;
#pragma unroll
            for (int w = 0; w < CRC64_WAVES_PER_TILE; w++) t ^= wavePart[w];
            partial[tile] = t;
        }
        __syncthreads(); // wavePart is rewritten in the next pass
    }
}

// ---------------------------------------------------------------------------
// --dataprofile (contract: dataprofile.h)
// ---------------------------------------------------------------------------

// The bytes of one u64 word (the first nBytes are real, the rest masked to 0)
// for the byte histogram. Zero bytes are counted in a register: zero-heavy
// data is the expected input, and 64 lanes adding to one LDS address
// serialise. The others go to the wave's private LDS histogram h.
__device__ __forceinline__ void d_profileWord(uint64_t w, uint32_t nBytes,
                                              uint32_t* __restrict__ h,
                                              unsigned long long& zeros)
{
    if (w == 0) {
        zeros += nBytes;
        return;
    }
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) {
        const uint32_t b = (uint32_t)(w >> (8 * j)) & 0xFFu;
        if (j < nBytes) {
            if (b)
                atomicAdd(&h[b], 1u);
            else
                zeros++;
        }
    }
}

// One team owns one chunk at a time and strides over the chunks: a wave
// (WG = false, chunks below DP_WG_CHUNK_BYTES) or the whole workgroup (WG =
// true: larger chunks would leave one wave alone with too many bytes). Lanes
// take 16 B elements of the chunk, four loads in flight each; an element that
// the chunk's end cuts is masked by byte, so nothing at or past len is
// counted (the load itself may cover up to 15 bytes past len: the caller
// keeps those inside the allocation). The team sum-reduces S and OR-reduces
// "any non-zero byte" (wave64 shuffles, plus LDS between the waves of a
// workgroup team); one lane finishes the fingerprint and does the one
// atomicMax on its sketch register. Counters are summed per workgroup, the
// byte histogram per wave in LDS (4 KiB per workgroup); at the end one global
// 64-bit atomic per non-empty bin and per counter. The kernel reads buf and
// writes regs, hist and counters only.
constexpr uint64_t DP_WG_CHUNK_BYTES = 16384;
constexpr int DP_LOADS_IN_FLIGHT = 4;

template <bool WG>
__global__ __launch_bounds__(256) void ebDataProfileKernel(
    const ulonglong2* __restrict__ buf, uint64_t len, uint32_t chunkShift,
    unsigned int* __restrict__ regs,          // [DP_HLL_M]
    unsigned long long* __restrict__ hist,    // [256]
    unsigned long long* __restrict__ counters) // chunks, bytes, zeroChunks
{
    __shared__ uint32_t sHist[4][256];
    __shared__ unsigned long long sPart[4][2]; // workgroup team: per-wave S, any
    __shared__ unsigned long long sCnt[4][4];  // per wave: the counters, zero bytes

    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < 4 * 256; i += 256) (&sHist[0][0])[i] = 0;
    __syncthreads();

    constexpr uint32_t TEAM = WG ? 256 : 64;
    const uint64_t chunkBytes = 1ULL << chunkShift;
    const uint64_t nChunks = (len + chunkBytes - 1) >> chunkShift;
    const uint64_t team = WG ? (uint64_t)blockIdx.x : (uint64_t)blockIdx.x * 4 + wave;
    const uint64_t nTeams = WG ? (uint64_t)gridDim.x : (uint64_t)gridDim.x * 4;
    const uint32_t teamLane = WG ? threadIdx.x : lane;
    const bool finisher = teamLane == 0;
    uint32_t* __restrict__ h = sHist[wave];

    unsigned long long zeros = 0; // per lane
    unsigned long long myChunks = 0, myBytes = 0, myZeroChunks = 0; // finisher only

    for (uint64_t k = team; k < nChunks; k += nTeams) {
        const uint64_t start = k << chunkShift;
        const uint64_t n = (len - start < chunkBytes) ? len - start : chunkBytes;
        const uint64_t nv = (n + 15) / 16; // 16 B elements, the last one maybe cut
        const ulonglong2* __restrict__ src = buf + (start >> 4);

        unsigned long long S = 0, any = 0;
        for (uint64_t base = 0; base < nv; base += (uint64_t)TEAM * DP_LOADS_IN_FLIGHT) {
            ulonglong2 val[DP_LOADS_IN_FLIGHT];
#pragma unroll
            for (int u = 0; u < DP_LOADS_IN_FLIGHT; u++) {
                const uint64_t v = base + (uint64_t)u * TEAM + teamLane;
                val[u].x = 0;
                val[u].y = 0;
                if (v < nv) val[u] = src[v]; // 16 B/lane coalesced read
            }
#pragma unroll
            for (int u = 0; u < DP_LOADS_IN_FLIGHT; u++) {
                const uint64_t v = base + (uint64_t)u * TEAM + teamLane;
                if (v >= nv) continue;
                const uint64_t rem = n - v * 16; // real bytes from this element on, >= 1
                uint64_t x = val[u].x, y = val[u].y;
                uint32_t nx = 8, ny = 8;
                if (rem < 16) { // the chunk ends inside this element
                    nx = rem < 8 ? (uint32_t)rem : 8;
                    ny = rem > 8 ? (uint32_t)rem - 8 : 0;
                    if (nx < 8) x &= (1ULL << (8 * nx)) - 1;
                    y = ny ? y & ((1ULL << (8 * ny)) - 1) : 0; // ny <= 7 here
                }
                S += dpWordTerm(x, 2 * v);
                if (ny) S += dpWordTerm(y, 2 * v + 1);
                any |= x | y;
                d_profileWord(x, nx, h, zeros);
                d_profileWord(y, ny, h, zeros);
            }
        }

#pragma unroll
        for (int delta = 32; delta > 0; delta >>= 1) {
            S += __shfl_down(S, delta, 64);
            any |= __shfl_down(any, delta, 64);
        }
        if (WG) { // k depends on blockIdx alone: every thread gets here
            if (lane == 0) {
                sPart[wave][0] = S;
                sPart[wave][1] = any;
            }
            __syncthreads();
            if (finisher) {
                S = sPart[0][0] + sPart[1][0] + sPart[2][0] + sPart[3][0];
                any = sPart[0][1] | sPart[1][1] | sPart[2][1] | sPart[3][1];
            }
            __syncthreads(); // sPart is rewritten for the next chunk
        }
        if (finisher) {
            const uint64_t fp = dpFingerprint(S, n);
            atomicMax(&regs[dpRegIndex(fp)], dpRho(fp));
            myChunks++;
            myBytes += n;
            if (!any) myZeroChunks++;
        }
    }

#pragma unroll
    for (int delta = 32; delta > 0; delta >>= 1) zeros += __shfl_down(zeros, delta, 64);
    if (lane == 0) {
        sCnt[wave][0] = myChunks;
        sCnt[wave][1] = myBytes;
        sCnt[wave][2] = myZeroChunks;
        sCnt[wave][3] = zeros;
    }
    __syncthreads();

    const uint32_t t = threadIdx.x; // owns bin t; threads 0..2 a counter too
    unsigned long long bin = (unsigned long long)sHist[0][t] + sHist[1][t] + sHist[2][t] +
                             sHist[3][t];
    if (t == 0) bin += sCnt[0][3] + sCnt[1][3] + sCnt[2][3] + sCnt[3][3];
    if (bin) atomicAdd(&hist[t], bin);
    if (t < 3) {
        const unsigned long long c = sCnt[0][t] + sCnt[1][t] + sCnt[2][t] + sCnt[3][t];
        if (c) atomicAdd(&counters[t], c);
    }
}

// ---------------------------------------------------------------------------
// host wrappers
// ---------------------------------------------------------------------------

// A/B micro-bench: verify-kernel effective read bandwidth (GB/s), LDS-free
// vs LDS-tiled variant. Used to justify the LDS-free production kernel.
double gpuVerifyBenchGBs(uint64_t len, int iters, bool lds, int dev);

bool gpuHostRegisterTry(void* ptr, uint64_t len)
{
    return hipHostRegister(ptr, len, hipHostRegisterDefault) == hipSuccess;
}

void gpuHostRegister(void* ptr, uint64_t len)
{
    HIP_CHECK(hipHostRegister(ptr, len, hipHostRegisterDefault));
}

void gpuHostUnregister(void* ptr) { (void)hipHostUnregister(ptr); }

int gpuDeviceCount()
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return 0;
    return n;
}

std::string gpuProbeError()
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return hipGetErrorString(e);
    return "ok: " + std::to_string(n) + " device(s)";
}

std::string gpuDeviceName(int deviceId)
{
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, deviceId) != hipSuccess) return "";
    return prop.name;
}

// NUMA node the GPU's PCIe device hangs off (-1 unknown). At multi-GPU
// scale, binding each rank's workers (and so its page-cache pages) to its
// GPU's node keeps the H2D DMA on-socket — 8 GPUs x ~50 GB/s would
// otherwise saturate the inter-socket fabric.
int gpuNumaNode(int deviceId)
{
    char busId[32] = {0};
    if (hipDeviceGetPCIBusId(busId, sizeof(busId), deviceId) != hipSuccess)
        return -1;
    for (char* c = busId; *c; ++c) *c = (char)tolower(*c);
    std::string path = std::string("/sys/bus/pci/devices/") + busId + "/numa_node";
    FILE* f = fopen(path.c_str(), "r");
    if (!f) return -1;
    int node = -1;
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
    return node;
}

static dim3 gridForBytes(uint64_t workItems)
{
    // memory-bound grid sizing: >= a few thousand workgroups fills 256 CUs
    // across 8 XCDs; grid-stride handles the remainder.
    uint64_t blocks = (workItems + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks == 0) blocks = 1;
    return dim3((uint32_t)blocks);
}

// Optional process-wide shared stream pool (EB_GPU_SHARED_STREAMS=N): many
// worker threads funnel their staging copies through N HIP streams per
// device instead of one stream each — fewer SDMA queues, less switching.
static hipStream_t sharedStream(int devId, int& poolSizeOut)
{
    static std::mutex mtx;
    static std::map<int, std::vector<hipStream_t>> pools;
    static std::map<int, int> next;
    // default 8: measured best on MI355X for 16-worker staging (see
    // profiles/r01_staging_tuning.md); EB_GPU_SHARED_STREAMS=0 gives each
    // worker its own stream
    static const int poolSize = [] {
        const char* v = getenv("EB_GPU_SHARED_STREAMS");
        int n = v ? atoi(v) : 8;
        return (n >= 1 && n <= 64) ? n : 0;
    }();

    poolSizeOut = poolSize;
    if (!poolSize) return nullptr;

    std::lock_guard<std::mutex> lk(mtx);
    auto& pool = pools[devId];
    if (pool.empty()) {
        pool.resize(poolSize);
        for (int i = 0; i < poolSize; i++)
            HIP_CHECK(hipStreamCreateWithFlags(&pool[i], hipStreamNonBlocking));
    }
    return pool[next[devId]++ % poolSize];
}

struct GpuCtx::Impl {
    hipStream_t stream = nullptr;
    bool ownStream = true;
    char* devBase = nullptr;
    char* hostBase = nullptr;
    uint64_t slotStride = 0;
    std::vector<char*> devBufs;
    std::vector<char*> hostBufs;
    std::vector<hipEvent_t> slotEvents;
    // --lat timed pairs (timing-enabled events, lazily created)
    std::vector<hipEvent_t> timedStart, timedEnd;
    std::vector<char> timedActive;
    bool hostPinned = false;
    unsigned long long* verifyOutDev = nullptr;  // [2]
    unsigned long long* verifyOutHost = nullptr; // pinned [2]
    uint64_t fillCallCounter = 0;
    bool verifyDirty = false; // device counters hold accumulated results

    // --verifydiag record, allocated by the first diag launch
    unsigned long long* diagDev = nullptr;  // [GpuVerifyDiag::NUM_FIELDS]
    unsigned long long* diagHost = nullptr; // pinned mirror
    bool diagDirty = false;

    // CRC state, allocated by the first crcDevAsync (runs without a
    // checksum pay nothing)
    uint32_t* crcTabDev[2] = {nullptr, nullptr}; // per CrcAlgo, CRC_TAB_COUNT*256 words
    CrcShift crcTileShift[2];                    // host fold: shift by one tile
    uint32_t* crcPartDev = nullptr;              // partial[tile], growable
    uint32_t* crcPartHost = nullptr;             // pinned mirror
    uint64_t crcPartCap = 0;                     // in partials
    struct CrcCall { uint64_t base, len; };
    std::vector<CrcCall> crcPending;             // enqueued since the last fetch

    // CRC-64/NVME state: its own, allocated by the first crc64DevAsync
    uint64_t* crc64TabDev = nullptr;             // CRC64_TAB_COUNT*256 words
    std::unique_ptr<Crc64Shift> crc64TileShift;  // host fold: shift by one tile
    uint64_t* crc64PartDev = nullptr;            // partial[tile], growable
    uint64_t* crc64PartHost = nullptr;           // pinned mirror
    uint64_t crc64PartCap = 0;                   // in partials
    std::vector<CrcCall> crc64Pending;           // enqueued since the last fetch

    // --dataprofile accumulators, allocated by the first dataProfile* call:
    // u32 regs[DP_HLL_M], then u64 hist[256], then u64 counters[4] (3 used)
    char* dpDev = nullptr;
    char* dpHost = nullptr; // pinned mirror
};

constexpr size_t DP_REGS_BYTES = DP_HLL_M * sizeof(unsigned int);
constexpr size_t DP_HIST_BYTES = 256 * sizeof(unsigned long long);
constexpr size_t DP_DEV_BYTES = DP_REGS_BYTES + DP_HIST_BYTES + 4 * sizeof(unsigned long long);

GpuCtx::GpuCtx(int deviceId, int numSlots, uint64_t bufSize, bool pinnedHostBufs)
    : impl(new Impl), devId(deviceId), slotSize(bufSize), slots(numSlots)
{
    HIP_CHECK(hipSetDevice(deviceId));
    int poolSize = 0;
    hipStream_t shared = sharedStream(deviceId, poolSize);
    if (shared) {
        impl->stream = shared;
        impl->ownStream = false;
    } else {
        HIP_CHECK(hipStreamCreateWithFlags(&impl->stream, hipStreamNonBlocking));
    }

    impl->hostPinned = pinnedHostBufs;
    impl->devBufs.resize(numSlots, nullptr);
    impl->hostBufs.resize(numSlots, nullptr);

    // one contiguous slab per side: slot i at base + i*slotStride. Contiguous
    // slots let small-block staging batch N slots into ONE ranged memcpy.
    impl->slotStride = (bufSize + 4095) & ~4095ULL; // keep O_DIRECT alignment
    HIP_CHECK(hipMalloc(&impl->devBase, impl->slotStride * numSlots));
    if (pinnedHostBufs) {
        // EB_GPU_HOSTALLOC=nc: non-coherent pinned pages (device-optimized)
        static const unsigned hostFlags = [] {
            const char* v = getenv("EB_GPU_HOSTALLOC");
            return (v && v[0] == 'n') ? hipHostMallocNonCoherent : hipHostMallocDefault;
        }();
        HIP_CHECK(hipHostMalloc(&impl->hostBase, impl->slotStride * numSlots, hostFlags));
    } else {
        if (posix_memalign((void**)&impl->hostBase, 4096, impl->slotStride * numSlots))
            throw std::runtime_error("host buffer alloc failed");
    }
    for (int i = 0; i < numSlots; i++) {
        impl->devBufs[i] = impl->devBase + (uint64_t)i * impl->slotStride;
        impl->hostBufs[i] = impl->hostBase + (uint64_t)i * impl->slotStride;
    }

    impl->slotEvents.resize(numSlots, nullptr);
    // EB_GPU_EVBLOCK=1: block instead of spin in hipEventSynchronize — frees
    // host cores for pread/pwrite when many worker threads wait on events
    static const bool evBlock = [] {
        const char* v = getenv("EB_GPU_EVBLOCK");
        return v && v[0] == '1';
    }();
    unsigned evFlags = hipEventDisableTiming | (evBlock ? hipEventBlockingSync : 0);
    for (int i = 0; i < numSlots; i++)
        HIP_CHECK(hipEventCreateWithFlags(&impl->slotEvents[i], evFlags));

    HIP_CHECK(hipMalloc(&impl->verifyOutDev, 2 * sizeof(unsigned long long)));
    HIP_CHECK(hipHostMalloc(&impl->verifyOutHost, 2 * sizeof(unsigned long long),
                            hipHostMallocDefault));

    // zero the persistent verify counters (first bad offset = UINT64_MAX)
    impl->verifyOutHost[0] = 0;
    impl->verifyOutHost[1] = ~0ULL;
    HIP_CHECK(hipMemcpy(impl->verifyOutDev, impl->verifyOutHost,
                        2 * sizeof(unsigned long long), hipMemcpyHostToDevice));
}

GpuCtx::~GpuCtx()
{
    (void)hipSetDevice(devId);
    if (impl->devBase) (void)hipFree(impl->devBase);
    if (impl->hostBase) {
        if (impl->hostPinned)
            (void)hipHostFree(impl->hostBase);
        else
            free(impl->hostBase);
    }
    for (auto e : impl->slotEvents)
        if (e) (void)hipEventDestroy(e);
    for (auto e : impl->timedStart)
        if (e) (void)hipEventDestroy(e);
    for (auto e : impl->timedEnd)
        if (e) (void)hipEventDestroy(e);
    if (impl->verifyOutDev) (void)hipFree(impl->verifyOutDev);
    if (impl->verifyOutHost) (void)hipHostFree(impl->verifyOutHost);
    if (impl->diagDev) (void)hipFree(impl->diagDev);
    if (impl->diagHost) (void)hipHostFree(impl->diagHost);
    for (auto p : impl->crcTabDev)
        if (p) (void)hipFree(p);
    if (impl->crcPartDev) (void)hipFree(impl->crcPartDev);
    if (impl->crcPartHost) (void)hipHostFree(impl->crcPartHost);
    if (impl->crc64TabDev) (void)hipFree(impl->crc64TabDev);
    if (impl->crc64PartDev) (void)hipFree(impl->crc64PartDev);
    if (impl->crc64PartHost) (void)hipHostFree(impl->crc64PartHost);
    if (impl->dpDev) (void)hipFree(impl->dpDev);
    if (impl->dpHost) (void)hipHostFree(impl->dpHost);
    if (impl->stream && impl->ownStream) (void)hipStreamDestroy(impl->stream);
    delete impl;
}

char* GpuCtx::hostBuf(int slot) const { return impl->hostBufs[slot]; }

void GpuCtx::bindThread() { HIP_CHECK(hipSetDevice(devId)); }

uint64_t GpuCtx::slotStride() const { return impl->slotStride; }

void GpuCtx::snapshotSlots(std::vector<char>& dst)
{
    dst.resize(impl->slotStride * (uint64_t)slots);
    if (dst.empty()) return;
    HIP_CHECK(hipMemcpyAsync(dst.data(), impl->devBase, dst.size(), hipMemcpyDeviceToHost,
                             impl->stream));
    HIP_CHECK(hipStreamSynchronize(impl->stream));
}

uint64_t GpuCtx::streamId() const { return (uint64_t)(uintptr_t)impl->stream; }

bool GpuCtx::streamShared() const { return !impl->ownStream; }

void GpuCtx::copyFromHostAsync(int slot, const void* src, uint64_t len)
{
    HIP_CHECK(hipMemcpyAsync(impl->devBufs[slot], src, len, hipMemcpyHostToDevice,
                             impl->stream));
}

void GpuCtx::copyToHostAsync(int slot, void* dst, uint64_t len)
{
    HIP_CHECK(hipMemcpyAsync(dst, impl->devBufs[slot], len, hipMemcpyDeviceToHost,
                             impl->stream));
}

void GpuCtx::copyH2DAsync(int slot, uint64_t len)
{
    HIP_CHECK(hipMemcpyAsync(impl->devBufs[slot], impl->hostBufs[slot], len,
                             hipMemcpyHostToDevice, impl->stream));
}

// one memcpy spanning `count` consecutive slots (small-block batching)
void GpuCtx::copyH2DRangeAsync(int firstSlot, int count)
{
    HIP_CHECK(hipMemcpyAsync(impl->devBufs[firstSlot], impl->hostBufs[firstSlot],
                             impl->slotStride * count, hipMemcpyHostToDevice,
                             impl->stream));
}

void GpuCtx::copyD2HAsync(int slot, uint64_t len)
{
    HIP_CHECK(hipMemcpyAsync(impl->hostBufs[slot], impl->devBufs[slot], len,
                             hipMemcpyDeviceToHost, impl->stream));
}

void GpuCtx::syncStream() { HIP_CHECK(hipStreamSynchronize(impl->stream)); }

void GpuCtx::recordSlotEvent(int slot)
{
    HIP_CHECK(hipEventRecord(impl->slotEvents[slot], impl->stream));
}

void GpuCtx::waitSlotEvent(int slot)
{
    HIP_CHECK(hipEventSynchronize(impl->slotEvents[slot]));
}

// --- timed pairs for --lat on the pipelined fast path ---

void GpuCtx::recordTimedStart(int slot)
{
    if (impl->timedStart.empty()) { // lazy: timing ENABLED (no DisableTiming)
        impl->timedStart.resize(slots, nullptr);
        impl->timedEnd.resize(slots, nullptr);
        impl->timedActive.assign(slots, 0);
        for (int i = 0; i < slots; i++) {
            HIP_CHECK(hipEventCreateWithFlags(&impl->timedStart[i], hipEventDefault));
            HIP_CHECK(hipEventCreateWithFlags(&impl->timedEnd[i], hipEventDefault));
        }
    }
    HIP_CHECK(hipEventRecord(impl->timedStart[slot], impl->stream));
}

void GpuCtx::recordTimedEnd(int slot)
{
    HIP_CHECK(hipEventRecord(impl->timedEnd[slot], impl->stream));
    impl->timedActive[slot] = 1;
}

bool GpuCtx::timedPairActive(int slot) const
{
    return !impl->timedActive.empty() && impl->timedActive[slot];
}

uint64_t GpuCtx::timedElapsedUSec(int slot)
{
    HIP_CHECK(hipEventSynchronize(impl->timedEnd[slot]));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, impl->timedStart[slot], impl->timedEnd[slot]));
    impl->timedActive[slot] = 0;
    return (uint64_t)(ms * 1000.0f);
}

void GpuCtx::dropTimedPairs()
{
    for (auto& a : impl->timedActive) a = 0;
}

static void requireAligned(const char* what, uint64_t len, uint64_t lenAlign,
                           uint64_t fileOff = 0)
{
    if (len % lenAlign)
        throw std::invalid_argument(std::string(what) + ": len " + std::to_string(len) +
                                    " is not a multiple of " + std::to_string(lenAlign));
    if (fileOff % 8)
        throw std::invalid_argument(std::string(what) + ": fileOff " +
                                    std::to_string(fileOff) + " is not a multiple of 8");
}

void GpuCtx::verifyChecksumDevAsync(int slot, uint64_t len, uint64_t fileOff, uint64_t salt,
                                    bool ldsVariant)
{
    requireAligned("verifyChecksumDev", len, 8, fileOff);
    uint64_t n64 = len / 8;
    if (!n64) return;
    dim3 grid = gridForBytes(n64 / 2);
    if (ldsVariant)
        hipLaunchKernelGGL(ebVerifyChecksumLdsKernel, grid, dim3(256), 0, impl->stream,
                           (const ulonglong2*)impl->devBufs[slot], n64, fileOff, salt,
                           impl->verifyOutDev);
    else
        hipLaunchKernelGGL(ebVerifyChecksumKernel, grid, dim3(256), 0, impl->stream,
                           (const ulonglong2*)impl->devBufs[slot], n64, fileOff, salt,
                           impl->verifyOutDev);
    HIP_CHECK(hipGetLastError());
    impl->verifyDirty = true;
}

GpuVerifyResult GpuCtx::fetchVerifyResult()
{
    if (!impl->verifyDirty) return GpuVerifyResult{0, ~0ULL};
    HIP_CHECK(hipMemcpyAsync(impl->verifyOutHost, impl->verifyOutDev,
                             2 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                             impl->stream));
    HIP_CHECK(hipStreamSynchronize(impl->stream));
    GpuVerifyResult r{impl->verifyOutHost[0], impl->verifyOutHost[1]};
    impl->verifyOutHost[0] = 0;
    impl->verifyOutHost[1] = ~0ULL;
    HIP_CHECK(hipMemcpyAsync(impl->verifyOutDev, impl->verifyOutHost,
                             2 * sizeof(unsigned long long), hipMemcpyHostToDevice,
                             impl->stream));
    HIP_CHECK(hipStreamSynchronize(impl->stream));
    impl->verifyDirty = false;
    return r;
}

void GpuCtx::fillRandDev(int slot, uint64_t len, uint64_t seed, bool fastAlgo)
{
    requireAligned("fillRandDev", len, 16);
    uint64_t nVec2 = len / 16;
    uint64_t seq = ++impl->fillCallCounter;
    if (nVec2) {
        if (fastAlgo) {
            dim3 grid = gridForBytes(nVec2);
            hipLaunchKernelGGL(ebFillFastKernel, grid, dim3(256), 0, impl->stream,
                               (ulonglong2*)impl->devBufs[slot], nVec2,
                               seed + seq * 0x9E3779B9ULL);
        } else {
            dim3 grid = gridForBytes(nVec2 / (FILL_U64S_PER_STEP / 2));
            hipLaunchKernelGGL(ebFillRandKernel, grid, dim3(256), 0, impl->stream,
                               (ulonglong2*)impl->devBufs[slot], nVec2,
                               seed + seq * 0x9E3779B9ULL);
        }
        HIP_CHECK(hipGetLastError());
    }
}

void GpuCtx::fillChecksumDev(int slot, uint64_t len, uint64_t fileOff, uint64_t salt)
{
    requireAligned("fillChecksumDev", len, 8, fileOff);
    uint64_t n64 = len / 8;
    if (!n64) return;
    dim3 grid = gridForBytes(n64);
    hipLaunchKernelGGL(ebFillChecksumKernel, grid, dim3(256), 0, impl->stream,
                       (uint64_t*)impl->devBufs[slot], n64, fileOff, salt);
    HIP_CHECK(hipGetLastError());
}

GpuVerifyResult GpuCtx::verifyChecksumDev(int slot, uint64_t len, uint64_t fileOff, uint64_t salt,
                                          bool ldsVariant)
{
    verifyChecksumDevAsync(slot, len, fileOff, salt, ldsVariant);
    return fetchVerifyResult();
}

// --verifymixpct launch contract on top of requireAligned(len 8, fileOff 8):
// one launch never spans more than one block length, so the kernels need a
// single conditional subtract to find a word's place in its block
static void requireMixGeometry(const char* what, uint64_t len, uint64_t blockSize,
                               uint64_t mixLen)
{
    if (!blockSize || blockSize % 8)
        throw std::invalid_argument(std::string(what) + ": block size " +
                                    std::to_string(blockSize) +
                                    " is not a positive multiple of 8");
    if (mixLen % 8)
        throw std::invalid_argument(std::string(what) + ": mix length " +
                                    std::to_string(mixLen) + " is not a multiple of 8");
    if (mixLen > blockSize)
        throw std::invalid_argument(std::string(what) + ": mix length " +
                                    std::to_string(mixLen) + " exceeds the block size " +
                                    std::to_string(blockSize));
    if (len > blockSize)
        throw std::invalid_argument(std::string(what) + ": len " + std::to_string(len) +
                                    " exceeds the block size " + std::to_string(blockSize));
}

void GpuCtx::fillChecksumMixDev(int slot, uint64_t len, uint64_t fileOff, uint64_t salt,
                                uint64_t blockSize, uint64_t mixLen)
{
    requireAligned("fillChecksumMixDev", len, 8, fileOff);
    requireMixGeometry("fillChecksumMixDev", len, blockSize, mixLen);
    if (len > impl->slotStride)
        throw std::invalid_argument("fillChecksumMixDev: len " + std::to_string(len) +
                                    " exceeds the slot size");
    uint64_t n64 = len / 8;
    if (!n64) return;
    dim3 grid = gridForBytes(n64);
    hipLaunchKernelGGL(ebFillChecksumMixKernel, grid, dim3(256), 0, impl->stream,
                       (uint64_t*)impl->devBufs[slot], n64, fileOff, salt,
                       fileOff % blockSize, blockSize, mixLen);
    HIP_CHECK(hipGetLastError());
}

void GpuCtx::verifyChecksumMixDevAsync(int slot, uint64_t len, uint64_t fileOff,
                                       uint64_t salt, uint64_t blockSize, uint64_t mixLen)
{
    requireAligned("verifyChecksumMixDev", len, 8, fileOff);
    requireMixGeometry("verifyChecksumMixDev", len, blockSize, mixLen);
    if (len > impl->slotStride)
        throw std::invalid_argument("verifyChecksumMixDev: len " + std::to_string(len) +
                                    " exceeds the slot size");
    uint64_t n64 = len / 8;
    if (!n64) return;
    dim3 grid = gridForBytes(n64 / 2);
    hipLaunchKernelGGL(ebVerifyChecksumMixKernel, grid, dim3(256), 0, impl->stream,
                       (const ulonglong2*)impl->devBufs[slot], n64, fileOff, salt,
                       fileOff % blockSize, blockSize, mixLen, impl->verifyOutDev);
    HIP_CHECK(hipGetLastError());
    impl->verifyDirty = true;
}

GpuVerifyResult GpuCtx::verifyChecksumMixDev(int slot, uint64_t len, uint64_t fileOff,
                                             uint64_t salt, uint64_t blockSize,
                                             uint64_t mixLen)
{
    verifyChecksumMixDevAsync(slot, len, fileOff, salt, blockSize, mixLen);
    return fetchVerifyResult();
}

// --- --verifydiag ---

// the empty record in device layout (GpuVerifyDiag's field order)
static void diagInitWords(unsigned long long* w)
{
    const GpuVerifyDiag init;
    w[0] = init.numMismatches;
    w[1] = init.firstBadFileOffset;
    w[2] = init.lastBadFileOffset;
    w[3] = init.runs;
    w[4] = init.zero;
    w[5] = init.pattern;
    w[6] = init.bitflip;
    w[7] = init.other;
    w[8] = (unsigned long long)init.deltaMin;
    w[9] = (unsigned long long)init.deltaMax;
    w[10] = init.flipOr;
}

unsigned long long* GpuCtx::diagRecordDev()
{
    if (!impl->diagDev) { // first diag launch of this context
        constexpr size_t bytes = GpuVerifyDiag::NUM_FIELDS * sizeof(unsigned long long);
        HIP_CHECK(hipMalloc(&impl->diagDev, bytes));
        HIP_CHECK(hipHostMalloc(&impl->diagHost, bytes, hipHostMallocDefault));
        diagInitWords(impl->diagHost);
        HIP_CHECK(hipMemcpy(impl->diagDev, impl->diagHost, bytes, hipMemcpyHostToDevice));
    }
    return impl->diagDev;
}

void GpuCtx::verifyDiagDevAsync(int slot, uint64_t len, uint64_t fileOff, uint64_t salt)
{
    requireAligned("verifyDiagDev", len, 8, fileOff);
    if (len > impl->slotStride)
        throw std::invalid_argument("verifyDiagDev: len " + std::to_string(len) +
                                    " exceeds the slot size");
    uint64_t n64 = len / 8;
    if (!n64) return;
    unsigned long long* rec = diagRecordDev();
    hipLaunchKernelGGL(ebVerifyDiagKernel, gridForBytes(n64 / 2), dim3(256), 0, impl->stream,
                       (const ulonglong2*)impl->devBufs[slot], n64, fileOff, salt, rec);
    HIP_CHECK(hipGetLastError());
    impl->diagDirty = true;
}

void GpuCtx::verifyDiagMixDevAsync(int slot, uint64_t len, uint64_t fileOff, uint64_t salt,
                                   uint64_t blockSize, uint64_t mixLen)
{
    requireAligned("verifyDiagMixDev", len, 8, fileOff);
    requireMixGeometry("verifyDiagMixDev", len, blockSize, mixLen);
    if (len > impl->slotStride)
        throw std::invalid_argument("verifyDiagMixDev: len " + std::to_string(len) +
                                    " exceeds the slot size");
    uint64_t n64 = len / 8;
    if (!n64) return;
    unsigned long long* rec = diagRecordDev();
    hipLaunchKernelGGL(ebVerifyDiagMixKernel, gridForBytes(n64 / 2), dim3(256), 0,
                       impl->stream, (const ulonglong2*)impl->devBufs[slot], n64, fileOff,
                       salt, fileOff % blockSize, blockSize, mixLen, rec);
    HIP_CHECK(hipGetLastError());
    impl->diagDirty = true;
}

GpuVerifyDiag GpuCtx::fetchVerifyDiag()
{
    GpuVerifyDiag r;
    if (!impl->diagDirty) return r;
    constexpr size_t bytes = GpuVerifyDiag::NUM_FIELDS * sizeof(unsigned long long);
    unsigned long long* h = impl->diagHost;
    HIP_CHECK(hipMemcpyAsync(h, impl->diagDev, bytes, hipMemcpyDeviceToHost, impl->stream));
    HIP_CHECK(hipStreamSynchronize(impl->stream));
    r.numMismatches = h[0];
    r.firstBadFileOffset = h[1];
    r.lastBadFileOffset = h[2];
    r.runs = h[3];
    r.zero = h[4];
    r.pattern = h[5];
    r.bitflip = h[6];
    r.other = h[7];
    r.deltaMin = (int64_t)h[8];
    r.deltaMax = (int64_t)h[9];
    r.flipOr = h[10];
    diagInitWords(h);
    HIP_CHECK(hipMemcpyAsync(impl->diagDev, h, bytes, hipMemcpyHostToDevice, impl->stream));
    HIP_CHECK(hipStreamSynchronize(impl->stream));
    impl->diagDirty = false;
    return r;
}

GpuVerifyDiag GpuCtx::verifyDiagDev(int slot, uint64_t len, uint64_t fileOff, uint64_t salt)
{
    verifyDiagDevAsync(slot, len, fileOff, salt);
    return fetchVerifyDiag();
}

GpuVerifyDiag GpuCtx::verifyDiagMixDev(int slot, uint64_t len, uint64_t fileOff, uint64_t salt,
                                       uint64_t blockSize, uint64_t mixLen)
{
    verifyDiagMixDevAsync(slot, len, fileOff, salt, blockSize, mixLen);
    return fetchVerifyDiag();
}

void GpuCtx::blockVarRefillDev(int slot, uint64_t len, uint64_t refillLen, uint64_t seed,
                               bool fastAlgo)
{
    requireAligned("blockVarRefillDev", len, 16);
    uint64_t nVec2 = len / 16;
    if (!nVec2) return;
    uint64_t refillVec2 = refillLen / 16;
    uint64_t seq = ++impl->fillCallCounter;
    uint64_t sm = seed + seq;
    // host-side splitmix for the dedup-defeating constant
    uint64_t z = (sm += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    uint64_t fillConst = z ^ (z >> 31);

    if (fastAlgo) {
        dim3 grid = gridForBytes(nVec2);
        hipLaunchKernelGGL(ebBlockVarFastKernel, grid, dim3(256), 0, impl->stream,
                           (ulonglong2*)impl->devBufs[slot], nVec2, refillVec2,
                           seed + seq * 0x9E3779B9ULL, fillConst);
    } else {
        dim3 grid = gridForBytes(nVec2 / (FILL_U64S_PER_STEP / 2));
        hipLaunchKernelGGL(ebBlockVarKernel, grid, dim3(256), 0, impl->stream,
                           (ulonglong2*)impl->devBufs[slot], nVec2, refillVec2,
                           seed + seq * 0x9E3779B9ULL, fillConst);
    }
    HIP_CHECK(hipGetLastError());
}

// --dedupepct / --compresspct launch contract on top of requireAligned(len 16)
static void requireReduceGeometry(const char* what, uint64_t firstChunk, uint64_t chunkBytes,
                                  uint64_t randBytes, int dedupePct, uint64_t pool)
{
    if (chunkBytes < 16 || (chunkBytes & (chunkBytes - 1)))
        throw std::invalid_argument(std::string(what) + ": chunk size " +
                                    std::to_string(chunkBytes) +
                                    " is not a power of two >= 16");
    if (randBytes % 16 || randBytes > chunkBytes)
        throw std::invalid_argument(std::string(what) + ": random length " +
                                    std::to_string(randBytes) +
                                    " is not a multiple of 16 within the chunk size " +
                                    std::to_string(chunkBytes));
    if (dedupePct < 0 || dedupePct > 100)
        throw std::invalid_argument(std::string(what) + ": dedupe percentage " +
                                    std::to_string(dedupePct) + " is not in 0..100");
    if (!pool)
        throw std::invalid_argument(std::string(what) + ": pool size must be >= 1");
    // the kernel decides pool chunks from n % 100; that equals the pattern's
    // (n+1)*d/100 > n*d/100 as long as the 64-bit products do not wrap
    if (firstChunk >= (1ULL << 56))
        throw std::invalid_argument(std::string(what) + ": first chunk " +
                                    std::to_string(firstChunk) + " is not below 2^56");
}

void GpuCtx::fillReduceDev(int slot, uint64_t len, uint64_t firstChunk, uint64_t chunkBytes,
                           uint64_t randBytes, int dedupePct, uint64_t pool,
                           uint64_t uniqSeed, uint64_t poolSeed)
{
    requireAligned("fillReduceDev", len, 16);
    requireReduceGeometry("fillReduceDev", firstChunk, chunkBytes, randBytes, dedupePct, pool);
    if (len > impl->slotStride)
        throw std::invalid_argument("fillReduceDev: len " + std::to_string(len) +
                                    " exceeds the slot size");
    uint64_t nVec2 = len / 16;
    if (!nVec2) return;
    hipLaunchKernelGGL(ebFillReduceKernel, gridForBytes(nVec2), dim3(256), 0, impl->stream,
                       (ulonglong2*)impl->devBufs[slot], nVec2, firstChunk,
                       (uint32_t)(firstChunk % 100), (uint32_t)__builtin_ctzll(chunkBytes / 16),
                       randBytes / 16, (uint32_t)dedupePct, pool, uniqSeed, poolSeed);
    HIP_CHECK(hipGetLastError());
}

void GpuCtx::verifyReduceDevAsync(int slot, uint64_t len, uint64_t fileOff, uint64_t firstChunk,
                                  uint64_t chunkBytes, uint64_t randBytes, int dedupePct,
                                  uint64_t pool, uint64_t uniqSeed, uint64_t poolSeed)
{
    requireAligned("verifyReduceDev", len, 16, fileOff);
    requireReduceGeometry("verifyReduceDev", firstChunk, chunkBytes, randBytes, dedupePct, pool);
    if (len > impl->slotStride)
        throw std::invalid_argument("verifyReduceDev: len " + std::to_string(len) +
                                    " exceeds the slot size");
    uint64_t nVec2 = len / 16;
    if (!nVec2) return;
    hipLaunchKernelGGL(ebVerifyReduceKernel, gridForBytes(nVec2), dim3(256), 0, impl->stream,
                       (const ulonglong2*)impl->devBufs[slot], nVec2, fileOff, firstChunk,
                       (uint32_t)(firstChunk % 100), (uint32_t)__builtin_ctzll(chunkBytes / 16),
                       randBytes / 16, (uint32_t)dedupePct, pool, uniqSeed, poolSeed,
                       impl->verifyOutDev);
    HIP_CHECK(hipGetLastError());
    impl->verifyDirty = true;
}

GpuVerifyResult GpuCtx::verifyReduceDev(int slot, uint64_t len, uint64_t fileOff,
                                        uint64_t firstChunk, uint64_t chunkBytes,
                                        uint64_t randBytes, int dedupePct, uint64_t pool,
                                        uint64_t uniqSeed, uint64_t poolSeed)
{
    verifyReduceDevAsync(slot, len, fileOff, firstChunk, chunkBytes, randBytes, dedupePct, pool,
                         uniqSeed, poolSeed);
    return fetchVerifyResult();
}

// --- CRC-32 / CRC-32C in HBM ---

uint64_t gpuCrcTileBytes() { return CRC_TILE_BYTES; }
uint64_t gpuCrcWaveBytes() { return CRC_WAVE_BYTES; }

void GpuCtx::dataProfileAlloc()
{
    if (impl->dpDev) return;
    HIP_CHECK(hipMalloc(&impl->dpDev, DP_DEV_BYTES));
    HIP_CHECK(hipHostMalloc(&impl->dpHost, DP_DEV_BYTES, hipHostMallocDefault));
    HIP_CHECK(hipMemsetAsync(impl->dpDev, 0, DP_DEV_BYTES, impl->stream));
}

void GpuCtx::dataProfileReset()
{
    const bool fresh = !impl->dpDev;
    dataProfileAlloc();
    if (!fresh) HIP_CHECK(hipMemsetAsync(impl->dpDev, 0, DP_DEV_BYTES, impl->stream));
}

static dim3 gridForProfile(uint64_t nChunks, bool wgTeam)
{
    // one team per chunk until the grid fills the chip several times over;
    // every workgroup ends with up to 259 global atomics, so no more than that
    uint64_t blocks = wgTeam ? nChunks : (nChunks + 3) / 4;
    if (blocks > 2048) blocks = 2048;
    if (blocks == 0) blocks = 1;
    return dim3((uint32_t)blocks);
}

static void launchDataProfile(hipStream_t stream, const void* buf, uint64_t len,
                              uint64_t chunkBytes, char* acc)
{
    const uint32_t chunkShift = (uint32_t)__builtin_ctzll(chunkBytes);
    const uint64_t nChunks = (len + chunkBytes - 1) / chunkBytes;
    const bool wgTeam = chunkBytes >= DP_WG_CHUNK_BYTES;
    unsigned int* regs = (unsigned int*)acc;
    unsigned long long* hist = (unsigned long long*)(acc + DP_REGS_BYTES);
    unsigned long long* counters = hist + 256;
    if (wgTeam)
        hipLaunchKernelGGL(ebDataProfileKernel<true>, gridForProfile(nChunks, true), dim3(256),
                           0, stream, (const ulonglong2*)buf, len, chunkShift, regs, hist,
                           counters);
    else
        hipLaunchKernelGGL(ebDataProfileKernel<false>, gridForProfile(nChunks, false),
                           dim3(256), 0, stream, (const ulonglong2*)buf, len, chunkShift, regs,
                           hist, counters);
    HIP_CHECK(hipGetLastError());
}

void GpuCtx::dataProfileDevAsync(int slot, uint64_t len, uint64_t chunkBytes)
{
    if (!dataProfileChunkOk(chunkBytes))
        throw std::invalid_argument("dataProfileDev: chunk must be a power of two in 512..16M");
    if (slot < 0 || slot >= slots)
        throw std::invalid_argument("dataProfileDev: no such slot");
    // a cut last 16 B element is loaded whole: it must end inside the slot
    if (len > impl->slotStride)
        throw std::invalid_argument("dataProfileDev: len " + std::to_string(len) +
                                    " exceeds the slot size");
    dataProfileAlloc();
    if (!len) return;
    launchDataProfile(impl->stream, impl->devBufs[slot], len, chunkBytes, impl->dpDev);
}

void GpuCtx::dataProfileFetch(DataProfileAcc& acc)
{
    if (!impl->dpDev) return; // nothing was ever enqueued
    HIP_CHECK(hipMemcpyAsync(impl->dpHost, impl->dpDev, DP_DEV_BYTES, hipMemcpyDeviceToHost,
                             impl->stream));
    HIP_CHECK(hipStreamSynchronize(impl->stream));
    const unsigned int* regs = (const unsigned int*)impl->dpHost;
    const unsigned long long* hist = (const unsigned long long*)(impl->dpHost + DP_REGS_BYTES);
    const unsigned long long* counters = hist + 256;
    for (uint32_t i = 0; i < DP_HLL_M; i++)
        acc.regs[i] = (uint8_t)std::max<unsigned int>(acc.regs[i], regs[i]);
    for (int i = 0; i < 256; i++) acc.hist[i] += hist[i];
    acc.chunks += counters[0];
    acc.bytes += counters[1];
    acc.zeroChunks += counters[2];
}

void GpuCtx::crcDevAsync(int slot, uint64_t len, CrcAlgo algo, uint64_t partialBase)
{
    requireAligned("crcDevAsync", len, 16);
    if (len > impl->slotStride)
        throw std::invalid_argument("crcDevAsync: len " + std::to_string(len) +
                                    " exceeds the slot size");
    if (!len) return;
    const int a = (int)algo;
    const uint64_t tiles = (len + CRC_TILE_BYTES - 1) / CRC_TILE_BYTES;

    if (!impl->crcTabDev[a]) { // first use of this algorithm: build + upload tables
        std::vector<uint32_t> tab = crcBuildTileTables(algo, CRC_STEPS_PER_WAVE);
        HIP_CHECK(hipMalloc(&impl->crcTabDev[a], tab.size() * sizeof(uint32_t)));
        HIP_CHECK(hipMemcpy(impl->crcTabDev[a], tab.data(), tab.size() * sizeof(uint32_t),
                            hipMemcpyHostToDevice));
        impl->crcTileShift[a] = CrcShift(algo, CRC_TILE_BYTES);
    }

    if (partialBase + tiles > impl->crcPartCap) { // grow, keeping earlier partials
        uint64_t cap = std::max<uint64_t>(4096, impl->crcPartCap * 2);
        while (cap < partialBase + tiles) cap *= 2;
        uint32_t* dev = nullptr;
        uint32_t* host = nullptr;
        HIP_CHECK(hipMalloc(&dev, cap * sizeof(uint32_t)));
        HIP_CHECK(hipHostMalloc(&host, cap * sizeof(uint32_t), hipHostMallocDefault));
        if (impl->crcPartDev) {
            HIP_CHECK(hipStreamSynchronize(impl->stream)); // kernels still writing the old one
            HIP_CHECK(hipMemcpy(dev, impl->crcPartDev, impl->crcPartCap * sizeof(uint32_t),
                                hipMemcpyDeviceToDevice));
            (void)hipFree(impl->crcPartDev);
            (void)hipHostFree(impl->crcPartHost);
        }
        impl->crcPartDev = dev;
        impl->crcPartHost = host;
        impl->crcPartCap = cap;
    }

    dim3 grid = gridForBytes(tiles * 256); // one workgroup per tile, capped
    hipLaunchKernelGGL(ebCrcTilesKernel, grid, dim3(256), 0, impl->stream,
                       (const ulonglong2*)impl->devBufs[slot], len / 16,
                       (const uint32_t*)impl->crcTabDev[a], impl->crcPartDev + partialBase);
    HIP_CHECK(hipGetLastError());
    impl->crcPending.push_back({partialBase, len});
}

uint32_t GpuCtx::crcFetch(CrcAlgo algo, uint64_t totalLen, uint64_t tileCount)
{
    // the calls since the last fetch must tile [0, tileCount) in order and
    // add up to totalLen; each call's last tile may be short
    std::vector<Impl::CrcCall> calls;
    calls.swap(impl->crcPending);
    uint64_t tiles = 0, bytes = 0;
    for (const auto& c : calls) {
        if (c.base != tiles)
            throw std::invalid_argument("crcFetch: partials are not contiguous in call order");
        tiles += (c.len + CRC_TILE_BYTES - 1) / CRC_TILE_BYTES;
        bytes += c.len;
    }
    if (tiles != tileCount || bytes != totalLen)
        throw std::invalid_argument("crcFetch: " + std::to_string(tileCount) + " tiles / " +
                                    std::to_string(totalLen) + " bytes asked, " +
                                    std::to_string(tiles) + " / " + std::to_string(bytes) +
                                    " enqueued");
    if (!tileCount) return crcFinishRaw(algo, 0, 0);

    HIP_CHECK(hipMemcpyAsync(impl->crcPartHost, impl->crcPartDev, tileCount * sizeof(uint32_t),
                             hipMemcpyDeviceToHost, impl->stream));
    HIP_CHECK(hipStreamSynchronize(impl->stream));

    const CrcShift& tileShift = impl->crcTileShift[(int)algo];
    const uint32_t* part = impl->crcPartHost;
    uint32_t raw = 0;
    for (const auto& c : calls) {
        const uint64_t full = c.len / CRC_TILE_BYTES;
        for (uint64_t i = 0; i < full; i++) raw = tileShift.apply(raw) ^ *part++;
        if (c.len % CRC_TILE_BYTES) raw = crcCombine(algo, raw, *part++, c.len % CRC_TILE_BYTES);
    }
    return crcFinishRaw(algo, raw, totalLen);
}

uint32_t GpuCtx::crcDev(int slot, uint64_t len, CrcAlgo algo)
{
    impl->crcPending.clear();
    crcDevAsync(slot, len, algo, 0);
    return crcFetch(algo, len, (len + CRC_TILE_BYTES - 1) / CRC_TILE_BYTES);
}

// --- CRC-64/NVME in HBM: the same trio on state of its own ---

uint64_t gpuCrc64TileBytes() { return CRC64_TILE_BYTES; }
uint64_t gpuCrc64WaveBytes() { return CRC64_WAVE_BYTES; }

void GpuCtx::crc64DevAsync(int slot, uint64_t len, uint64_t partialBase)
{
    requireAligned("crc64DevAsync", len, 16);
    if (len > impl->slotStride)
        throw std::invalid_argument("crc64DevAsync: len " + std::to_string(len) +
                                    " exceeds the slot size");
    if (!len) return;
    const uint64_t tiles = (len + CRC64_TILE_BYTES - 1) / CRC64_TILE_BYTES;

    if (!impl->crc64TabDev) { // first use: build + upload the table image
        std::vector<uint64_t> tab = crc64BuildTileTables();
        HIP_CHECK(hipMalloc(&impl->crc64TabDev, tab.size() * sizeof(uint64_t)));
        HIP_CHECK(hipMemcpy(impl->crc64TabDev, tab.data(), tab.size() * sizeof(uint64_t),
                            hipMemcpyHostToDevice));
        impl->crc64TileShift = std::make_unique<Crc64Shift>(CRC64_TILE_BYTES);
    }

    if (partialBase + tiles > impl->crc64PartCap) { // grow, keeping earlier partials
        uint64_t cap = std::max<uint64_t>(4096, impl->crc64PartCap * 2);
        while (cap < partialBase + tiles) cap *= 2;
        uint64_t* dev = nullptr;
        uint64_t* host = nullptr;
        HIP_CHECK(hipMalloc(&dev, cap * sizeof(uint64_t)));
        HIP_CHECK(hipHostMalloc(&host, cap * sizeof(uint64_t), hipHostMallocDefault));
        if (impl->crc64PartDev) {
            HIP_CHECK(hipStreamSynchronize(impl->stream)); // kernels still writing the old one
            HIP_CHECK(hipMemcpy(dev, impl->crc64PartDev, impl->crc64PartCap * sizeof(uint64_t),
                                hipMemcpyDeviceToDevice));
            (void)hipFree(impl->crc64PartDev);
            (void)hipHostFree(impl->crc64PartHost);
        }
        impl->crc64PartDev = dev;
        impl->crc64PartHost = host;
        impl->crc64PartCap = cap;
    }

    dim3 grid = gridForBytes(tiles * 256); // one workgroup per tile, capped
    hipLaunchKernelGGL(ebCrc64TilesKernel, grid, dim3(256), 0, impl->stream,
                       (const ulonglong2*)impl->devBufs[slot], len / 16,
                       (const uint64_t*)impl->crc64TabDev, impl->crc64PartDev + partialBase);
    HIP_CHECK(hipGetLastError());
    impl->crc64Pending.push_back({partialBase, len});
}

uint64_t GpuCtx::crc64Fetch(uint64_t totalLen, uint64_t tileCount)
{
    // the calls since the last fetch must tile [0, tileCount) in order and
    // add up to totalLen; each call's last tile may be short
    std::vector<Impl::CrcCall> calls;
    calls.swap(impl->crc64Pending);
    uint64_t tiles = 0, bytes = 0;
    for (const auto& c : calls) {
        if (c.base != tiles)
            throw std::invalid_argument("crc64Fetch: partials are not contiguous in call order");
        tiles += (c.len + CRC64_TILE_BYTES - 1) / CRC64_TILE_BYTES;
        bytes += c.len;
    }
    if (tiles != tileCount || bytes != totalLen)
        throw std::invalid_argument("crc64Fetch: " + std::to_string(tileCount) + " tiles / " +
                                    std::to_string(totalLen) + " bytes asked, " +
                                    std::to_string(tiles) + " / " + std::to_string(bytes) +
                                    " enqueued");
    if (!tileCount) return crc64FinishRaw(0, 0);

    HIP_CHECK(hipMemcpyAsync(impl->crc64PartHost, impl->crc64PartDev,
                             tileCount * sizeof(uint64_t), hipMemcpyDeviceToHost, impl->stream));
    HIP_CHECK(hipStreamSynchronize(impl->stream));

    const uint64_t* part = impl->crc64PartHost;
    uint64_t raw = 0;
    for (const auto& c : calls) {
        raw = crc64FoldTiles(*impl->crc64TileShift, raw, part, c.len);
        part += (c.len + CRC64_TILE_BYTES - 1) / CRC64_TILE_BYTES;
    }
    return crc64FinishRaw(raw, totalLen);
}

uint64_t GpuCtx::crc64Dev(int slot, uint64_t len)
{
    impl->crc64Pending.clear();
    crc64DevAsync(slot, len, 0);
    return crc64Fetch(len, (len + CRC64_TILE_BYTES - 1) / CRC64_TILE_BYTES);
}

double gpuVerifyBenchGBs(uint64_t len, int iters, bool lds, int dev)
{
    HIP_CHECK(hipSetDevice(dev));
    const uint64_t n64 = len / 8;
    ulonglong2* buf = nullptr;
    unsigned long long* out = nullptr;
    HIP_CHECK(hipMalloc(&buf, len));
    HIP_CHECK(hipMalloc(&out, 2 * sizeof(unsigned long long)));
    HIP_CHECK(hipMemset(out, 0, 2 * sizeof(unsigned long long)));

    hipStream_t s;
    HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    dim3 grid = gridForBytes(n64 / 2);

    hipLaunchKernelGGL(ebFillChecksumKernel, gridForBytes(len / 8), dim3(256), 0, s,
                       (uint64_t*)buf, len / 8, 0, 7);

    auto launch = [&] {
        if (lds)
            hipLaunchKernelGGL(ebVerifyChecksumLdsKernel, grid, dim3(256), 0, s,
                               buf, n64, 0, 7, out);
        else
            hipLaunchKernelGGL(ebVerifyChecksumKernel, grid, dim3(256), 0, s,
                               buf, n64, 0, 7, out);
    };

    launch(); // warmup
    launch();
    HIP_CHECK(hipStreamSynchronize(s));

    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    HIP_CHECK(hipEventRecord(e0, s));
    for (int i = 0; i < iters; i++) launch();
    HIP_CHECK(hipEventRecord(e1, s));
    HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));

    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipStreamDestroy(s);
    (void)hipFree(buf);
    (void)hipFree(out);

    return (double)len * iters / (ms / 1000.0) / 1e9;
}

double gpuVerifyDiagBenchGBs(uint64_t len, int iters, int dev)
{
    requireAligned("gpuVerifyDiagBenchGBs", len, 16);
    if (!len || iters < 1) throw std::invalid_argument("gpuVerifyDiagBenchGBs: nothing to run");
    HIP_CHECK(hipSetDevice(dev));
    const uint64_t n64 = len / 8;
    ulonglong2* buf = nullptr;
    unsigned long long* out = nullptr;
    unsigned long long init[GpuVerifyDiag::NUM_FIELDS];
    diagInitWords(init);
    HIP_CHECK(hipMalloc(&buf, len));
    HIP_CHECK(hipMalloc(&out, sizeof(init)));
    HIP_CHECK(hipMemcpy(out, init, sizeof(init), hipMemcpyHostToDevice));

    hipStream_t s;
    HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    dim3 grid = gridForBytes(n64 / 2);

    // clean data, as in gpuVerifyBenchGBs: no atomics in the timed loop
    hipLaunchKernelGGL(ebFillChecksumKernel, gridForBytes(n64), dim3(256), 0, s,
                       (uint64_t*)buf, n64, 0, 7);
    auto launch = [&] {
        hipLaunchKernelGGL(ebVerifyDiagKernel, grid, dim3(256), 0, s, buf, n64, 0, 7, out);
    };

    launch(); // warmup
    launch();
    HIP_CHECK(hipStreamSynchronize(s));

    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    HIP_CHECK(hipEventRecord(e0, s));
    for (int i = 0; i < iters; i++) launch();
    HIP_CHECK(hipEventRecord(e1, s));
    HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));

    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipStreamDestroy(s);
    (void)hipFree(buf);
    (void)hipFree(out);

    return (double)len * iters / (ms / 1000.0) / 1e9;
}

double gpuMixBenchGBs(uint64_t len, int iters, int dev, uint64_t blockSize, uint64_t mixLen,
                      bool fill, bool plainFill)
{
    requireAligned("gpuMixBenchGBs", len, 16);
    requireMixGeometry("gpuMixBenchGBs", len, blockSize, mixLen);
    if (!len || iters < 1) throw std::invalid_argument("gpuMixBenchGBs: nothing to run");
    HIP_CHECK(hipSetDevice(dev));
    const uint64_t n64 = len / 8;
    ulonglong2* buf = nullptr;
    unsigned long long* out = nullptr;
    HIP_CHECK(hipMalloc(&buf, len));
    HIP_CHECK(hipMalloc(&out, 2 * sizeof(unsigned long long)));
    HIP_CHECK(hipMemset(out, 0, 2 * sizeof(unsigned long long)));

    hipStream_t s;
    HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));

    auto launchFill = [&] {
        hipLaunchKernelGGL(ebFillChecksumMixKernel, gridForBytes(n64), dim3(256), 0, s,
                           (uint64_t*)buf, n64, 0, 7, 0, blockSize, mixLen);
    };
    auto launch = [&] {
        if (fill && plainFill)
            hipLaunchKernelGGL(ebFillChecksumKernel, gridForBytes(n64), dim3(256), 0, s,
                               (uint64_t*)buf, n64, 0, 7);
        else if (fill)
            launchFill();
        else
            hipLaunchKernelGGL(ebVerifyChecksumMixKernel, gridForBytes(n64 / 2), dim3(256), 0,
                               s, buf, n64, 0, 7, 0, blockSize, mixLen, out);
    };

    launchFill(); // the data the verify reads (clean: no atomics in the timed loop)
    launch();     // warmup
    launch();
    HIP_CHECK(hipStreamSynchronize(s));

    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    HIP_CHECK(hipEventRecord(e0, s));
    for (int i = 0; i < iters; i++) launch();
    HIP_CHECK(hipEventRecord(e1, s));
    HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));

    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipStreamDestroy(s);
    (void)hipFree(buf);
    (void)hipFree(out);

    return (double)len * iters / (ms / 1000.0) / 1e9;
}

double gpuReduceVerifyBenchGBs(uint64_t len, int iters, int dev, uint64_t chunkBytes,
                               uint64_t randBytes, int dedupePct)
{
    requireAligned("gpuReduceVerifyBenchGBs", len, 16);
    requireReduceGeometry("gpuReduceVerifyBenchGBs", 0, chunkBytes, randBytes, dedupePct, 256);
    if (!len || iters < 1)
        throw std::invalid_argument("gpuReduceVerifyBenchGBs: nothing to run");
    HIP_CHECK(hipSetDevice(dev));
    const uint64_t nVec2 = len / 16;
    ulonglong2* buf = nullptr;
    unsigned long long* out = nullptr;
    HIP_CHECK(hipMalloc(&buf, len));
    HIP_CHECK(hipMalloc(&out, 2 * sizeof(unsigned long long)));
    HIP_CHECK(hipMemset(out, 0, 2 * sizeof(unsigned long long)));

    hipStream_t s;
    HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    const uint32_t vecShift = (uint32_t)__builtin_ctzll(chunkBytes / 16);

    // the data the verify reads (clean: no atomics in the timed loop)
    hipLaunchKernelGGL(ebFillReduceKernel, gridForBytes(nVec2), dim3(256), 0, s, buf, nVec2,
                       (uint64_t)0, 0u, vecShift, randBytes / 16, (uint32_t)dedupePct,
                       (uint64_t)256, (uint64_t)42, (uint64_t)43);
    auto launch = [&] {
        hipLaunchKernelGGL(ebVerifyReduceKernel, gridForBytes(nVec2), dim3(256), 0, s, buf,
                           nVec2, (uint64_t)0, (uint64_t)0, 0u, vecShift, randBytes / 16,
                           (uint32_t)dedupePct, (uint64_t)256, (uint64_t)42, (uint64_t)43, out);
    };

    launch(); // warmup
    launch();
    HIP_CHECK(hipStreamSynchronize(s));

    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    HIP_CHECK(hipEventRecord(e0, s));
    for (int i = 0; i < iters; i++) launch();
    HIP_CHECK(hipEventRecord(e1, s));
    HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));

    unsigned long long bad = 0;
    HIP_CHECK(hipMemcpy(&bad, out, sizeof(bad), hipMemcpyDeviceToHost));

    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipStreamDestroy(s);
    (void)hipFree(buf);
    (void)hipFree(out);

    if (bad) throw std::runtime_error("gpuReduceVerifyBenchGBs: the clean buffer did not verify");
    return (double)len * iters / (ms / 1000.0) / 1e9;
}

double gpuDataProfileBenchGBs(uint64_t len, int iters, int dev, uint64_t chunkBytes, int kind)
{
    requireAligned("gpuDataProfileBenchGBs", len, 16);
    if (!dataProfileChunkOk(chunkBytes))
        throw std::invalid_argument(
            "gpuDataProfileBenchGBs: chunk must be a power of two in 512..16M");
    if (kind < 0 || kind > 2) throw std::invalid_argument("gpuDataProfileBenchGBs: bad kind");
    if (!len || iters < 1) throw std::invalid_argument("gpuDataProfileBenchGBs: nothing to run");
    HIP_CHECK(hipSetDevice(dev));
    const uint64_t nVec2 = len / 16;
    ulonglong2* buf = nullptr;
    char* acc = nullptr;
    HIP_CHECK(hipMalloc(&buf, len));
    HIP_CHECK(hipMalloc(&acc, DP_DEV_BYTES));
    HIP_CHECK(hipMemset(acc, 0, DP_DEV_BYTES));

    hipStream_t s;
    HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));

    // the data the kernel reads: 4 KiB pattern chunks, all unique, of which
    // everything (kind 0), the first half (1) or nothing (2) is random
    hipLaunchKernelGGL(ebFillReduceKernel, gridForBytes(nVec2), dim3(256), 0, s, buf, nVec2,
                       (uint64_t)0, 0u, 8u, (uint64_t)(kind == 0 ? 256 : kind == 1 ? 128 : 0),
                       0u, (uint64_t)256, (uint64_t)42, (uint64_t)43);
    auto launch = [&] { launchDataProfile(s, buf, len, chunkBytes, acc); };

    launch(); // warmup
    launch();
    HIP_CHECK(hipStreamSynchronize(s));

    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    HIP_CHECK(hipEventRecord(e0, s));
    for (int i = 0; i < iters; i++) launch();
    HIP_CHECK(hipEventRecord(e1, s));
    HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));

    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipStreamDestroy(s);
    (void)hipFree(buf);
    (void)hipFree(acc);

    return (double)len * iters / (ms / 1000.0) / 1e9;
}

} // namespace eb
