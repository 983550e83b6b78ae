// --dataprofile: dedupe/entropy profile of the data a READ phase moves.
//
// The definitions here are the contract that the gfx950 kernel
// (ebDataProfileKernel, gpu_kernels.hip), the CPU twin below and the test
// model (tests/data_profile_model.py) agree on bit for bit; docs/usage.md
// ("Data profile") states them for users.
//
//   chunks       a block of len bytes is cut by position in the block: chunk k
//                is bytes [k*C, min((k+1)*C, len)); a short last chunk counts
//   words        a chunk of n bytes is ceil(n/8) little-endian u64 words, the
//                last one zero-padded
//   fingerprint  S = sum_i mix(w_i + GOLD*(i+1)) (wrapping), fp = mix(S ^ n),
//                mix = the splitmix64 step, GOLD its increment. The sum
//                commutes, so any reduction order gives the same fp. Not a
//                cryptographic hash: adversarial collisions are out of scope.
//   sketch       HyperLogLog, p = 14: idx = fp >> 50, rest = fp << 14,
//                rho = rest ? clz64(rest) + 1 : 51, reg[idx] = max(reg[idx], rho)
//   counters     chunks, bytes, zeroChunks (every real byte zero) and a
//                byte-value histogram over real bytes only (never padding)
//
// Sketches merge by max, everything else by sum, so the profile of a data set
// does not depend on how its blocks were spread over workers, services or
// ranks. The derived figures (estimate, entropy, suggestion) are computed in
// Python only (elbencho_amd/dataprofile.py).

#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define EB_DP_HD __host__ __device__
#else
#define EB_DP_HD
#endif

namespace eb {

constexpr uint64_t DP_GOLD = 0x9E3779B97F4A7C15ULL;
constexpr int DP_HLL_P = 14;
constexpr uint32_t DP_HLL_M = 1u << DP_HLL_P;      // registers
constexpr uint32_t DP_RHO_MAX = 64 - DP_HLL_P + 1; // 51: rest == 0
constexpr uint64_t DP_CHUNK_MIN = 512;             // the range of --dedupechunk
constexpr uint64_t DP_CHUNK_MAX = 16ULL << 20;

EB_DP_HD inline uint64_t dpMix64(uint64_t x)
{
    uint64_t z = x + DP_GOLD;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// what word w at index i of its chunk adds to S
EB_DP_HD inline uint64_t dpWordTerm(uint64_t w, uint64_t i)
{
    return dpMix64(w + DP_GOLD * (i + 1));
}

// fingerprint of a chunk of n bytes whose word terms sum to S
EB_DP_HD inline uint64_t dpFingerprint(uint64_t S, uint64_t n) { return dpMix64(S ^ n); }

EB_DP_HD inline uint32_t dpRegIndex(uint64_t fp) { return (uint32_t)(fp >> (64 - DP_HLL_P)); }

EB_DP_HD inline uint32_t dpRho(uint64_t fp)
{
    const uint64_t rest = fp << DP_HLL_P;
    return rest ? (uint32_t)__builtin_clzll(rest) + 1 : DP_RHO_MAX;
}

inline bool dataProfileChunkOk(uint64_t chunk)
{
    return chunk >= DP_CHUNK_MIN && chunk <= DP_CHUNK_MAX && !(chunk & (chunk - 1));
}

// Host accumulator: what a worker, a service or a run has seen so far.
struct DataProfileAcc {
    uint64_t chunks = 0;
    uint64_t bytes = 0;
    uint64_t zeroChunks = 0;
    uint64_t hist[256] = {};
    uint8_t regs[DP_HLL_M] = {};

    void merge(const DataProfileAcc& o)
    {
        chunks += o.chunks;
        bytes += o.bytes;
        zeroChunks += o.zeroChunks;
        for (int i = 0; i < 256; i++) hist[i] += o.hist[i];
        for (uint32_t i = 0; i < DP_HLL_M; i++) regs[i] = std::max(regs[i], o.regs[i]);
    }
};

// CPU twin of ebDataProfileKernel: adds the profile of buf[0, len) cut into
// chunks of `chunk` bytes (dataProfileChunkOk) into acc. Any len, any alignment.
inline void dataProfileCPU(const char* buf, uint64_t len, uint64_t chunk, DataProfileAcc& acc)
{
    const unsigned char* p = (const unsigned char*)buf;
    for (uint64_t pos = 0; pos < len; pos += chunk) {
        const uint64_t n = std::min(chunk, len - pos);
        uint64_t S = 0, any = 0;
        for (uint64_t o = 0; o < n; o += 8) {
            uint64_t w = 0;
            std::memcpy(&w, p + pos + o, (size_t)std::min<uint64_t>(8, n - o));
            S += dpWordTerm(w, o / 8);
            any |= w;
        }
        for (uint64_t o = 0; o < n; o++) acc.hist[p[pos + o]]++;
        const uint64_t fp = dpFingerprint(S, n);
        const uint32_t idx = dpRegIndex(fp);
        acc.regs[idx] = (uint8_t)std::max<uint32_t>(acc.regs[idx], dpRho(fp));
        acc.chunks++;
        acc.bytes += n;
        if (!any) acc.zeroChunks++;
    }
}

} // namespace eb
