// Reflected CRC-32 (zlib polynomial) and CRC-32C (Castagnoli) on the host:
// incremental slice-by-8 update, zlib-style combine, and fixed-distance
// shift operators for folding many equal-length partial CRCs.
//
// Both variants use init 0xFFFFFFFF and xorout 0xFFFFFFFF. Values that cross
// this interface are FINISHED CRCs unless a name says "raw": a raw CRC has
// init 0 and no xorout, i.e. raw(D) = D(x) * x^32 mod P, which is linear in
// D and ignores leading zero bytes. That is what the device kernel produces
// per tile (gpu_kernels.hip) and what CrcShift folds.
//
// Polynomials are kept in the reflected representation throughout: bit 31
// of a word is the coefficient of x^0, bit 0 that of x^31.
//
// HIP-free: included by the engine, the native S3 plane and the HIP unit.

#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace eb {

enum class CrcAlgo { CRC32 = 0, CRC32C = 1 };

inline uint32_t crcPoly(CrcAlgo a)
{
    return a == CrcAlgo::CRC32 ? 0xEDB88320u : 0x82F63B78u;
}

inline CrcAlgo crcAlgoFromName(const std::string& name)
{
    if (name == "CRC32") return CrcAlgo::CRC32;
    if (name == "CRC32C") return CrcAlgo::CRC32C;
    throw std::invalid_argument("unknown CRC algorithm '" + name +
                                "' (CRC32 or CRC32C)");
}

// Byte tables: slice[s][b] = raw CRC of byte b followed by s zero bytes.
// Slices 0..7 serve the host's slice-by-8 loop, 0..15 the device kernel's
// 16 B/lane step.
constexpr int CRC_SLICES = 16;

struct CrcSliceTable {
    uint32_t slice[CRC_SLICES][256];

    explicit CrcSliceTable(uint32_t poly)
    {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1) ? (poly ^ (c >> 1)) : (c >> 1);
            slice[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; i++)
            for (int s = 1; s < CRC_SLICES; s++)
                slice[s][i] = slice[0][slice[s - 1][i] & 0xFF] ^ (slice[s - 1][i] >> 8);
    }
};

inline const CrcSliceTable& crcSliceTable(CrcAlgo a)
{
    static const CrcSliceTable t32(crcPoly(CrcAlgo::CRC32));
    static const CrcSliceTable t32c(crcPoly(CrcAlgo::CRC32C));
    return a == CrcAlgo::CRC32 ? t32 : t32c;
}

// CRC of (what `crc` already covers) followed by p[0..n). Start with crc = 0.
inline uint32_t crcUpdate(CrcAlgo algo, uint32_t crc, const void* data, size_t n)
{
    const uint32_t(*t)[256] = crcSliceTable(algo).slice;
    const unsigned char* p = (const unsigned char*)data;
    uint32_t c = ~crc;
    while (n >= 8) {
        uint64_t w;
        memcpy(&w, p, 8);
        w ^= c;
        c = t[7][w & 0xFF] ^ t[6][(w >> 8) & 0xFF] ^ t[5][(w >> 16) & 0xFF] ^
            t[4][(w >> 24) & 0xFF] ^ t[3][(w >> 32) & 0xFF] ^ t[2][(w >> 40) & 0xFF] ^
            t[1][(w >> 48) & 0xFF] ^ t[0][(w >> 56) & 0xFF];
        p += 8;
        n -= 8;
    }
    while (n--) c = t[0][(c ^ *p++) & 0xFF] ^ (c >> 8);
    return ~c;
}

// a(x) * b(x) mod P
inline uint32_t crcMulMod(uint32_t poly, uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1) ? (b >> 1) ^ poly : b >> 1;
    }
    return p;
}

// x^(8*len) mod P: what appending len bytes multiplies a CRC register by.
// Square-and-multiply over the bits of len; the squares x^(2^k) are computed
// for every k up to 66 rather than taken mod 32, because the CRC-32C
// polynomial has a factor of degree 31 and x^(2^32) != x there.
inline uint32_t crcShiftPoly(CrcAlgo algo, uint64_t len)
{
    struct Squares {
        uint32_t x2n[67]; // x^(2^k)
        explicit Squares(uint32_t poly)
        {
            uint32_t p = 0x40000000u; // x^1
            x2n[0] = p;
            for (int k = 1; k < 67; k++) x2n[k] = p = crcMulMod(poly, p, p);
        }
    };
    static const Squares s32(crcPoly(CrcAlgo::CRC32));
    static const Squares s32c(crcPoly(CrcAlgo::CRC32C));
    const Squares& s = algo == CrcAlgo::CRC32 ? s32 : s32c;
    const uint32_t poly = crcPoly(algo);

    uint32_t p = 0x80000000u; // x^0
    for (int k = 3; len; len >>= 1, k++) // bit i of len contributes x^(2^(i+3))
        if (len & 1) p = crcMulMod(poly, s.x2n[k], p);
    return p;
}

// Combine with a precomputed xp = crcShiftPoly(algo, lenB).
inline uint32_t crcCombineXp(CrcAlgo algo, uint32_t xp, uint32_t crcA, uint32_t crcB)
{
    return crcMulMod(crcPoly(algo), xp, crcA) ^ crcB;
}

// CRC of A||B from the finished CRCs of A and B (zlib crc32_combine
// semantics, either polynomial). The init/xorout terms of the two inputs
// cancel, so the same formula serves raw CRCs.
inline uint32_t crcCombine(CrcAlgo algo, uint32_t crcA, uint32_t crcB, uint64_t lenB)
{
    if (!lenB) return crcA;
    return crcCombineXp(algo, crcShiftPoly(algo, lenB), crcA, crcB);
}

// Finished CRC of a totalLen-byte message from its raw CRC: adds what the
// 0xFFFFFFFF init turns into after totalLen bytes, and the xorout.
inline uint32_t crcFinishRaw(CrcAlgo algo, uint32_t raw, uint64_t totalLen)
{
    return raw ^ crcMulMod(crcPoly(algo), crcShiftPoly(algo, totalLen), 0xFFFFFFFFu) ^
           0xFFFFFFFFu;
}

// Fixed-distance operator: v -> v * x^(8*len) mod P as four byte-table
// lookups. Built once per distance (1024 multiplications), then O(1) per
// use — folding N equal-length partials costs N applications, not N
// log-time exponentiations. The same tables are what the device kernel
// keeps in LDS for its fixed strides.
struct CrcShift {
    uint32_t t[4][256];

    CrcShift() { memset(t, 0, sizeof(t)); }

    CrcShift(CrcAlgo algo, uint64_t len)
    {
        const uint32_t poly = crcPoly(algo);
        const uint32_t xp = crcShiftPoly(algo, len);
        for (int k = 0; k < 4; k++)
            for (uint32_t b = 0; b < 256; b++) t[k][b] = crcMulMod(poly, xp, b << (8 * k));
    }

    uint32_t apply(uint32_t v) const
    {
        return t[0][v & 0xFF] ^ t[1][(v >> 8) & 0xFF] ^ t[2][(v >> 16) & 0xFF] ^ t[3][v >> 24];
    }
};

// ---------------------------------------------------------------------------
// Table image for the device tile kernel (ebCrcTilesKernel)
// ---------------------------------------------------------------------------
//
// A tile is `waves` consecutive wave regions; a wave region is `steps` rows
// of 64 lanes x 16 B. The kernel needs, as [256]-word byte tables:
//   words [0, 16*256)            raw CRC of one 16 B element: table k serves
//                                byte k of the element (= slice[15 - k])
//   then 4 tables                shift by one row (64 * 16 B)
//   then 6 x 4 tables            shift by 16 B << i, i = 0..5 (lane tree)
//   then 4 tables                shift by one wave region
// The layout is fixed here so a host program can check it without a GPU.
constexpr int CRC_LANE_BYTES = 16;
constexpr int CRC_WAVE_LANES = 64;
constexpr int CRC_ROW_BYTES = CRC_LANE_BYTES * CRC_WAVE_LANES; // 1 KiB
constexpr int CRC_TAB_ELEM = 0;
constexpr int CRC_TAB_ROW = 16;
constexpr int CRC_TAB_LANE = 20;
constexpr int CRC_TAB_WAVE = 44;
constexpr int CRC_TAB_COUNT = 48; // x 256 words = 48 KiB

inline std::vector<uint32_t> crcBuildTileTables(CrcAlgo algo, int steps)
{
    std::vector<uint32_t> out((size_t)CRC_TAB_COUNT * 256);
    const CrcSliceTable& st = crcSliceTable(algo);
    for (int k = 0; k < 16; k++)
        memcpy(&out[(size_t)(CRC_TAB_ELEM + k) * 256], st.slice[15 - k], 1024);
    auto put = [&](int first, uint64_t len) {
        CrcShift sh(algo, len);
        memcpy(&out[(size_t)first * 256], sh.t, sizeof(sh.t));
    };
    put(CRC_TAB_ROW, CRC_ROW_BYTES);
    for (int i = 0; i < 6; i++) put(CRC_TAB_LANE + 4 * i, (uint64_t)CRC_LANE_BYTES << i);
    put(CRC_TAB_WAVE, (uint64_t)CRC_ROW_BYTES * steps);
    return out;
}

} // namespace eb
