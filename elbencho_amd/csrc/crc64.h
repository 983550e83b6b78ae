// Reflected CRC-64/NVME on the host: incremental slice-by-8 update,
// zlib-style combine, fixed-distance shift operators, and the table image
// and a plain-C++ emulation of the device tile kernel (ebCrc64TilesKernel).
// The 64-bit sibling of crc.h; S3 carries this checksum as
// x-amz-checksum-crc64nvme.
//
// Width 64, polynomial 0xAD93D23594C93659, reflected in and out, init and
// xorout all ones. Values that cross this interface are FINISHED CRCs unless
// a name says "raw": a raw CRC has init 0 and no xorout, i.e.
// raw(D) = D(x) * x^64 mod P, which is linear in D and ignores leading zero
// bytes. That is what the device kernel produces per tile and what
// Crc64Shift folds.
//
// The polynomial is kept in the reflected representation throughout: bit 63
// of a word is the coefficient of x^0, bit 0 that of x^63.
//
// HIP-free: included by the native S3 plane, the bindings and the HIP unit.

#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace eb {

constexpr uint64_t CRC64_NVME_POLY = 0x9A6C9329AC4BC9B5ull; // reflected 0xAD93D23594C93659
constexpr const char* CRC64_NVME_NAME = "CRC64NVME";

// Byte tables: slice[s][b] = raw CRC of byte b followed by s zero bytes.
// Slices 0..7 serve the host's slice-by-8 loop, 0..15 the device kernel's
// 16 B/lane step.
constexpr int CRC64_SLICES = 16;

struct Crc64SliceTable {
    uint64_t slice[CRC64_SLICES][256];

    Crc64SliceTable()
    {
        for (uint64_t i = 0; i < 256; i++) {
            uint64_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1) ? (CRC64_NVME_POLY ^ (c >> 1)) : (c >> 1);
            slice[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; i++)
            for (int s = 1; s < CRC64_SLICES; s++)
                slice[s][i] = slice[0][slice[s - 1][i] & 0xFF] ^ (slice[s - 1][i] >> 8);
    }
};

inline const Crc64SliceTable& crc64SliceTable()
{
    static const Crc64SliceTable t;
    return t;
}

// CRC of (what `crc` already covers) followed by p[0..n). Start with crc = 0.
inline uint64_t crc64Update(uint64_t crc, const void* data, size_t n)
{
    const uint64_t(*t)[256] = crc64SliceTable().slice;
    const unsigned char* p = (const unsigned char*)data;
    uint64_t c = ~crc;
    while (n >= 8) {
        uint64_t w;
        memcpy(&w, p, 8);
        w ^= c;
        c = t[7][w & 0xFF] ^ t[6][(w >> 8) & 0xFF] ^ t[5][(w >> 16) & 0xFF] ^
            t[4][(w >> 24) & 0xFF] ^ t[3][(w >> 32) & 0xFF] ^ t[2][(w >> 40) & 0xFF] ^
            t[1][(w >> 48) & 0xFF] ^ t[0][w >> 56];
        p += 8;
        n -= 8;
    }
    while (n--) c = t[0][(c ^ *p++) & 0xFF] ^ (c >> 8);
    return ~c;
}

// a(x) * b(x) mod P
inline uint64_t crc64MulMod(uint64_t a, uint64_t b)
{
    uint64_t p = 0;
    for (uint64_t m = 1ull << 63; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1) ? (b >> 1) ^ CRC64_NVME_POLY : b >> 1;
    }
    return p;
}

// x^(8*len) mod P: what appending len bytes multiplies a CRC register by.
// Square-and-multiply over the bits of len; the squares x^(2^k) are computed
// outright for every k up to 66 (a 64-bit length plus the 3 bits of the
// factor 8) — no period of x mod P is assumed.
inline uint64_t crc64ShiftPoly(uint64_t len)
{
    struct Squares {
        uint64_t x2n[67]; // x^(2^k)
        Squares()
        {
            uint64_t p = 1ull << 62; // x^1
            x2n[0] = p;
            for (int k = 1; k < 67; k++) x2n[k] = p = crc64MulMod(p, p);
        }
    };
    static const Squares s;

    uint64_t p = 1ull << 63; // x^0
    for (int k = 3; len; len >>= 1, k++) // bit i of len contributes x^(2^(i+3))
        if (len & 1) p = crc64MulMod(s.x2n[k], p);
    return p;
}

// Combine with a precomputed xp = crc64ShiftPoly(lenB).
inline uint64_t crc64CombineXp(uint64_t xp, uint64_t crcA, uint64_t crcB)
{
    return crc64MulMod(xp, crcA) ^ crcB;
}

// CRC of A||B from the finished CRCs of A and B. The init/xorout terms of
// the two inputs cancel, so the same formula serves raw CRCs.
inline uint64_t crc64Combine(uint64_t crcA, uint64_t crcB, uint64_t lenB)
{
    if (!lenB) return crcA;
    return crc64CombineXp(crc64ShiftPoly(lenB), crcA, crcB);
}

// Finished CRC of a totalLen-byte message from its raw CRC: adds what the
// all-ones init turns into after totalLen bytes, and the xorout.
inline uint64_t crc64FinishRaw(uint64_t raw, uint64_t totalLen)
{
    return raw ^ crc64MulMod(crc64ShiftPoly(totalLen), ~0ull) ^ ~0ull;
}

// Fixed-distance operator: v -> v * x^(8*len) mod P as eight byte-table
// lookups. Built once per distance (2048 multiplications), then O(1) per
// use. The device kernel keeps one of these (the row shift) in LDS.
struct Crc64Shift {
    uint64_t t[8][256];

    Crc64Shift() { memset(t, 0, sizeof(t)); }

    explicit Crc64Shift(uint64_t len)
    {
        const uint64_t xp = crc64ShiftPoly(len);
        for (int k = 0; k < 8; k++)
            for (uint64_t b = 0; b < 256; b++) t[k][b] = crc64MulMod(xp, b << (8 * k));
    }

    uint64_t apply(uint64_t v) const
    {
        return t[0][v & 0xFF] ^ t[1][(v >> 8) & 0xFF] ^ t[2][(v >> 16) & 0xFF] ^
               t[3][(v >> 24) & 0xFF] ^ t[4][(v >> 32) & 0xFF] ^ t[5][(v >> 40) & 0xFF] ^
               t[6][(v >> 48) & 0xFF] ^ t[7][v >> 56];
    }
};

// ---------------------------------------------------------------------------
// Geometry and table image of the device tile kernel (ebCrc64TilesKernel)
// ---------------------------------------------------------------------------
//
// A tile is CRC64_WAVES_PER_TILE consecutive wave regions; a wave region is
// CRC64_STEPS_PER_WAVE rows of 64 lanes x 16 B. Thread (wave, lane) takes the
// lane-th 16 B element of each row of its wave region, Horner-joins them with
// the row shift, then multiplies the result ONCE by its own weight,
// x^(8 * bytes that follow its last-row element inside the tile). Raw CRCs
// are linear, so the tile's raw CRC is the XOR of the 256 weighted values.
//
// The image, as [256]-word tables of uint64_t:
//   tables [0, 16)     raw CRC of one 16 B element: table k serves byte k of
//                      the element (= slice[15 - k])
//   tables [16, 24)    shift by one row (64 * 16 B), eight byte tables
//   table  24          the 256 thread weights, index wave * 64 + lane
// Tables [0, 24) (48 KiB) go to LDS; a thread reads its weight straight into
// a register. The layout and the geometry are fixed here, and the kernel
// takes both from this header, so a host program can check them without a
// GPU (crc64TilesHost below).
constexpr int CRC64_LANE_BYTES = 16;
constexpr int CRC64_WAVE_LANES = 64;
constexpr int CRC64_ROW_BYTES = CRC64_LANE_BYTES * CRC64_WAVE_LANES; // 1 KiB
constexpr int CRC64_STEPS_PER_WAVE = 8; // rows per wave and tile
constexpr int CRC64_WAVES_PER_TILE = 4; // = 256 threads / 64
constexpr uint64_t CRC64_WAVE_BYTES = (uint64_t)CRC64_ROW_BYTES * CRC64_STEPS_PER_WAVE; // 8 KiB
constexpr uint64_t CRC64_TILE_BYTES = CRC64_WAVE_BYTES * CRC64_WAVES_PER_TILE;          // 32 KiB
constexpr int CRC64_TAB_ELEM = 0;
constexpr int CRC64_TAB_ROW = 16;
constexpr int CRC64_TAB_WEIGHT = 24;
constexpr int CRC64_TAB_LDS = 24;   // tables kept in LDS: x 256 x 8 B = 48 KiB
constexpr int CRC64_TAB_COUNT = 25; // x 256 x 8 B = 50 KiB

// Bytes of the tile that follow thread (wave, lane)'s last-row element.
constexpr uint64_t crc64ThreadTailBytes(int wave, int lane)
{
    return CRC64_TILE_BYTES -
           ((uint64_t)(wave * CRC64_STEPS_PER_WAVE + CRC64_STEPS_PER_WAVE - 1) *
                CRC64_WAVE_LANES + lane + 1) * CRC64_LANE_BYTES;
}

inline std::vector<uint64_t> crc64BuildTileTables()
{
    std::vector<uint64_t> out((size_t)CRC64_TAB_COUNT * 256);
    const Crc64SliceTable& st = crc64SliceTable();
    for (int k = 0; k < 16; k++)
        memcpy(&out[(size_t)(CRC64_TAB_ELEM + k) * 256], st.slice[15 - k], 2048);
    Crc64Shift row(CRC64_ROW_BYTES);
    memcpy(&out[(size_t)CRC64_TAB_ROW * 256], row.t, sizeof(row.t));
    for (int w = 0; w < CRC64_WAVES_PER_TILE; w++)
        for (int l = 0; l < CRC64_WAVE_LANES; l++)
            out[(size_t)CRC64_TAB_WEIGHT * 256 + w * CRC64_WAVE_LANES + l] =
                crc64ShiftPoly(crc64ThreadTailBytes(w, l));
    return out;
}

// The device algorithm in plain C++, from the same table image: one raw
// partial per CRC64_TILE_BYTES tile of data[0, len), len % 16 == 0. A short
// final tile is right-aligned in the tile frame (its missing leading
// elements count as zeros), and a tile's 256 weighted values are joined in
// the kernel's order: lanes within a wave, then the waves.
inline std::vector<uint64_t> crc64TilesHost(const void* data, uint64_t len)
{
    static const std::vector<uint64_t> tab = crc64BuildTileTables();
    const unsigned char* p = (const unsigned char*)data;
    constexpr uint64_t TILE_VEC2 = CRC64_TILE_BYTES / 16;
    const uint64_t nVec2 = len / 16;
    const uint64_t nTiles = (nVec2 + TILE_VEC2 - 1) / TILE_VEC2;
    std::vector<uint64_t> partial(nTiles);

    auto lut8 = [&](int first, uint64_t v) {
        uint64_t r = 0;
        for (int k = 0; k < 8; k++) r ^= tab[(size_t)(first + k) * 256 + ((v >> (8 * k)) & 0xFF)];
        return r;
    };

    for (uint64_t tile = 0; tile < nTiles; tile++) {
        const uint64_t first = tile * TILE_VEC2;
        const uint64_t have = (nVec2 - first < TILE_VEC2) ? nVec2 - first : TILE_VEC2;
        const uint64_t pad = TILE_VEC2 - have; // leading zero elements of a short tile
        uint64_t t = 0;
        for (int wave = 0; wave < CRC64_WAVES_PER_TILE; wave++) {
            uint64_t wv = 0;
            for (int lane = 0; lane < CRC64_WAVE_LANES; lane++) {
                uint64_t acc = 0;
                for (int j = 0; j < CRC64_STEPS_PER_WAVE; j++) {
                    uint64_t pos = (uint64_t)(wave * CRC64_STEPS_PER_WAVE + j) * 64 + lane;
                    uint64_t x = 0, y = 0;
                    if (pos >= pad) {
                        memcpy(&x, p + (first + pos - pad) * 16, 8);
                        memcpy(&y, p + (first + pos - pad) * 16 + 8, 8);
                    }
                    acc = lut8(CRC64_TAB_ROW, acc) ^ lut8(CRC64_TAB_ELEM, x) ^
                          lut8(CRC64_TAB_ELEM + 8, y);
                }
                wv ^= crc64MulMod(tab[(size_t)CRC64_TAB_WEIGHT * 256 + wave * 64 + lane], acc);
            }
            t ^= wv;
        }
        partial[tile] = t;
    }
    return partial;
}

// Host fold of per-tile raw partials of one len-byte run (len % 16 == 0)
// onto `raw`, in tile order; the last tile may be short.
inline uint64_t crc64FoldTiles(const Crc64Shift& tileShift, uint64_t raw, const uint64_t* part,
                               uint64_t len)
{
    const uint64_t full = len / CRC64_TILE_BYTES;
    for (uint64_t i = 0; i < full; i++) raw = tileShift.apply(raw) ^ *part++;
    if (len % CRC64_TILE_BYTES) raw = crc64Combine(raw, *part, len % CRC64_TILE_BYTES);
    return raw;
}

} // namespace eb
