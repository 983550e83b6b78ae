// Native S3/HTTP data plane — the block-transfer hot loop in C++.
//
// the pure-Python client (GIL, per-chunk allocations) caps
// the S3 engine's local data-plane at ~1.6 GiB/s GET; the reference's
// largest engine is its async multipart pipeline (LocalWorker.cpp:4905-6488,
// AWS SDK C++ under the hood). Here the control plane (SigV4 signing, XML,
// retries, listings) stays in Python — this class only executes fully
// formed requests over a persistent connection and generates/consumes the
// object BODY natively:
//   PUT: headers from Python (UNSIGNED-PAYLOAD signed), body generated
//        on the fly — integrity-checksum pattern (GPU fill kernel + D2H
//        through pinned staging when a device is attached, CPU otherwise)
//        or a prefilled random buffer;
//   GET: body received straight into a pinned buffer and verified in
//        place (gfx950 verify kernel via H2D staging, or CPU) — no Python
//        bytes objects, no GIL on the wire.
// On any socket error the connection is dropped and status -1 returned;
// the Python caller retries once and can fall back to the pure path.

#pragma once

#include <arpa/inet.h>
#include <netdb.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <sys/socket.h>
#include <unistd.h>

#include <atomic>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

#include "crc.h"
#include "crc64.h"
#include "gpu.h"
#include "rand.h"

namespace eb {

void fillChecksumCPU(char* buf, uint64_t len, uint64_t fileOff, uint64_t salt);
uint64_t verifyChecksumCPU(const char* buf, uint64_t len, uint64_t fileOff,
                           uint64_t salt);

class HttpDataPlane {
public:
    // live-instance counter (leak tests): constructor ++, destructor --
    static std::atomic<int>& liveCount()
    {
        static std::atomic<int> n{0};
        return n;
    }

    HttpDataPlane(std::string hostIn, int portIn, int dev, uint64_t maxBlockIn,
                  uint64_t randSeed)
        : host(std::move(hostIn)), port(portIn),
          maxBlock(std::max<uint64_t>(maxBlockIn, 4096))
    {
        if (dev >= 0) {
            gpu.reset(new GpuCtx(dev, 2, maxBlock, true));
            buf = gpu->hostBuf(0);
        } else {
            if (posix_memalign((void**)&ownBuf, 4096, maxBlock))
                throw std::runtime_error("httpdata: buffer alloc failed");
            buf = ownBuf;
        }
        // prefilled random body for non-verify PUTs (defeats compression)
        randBuf.resize(maxBlock);
        RandAlgoXoshiro256ppSIMD<8> rng(randSeed);
        rng.fillBuf(randBuf.data(), maxBlock);
        liveCount().fetch_add(1);
    }

    ~HttpDataPlane()
    {
        closeConn();
        free(ownBuf);
        liveCount().fetch_sub(1);
    }

    HttpDataPlane(const HttpDataPlane&) = delete;
    HttpDataPlane& operator=(const HttpDataPlane&) = delete;

    // GET: returns {status, bytesReceived, numMismatches, firstBadOffset}.
    // status -1 = connection error (caller retries). Body larger than
    // expectLen is an error (-2). Only a 2xx body with salt >= 0 is verified,
    // against the checksum pattern at patternOff; otherwise the result is
    // {.., 0, UINT64_MAX}.
    //
    // What numMismatches and firstBadOffset mean (tests/
    // test_s3_dataplane_exact.py holds the code to exactly this rule): the
    // body is cut into chunks of C bytes, the last one shorter, with
    // C = min(maxBlock, 2 MiB) when a device is attached and C = maxBlock
    // otherwise (maxBlock is at least 4096).
    //   - A chunk is checked on the GPU iff a device is attached,
    //     patternOff % 8 == 0, the chunk's pattern offset is a multiple of 8
    //     and its length is a multiple of 16. It contributes the number of
    //     its mismatching u64 words and the pattern offset of the first such
    //     word.
    //   - Any other chunk is checked on the host. If it has a mismatch it
    //     contributes 1 and the pattern offset of its first bad byte.
    // numMismatches is the sum over the chunks, firstBadOffset the numeric
    // minimum (UINT64_MAX when clean). Pattern offsets are taken mod 2^64.
    // Every call starts from zero: mismatches that an aborted request (-1)
    // had already found are dropped with it.
    std::tuple<int, uint64_t, uint64_t, uint64_t> get(const std::string& rawReq,
                                                      uint64_t expectLen,
                                                      uint64_t patternOff,
                                                      int64_t salt)
    {
        if (!sendReq(rawReq)) return {-1, 0, 0, ~0ULL};
        int status;
        uint64_t contentLen;
        if (!readHeader(status, contentLen)) return {-1, 0, 0, ~0ULL};
        if (contentLen > expectLen && status < 300) { // oversized body
            closeConn();
            return {-2, contentLen, 0, ~0ULL};
        }

        uint64_t nbad = 0, firstBad = ~0ULL;
        uint64_t got = 0;
        const bool doVerify = salt >= 0 && status < 300;
        const bool gpuVerify = doVerify && gpu && (patternOff % 8 == 0);
        const bool gpuStage = gpu && status < 300;

        // GPU path: chunk the body and pipeline recv with H2D + async
        // verify across the slot ring (recv of chunk i overlaps the PCIe
        // copy + verify kernel of chunk i-1)
        const int nSlots = gpu ? gpu->numSlots() : 1;
        const uint64_t chunk = gpuStage
                                   ? std::min<uint64_t>(maxBlock, 2 << 20)
                                   : maxBlock;
        std::vector<char> busy(nSlots, 0);
        int slot = 0;
        bool asyncVerifyUsed = false;

        while (got < contentLen) {
            uint64_t want = std::min<uint64_t>(contentLen - got, chunk);
            char* dst = gpuStage ? gpu->hostBuf(slot) : buf;
            if (gpuStage && busy[slot]) {
                gpu->waitSlotEvent(slot);
                busy[slot] = 0;
            }
            uint64_t have = 0;
            while (have < want) {
                ssize_t r = recvSome(dst + have, want - have);
                if (r <= 0) {
                    closeConn();
                    // the caller retries on this plane: leave no copy in
                    // flight on the slots and no mismatch of this request
                    // in the context's persistent verify counters
                    if (gpuStage) gpu->syncStream();
                    if (asyncVerifyUsed) (void)gpu->fetchVerifyResult();
                    return {-1, got + have, 0, ~0ULL};
                }
                have += (uint64_t)r;
            }
            uint64_t off = patternOff + got;
            if (gpuStage) {
                gpu->copyH2DAsync(slot, have);
                if (gpuVerify && off % 8 == 0 && have % 16 == 0) {
                    gpu->verifyChecksumDevAsync(slot, have, off,
                                                (uint64_t)salt);
                    asyncVerifyUsed = true;
                } else if (doVerify) { // odd tail: check on host
                    uint64_t bad = verifyChecksumCPU(dst, have, off,
                                                     (uint64_t)salt);
                    if (bad != ~0ULL) {
                        nbad++;
                        if (bad < firstBad) firstBad = bad;
                    }
                }
                gpu->recordSlotEvent(slot);
                busy[slot] = 1;
                slot = (slot + 1) % nSlots;
            } else if (doVerify) {
                uint64_t bad = verifyChecksumCPU(buf, have, off,
                                                 (uint64_t)salt);
                if (bad != ~0ULL) {
                    nbad++;
                    if (bad < firstBad) firstBad = bad;
                }
            }
            got += have;
        }
        if (gpuStage) gpu->syncStream(); // drain copies before buffer reuse
        if (asyncVerifyUsed) {
            GpuVerifyResult r = gpu->fetchVerifyResult();
            nbad += r.numMismatches;
            if (r.firstBadFileOffset < firstBad)
                firstBad = r.firstBadFileOffset;
        }
        return {status, got, nbad, firstBad};
    }

    // GET returning the body (small/correctness paths): {status, body}.
    std::pair<int, std::string> getData(const std::string& rawReq,
                                        uint64_t maxLen)
    {
        if (!sendReq(rawReq)) return {-1, ""};
        int status;
        uint64_t contentLen;
        if (!readHeader(status, contentLen)) return {-1, ""};
        if (contentLen > maxLen) {
            closeConn();
            return {-2, ""};
        }
        std::string body(contentLen, '\0');
        uint64_t got = 0;
        while (got < contentLen) {
            ssize_t r = recvSome(&body[got], contentLen - got);
            if (r <= 0) {
                closeConn();
                return {-1, ""};
            }
            got += (uint64_t)r;
        }
        return {status, std::move(body)};
    }

    // PUT: send rawReqHeaders then a generated body of len bytes.
    // salt >= 0: checksum pattern at patternOff (GPU fill + D2H when
    // attached); salt < 0: prefilled random data. Returns {status,
    // responseHeaders} (Python parses the ETag).
    std::pair<int, std::string> put(const std::string& rawReqHeaders,
                                    uint64_t len, uint64_t patternOff,
                                    int64_t salt)
    {
        if (!sendReq(rawReqHeaders)) return {-1, ""};
        uint64_t sent = 0;
        if (salt >= 0 && gpu && patternOff % 8 == 0) {
            // pipelined: the gfx950 fill + D2H of chunk i+1 overlaps the
            // socket send of chunk i (2-slot ring)
            const uint64_t chunk = std::min<uint64_t>(maxBlock, 2 << 20);
            const int nSlots = gpu->numSlots();
            std::vector<char> gpuPrepped(nSlots, 0);

            auto prepChunk = [&](int s, uint64_t off, uint64_t n) {
                // what the fill kernel does not take (ragged length, or a
                // chunk that starts inside a word because maxBlock % 8 != 0)
                // is CPU-filled at send time, as in bodyCrc()
                if (n % 8 || off % 8) {
                    gpuPrepped[s] = 0;
                    return;
                }
                gpu->fillChecksumDev(s, n, off, (uint64_t)salt);
                gpu->copyD2HAsync(s, n);
                gpu->recordSlotEvent(s);
                gpuPrepped[s] = 1;
            };

            int cur = 0;
            prepChunk(cur, patternOff, std::min<uint64_t>(len, chunk));
            while (sent < len) {
                uint64_t n = std::min<uint64_t>(len - sent, chunk);
                int nxt = (cur + 1) % nSlots;
                if (sent + n < len)
                    prepChunk(nxt, patternOff + sent + n,
                              std::min<uint64_t>(len - sent - n, chunk));
                if (gpuPrepped[cur])
                    gpu->waitSlotEvent(cur);
                else
                    fillChecksumCPU(gpu->hostBuf(cur), n, patternOff + sent,
                                    (uint64_t)salt);
                if (!sendAll(gpu->hostBuf(cur), n)) return {-1, ""};
                sent += n;
                cur = nxt;
            }
        }
        while (sent < len) {
            uint64_t n = std::min<uint64_t>(len - sent, maxBlock);
            const char* src;
            if (salt >= 0) {
                uint64_t off = patternOff + sent;
                fillChecksumCPU(buf, n, off, (uint64_t)salt);
                src = buf;
            } else {
                src = randBuf.data(); // same random block every time is fine
            }
            if (!sendAll(src, n)) return {-1, ""};
            sent += n;
        }
        int status;
        uint64_t contentLen;
        std::string rawHdrs;
        if (!readHeader(status, contentLen, &rawHdrs)) return {-1, ""};
        // drain (small) response body
        uint64_t got = 0;
        while (got < contentLen) {
            uint64_t n = std::min<uint64_t>(contentLen - got, maxBlock);
            ssize_t r = recvSome(buf, n);
            if (r <= 0) {
                closeConn();
                return {-1, ""};
            }
            got += (uint64_t)r;
        }
        return {status, std::move(rawHdrs)};
    }

    // Checksum (finished CRC-32 / CRC-32C) of exactly the len bytes that
    // put(..., len, patternOff, salt) sends, so the caller can sign an
    // x-amz-checksum-* header without the body ever reaching Python.
    // Pattern bodies with a device attached are generated a second time in
    // HBM and reduced there by the CRC tile kernel: fill + CRC per chunk on
    // the one in-order stream (so the slot ring needs no events), one fetch
    // and therefore one synchronization per object. The stream is drained on
    // return, so put() finds the slots free. Random bodies are randBuf
    // repeated: its CRC is computed once per plane and extended by
    // crcCombine, with no GPU work.
    uint32_t bodyCrc(uint64_t len, uint64_t patternOff, int64_t salt, CrcAlgo algo)
    {
        return bodyCrcT(Crc32Ops{algo, randCrc[(int)algo]}, len, patternOff, salt);
    }

    // The same for CRC-64/NVME (x-amz-checksum-crc64nvme), through the same
    // three branches; the device branch runs ebCrc64TilesKernel.
    uint64_t bodyCrc64(uint64_t len, uint64_t patternOff, int64_t salt)
    {
        return bodyCrcT(Crc64Ops{randCrc64}, len, patternOff, salt);
    }

    void close() { closeConn(); }

private:
    template <typename W>
    struct RandCrcT {
        bool valid = false;
        W full = 0; // CRC of randBuf[0, maxBlock)
        W xp = 0;   // x^(8*maxBlock) mod P
    };
    RandCrcT<uint32_t> randCrc[2]; // per CrcAlgo
    RandCrcT<uint64_t> randCrc64;

    // What bodyCrcT needs of a checksum: the host library and the device trio.
    struct Crc32Ops {
        using Word = uint32_t;
        CrcAlgo algo;
        RandCrcT<uint32_t>& rand;
        Word update(Word c, const void* p, size_t n) const { return crcUpdate(algo, c, p, n); }
        Word shiftPoly(uint64_t n) const { return crcShiftPoly(algo, n); }
        Word combineXp(Word xp, Word a, Word b) const { return crcCombineXp(algo, xp, a, b); }
        Word combine(Word a, Word b, uint64_t n) const { return crcCombine(algo, a, b, n); }
        uint64_t tileBytes() const { return gpuCrcTileBytes(); }
        void devAsync(GpuCtx& g, int slot, uint64_t n, uint64_t base) const
        {
            g.crcDevAsync(slot, n, algo, base);
        }
        Word fetch(GpuCtx& g, uint64_t n, uint64_t tiles) const
        {
            return g.crcFetch(algo, n, tiles);
        }
    };
    struct Crc64Ops {
        using Word = uint64_t;
        RandCrcT<uint64_t>& rand;
        Word update(Word c, const void* p, size_t n) const { return crc64Update(c, p, n); }
        Word shiftPoly(uint64_t n) const { return crc64ShiftPoly(n); }
        Word combineXp(Word xp, Word a, Word b) const { return crc64CombineXp(xp, a, b); }
        Word combine(Word a, Word b, uint64_t n) const { return crc64Combine(a, b, n); }
        uint64_t tileBytes() const { return gpuCrc64TileBytes(); }
        void devAsync(GpuCtx& g, int slot, uint64_t n, uint64_t base) const
        {
            g.crc64DevAsync(slot, n, base);
        }
        Word fetch(GpuCtx& g, uint64_t n, uint64_t tiles) const { return g.crc64Fetch(n, tiles); }
    };

    template <typename Ops>
    typename Ops::Word bodyCrcT(Ops ops, uint64_t len, uint64_t patternOff, int64_t salt)
    {
        typename Ops::Word crc = 0;
        uint64_t done = 0;

        if (salt < 0) {
            auto& rc = ops.rand;
            if (!rc.valid) {
                rc.full = ops.update(0, randBuf.data(), maxBlock);
                rc.xp = ops.shiftPoly(maxBlock);
                rc.valid = true;
            }
            for (; len - done >= maxBlock; done += maxBlock)
                crc = ops.combineXp(rc.xp, crc, rc.full);
            return ops.update(crc, randBuf.data(), len - done);
        }

        if (gpu && patternOff % 8 == 0) {
            // same chunks as put(); a chunk the kernels cannot take (ragged
            // length) is filled and summed on the host
            const uint64_t chunk = std::min<uint64_t>(maxBlock, 2 << 20);
            const int nSlots = gpu->numSlots();
            uint64_t devLen = 0, devTiles = 0; // enqueued, not yet fetched
            const uint64_t tileBytes = ops.tileBytes();
            auto fetch = [&] {
                if (!devLen) return;
                crc = ops.combine(crc, ops.fetch(*gpu, devLen, devTiles), devLen);
                devLen = devTiles = 0;
            };
            int slot = 0;
            while (done < len) {
                uint64_t n = std::min<uint64_t>(len - done, chunk);
                uint64_t off = patternOff + done;
                if (n % 16 == 0 && off % 8 == 0) {
                    gpu->fillChecksumDev(slot, n, off, (uint64_t)salt);
                    ops.devAsync(*gpu, slot, n, devTiles);
                    devLen += n;
                    devTiles += (n + tileBytes - 1) / tileBytes;
                    slot = (slot + 1) % nSlots;
                } else {
                    fetch();
                    fillChecksumCPU(buf, n, off, (uint64_t)salt);
                    crc = ops.update(crc, buf, n);
                }
                done += n;
            }
            fetch();
            return crc;
        }

        while (done < len) {
            uint64_t n = std::min<uint64_t>(len - done, maxBlock);
            fillChecksumCPU(buf, n, patternOff + done, (uint64_t)salt);
            crc = ops.update(crc, buf, n);
            done += n;
        }
        return crc;
    }

    std::string host;
    int port;
    uint64_t maxBlock;
    int fd = -1;
    char* buf = nullptr;    // pinned (GPU mode) or aligned heap
    char* ownBuf = nullptr; // owned when no GPU
    std::vector<char> randBuf;
    std::unique_ptr<GpuCtx> gpu;
    std::string pending; // bytes read past the current response header

    bool connectIfNeeded()
    {
        if (fd >= 0) return true;
        struct addrinfo hints{};
        hints.ai_family = AF_UNSPEC;
        hints.ai_socktype = SOCK_STREAM;
        struct addrinfo* res = nullptr;
        if (getaddrinfo(host.c_str(), std::to_string(port).c_str(), &hints,
                        &res) || !res)
            return false;
        fd = ::socket(res->ai_family, SOCK_STREAM, 0);
        if (fd < 0 || ::connect(fd, res->ai_addr, res->ai_addrlen)) {
            if (fd >= 0) ::close(fd);
            fd = -1;
            freeaddrinfo(res);
            return false;
        }
        freeaddrinfo(res);
        int one = 1;
        setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));
        // big socket buffers: fewer syscalls per MiB on the recv side
        int bufsz = 4 << 20;
        setsockopt(fd, SOL_SOCKET, SO_RCVBUF, &bufsz, sizeof(bufsz));
        setsockopt(fd, SOL_SOCKET, SO_SNDBUF, &bufsz, sizeof(bufsz));
        pending.clear();
        return true;
    }

    void closeConn()
    {
        if (fd >= 0) ::close(fd);
        fd = -1;
        pending.clear();
    }

    bool sendReq(const std::string& req)
    {
        for (int attempt = 0; attempt < 2; attempt++) {
            if (!connectIfNeeded()) continue;
            if (sendAll(req.data(), req.size())) return true;
            closeConn(); // stale keep-alive: reconnect once
        }
        return false;
    }

    bool sendAll(const char* p, size_t n)
    {
        while (n) {
            ssize_t r = send(fd, p, n, MSG_NOSIGNAL);
            if (r <= 0) return false;
            p += r;
            n -= (size_t)r;
        }
        return true;
    }

    ssize_t recvSome(char* dst, uint64_t max)
    {
        if (!pending.empty()) {
            uint64_t n = std::min<uint64_t>(max, pending.size());
            std::memcpy(dst, pending.data(), n);
            pending.erase(0, n);
            return (ssize_t)n;
        }
        return recv(fd, dst, max, 0);
    }

    bool readHeader(int& status, uint64_t& contentLen,
                    std::string* rawOut = nullptr)
    {
        std::string hdr = std::move(pending);
        pending.clear();
        size_t end;
        while ((end = hdr.find("\r\n\r\n")) == std::string::npos) {
            char tmp[16384];
            ssize_t r = recv(fd, tmp, sizeof(tmp), 0);
            if (r <= 0) {
                closeConn();
                return false;
            }
            hdr.append(tmp, (size_t)r);
            if (hdr.size() > (1 << 20)) {
                closeConn();
                return false;
            }
        }
        pending = hdr.substr(end + 4);
        hdr.resize(end + 4);

        if (hdr.rfind("HTTP/1.", 0) != 0 || hdr.size() < 12) {
            closeConn();
            return false;
        }
        status = atoi(hdr.c_str() + 9);

        contentLen = 0;
        size_t pos = hdr.find("\r\n");
        while (pos != std::string::npos && pos < end) {
            size_t eol = hdr.find("\r\n", pos + 2);
            if (eol == std::string::npos) break;
            std::string line = hdr.substr(pos + 2, eol - pos - 2);
            size_t colon = line.find(':');
            if (colon != std::string::npos) {
                std::string key = line.substr(0, colon);
                for (auto& c : key) c = (char)tolower(c);
                if (key == "content-length")
                    contentLen = strtoull(line.c_str() + colon + 1, nullptr, 10);
            }
            pos = eol;
        }
        if (rawOut) *rawOut = hdr;
        return true;
    }
};

} // namespace eb
