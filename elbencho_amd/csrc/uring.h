// Minimal raw io_uring wrapper (no liburing dependency).
//
// MI355X-native replacement for the reference's libaio engine
// (/root/reference/source/workers/LocalWorker.cpp:1828-2070 aioBlockSized):
// io_uring is the one and only async engine here (no libaio path), per
// BASELINE.json's north star ("libaio/io_uring").
//
// Self-contained: io_uring_setup/io_uring_enter syscalls + ring mmaps,
// straight from the uapi contract in <linux/io_uring.h>.

#pragma once

#include <fcntl.h>
#include <linux/io_uring.h>
#include <linux/stat.h>
#include <linux/time_types.h>
#include <sys/mman.h>
#include <sys/syscall.h>
#include <sys/uio.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace eb {

class IoUring {
public:
    struct Completion {
        uint64_t userData;
        int32_t res; // bytes or -errno
    };

    IoUring() = default;
    IoUring(const IoUring&) = delete;
    IoUring& operator=(const IoUring&) = delete;
    ~IoUring() { destroy(); }

    // EB_URING_SQPOLL=1: kernel SQ polling thread (no submit syscalls while
    // the thread is awake; needs privileges — silently retried without on
    // EPERM). EB_URING_IOPOLL=1: completion polling for O_DIRECT on devices
    // that support it (NVMe) — opt-in, fails loudly elsewhere.
    void init(unsigned entries)
    {
        static const bool wantSqPoll = [] {
            const char* v = getenv("EB_URING_SQPOLL");
            return v && v[0] == '1';
        }();
        static const bool wantIoPoll = [] {
            const char* v = getenv("EB_URING_IOPOLL");
            return v && v[0] == '1';
        }();

        struct io_uring_params p;
        std::memset(&p, 0, sizeof(p));
        if (wantSqPoll) {
            p.flags |= IORING_SETUP_SQPOLL;
            p.sq_thread_idle = 2000; // ms before the SQ thread sleeps
        }
        if (wantIoPoll) p.flags |= IORING_SETUP_IOPOLL;

        ringFd = (int)syscall(__NR_io_uring_setup, entries, &p);
        // Unprivileged users: ring memory and registered buffers count
        // against RLIMIT_MEMLOCK per user, and the kernel gives back what a
        // closed ring held from a work queue, some time after close(). Rings
        // of the phase or engine just torn down can so make this setup fail
        // with ENOMEM for a moment: wait for the release (1 s at the most).
        for (int tries = 0; ringFd < 0 && errno == ENOMEM && tries < 50; tries++) {
            usleep(20 * 1000);
            ringFd = (int)syscall(__NR_io_uring_setup, entries, &p);
        }
        if (ringFd < 0 && wantSqPoll && (errno == EPERM || errno == EINVAL)) {
            // unprivileged: fall back to plain submission
            p.flags &= ~(unsigned)IORING_SETUP_SQPOLL;
            p.sq_thread_idle = 0;
            ringFd = (int)syscall(__NR_io_uring_setup, entries, &p);
        }
        if (ringFd < 0)
            throw std::runtime_error(std::string("io_uring_setup failed: ") + strerror(errno));
        sqPollActive = (p.flags & IORING_SETUP_SQPOLL) != 0;

        sqEntries = p.sq_entries;
        cqEntries = p.cq_entries;

        size_t sqRingSz = p.sq_off.array + p.sq_entries * sizeof(unsigned);
        size_t cqRingSz = p.cq_off.cqes + p.cq_entries * sizeof(struct io_uring_cqe);

        bool singleMmap = p.features & IORING_FEAT_SINGLE_MMAP;
        if (singleMmap && cqRingSz > sqRingSz) sqRingSz = cqRingSz;

        sqRing = mmap(nullptr, sqRingSz, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_POPULATE,
                      ringFd, IORING_OFF_SQ_RING);
        if (sqRing == MAP_FAILED)
            throw std::runtime_error("io_uring SQ ring mmap failed");
        sqRingSize = sqRingSz;

        if (singleMmap) {
            cqRing = sqRing;
            cqRingSize = 0; // shared mapping
        } else {
            cqRing = mmap(nullptr, cqRingSz, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_POPULATE,
                          ringFd, IORING_OFF_CQ_RING);
            if (cqRing == MAP_FAILED)
                throw std::runtime_error("io_uring CQ ring mmap failed");
            cqRingSize = cqRingSz;
        }

        sqesSize = p.sq_entries * sizeof(struct io_uring_sqe);
        sqes = (struct io_uring_sqe*)mmap(nullptr, sqesSize, PROT_READ | PROT_WRITE,
                                          MAP_SHARED | MAP_POPULATE, ringFd, IORING_OFF_SQES);
        if (sqes == MAP_FAILED)
            throw std::runtime_error("io_uring SQE array mmap failed");

        auto base = (char*)sqRing;
        sqHead = (std::atomic<unsigned>*)(base + p.sq_off.head);
        sqTail = (std::atomic<unsigned>*)(base + p.sq_off.tail);
        sqMask = *(unsigned*)(base + p.sq_off.ring_mask);
        sqArray = (unsigned*)(base + p.sq_off.array);
        sqFlags = (std::atomic<unsigned>*)(base + p.sq_off.flags);

        auto cbase = (char*)cqRing;
        cqHead = (std::atomic<unsigned>*)(cbase + p.cq_off.head);
        cqTail = (std::atomic<unsigned>*)(cbase + p.cq_off.tail);
        cqMask = *(unsigned*)(cbase + p.cq_off.ring_mask);
        cqes = (struct io_uring_cqe*)(cbase + p.cq_off.cqes);
    }

    bool valid() const { return ringFd >= 0; }

    // Pre-register the per-slot I/O buffers (IORING_REGISTER_BUFFERS): the
    // kernel pins the pages once instead of per operation, which matters at
    // high queue depth with small blocks (BASELINE config 3: 4K QD128).
    // Returns false (and stays unregistered) if the kernel refuses.
    bool registerBuffers(const struct iovec* iovs, unsigned n)
    {
        int ret = (int)syscall(__NR_io_uring_register, ringFd, IORING_REGISTER_BUFFERS,
                               (void*)iovs, n);
        buffersRegistered = (ret == 0);
        return buffersRegistered;
    }

    // Pre-register the target fds (IORING_REGISTER_FILES): skips the per-op
    // fd refcount. prep() then takes the table index with fixedFile=true.
    bool registerFiles(const int* fds, unsigned n)
    {
        int ret = (int)syscall(__NR_io_uring_register, ringFd, IORING_REGISTER_FILES,
                               (void*)fds, n);
        filesRegistered = (ret == 0);
        return filesRegistered;
    }

    bool hasFixedBuffers() const { return buffersRegistered; }
    bool hasFixedFiles() const { return filesRegistered; }

    // Queue one read or write; does not submit to the kernel yet.
    // Returns false if the SQ is full. bufIndex >= 0 uses the registered
    // buffer table (READ_FIXED/WRITE_FIXED); fixedFile makes fd a table index.
    bool prep(bool isWrite, int fd, void* buf, uint64_t len, uint64_t fileOff,
              uint64_t userData, int bufIndex = -1, bool fixedFile = false,
              bool link = false)
    {
        struct io_uring_sqe* sqe = nextSqe();
        if (!sqe) return false;
        if (bufIndex >= 0) {
            sqe->opcode = isWrite ? IORING_OP_WRITE_FIXED : IORING_OP_READ_FIXED;
            sqe->buf_index = (uint16_t)bufIndex;
        } else {
            sqe->opcode = isWrite ? IORING_OP_WRITE : IORING_OP_READ;
        }
        sqe->fd = fd;
        if (fixedFile) sqe->flags |= IOSQE_FIXED_FILE;
        if (link) sqe->flags |= IOSQE_IO_LINK;
        sqe->addr = (uint64_t)buf;
        sqe->len = (uint32_t)len;
        sqe->off = fileOff;
        sqe->user_data = userData;
        return true;
    }

    // --- small-file metadata pipeline ops (open/close into the fixed file
    // table as "direct descriptors": the fd never surfaces to userspace) ---

    // Register an all-sparse fixed file table of n slots (kernel >= 5.13:
    // -1 entries allowed). Required for the direct-descriptor ops below.
    bool registerFilesSparse(unsigned n)
    {
        std::vector<int> fds(n, -1);
        int ret = (int)syscall(__NR_io_uring_register, ringFd, IORING_REGISTER_FILES,
                               fds.data(), n);
        filesRegistered = (ret == 0);
        return filesRegistered;
    }

    // Cap this ring's io-wq worker pool (bounded, unbounded). Punted ops
    // (openat etc on filesystems without async support) otherwise spawn up
    // to RLIMIT_NPROC workers — per-ring caps stop worker thrash when many
    // engine threads each run a ring.
    bool limitWorkers(unsigned bounded, unsigned unbounded)
    {
        unsigned vals[2] = {bounded, unbounded};
        return syscall(__NR_io_uring_register, ringFd,
                       IORING_REGISTER_IOWQ_MAX_WORKERS, vals, 2) == 0;
    }

    // OPENAT into fixed-table slot fileIndex. `path` must stay alive until
    // the CQE arrives. link chains the following SQE.
    bool prepOpenAt(const char* path, int openFlags, unsigned mode,
                    unsigned fileIndex, uint64_t userData, bool link)
    {
        struct io_uring_sqe* sqe = nextSqe();
        if (!sqe) return false;
        sqe->opcode = IORING_OP_OPENAT;
        sqe->fd = AT_FDCWD;
        sqe->addr = (uint64_t)path;
        sqe->open_flags = (uint32_t)openFlags;
        sqe->len = mode;
        sqe->file_index = fileIndex + 1; // 0 = allocate a normal fd
        if (link) sqe->flags |= IOSQE_IO_LINK;
        sqe->user_data = userData;
        return true;
    }

    // CLOSE of fixed-table slot fileIndex.
    bool prepCloseDirect(unsigned fileIndex, uint64_t userData, bool link = false)
    {
        struct io_uring_sqe* sqe = nextSqe();
        if (!sqe) return false;
        sqe->opcode = IORING_OP_CLOSE;
        sqe->fd = 0;
        sqe->file_index = fileIndex + 1;
        if (link) sqe->flags |= IOSQE_IO_LINK;
        sqe->user_data = userData;
        return true;
    }

    // STATX by path. `path` and `stx` must stay alive until the CQE.
    bool prepStatx(const char* path, struct statx* stx, unsigned mask,
                   uint64_t userData)
    {
        struct io_uring_sqe* sqe = nextSqe();
        if (!sqe) return false;
        sqe->opcode = IORING_OP_STATX;
        sqe->fd = AT_FDCWD;
        sqe->addr = (uint64_t)path;
        sqe->len = mask;
        sqe->off = (uint64_t)stx;
        sqe->user_data = userData;
        return true;
    }

    // UNLINKAT by path.
    bool prepUnlink(const char* path, uint64_t userData)
    {
        struct io_uring_sqe* sqe = nextSqe();
        if (!sqe) return false;
        sqe->opcode = IORING_OP_UNLINKAT;
        sqe->fd = AT_FDCWD;
        sqe->addr = (uint64_t)path;
        sqe->user_data = userData;
        return true;
    }

    // Submit queued SQEs; optionally wait for at least `waitNr` completions.
    // timeoutMs >= 0 bounds the wait (IORING_ENTER_EXT_ARG) so callers can
    // run interrupt checks while a slow/hung device sits on the CQ — the
    // reference's libaio loop uses a 5 s io_getevents timeout for the same
    // reason (LocalWorker.cpp:71).
    int submitAndWait(unsigned waitNr, int timeoutMs = -1)
    {
        if (timeoutMs >= 0 && waitNr && !sqPollActive) {
            unsigned toSubmit = pending;
            struct __kernel_timespec ts;
            ts.tv_sec = timeoutMs / 1000;
            ts.tv_nsec = (long long)(timeoutMs % 1000) * 1000000;
            struct io_uring_getevents_arg arg;
            std::memset(&arg, 0, sizeof(arg));
            arg.ts = (uint64_t)&ts;
            int ret = (int)syscall(__NR_io_uring_enter, ringFd, toSubmit, waitNr,
                                   IORING_ENTER_GETEVENTS | IORING_ENTER_EXT_ARG,
                                   &arg, sizeof(arg));
            if (ret < 0) {
                if (errno == EINTR || errno == ETIME) {
                    // keep `pending` as is: to_submit is clamped by the
                    // kernel to what is actually queued, so an overstated
                    // count is harmless and nothing gets lost
                    return 0;
                }
                throw std::runtime_error(std::string("io_uring_enter failed: ") +
                                         strerror(errno));
            }
            pending -= (unsigned)ret;
            return ret;
        }

        if (sqPollActive) {
            // the kernel SQ thread consumes the ring; only enter to wake a
            // sleeping thread or to wait for completions
            unsigned flags = waitNr ? IORING_ENTER_GETEVENTS : 0;
            if (sqFlags->load(std::memory_order_relaxed) & IORING_SQ_NEED_WAKEUP)
                flags |= IORING_ENTER_SQ_WAKEUP;
            unsigned submitted = pending;
            pending = 0;
            if (!flags) return (int)submitted;
            int ret = (int)syscall(__NR_io_uring_enter, ringFd, submitted, waitNr,
                                   flags, nullptr, 0);
            if (ret < 0) {
                if (errno == EINTR) return 0;
                throw std::runtime_error(std::string("io_uring_enter failed: ") +
                                         strerror(errno));
            }
            return (int)submitted;
        }

        unsigned toSubmit = pending;
        int ret = (int)syscall(__NR_io_uring_enter, ringFd, toSubmit, waitNr,
                               waitNr ? IORING_ENTER_GETEVENTS : 0, nullptr, 0);
        if (ret < 0) {
            if (errno == EINTR) return 0;
            throw std::runtime_error(std::string("io_uring_enter failed: ") + strerror(errno));
        }
        pending -= (unsigned)ret;
        return ret;
    }

    // Reap up to maxEvents completions without blocking.
    unsigned reap(Completion* out, unsigned maxEvents)
    {
        unsigned head = cqHead->load(std::memory_order_relaxed);
        unsigned tail = cqTail->load(std::memory_order_acquire);
        unsigned n = 0;
        while (head != tail && n < maxEvents) {
            const struct io_uring_cqe* cqe = &cqes[head & cqMask];
            out[n].userData = cqe->user_data;
            out[n].res = cqe->res;
            n++;
            head++;
        }
        cqHead->store(head, std::memory_order_release);
        return n;
    }

    unsigned entries() const { return sqEntries; }

private:
    // Claim the next SQE (zeroed) or nullptr when the SQ is full.
    struct io_uring_sqe* nextSqe()
    {
        unsigned tail = sqTail->load(std::memory_order_relaxed);
        unsigned head = sqHead->load(std::memory_order_acquire);
        if (tail - head >= sqEntries) return nullptr;
        unsigned idx = tail & sqMask;
        struct io_uring_sqe* sqe = &sqes[idx];
        std::memset(sqe, 0, sizeof(*sqe));
        sqArray[idx] = idx;
        sqTail->store(tail + 1, std::memory_order_release);
        pending++;
        return sqe;
    }

public:

    void destroy()
    {
        if (sqes && sqes != MAP_FAILED) munmap(sqes, sqesSize);
        if (cqRing && cqRing != MAP_FAILED && cqRingSize) munmap(cqRing, cqRingSize);
        if (sqRing && sqRing != MAP_FAILED) munmap(sqRing, sqRingSize);
        if (ringFd >= 0) close(ringFd);
        sqes = nullptr;
        cqRing = nullptr;
        sqRing = nullptr;
        ringFd = -1;
    }

private:
    int ringFd = -1;
    unsigned sqEntries = 0, cqEntries = 0, pending = 0;
    bool buffersRegistered = false, filesRegistered = false;
    bool sqPollActive = false;
    void* sqRing = nullptr;
    void* cqRing = nullptr;
    struct io_uring_sqe* sqes = nullptr;
    size_t sqRingSize = 0, cqRingSize = 0, sqesSize = 0;

    std::atomic<unsigned>* sqHead = nullptr;
    std::atomic<unsigned>* sqTail = nullptr;
    unsigned sqMask = 0;
    unsigned* sqArray = nullptr;
    std::atomic<unsigned>* sqFlags = nullptr;

    std::atomic<unsigned>* cqHead = nullptr;
    std::atomic<unsigned>* cqTail = nullptr;
    unsigned cqMask = 0;
    struct io_uring_cqe* cqes = nullptr;
};

} // namespace eb
