// Owners of device and pinned host memory: the only place of the library that allocates or frees either.  A block belongs
// to exactly one owner (move-only) and goes with it, so neither the handle nor a failing capacity change lists buffers.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <utility>

namespace mlvdb {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            bytes = std::exchange(o.bytes, 0);
        }
        return *this;
    }
    ~DevBuf() { release(); }
    // Workspaces (grow only): 25 % slack when the card has it, so a slowly growing need does not reallocate per call.
    hipError_t ensure(size_t need) {
        if (need <= bytes) return hipSuccess;
        if (exact(need + need / 4) == hipSuccess) return hipSuccess;
        return exact(need);
    }
    // A fresh block of exactly `need` bytes (what it held goes first): the rows, their norms and shadow, attribute columns,
    // list pools -- blocks sized by the corpus, where the slack would be gigabytes.
    hipError_t exact(size_t need) {
        release();
        const hipError_t e = hipMalloc(&p, need);
        if (e == hipSuccess)
            bytes = need;
        else
            p = nullptr;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T>
    T* as() const {
        return static_cast<T*>(p);
    }
};

// Pinned host staging (grow only): a hipMemcpyAsync from / to pageable memory goes through the runtime's own staging with
// a synchronisation per copy -- four small D2H copies and one 786 KB H2D copy cost a 256-query wave 0.33 ms on top of its
// 2.0 ms of kernels (round 2: p50_ms_per_wave_host_io 2.349 vs 2.016 device-resident).
struct PinBuf {
    void* p = nullptr;
    size_t bytes = 0;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    PinBuf(PinBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    PinBuf& operator=(PinBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            bytes = std::exchange(o.bytes, 0);
        }
        return *this;
    }
    ~PinBuf() { release(); }
    hipError_t ensure(size_t need) {
        if (need <= bytes) return hipSuccess;
        release();
        const size_t want = need + need / 4;
        const hipError_t e = hipHostMalloc(&p, want, 0);
        if (e == hipSuccess)
            bytes = want;
        else
            p = nullptr;
        return e;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// The new blocks of a capacity change (regrowth, compaction, a new column, a pool): Blocks is a DevBuf or a struct of them,
// filled by work enqueued on `stream` and moved into the handle once that work has drained.  Abandoned before that -- an
// early return, an exception -- the blocks may still be written by kernels in flight, so the scope drains the stream before
// its base, the blocks, is destroyed.  This is the one home of "drain before free"; nothing relies on hipFree synchronising.
// (After a commit the stream is idle and the blocks are empty: the wait returns at once and nothing is freed.)
template <class Blocks>
struct Staged : Blocks {
    hipStream_t stream;
    explicit Staged(hipStream_t s) : stream(s) {}
    ~Staged() { (void)hipStreamSynchronize(stream); }
};

// One block of several arrays, a DevBuf's or its copy on the host, stated once as a list of take<T>(n) calls: the next n
// values of T.  The list runs twice -- over no block (base == nullptr) it only measures, `at` being the bytes the block
// needs; over the block it hands out the fields.  A block's size is therefore never a formula of its own.  Nothing is
// rounded silently: a field whose offset is no multiple of its alignment sets `misaligned`, which the caller reports before
// any pointer is used; slack and alignment steps are written into the list (take<char>(16), pad_to(64)).
struct Carver {
    char* base = nullptr;
    size_t at = 0;
    bool misaligned = false;
    template <class T>
    T* take(size_t n) {
        misaligned |= at % alignof(T) != 0;
        T* first = base ? reinterpret_cast<T*>(base + at) : nullptr;
        at += n * sizeof(T);
        return first;
    }
    void pad_to(size_t align) { at = (at + align - 1) / align * align; }
};

// The layout most blocks have, [d64 | labels | dist | counts]: n entries and nq counts.
struct ListBlock {
    double* d64 = nullptr;
    int64_t* lab = nullptr;
    float* dist = nullptr;
    int32_t* cnt = nullptr;
    void take(Carver& c, size_t n, size_t nq) {
        d64 = c.take<double>(n);
        lab = c.take<int64_t>(n);
        dist = c.take<float>(n);
        cnt = c.take<int32_t>(nq);
    }
};

}  // namespace mlvdb
