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

// A bump carver over one block of several arrays, a DevBuf's or its copy on the host: take<T>(n) is the next n values of T.
// It pads nothing.  Every layout carved with it lists its 8-byte fields (double, int64) before its 4-byte ones (float,
// int32) -- descending alignment -- so every field lies aligned whatever the counts are.
struct Carver {
    char* at;
    template <class T>
    T* take(size_t n) {
        T* first = reinterpret_cast<T*>(at);
        at += n * sizeof(T);
        return first;
    }
};

// The layout most blocks have, [d64 | labels | dist | counts]: n entries and nq counts.
struct ListBlock {
    double* d64;
    int64_t* lab;
    float* dist;
    int32_t* cnt;
    static size_t bytes(size_t n, size_t nq) { return n * (sizeof(double) + sizeof(int64_t) + sizeof(float)) + nq * sizeof(int32_t); }
    ListBlock(void* block, size_t n, size_t nq) {
        Carver c{static_cast<char*>(block)};
        d64 = c.take<double>(n);
        lab = c.take<int64_t>(n);
        dist = c.take<float>(n);
        cnt = c.take<int32_t>(nq);
    }
};

}  // namespace mlvdb
