// Host-only check of csrc/device_memory.h: the HIP allocator calls are faked over malloc here (no HIP library is linked),
// the fakes count live blocks and can be told which allocation fails.  Built and run by tests/test_device_memory_host.py
// under -fsanitize=address,undefined; exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "device_memory.h"

namespace {
int live = 0;         // blocks allocated and not yet freed, device and pinned together
int allocs = 0;       // allocation calls so far
int fail_mask = 0;    // bit i set: the i-th allocation call from now on fails
int drains = 0;       // hipStreamSynchronize calls
int live_at_drain = -1;  // `live` at the last of them
size_t last_size = 0;

hipError_t fake_alloc(void** p, size_t bytes) {
    ++allocs;
    const bool failing = fail_mask & 1;
    fail_mask >>= 1;
    if (failing) {
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes ? bytes : 1);
    last_size = bytes;
    ++live;
    return hipSuccess;
}
hipError_t fake_free(void* p) {
    if (p) --live;
    std::free(p);
    return hipSuccess;
}

int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);         \
            ++failures;                                                     \
        }                                                                   \
    } while (0)
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return fake_alloc(p, bytes); }
hipError_t hipFree(void* p) { return fake_free(p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return fake_alloc(p, bytes); }
hipError_t hipHostFree(void* p) { return fake_free(p); }
hipError_t hipStreamSynchronize(hipStream_t) {
    ++drains;
    live_at_drain = live;
    return hipSuccess;
}
}

using mlvdb::DevBuf;
using mlvdb::PinBuf;
using mlvdb::Staged;

struct Two {
    DevBuf a, b;
};

int main() {
    static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "DevBuf copies");
    static_assert(!std::is_copy_constructible<PinBuf>::value && !std::is_copy_assignable<PinBuf>::value, "PinBuf copies");
    {  // a scope of several owners frees them all
        DevBuf a, b, c;
        PinBuf p, q;
        CHECK(a.ensure(100) == hipSuccess && b.ensure(1) == hipSuccess && p.ensure(64) == hipSuccess);
        CHECK(live == 3 && c.p == nullptr && q.p == nullptr);
    }
    CHECK(live == 0);
    {  // moves: the source is left empty, an assignment frees what the target held
        DevBuf a, b;
        CHECK(a.ensure(100) == hipSuccess && b.ensure(200) == hipSuccess && live == 2);
        void* const was = b.p;
        a = std::move(b);
        CHECK(live == 1 && a.p == was && a.bytes == 250 && b.p == nullptr && b.bytes == 0);
        DevBuf c(std::move(a));
        CHECK(live == 1 && c.p == was && c.bytes == 250 && a.p == nullptr && a.bytes == 0);
        CHECK(a.ensure(8) == hipSuccess && live == 2);  // a moved-from owner is an empty one: usable
        PinBuf p, q;
        CHECK(p.ensure(100) == hipSuccess && q.ensure(200) == hipSuccess && live == 4);
        void* const pwas = q.p;
        p = std::move(q);
        CHECK(live == 3 && p.p == pwas && p.bytes == 250 && q.p == nullptr && q.bytes == 0);
        PinBuf r(std::move(p));
        CHECK(live == 3 && r.p == pwas && p.p == nullptr && p.bytes == 0);
    }
    CHECK(live == 0);
    {  // ensure: grow only, need + need/4 first, the old block freed
        DevBuf a;
        CHECK(a.ensure(1000) == hipSuccess && a.bytes == 1250 && last_size == 1250 && live == 1);
        void* const was = a.p;
        const int before = allocs;
        CHECK(a.ensure(1250) == hipSuccess && a.p == was && allocs == before);  // fits: nothing happens
        CHECK(a.ensure(2000) == hipSuccess && a.bytes == 2500 && live == 1);    // grew: one block, the old one freed
        PinBuf p;
        CHECK(p.ensure(1000) == hipSuccess && p.bytes == 1250 && live == 2);
        CHECK(p.ensure(4000) == hipSuccess && p.bytes == 5000 && live == 2);
    }
    CHECK(live == 0);
    {  // the request with slack fails: the retry asks for exactly `need`
        DevBuf a;
        fail_mask = 1;
        CHECK(a.ensure(1000) == hipSuccess && a.bytes == 1000 && last_size == 1000 && live == 1);
        fail_mask = 3;  // both fail: empty, and usable afterwards
        CHECK(a.ensure(5000) == hipErrorOutOfMemory && a.p == nullptr && a.bytes == 0 && live == 0);
        CHECK(a.ensure(16) == hipSuccess && a.bytes == 20 && live == 1);
        PinBuf p;
        fail_mask = 1;
        CHECK(p.ensure(64) == hipErrorOutOfMemory && p.p == nullptr && p.bytes == 0);
        CHECK(p.ensure(64) == hipSuccess && p.bytes == 80);
    }
    CHECK(live == 0);
    {  // release twice; exact sizes exactly and replaces what was held
        DevBuf a;
        PinBuf p;
        CHECK(a.ensure(10) == hipSuccess && p.ensure(10) == hipSuccess);
        a.release();
        a.release();
        p.release();
        p.release();
        CHECK(live == 0 && a.p == nullptr && a.bytes == 0 && p.p == nullptr && p.bytes == 0);
        CHECK(a.exact(1000) == hipSuccess && a.bytes == 1000 && last_size == 1000 && live == 1);
        CHECK(a.exact(300) == hipSuccess && a.bytes == 300 && last_size == 300 && live == 1);
        fail_mask = 1;
        CHECK(a.exact(300) == hipErrorOutOfMemory && a.p == nullptr && a.bytes == 0 && live == 0);
        CHECK(a.as<int>() == nullptr);
    }
    CHECK(live == 0);
    {  // an abandoned capacity change drains the stream while its blocks are still allocated, then frees them
        drains = 0;
        {
            Staged<Two> nb(nullptr);
            CHECK(nb.a.exact(64) == hipSuccess && nb.b.exact(64) == hipSuccess && live == 2);
        }
        CHECK(drains == 1 && live_at_drain == 2 && live == 0);
        Two kept;
        {  // a committed one hands its blocks over
            Staged<Two> nb(nullptr);
            CHECK(nb.a.exact(64) == hipSuccess && nb.b.exact(64) == hipSuccess);
            kept = std::move(nb);
            CHECK(nb.a.p == nullptr && nb.b.p == nullptr);
        }
        CHECK(live == 2 && kept.a.bytes == 64);
        Staged<DevBuf> one(nullptr);
        CHECK(one.exact(32) == hipSuccess);
        kept.a = std::move(one);
        CHECK(live == 2 && kept.a.bytes == 32 && one.p == nullptr);
    }
    CHECK(live == 0);
    {  // a field list measures over no block (no pointer, no arithmetic on null) and carves over one: same offsets, same size
        mlvdb::ListBlock a, b;
        auto fields = [](mlvdb::Carver& c, mlvdb::ListBlock& l, mlvdb::ListBlock& m) {
            l.take(c, 5, 3);  // 5 * (8 + 8 + 4) + 3 * 4 = 112 bytes
            c.take<char>(3);
            c.pad_to(8);      // 115 -> 120: the next block's doubles lie aligned
            m.take(c, 2, 1);  // 2 * 20 + 4 = 44
        };
        mlvdb::Carver measure;
        fields(measure, a, b);
        CHECK(measure.at == 164 && !measure.misaligned);
        CHECK(a.d64 == nullptr && a.lab == nullptr && a.dist == nullptr && a.cnt == nullptr && b.d64 == nullptr);
        alignas(8) static char block[164];
        mlvdb::Carver carve{block};
        fields(carve, a, b);
        CHECK(carve.at == measure.at && !carve.misaligned);
        CHECK((char*)a.d64 == block && (char*)a.lab == block + 40 && (char*)a.dist == block + 80 && (char*)a.cnt == block + 100);
        CHECK((char*)b.d64 == block + 120 && (char*)(b.cnt + 1) == block + 164);
        b.cnt[0] = 7;  // the last field's last value is inside the block (ASan)
        mlvdb::Carver odd;  // an 8-byte field behind an odd count of 4-byte ones: flagged, not rounded
        odd.take<float>(3);
        odd.take<double>(1);
        CHECK(odd.misaligned && odd.at == 20);
        mlvdb::Carver bytes;  // ... and a byte field needs no alignment
        bytes.take<int64_t>(2);
        bytes.take<unsigned char>(5);
        CHECK(!bytes.misaligned && bytes.at == 21);
    }
    if (failures) return 1;
    std::puts("device_memory ok");
    return 0;
}
