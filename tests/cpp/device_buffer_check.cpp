// device_buffer_check.cpp -- csrc/device_buffer.hpp against a runtime of this file's own (tests/test_device_buffer.py builds it with
// g++ -fsanitize=address,undefined and runs it; no HIP library is linked): hipMalloc, hipFree, hipMemcpy and hipStreamSynchronize on
// malloc'd memory, with a count of live allocations, a log of frees and a switch that fails the next allocation.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "device_buffer.hpp"

namespace {
std::set<void *> g_live;
long g_mallocs = 0, g_frees = 0, g_bad_frees = 0, g_syncs = 0;
bool g_fail_next = false;
int g_failed = 0;
}  // namespace

extern "C" {
hipError_t hipMalloc(void **ptr, size_t size)
{
    if (g_fail_next) { g_fail_next = false; *ptr = nullptr; return hipErrorOutOfMemory; }
    *ptr = std::malloc(size ? size : 1);
    if (!*ptr) return hipErrorOutOfMemory;
    g_live.insert(*ptr);
    ++g_mallocs;
    return hipSuccess;
}
hipError_t hipFree(void *ptr)
{
    if (!ptr) return hipSuccess;
    if (!g_live.erase(ptr)) { ++g_bad_frees; return hipErrorInvalidValue; }   // a second free, or of something never allocated
    ++g_frees;
    std::free(ptr);
    return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind)
{
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t)
{
    ++g_syncs;
    return hipSuccess;
}
}

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { ++g_failed; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } \
    } while (0)

using sgx::DeviceBuffer;

static void upload_returns_the_bytes()
{
    std::vector<float> v(1000);
    for (size_t i = 0; i < v.size(); ++i) v[i] = (float)i * 0.25f - 3.0f;
    DeviceBuffer<float> b;
    CHECK(b.get() == nullptr && b.size() == 0);
    CHECK(b.upload(v) == hipSuccess);
    CHECK(b.size() == v.size() && b.get() && std::memcmp(b.get(), v.data(), v.size() * sizeof(float)) == 0);
    // a second table in place of the first: the first is freed, once
    const long frees = g_frees;
    const double w[3] = {1.5, -2.5, 1e300};
    DeviceBuffer<double> d;
    CHECK(d.upload(w, 3) == hipSuccess && d.size() == 3 && std::memcmp(d.get(), w, sizeof w) == 0);
    CHECK(b.upload(v.data(), 10) == hipSuccess && b.size() == 10 && g_frees == frees + 1 && std::memcmp(b.get(), v.data(), 10 * sizeof(float)) == 0);
    CHECK(g_live.size() == 2);
    b.reset();
    CHECK(b.get() == nullptr && b.size() == 0 && g_live.size() == 1);
    b.reset();   // (nothing to free)
    CHECK(g_bad_frees == 0);
    std::printf("upload ok\n");
}

static void moves_transfer_ownership()
{
    const long mallocs = g_mallocs, frees = g_frees;
    {
        DeviceBuffer<int> a;
        CHECK(a.alloc(64) == hipSuccess && a.size() == 64);
        int *const pa = a.get();
        DeviceBuffer<int> b(std::move(a));
        CHECK(a.get() == nullptr && a.size() == 0 && b.get() == pa && b.size() == 64);
        DeviceBuffer<int> c;
        CHECK(c.alloc(8) == hipSuccess);
        int *const pc = c.get();
        c = std::move(b);   // c's own allocation is freed, b's moves in
        CHECK(b.get() == nullptr && b.size() == 0 && c.get() == pa && c.size() == 64 && !g_live.count(pc) && g_live.count(pa));
        DeviceBuffer<int> d;
        CHECK(d.alloc(16) == hipSuccess);
        int *const pd = d.get();
        std::swap(c, d);    // the live ring's ping-pong
        CHECK(c.get() == pd && c.size() == 16 && d.get() == pa && d.size() == 64);
        CHECK(g_frees == frees + 1);
    }
    CHECK(g_mallocs == mallocs + 3 && g_frees == frees + 3 && g_bad_frees == 0);   // one free per allocation, none for a moved-from object
    std::printf("move ok\n");
}

static void grow_keeps_reallocates_and_fails_clean()
{
    const hipStream_t stream = nullptr;
    DeviceBuffer<float> b;
    long syncs = g_syncs;
    CHECK(b.grow(stream, 0) == hipSuccess && b.get() == nullptr && g_syncs == syncs);
    CHECK(b.grow(stream, 100) == hipSuccess && b.size() == 100 && g_syncs == syncs + 1);   // the stream is waited for before the old buffer goes
    float *const p = b.get();
    syncs = g_syncs;
    const long mallocs = g_mallocs;
    CHECK(b.grow(stream, 100) == hipSuccess && b.grow(stream, 7) == hipSuccess && b.grow(stream, 0) == hipSuccess);
    CHECK(b.get() == p && b.size() == 100 && g_syncs == syncs && g_mallocs == mallocs);    // kept: no wait, no allocation
    CHECK(b.grow(stream, 101) == hipSuccess && b.size() == 101 && g_syncs == syncs + 1 && g_mallocs == mallocs + 1 && !g_live.count(p));
    b.get()[100] = 1.0f;   // (the last element is the buffer's: the sanitizer would say otherwise)
    float *const q = b.get();
    const long frees = g_frees;
    g_fail_next = true;
    CHECK(b.grow(stream, 5000) == hipErrorOutOfMemory);
    CHECK(b.get() == nullptr && b.size() == 0 && !g_live.count(q) && g_frees == frees + 1 && g_bad_frees == 0);   // null, size 0, the old one freed once
    CHECK(b.grow(stream, 5) == hipSuccess && b.size() == 5);   // and usable again
    g_fail_next = true;
    DeviceBuffer<float> c;
    CHECK(c.alloc(3) == hipErrorOutOfMemory && c.get() == nullptr && c.size() == 0);
    std::printf("grow ok\n");
}

static void empty_tables_follow_their_rule()
{
    const std::vector<float> none;
    const long mallocs = g_mallocs;
    DeviceBuffer<float> b;
    CHECK(b.upload(std::vector<float>{1.0f, 2.0f}) == hipSuccess && b.get());
    CHECK(b.upload(none) == hipSuccess && b.get() == nullptr && b.size() == 0);            // upload: null for an empty table, the old one gone
    CHECK(b.upload(nullptr, 0) == hipSuccess && b.get() == nullptr && g_mallocs == mallocs + 1);
    CHECK(b.alloc(0) == hipSuccess && b.get() == nullptr && b.size() == 0);
    DeviceBuffer<float> one;
    CHECK(one.upload_at_least_one(none) == hipSuccess && one.get() && one.size() == 1);     // upload_at_least_one: one element
    one.get()[0] = 0.0f;
    const std::vector<float> three{3.0f, 4.0f, 5.0f};
    CHECK(one.upload_at_least_one(three) == hipSuccess && one.size() == 3 && std::memcmp(one.get(), three.data(), 12) == 0);
    std::printf("empty ok\n");
}

int main()
{
    upload_returns_the_bytes();
    moves_transfer_ownership();
    grow_keeps_reallocates_and_fails_clean();
    empty_tables_follow_their_rule();
    CHECK(g_live.empty() && g_mallocs == g_frees && g_bad_frees == 0);
    std::printf("%ld allocations, %ld frees, %zu live\n", g_mallocs, g_frees, g_live.size());
    if (g_failed) return 1;
    std::printf("device buffer ok\n");
    return 0;
}
