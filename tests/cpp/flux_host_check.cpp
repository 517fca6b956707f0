// The range arithmetic of sgx_flux_batch (csrc/flux_host.hpp) as a stand-alone program: built with the address and undefined-behaviour
// sanitizers by tests/test_flux_host.py and run directly.  It walks the ranges of many calls the way the host dispatch does and keeps a
// map of the workspace's rows on the heap, exactly sized, so that a range that asks for a row too many is an overflow the sanitizer sees.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "flux_host.hpp"

namespace flux = sgx::flux;

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
            ++failures;                                                              \
        }                                                                            \
    } while (0)

// one call: its ranges tile [first_frame, first_frame + n), every range's back is min(lag, a), no range exceeds the cap, every frame's
// predecessor lies in the same range's rows (or the frame has none), and the workspace the call grows holds every range
static size_t walk(size_t first_frame, size_t n, uint32_t lag, size_t cap)
{
    const size_t end = first_frame + n, grown = flux::rows_needed(first_frame, n, lag, cap);
    CHECK(grown <= cap);
    std::vector<unsigned char> rows(grown, 0);   // the workspace, a byte per row
    size_t next = first_frame, ranges = 0;
    for (size_t a = first_frame; a < end;) {
        const flux::Range r = flux::range_at(a, end, lag, cap);
        CHECK(r.a == a && a == next);
        CHECK(r.back == (a < lag ? a : (size_t)lag));
        CHECK(r.m >= 1 && r.back + r.m <= cap && r.back + r.m <= grown);
        CHECK(a + r.m <= end);
        CHECK(a + r.m == end || r.back + r.m == cap);   // only the call's last range is short
        for (size_t i = 0; i < r.back + r.m; ++i) rows[i] = 1;   // rows_to_workspace(a - back, back + m)
        // the first and the last frame of the range, as the kernel finds their rows
        for (size_t f : {(size_t)0, r.m - 1}) {
            const size_t row = r.back + f, t = a + f;
            CHECK((row < lag) == (t < lag));                     // no predecessor in the range exactly where the stream has none
            if (row >= lag) {
                CHECK(rows[row - lag] == 1 && rows[row] == 1);
                CHECK(a - r.back + (row - lag) == t - lag);      // and it is frame t - lag
            }
        }
        next = a + r.m;
        a += r.m;
        ++ranges;
    }
    CHECK(next == end);
    return ranges;
}

int main()
{
    // the caps the header and the issue state
    CHECK(flux::kWorkspaceBytes == (size_t)192 << 20);
    CHECK(flux::max_lag((size_t)1 * 2047 * 8) == 64);                      // W 2048, two channels
    CHECK(flux::max_lag((size_t)1 * ((1u << 20) - 1) * 8) == 23);          // W 2^20, two channels
    CHECK(flux::max_lag((size_t)2 * ((1u << 20) - 1) * 8) == 11);          // W 2^20, four channels
    CHECK(flux::max_lag(((size_t)96 << 20) + 8) == 0);                     // fewer than two rows fit
    CHECK(flux::max_lag((size_t)96 << 20) == 1);
    CHECK(flux::max_lag((size_t)400 << 20) == 0 && flux::max_lag(0) == 0);
    CHECK(flux::max_lag((size_t)1 * 3 * 8) == 64);
    for (size_t cap = 2; cap <= 70; ++cap) CHECK(flux::max_lag(flux::kWorkspaceBytes / cap) == (cap - 1 < 64 ? cap - 1 : 64));
    std::printf("max_lag ok\n");

    // every small call at small caps: lag up to the cap's own limit
    size_t calls = 0;
    for (size_t cap = 2; cap <= 9; ++cap)
        for (uint32_t lag = 1; lag < cap && lag <= flux::kMaxLag; ++lag)
            for (size_t first = 0; first <= 12; ++first)
                for (size_t n = 1; n <= 30; ++n) {
                    const size_t ranges = walk(first, n, lag, cap);
                    CHECK(ranges >= (n + cap - 1) / cap);
                    ++calls;
                }
    std::printf("small calls ok: %zu\n", calls);

    // the caps of real contexts: W 2048 mono (12 294 rows), W 8192 with 8 channels (768), W 2^20 with two (24)
    const size_t caps[] = {flux::row_cap((size_t)2047 * 8), flux::row_cap((size_t)4 * 8191 * 8), flux::row_cap((size_t)((1u << 20) - 1) * 8)};
    CHECK(caps[0] == 12294 && caps[1] == 768 && caps[2] == 24);
    for (size_t cap : caps)
        for (uint32_t lag : {1u, 2u, 23u, 64u}) {
            if (lag > cap - 1) continue;
            for (size_t first : {(size_t)0, (size_t)1, (size_t)lag - 1, (size_t)lag, (size_t)lag + 1, (size_t)17, cap - 1, cap, cap + 1})
                for (size_t n : {(size_t)1, cap - lag - 1, cap - lag, cap - lag + 1, cap, 3 * cap + 5}) {
                    if (n == 0) continue;
                    walk(first, n, lag, cap);
                }
        }
    CHECK(walk(0, 800, 64, 768) == 2 && walk(0, 768, 64, 768) == 1 && walk(0, 769, 64, 768) == 2 && walk(100, 2000, 64, 768) == 3);
    std::printf("context caps ok\n");

    // frame indices around 2^32
    if (sizeof(size_t) >= 8) {
        const size_t big = (size_t)1 << 32;
        for (size_t first : {big - 70, big - 64, big - 1, big, big + 1, (big << 8) + 3})
            for (uint32_t lag : {1u, 64u})
                for (size_t cap : {(size_t)65, (size_t)768, (size_t)12294}) {
                    walk(first, 1, lag, cap);
                    walk(first, 200, lag, cap);
                    walk(first, 30000, lag, cap);
                }
        const flux::Range r = flux::range_at(big - 1, big + 5000, 64, 768);
        CHECK(r.back == 64 && r.m == 704 && r.a - r.back == big - 65);
        std::printf("far frames ok\n");
    }
    std::printf(failures ? "flux host FAILED\n" : "flux host ok\n");
    return failures ? 1 : 0;
}
