// The plan rule of the multi-pass transform (csrc/large_plan.hpp) for every W it may be asked for: prints one summary line, exits non-zero
// on the first W whose plan is wrong.
#include <cstdio>

#include "large_plan.hpp"

using namespace sgx::large;

static bool in_lds(uint32_t W)   // the lengths the in-LDS kernels serve (sgx_create): no plan needed there, but one must exist anyway
{
    const uint32_t P = 2 * W;
    return ((P & (P - 1)) == 0 && P <= 16384) || 3ull * W - 1 <= 16384 || (P <= 20480 && smooth7(P));
}

int main()
{
    unsigned long long n_direct = 0, n_chirp = 0, n_large = 0, max_l = 0;
    for (uint32_t W = 4; W <= kMaxW; ++W) {
        Plan pl;
        if (!make_plan(W, pl)) { std::printf("FAIL W %u: no plan\n", W); return 1; }
        uint8_t r1[kMaxStages], r2[kMaxStages];
        const uint32_t s1 = sub_radices(pl.N1, r1), s2 = sub_radices(pl.N2, r2);
        if (!s1 || !s2) { std::printf("FAIL W %u: factor %u x %u not a stage-engine length\n", W, pl.N1, pl.N2); return 1; }
        for (uint32_t i = 0; i < s1; ++i) if (r1[i] != 2 && r1[i] != 3 && r1[i] != 4 && r1[i] != 5 && r1[i] != 7) return 1;
        for (uint32_t i = 0; i < s2; ++i) if (r2[i] != 2 && r2[i] != 3 && r2[i] != 4 && r2[i] != 5 && r2[i] != 7) return 1;
        if ((uint64_t)pl.N1 * pl.N2 != pl.L) { std::printf("FAIL W %u: %u x %u != %u\n", W, pl.N1, pl.N2, pl.L); return 1; }
        if (pl.chirp == smooth7(2ull * W)) { std::printf("FAIL W %u: chirp-z iff 2W has a prime factor above 7\n", W); return 1; }
        if (!pl.chirp && pl.L != 2 * W) { std::printf("FAIL W %u: direct length %u != 2W\n", W, pl.L); return 1; }
        if (pl.chirp && ((uint64_t)pl.L < 3ull * W - 1 || (pl.L & (pl.L - 1)))) { std::printf("FAIL W %u: chirp-z L %u\n", W, pl.L); return 1; }
        // the LDS image of a workgroup: ping-pong over kBlockPts points, at least one whole sub-transform, within 160 KB
        if (pl.N1 > kBlockPts || pl.N2 > kBlockPts || 2ull * kBlockPts * 8 > 160 * 1024) { std::printf("FAIL W %u: LDS\n", W); return 1; }
        if (kScratchBytes / scratch_per_transform(pl) < 1) { std::printf("FAIL W %u: scratch\n", W); return 1; }
        if (!in_lds(W)) {
            ++n_large;
            (pl.chirp ? n_chirp : n_direct) += 1;
            if (pl.L > max_l) max_l = pl.L;
        }
    }
    Plan pl;
    if (make_plan(kMaxW + 1, pl) || make_plan(3, pl)) { std::printf("FAIL: out-of-range W planned\n"); return 1; }
    std::printf("plans ok: %llu lengths past the LDS, %llu direct, %llu chirp-z, longest L %llu\n", n_large, n_direct, n_chirp, max_l);
    return 0;
}
