// large_plan.hpp -- the plan rule of the multi-pass transform (stft_large.hip): host code only, no HIP, so that the CPU suite can
// compile it with g++ and check it for every window length.
//
//   2W 2-3-5-7-smooth:  the transform of exactly P = 2W points, P = N1 x N2 with N1 <= N2 <= kMaxSub, N1 the largest divisor <= sqrt(P)
//   otherwise:          chirp-z over L = pow2 >= 3W - 1 (the convolution of W non-zero inputs with P + W - 1 chirp values),
//                       L = N1 x N2 with N1 = 2^floor(log2(L) / 2)
//
// A sub-transform of N points runs in LDS as Stockham stages of radix 4, 2, 3, 5 and 7 (sub_radices); a workgroup holds one sub-transform
// of up to kBlockPts points, or several short ones (kBlockPts / 2 points), twice: at most 2 x 4096 x 8 B = 64 KiB of LDS.
#pragma once

#include <cstdint>
#include <cstddef>
#include <initializer_list>

namespace sgx {
namespace large {

constexpr uint32_t kMaxSub = 4096;                // longest sub-transform
constexpr uint32_t kBlockPts = 4096;              // the most complex points a workgroup holds (ping-pong: 64 KiB of LDS)
constexpr uint32_t kMaxW = 1u << 20;              // 2W <= 2^21
constexpr uint32_t kMaxStages = 16;
constexpr size_t kScratchBytes = (size_t)64 << 20;  // the context's scratch: one chunk's intermediate (Infinity Cache: 256 MiB)

struct Plan {
    uint32_t W = 0, P = 0;
    uint32_t L = 0;        // length of the transforms the passes run: P, or the chirp-z convolution length
    uint32_t N1 = 0, N2 = 0;
    bool chirp = false;
};

// radices of an N-point sub-transform, first stage first (4s, then a 2, then 3, 5, 7); 0 stages if N has another prime factor
inline uint32_t sub_radices(uint32_t N, uint8_t out[kMaxStages])
{
    if (N < 2 || N > kMaxSub) return 0;
    uint32_t n = N, k = 0;
    while (n % 4 == 0) { out[k++] = 4; n /= 4; }
    if (n % 2 == 0) { out[k++] = 2; n /= 2; }
    for (uint32_t f : {3u, 5u, 7u})
        while (n % f == 0) { out[k++] = (uint8_t)f; n /= f; }
    return n == 1 && k <= kMaxStages ? k : 0;
}

inline bool smooth7(uint64_t n)
{
    if (n == 0) return false;
    for (uint64_t f : {2u, 3u, 5u, 7u})
        while (n % f == 0) n /= f;
    return n == 1;
}

// the plan for window W (false: W out of range)
inline bool make_plan(uint32_t W, Plan &pl)
{
    pl = Plan{};
    if (W < 4 || W > kMaxW) return false;
    pl.W = W;
    pl.P = 2 * W;
    if (smooth7(pl.P)) {
        pl.L = pl.P;
        for (uint32_t d = 1; (uint64_t)d * d <= pl.P; ++d)
            if (pl.P % d == 0 && pl.P / d <= kMaxSub) pl.N1 = d;   // largest divisor <= sqrt(P) whose cofactor fits
    } else {
        pl.chirp = true;
        pl.L = 1;
        while (pl.L < 3 * W - 1) pl.L <<= 1;
        uint32_t lg = 0;
        while ((1u << lg) < pl.L) ++lg;
        pl.N1 = 1u << (lg / 2);
    }
    if (pl.N1 < 2) return false;
    pl.N2 = pl.L / pl.N1;
    uint8_t r[kMaxStages];
    return pl.N1 * pl.N2 == pl.L && sub_radices(pl.N1, r) && sub_radices(pl.N2, r);
}

// scratch bytes per transform: chirp-z works in place on one L-point buffer; the direct path writes its rows pass into a second P-point
// buffer in natural order (the split pairs bin k with bin P - k, which lies in another row)
inline size_t scratch_per_transform(const Plan &pl) { return (size_t)pl.L * 8 * (pl.chirp ? 1 : 2); }

}  // namespace large
}  // namespace sgx
