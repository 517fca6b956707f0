// sgx_quantile.hpp -- per-bin order statistics over groups of frames (include/sgx.h: sgx_quantile_batch, sgx_quantile_mags): the key that
// orders float32 words, the rank rule, the one device function that forms a result, and the launch.
//
// Words are ordered by key(u) = u ^ (u >> 31 ? 0xffffffff : 0x80000000) of their bit pattern u, compared as unsigned integers:
// -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN.  The result for q is the word of rank k = floor(q * (n - 1) + 0.5) of a column's n words
// in that order, bits unchanged.  That is the definition: the path, the tile, the split of a column's frames among the waves of a
// workgroup and the launch geometry do not enter it.
#pragma once

#include <cmath>

#include "sgx_internal.hpp"

namespace sgx {
namespace quantile {

constexpr uint32_t kMaxQ = 16;           // include/sgx.h fixes it: the ranks of a call live in registers, advanced on the same read of a key
// Path A keeps a column's keys of kTile consecutive elements in LDS as [frame][element]: kTile words are one wave's lanes and 256 B of every
// row, so the lanes of a wave read consecutive banks in every step.  The four waves of a workgroup split the column's frames and add their
// counts through an exchange area of 2 (parity) x 4 (waves) x n_q x kTile words.  kLdsFrames is what 160 KiB hold beside the exchange
// area of 16 ranks: (160 KiB - 32 KiB) / 256 B.  A device that grants less than a launch needs takes Path B for it.
constexpr uint32_t kTile = 64, kWaves = 4;
constexpr uint32_t kLdsFrames = 512;
constexpr size_t kLdsCap = (size_t)160 * 1024;
constexpr size_t lds_bytes(size_t frames, uint32_t n_q) { return (frames * kTile + (size_t)2 * kWaves * n_q * kTile) * sizeof(uint32_t); }
static_assert(lds_bytes(kLdsFrames, kMaxQ) == kLdsCap, "kLdsFrames follows from the image");

__host__ __device__ inline uint32_t to_key(uint32_t u) { return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u); }
__host__ __device__ inline uint32_t from_key(uint32_t k) { return k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu); }

// the rank of q among n >= 1 words: one double product, one add, one floor (nearest rank, a half goes up)
inline size_t rank_of(double q, size_t n) { return (size_t)std::floor(q * (double)(n - 1) + 0.5); }

#ifdef __HIPCC__
// The one place a result is formed: a bitwise radix select on the key, bit 31 down to 0.  A round counts the keys that share the prefix
// found so far and have this bit clear; each rank stays below that count, or subtracts it and sets the bit.  keys(t) is key t of this
// element's column -- from LDS on path A, from the rows where they lie on path B; [t_lo, t_hi) are the frames this thread counts and
// combine(cnt, round) adds the counts of the threads that share the element (path A: the four waves; path B: nobody).  Every rank is
// advanced on the same read of a key.  On return prefix[i] is the key of rank[i].
template <int NQ, typename Count, typename Keys, typename Combine>
__device__ __forceinline__ void select_keys(const Keys &keys, Count t_lo, Count t_hi, Count (&rank)[NQ], const Combine &combine, uint32_t (&prefix)[NQ])
{
#pragma unroll
    for (int i = 0; i < NQ; ++i) prefix[i] = 0;
    for (uint32_t round = 0; round < 32; ++round) {
        const uint32_t b = 31 - round;
        uint32_t want[NQ];   // what key >> b is for a key that shares the prefix and has bit b clear
        Count cnt[NQ];
#pragma unroll
        for (int i = 0; i < NQ; ++i) { want[i] = prefix[i] >> b; cnt[i] = 0; }
#pragma unroll 8
        for (Count t = t_lo; t < t_hi; ++t) {
            const uint32_t d = keys(t) >> b;
#pragma unroll
            for (int i = 0; i < NQ; ++i) cnt[i] += d == want[i] ? 1 : 0;
        }
        combine(cnt, round);
#pragma unroll
        for (int i = 0; i < NQ; ++i)
            if (rank[i] >= cnt[i]) { rank[i] -= cnt[i]; prefix[i] |= 1u << b; }
    }
}
#endif

// One launch: rows [n_frames][row_floats] in device memory, columns of g frames (the last one may be short), the n_q ranks of a full
// column and of the short last one, into d_out [columns][n_q][row_floats].  1 <= g <= n_frames, 1 <= n_q <= kMaxQ.
struct Piece {
    const float *rows;
    float *out;
    unsigned long long n_frames, g, row_floats;
    uint32_t n_q;
    unsigned long long rank_full[kMaxQ], rank_last[kMaxQ];
};
// (a column of at most kLdsFrames frames whose image the device grants is selected in LDS, path A; any other where its rows lie, path B)
hipError_t launch_quantile(const sgx_ctx *c, const float *d_rows, size_t n_frames, size_t g, const double *q, uint32_t n_q, float *d_out);

}  // namespace quantile
}  // namespace sgx
