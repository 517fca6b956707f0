// sgx_maxima.hpp -- the K strongest spectral maxima of a row (include/sgx.h: sgx_maxima_batch, sgx_maxima_mags): the key that orders the
// candidates, shared by the kernel and the host launch, and the launch itself.
//
// A candidate is an interior element j (1 <= j <= M - 2) with m[j] > m[j-1], m[j] >= m[j+1] and m[j] >= floor.  Candidates are ordered by
// descending m[j], ties by ascending j.  Magnitudes are >= +0, so their float bits order as unsigned integers, and a candidate's value is
// > m[j-1] >= +0: its bits are not zero.  One unsigned 64-bit key therefore carries the whole order,
//     key = (float bits of m[j]) << 32 | (0xffffffff - j),
// unique per row, larger = earlier in the result, and 0 is free to mean "no candidate".  That order is the definition: the launch
// geometry, the tile length and the lane that holds an element do not enter it.
#pragma once

#include "sgx_internal.hpp"

namespace sgx {
namespace maxima {

constexpr uint32_t kMaxK = 64;          // include/sgx.h fixes it: result r of a row lives in lane r of the wave that owns the row
constexpr unsigned long long kNone = 0;   // the key of an element that is no candidate

__host__ __device__ inline unsigned long long make_key(uint32_t value_bits, uint32_t j)
{
    return ((unsigned long long)value_bits << 32) | (unsigned long long)(0xffffffffu - j);
}
__host__ __device__ inline uint32_t key_element(unsigned long long key) { return 0xffffffffu - (uint32_t)key; }

// rows [n_rows][M] of (l, r) magnitudes, n_rows = columns * pairs -> d_max [n_rows][2][k][4] (16-byte aligned); 1 <= k <= kMaxK
hipError_t launch_maxima(const sgx_ctx *c, const float *d_rows, size_t n_rows, uint32_t k, float floor, float *d_max);   // sgx_maxima.hip

}  // namespace maxima
}  // namespace sgx
