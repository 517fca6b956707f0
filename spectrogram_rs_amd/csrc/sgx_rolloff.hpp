// sgx_rolloff.hpp -- where the running sum of a row crosses a share of its total (include/sgx.h: sgx_rolloff_batch, sgx_rolloff_mags): the
// constants of the definition, shared by the kernel and the host checks, and the launch itself.
//
// The cumulative value of element j = 32 b + i is c[j] = rn(o[b] + s[b][i]): s[b][.] one chain of float32 adds from +0 over the 32
// elements of segment b, o[.] one chain of float32 adds from +0 over the segment totals.  The segment length is part of the definition:
// the launch geometry, the tile length and the lane that holds a segment do not enter it.
#pragma once

#include "sgx_internal.hpp"

namespace sgx {
namespace rolloff {

constexpr uint32_t kSegment = 32;   // include/sgx.h fixes it: S, the elements of one chain of adds
constexpr uint32_t kMaxShares = 8;  // include/sgx.h fixes it: n_p

struct Shares {
    float p[kMaxShares];
};

// rows [n_rows][M] of (l, r) magnitudes, n_rows = columns * pairs -> d_out [n_rows][2][n_p][4] (16-byte aligned); power 1 or 2,
// 1 <= n_p <= kMaxShares, every p in (0, 1]
hipError_t launch_rolloff(const sgx_ctx *c, const float *d_rows, size_t n_rows, uint32_t power, const Shares &shares, uint32_t n_p,
                          float *d_out);   // sgx_rolloff.hip

}  // namespace rolloff
}  // namespace sgx
