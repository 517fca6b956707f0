// flux_host.hpp -- the host-only part of the flux calls (include/sgx.h: sgx_flux_batch, sgx_flux_max_lag): how a call's frames
// are cut into ranges whose rows, predecessors included, fit the bounded workspace.  No HIP: a plain C++ compiler builds it
// (tests/cpp/flux_host_check.cpp runs it under the sanitizers).
#pragma once

#include <cstddef>
#include <cstdint>

namespace sgx {
namespace flux {

constexpr uint32_t kMaxLag = 64;
constexpr size_t kWorkspaceBytes = (size_t)192u << 20;   // the workspace of every two-kernel route (sgx_api.hip holds its own to this)

// the rows one range may put into the workspace, head rows included: floor(workspace / bytes of one frame's rows)
inline size_t row_cap(size_t row_bytes, size_t workspace_bytes = kWorkspaceBytes) { return row_bytes ? workspace_bytes / row_bytes : 0; }

// sgx_flux_max_lag: a range holds a frame and its predecessor, so lag + 1 rows at least; 0 where fewer than two rows fit
inline uint32_t max_lag(size_t row_bytes, size_t workspace_bytes = kWorkspaceBytes)
{
    const size_t cap = row_cap(row_bytes, workspace_bytes);
    if (cap < 2) return 0;
    return cap - 1 < (size_t)kMaxLag ? (uint32_t)(cap - 1) : kMaxLag;
}

// One range: the records of frames [a, a + m) of the stream, from the rows of frames [a - back, a + m) in the workspace.
// back = min(lag, a): the frames before frame 0 do not exist, and a frame t < lag has no predecessor.
struct Range {
    size_t a, back, m;
};

// The range that starts at absolute frame a of a call that ends before frame `end` (a < end), lag <= max_lag: 1 <= m, back + m <= cap.
inline Range range_at(size_t a, size_t end, uint32_t lag, size_t cap)
{
    Range r;
    r.a = a;
    r.back = a < (size_t)lag ? a : (size_t)lag;
    const size_t room = cap - r.back, left = end - a;
    r.m = left < room ? left : room;
    return r;
}

// the rows the largest range of the call [first_frame, first_frame + n) holds: what the workspace is grown to before the first launch
inline size_t rows_needed(size_t first_frame, size_t n, uint32_t lag, size_t cap)
{
    const size_t back = first_frame < (size_t)lag ? first_frame : (size_t)lag;
    return n < cap - back ? back + n : cap;
}

}  // namespace flux
}  // namespace sgx
