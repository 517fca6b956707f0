// sgx_rolloff.hip -- the kernel of sgx_rolloff_batch / sgx_rolloff_mags (include/sgx.h): per (frame, pair) row of (l, r) magnitudes in
// device memory, the first element at which the cumulative value c[.] of sgx_rolloff.hpp reaches each share of the row's total, both
// sides from the same float2 loads.
//
// One wave (a workgroup of its own) owns a row and takes it in tiles of 64 segments x 32 elements.  The loads are those of
// sgx_maxima.hip: element e of lane l is j = tile + 64 e + l, a coalesced 512-byte float2 access.  The definition gives a lane the 32
// CONSECUTIVE elements of one segment, so the tile goes through LDS once: written as loaded, read back as lane l's segment l at a pitch
// of 33 float2 (dwords 66 l + 2 i: the 32 lanes of a ds_read_b64 group fall on 64 different banks, the 16 lanes of a ds_write_b64 group
// on 32).  Elements beyond the row are +0, which changes no sum: rn(a + +0) = a.  A lane then holds its segment's chain s[i] in
// registers.  The offsets o[.] are one chain over the 64 lane totals in lane order, continued from the tile before: every lane runs the
// same chain over readlane values and keeps the value at its own step.  A row of one tile knows its total T after that chain and
// searches at once; a longer row runs the tiles twice, first for T alone (the recomputation is the same arithmetic, so the same bits).
// The search needs no per-element loop: c[.] never decreases, so a ballot over the lanes' last c finds the segment, the segment's 32
// values of c (stored over the lane's own LDS slots) are read by 32 lanes and a second ballot finds the element; c[j*] and c[j* - 1]
// are two more LDS words.  Share i's record lives in lane i and leaves as one float4 per lane and side.
#include "sgx_rolloff.hpp"

namespace sgx {
namespace rolloff {

namespace {
constexpr uint32_t kLanes = 64, kTile = kLanes * kSegment, kPitch = kSegment + 1;   // (float2 words between two lanes' segments in LDS)

__device__ __forceinline__ float lane_value(float x, uint32_t lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), (int)lane));
}
__device__ __forceinline__ float side(const float2 &v, int s) { return s ? v.y : v.x; }
__device__ __forceinline__ uint32_t slot(uint32_t j) { return j + j / kSegment; }   // element j of the tile in LDS

// One tile of `len` elements at m: lane l's chain s[.] over segment l, and its offset o (returned), the chain over the lane totals
// continued from `carry`, which leaves as the cumulative value of the tile's last element.
template <uint32_t Power>
__device__ __forceinline__ float2 tile_chains(const float2 *__restrict__ m, uint32_t len, float2 *lds, uint32_t lane, float2 (&s)[kSegment],
                                              float2 &carry)
{
    float2 v[kSegment];
#pragma unroll
    for (uint32_t e = 0; e < kSegment; ++e) {
        const uint32_t i = e * kLanes + lane;
        v[e] = i < len ? m[i] : make_float2(0.0f, 0.0f);
    }
    __syncthreads();   // (the search of the tile before has read what it needs)
#pragma unroll
    for (uint32_t e = 0; e < kSegment; ++e) lds[slot(e * kLanes + lane)] = v[e];
    __syncthreads();
    float2 run = make_float2(0.0f, 0.0f);
#pragma unroll
    for (uint32_t i = 0; i < kSegment; ++i) {
        float2 x = lds[lane * kPitch + i];
        if (Power == 2) x = make_float2(__fmul_rn(x.x, x.x), __fmul_rn(x.y, x.y));   // (never contracted into the add)
        run = make_float2(__fadd_rn(run.x, x.x), __fadd_rn(run.y, x.y));
        s[i] = run;
    }
    // segments beyond the row have a total of +0 and leave the chain where it is: it stops at the last one that holds an element
    const uint32_t segments = (len + kSegment - 1) / kSegment;
    float2 o = make_float2(0.0f, 0.0f);
    for (uint32_t l0 = 0; l0 < segments; l0 += 8) {   // (in steps of 8: a step beyond `segments` adds +0)
#pragma unroll
        for (uint32_t l = l0; l < l0 + 8; ++l) {
            if (lane == l) o = carry;
            carry = make_float2(__fadd_rn(carry.x, lane_value(run.x, l)), __fadd_rn(carry.y, lane_value(run.y, l)));
        }
    }
    if (lane >= segments) o = carry;
    return o;
}

template <uint32_t Power>
__global__ void __launch_bounds__(kLanes) rolloff_kernel(const float2 *__restrict__ rows, unsigned long long n_rows, uint32_t M, Shares shares,
                                                         uint32_t n_p, float4 *__restrict__ out)
{
    __shared__ float2 lds[kLanes * kPitch];
    const uint32_t lane = threadIdx.x;
    for (unsigned long long row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const float2 *m = rows + row * M;
        float2 s[kSegment], total = make_float2(0.0f, 0.0f);
        if (M > kTile) {   // T before the search: the tiles once for their carries alone
            for (uint32_t t0 = 0; t0 < M; t0 += kTile) tile_chains<Power>(m + t0, M - t0 < kTile ? M - t0 : kTile, lds, lane, s, total);
        }
        float4 rec[2] = {make_float4(0.0f, 0.0f, 0.0f, 0.0f), make_float4(0.0f, 0.0f, 0.0f, 0.0f)};   // lane i: share i, per side
        uint32_t pending[2] = {0, 0};                                                              // shares not yet found (uniform)
        float2 carry = make_float2(0.0f, 0.0f);
        for (uint32_t t0 = 0; t0 < M; t0 += kTile) {
            const float2 before = carry;   // c[t0 - 1], +0 at the row's start
            const float2 o = tile_chains<Power>(m + t0, M - t0 < kTile ? M - t0 : kTile, lds, lane, s, carry);
            if (t0 == 0) {
                if (M <= kTile) total = carry;
                pending[0] = total.x > 0.0f ? (1u << n_p) - 1 : 0;   // !(T > 0): the record stays (0, 0, 0, T)
                pending[1] = total.y > 0.0f ? (1u << n_p) - 1 : 0;
            }
            if (!(pending[0] | pending[1])) break;
            // c[.] over the lane's own slots, the last one kept
            float2 last = o;
#pragma unroll
            for (uint32_t i = 0; i < kSegment; ++i) {
                last = make_float2(__fadd_rn(o.x, s[i].x), __fadd_rn(o.y, s[i].y));
                lds[lane * kPitch + i] = last;
            }
            __syncthreads();
#pragma unroll
            for (int sd = 0; sd < 2; ++sd) {
                for (uint32_t i = 0; i < n_p; ++i) {
                    if (!(pending[sd] >> i & 1)) continue;
                    const float thr = __fmul_rn(shares.p[i], side(total, sd));
                    const unsigned long long reached = __ballot(side(last, sd) >= thr);
                    if (!reached) continue;   // (uniform) the crossing lies in a later tile
                    const uint32_t seg = (uint32_t)__builtin_ctzll(reached);
                    const float2 c = lds[seg * kPitch + (lane & (kSegment - 1))];
                    const uint32_t in_seg = (uint32_t)__ballot(side(c, sd) >= thr);   // (lanes 32 .. 63 repeat lanes 0 .. 31)
                    const uint32_t j = seg * kSegment + (uint32_t)__builtin_ctz(in_seg);
                    const float at = side(lds[slot(j)], sd), below = j > 0 ? side(lds[slot(j - 1)], sd) : side(before, sd);
                    if (lane == i) rec[sd] = make_float4((float)(t0 + j + 1), below, at, 0.0f);
                    pending[sd] &= ~(1u << i);
                }
            }
        }
        if (lane < n_p) {
#pragma unroll
            for (int sd = 0; sd < 2; ++sd) {
                rec[sd].w = side(total, sd);
                out[(row * 2 + (unsigned long long)sd) * n_p + lane] = rec[sd];
            }
        }
    }
}
}  // namespace

hipError_t launch_rolloff(const sgx_ctx *c, const float *d_rows, size_t n_rows, uint32_t power, const Shares &shares, uint32_t n_p, float *d_out)
{
    if (n_rows == 0) return hipSuccess;
    if ((power != 1 && power != 2) || n_p < 1 || n_p > kMaxShares || c->M < 1) return hipErrorInvalidValue;
    // (rows beyond the grid are taken by striding: the grid is a matter of speed only)
    const unsigned long long cap = 1ull << 20;
    const dim3 grid((unsigned)((unsigned long long)n_rows < cap ? n_rows : cap));
    const float2 *rows = reinterpret_cast<const float2 *>(d_rows);
    float4 *out = reinterpret_cast<float4 *>(d_out);
    if (power == 1)
        hipLaunchKernelGGL(rolloff_kernel<1>, grid, dim3(kLanes), 0, c->stream, rows, (unsigned long long)n_rows, (uint32_t)c->M, shares, n_p, out);
    else
        hipLaunchKernelGGL(rolloff_kernel<2>, grid, dim3(kLanes), 0, c->stream, rows, (unsigned long long)n_rows, (uint32_t)c->M, shares, n_p, out);
    return hipGetLastError();
}

}  // namespace rolloff
}  // namespace sgx
