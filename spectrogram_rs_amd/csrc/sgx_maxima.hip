// sgx_maxima.hip -- the selection kernel of sgx_maxima_batch / sgx_maxima_mags (include/sgx.h): the K strongest local maxima of every
// (frame, pair) row of (l, r) magnitudes in device memory, both sides from the same float2 loads.
//
// One wave owns a row.  It takes the row in tiles of 64 lanes x 32 elements: element e of lane l is j = tile + 64 e + l, so every load is
// a coalesced 512-byte float2 access and a neighbour m[j-1] / m[j+1] sits in the next lane, one DPP wave shift away (the lane at either end
// of the wave takes it from the element before / after, the tile's own ends from one float2 beside the tile).  A lane keeps, per side, the float bits of its
// candidates and 0 for everything else; the key of sgx_maxima.hpp is formed from them where it is compared.  Selection is K rounds of
// "largest key below the last one taken": a lane-local maximum, a wave maximum, the winner kept in lane r of round r.  The lane-local
// maximum is kept per group of 8 elements: a round takes the maximum of a lane's four group maxima, and only the winner's group -- the
// one group in one lane whose maximum the round has used up -- is searched again, below the key just taken (the winner's element and lane
// are uniform, so that is one scalar branch).  A row longer than a tile carries the K keys it has so far into the next tile as one more
// key per lane, so a tile's rounds select from the union and the result is that of the whole row.  The records' neighbour values are then
// gathered from the row by the K lanes that hold a key (lines the wave has just read) and leave as one float4 per lane.
#include "sgx_maxima.hpp"

namespace sgx {
namespace maxima {

namespace {
constexpr uint32_t kLanes = 64, kPerLane = 32, kTile = kLanes * kPerLane, kWaves = 4;
constexpr uint32_t kGroup = 8, kGroups = kPerLane / kGroup;   // elements per group maximum, groups per lane

// Cross-lane moves as DPP modifiers of vector instructions (gfx9: no LDS pipe, no wait): a lane without a source keeps `old`.
constexpr int kRowShr = 0x110, kRowBcast15 = 0x142, kRowBcast31 = 0x143, kWaveShl1 = 0x130, kWaveShr1 = 0x138;
template <int Ctrl, int RowMask>
__device__ __forceinline__ uint32_t dpp(uint32_t old, uint32_t x)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)x, Ctrl, RowMask, 0xf, false);
}
template <int Ctrl, int RowMask>
__device__ __forceinline__ unsigned long long larger_dpp(unsigned long long v)
{
    const unsigned long long w = ((unsigned long long)dpp<Ctrl, RowMask>(0u, (uint32_t)(v >> 32)) << 32) | dpp<Ctrl, RowMask>(0u, (uint32_t)v);
    return w > v ? w : v;   // (a lane without a source compares with kNone)
}

// the wave's largest key, uniform: an inclusive maximum scan along each row of 16 lanes, rows 0 and 2 into rows 1 and 3, row 1 into rows
// 2 and 3; lane 63 holds the maximum of all 64
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v)
{
    v = larger_dpp<kRowShr + 1, 0xf>(v);
    v = larger_dpp<kRowShr + 2, 0xf>(v);
    v = larger_dpp<kRowShr + 4, 0xf>(v);
    v = larger_dpp<kRowShr + 8, 0xf>(v);
    v = larger_dpp<kRowBcast15, 0xa>(v);
    v = larger_dpp<kRowBcast31, 0xc>(v);
    const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), kLanes - 1), lo = __builtin_amdgcn_readlane((uint32_t)v, kLanes - 1);
    return ((unsigned long long)hi << 32) | lo;
}

// x of the lane below (lane 0: `below`) and of the lane above (lane 63: `above`)
__device__ __forceinline__ float from_lane_below(float x, float below)
{
    return __uint_as_float(dpp<kWaveShr1, 0xf>(__float_as_uint(below), __float_as_uint(x)));
}
__device__ __forceinline__ float from_lane_above(float x, float above)
{
    return __uint_as_float(dpp<kWaveShl1, 0xf>(__float_as_uint(above), __float_as_uint(x)));
}
__device__ __forceinline__ float lane_value(float x, int lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane));
}
// the largest key below `last` among elements [G * kGroup, (G + 1) * kGroup) of this lane, whose element 0 is j0; kNone: none
template <uint32_t G>
__device__ __forceinline__ unsigned long long group_max(const uint32_t (&bits)[kPerLane], uint32_t j0, unsigned long long last)
{
    unsigned long long best = kNone;
#pragma unroll
    for (uint32_t e = G * kGroup; e < (G + 1) * kGroup; ++e) {
        const unsigned long long key = bits[e] ? make_key(bits[e], j0 + e * kLanes) : kNone;
        if (key < last && key > best) best = key;
    }
    return best;
}
__device__ __forceinline__ unsigned long long larger(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
}  // namespace

__global__ void __launch_bounds__(kLanes * kWaves) maxima_kernel(const float2 *__restrict__ rows, unsigned long long n_rows, uint32_t M, uint32_t k,
                                                                 float floor, float4 *__restrict__ out)
{
    const uint32_t lane = threadIdx.x & (kLanes - 1);
    const unsigned long long wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
    for (unsigned long long row = (unsigned long long)blockIdx.x * kWaves + wave; row < n_rows; row += (unsigned long long)gridDim.x * kWaves) {
        const float2 *m = rows + row * M;
        unsigned long long held[2] = {kNone, kNone};   // lane r: result r of the tiles so far, per side
        for (uint32_t t0 = 0; t0 < M; t0 += kTile) {
            const uint32_t len = M - t0 < kTile ? M - t0 : kTile;
            // ---- the tile, once -------------------------------------------------------------------------------------------------------
            float2 v[kPerLane];
#pragma unroll
            for (uint32_t e = 0; e < kPerLane; ++e) {
                v[e] = make_float2(0.0f, 0.0f);
                if (e * kLanes < len) {
                    const uint32_t i = e * kLanes + lane;
                    if (i < len) v[e] = m[(unsigned long long)t0 + i];
                }
            }
            const float2 left = t0 > 0 ? m[(unsigned long long)t0 - 1] : make_float2(0.0f, 0.0f);                 // (element 0 is no candidate)
            const float2 right = M - t0 > kTile ? m[(unsigned long long)t0 + kTile] : make_float2(0.0f, 0.0f);     // (nor is element M - 1)
            // ---- candidates, in registers: the value's bits, or 0 ---------------------------------------------------------------------
            uint32_t bits[2][kPerLane];
#pragma unroll
            for (uint32_t e = 0; e < kPerLane; ++e) {
                bits[0][e] = bits[1][e] = 0;
                if (e * kLanes < len) {
                    const uint32_t j = t0 + e * kLanes + lane;
                    const float2 below = e > 0 ? make_float2(lane_value(v[e - 1].x, kLanes - 1), lane_value(v[e - 1].y, kLanes - 1)) : left;
                    const float2 above = e + 1 < kPerLane ? make_float2(lane_value(v[e + 1].x, 0), lane_value(v[e + 1].y, 0)) : right;
                    const float lx = from_lane_below(v[e].x, below.x), ly = from_lane_below(v[e].y, below.y);
                    const float rx = from_lane_above(v[e].x, above.x), ry = from_lane_above(v[e].y, above.y);
                    const bool interior = j >= 1 && (unsigned long long)j + 2 <= M;
                    if (interior && v[e].x > lx && v[e].x >= rx && v[e].x >= floor) bits[0][e] = __float_as_uint(v[e].x);
                    if (interior && v[e].y > ly && v[e].y >= ry && v[e].y >= floor) bits[1][e] = __float_as_uint(v[e].y);
                }
            }
            // ---- k rounds over the tile's keys and the keys carried in ----------------------------------------------------------------
            unsigned long long carried[2] = {held[0], held[1]}, top[2][kGroups];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                top[s][0] = group_max<0>(bits[s], t0 + lane, ~0ull);
                top[s][1] = len > 1 * kGroup * kLanes ? group_max<1>(bits[s], t0 + lane, ~0ull) : kNone;
                top[s][2] = len > 2 * kGroup * kLanes ? group_max<2>(bits[s], t0 + lane, ~0ull) : kNone;
                top[s][3] = len > 3 * kGroup * kLanes ? group_max<3>(bits[s], t0 + lane, ~0ull) : kNone;
            }
            held[0] = held[1] = kNone;
            for (uint32_t r = 0; r < k; ++r) {
                unsigned long long won[2];
#pragma unroll
                for (int s = 0; s < 2; ++s) won[s] = wave_max(larger(larger(larger(top[s][0], top[s][1]), larger(top[s][2], top[s][3])), carried[s]));
                if ((won[0] | won[1]) == kNone) break;   // (uniform) neither side has a candidate left: the other slots stay empty
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    if (won[s] == kNone) continue;       // (uniform)
                    if (lane == r) held[s] = won[s];
                    const uint32_t j = key_element(won[s]);
                    if (j < t0) {                        // a key of an earlier tile: the one lane that carries it lets it go
                        if (carried[s] == won[s]) carried[s] = kNone;
                        continue;
                    }
                    // the winner's lane searches the winner's group again, below the key just taken (every key taken before is above it)
                    const uint32_t i = j - t0, lane_won = i % kLanes;
                    switch (i / kLanes / kGroup) {
                    case 0: { const unsigned long long m0 = group_max<0>(bits[s], t0 + lane, won[s]); if (lane == lane_won) top[s][0] = m0; break; }
                    case 1: { const unsigned long long m1 = group_max<1>(bits[s], t0 + lane, won[s]); if (lane == lane_won) top[s][1] = m1; break; }
                    case 2: { const unsigned long long m2 = group_max<2>(bits[s], t0 + lane, won[s]); if (lane == lane_won) top[s][2] = m2; break; }
                    default: { const unsigned long long m3 = group_max<3>(bits[s], t0 + lane, won[s]); if (lane == lane_won) top[s][3] = m3; break; }
                    }
                }
            }
        }
        // ---- the records: lane r writes result r of either side ------------------------------------------------------------------------
        if (lane < k) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                float4 rec = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (held[s] != kNone) {
                    const uint32_t j = key_element(held[s]);
                    const float *p = reinterpret_cast<const float *>(m + j) + s;
                    rec = make_float4((float)(j + 1), p[-2], p[0], p[2]);
                }
                out[(row * 2 + (unsigned long long)s) * k + lane] = rec;
            }
        }
    }
}

hipError_t launch_maxima(const sgx_ctx *c, const float *d_rows, size_t n_rows, uint32_t k, float floor, float *d_max)
{
    if (n_rows == 0) return hipSuccess;
    if (k < 1 || k > kMaxK || c->M < 1) return hipErrorInvalidValue;
    // (rows beyond the grid are taken by striding: the grid is a matter of speed only)
    const unsigned long long blocks = ((unsigned long long)n_rows + kWaves - 1) / kWaves, cap = 1ull << 20;
    hipLaunchKernelGGL(maxima_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(kLanes * kWaves), 0, c->stream,
                       reinterpret_cast<const float2 *>(d_rows), (unsigned long long)n_rows, (uint32_t)c->M, k, floor, reinterpret_cast<float4 *>(d_max));
    return hipGetLastError();
}

}  // namespace maxima
}  // namespace sgx
