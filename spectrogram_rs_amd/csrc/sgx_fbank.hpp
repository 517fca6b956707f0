// sgx_fbank.hpp -- the filter pass of the filterbank calls (include/sgx.h: sgx_fbank_batch, sgx_fbank_mags): one body for the stage kernel
// (sgx_fbank.hip) and for the fused modes of the two 4096-point kernels (stft4096_wg.hip, stft4096_real.hip), so that a bank's output
// is the same bits on every route.  The cross pass (sgx_fbank_cross_batch, sgx_fbank_cross_spec) is the same order over the four
// products of a bin's (L, R) pair, one trip over the bank for all four.  The flux pass (sgx_flux_batch, sgx_flux_mags) is the
// cross pass over another four elements: the rise and the fall of a bin's (l, r) pair against the same bin of an earlier frame.
//
// A wave per filter.  Lane l takes the filter's elements i = l, l + 64, l + 128, ... in ascending order into one fused-multiply-add
// chain from +0; the 64 partial sums then meet in a halving tree (a[l] + a[l + 32], then + 16, 8, 4, 2, 1).  That order is the
// definition (include/sgx.h) -- lanes read consecutive bins of the column (conflict-free in LDS, coalesced in memory) and consecutive
// weights; the tree serves both components of the column at once (wave_tree2).
#pragma once

#include "fbank_host.hpp"
#include "flux_host.hpp"
#include "sgx_internal.hpp"

// A bank: its tables on the device.  It belongs to its context (sgx_destroy detaches the banks still alive: their calls then answer
// SGX_ERR_INVALID_ARG).
struct sgx_fbank {
    sgx_ctx *ctx = nullptr;
    uint32_t n_filters = 0, power = 1;
    size_t n_weights = 0;
    sgx::DeviceBuffer<sgx::fbank::Filter> d_filters;   // [n_filters]
    sgx::DeviceBuffer<float> d_weights;                // [n_weights] (one word where the bank has none)
    std::vector<sgx::fbank::Filter> h_filters;   // what the asynchronous uploads read: the caller's arrays are the caller's again when
    std::vector<float> h_weights;                // sgx_fbank_create returns
};

namespace sgx {

hipError_t launch_fbank_stage(const sgx_ctx *c, const sgx_fbank *fb, const float *d_mags, size_t n_columns, float *d_out);   // sgx_fbank.hip
bool wg4096_can_fuse_fbank(const sgx_ctx *c, const sgx_fbank *fb);   // stft4096_wg.hip
hipError_t launch_fbank_cross_stage(const sgx_ctx *c, const sgx_fbank *fb, const float *d_spec, size_t n_columns, float *d_out);   // sgx_fbank.hip
bool wg4096_can_fuse_fbank_cross(const sgx_ctx *c, const sgx_fbank *fb);   // stft4096_wg.hip
// The flux records of n_frames frames: d_rows holds skip + n_frames frames' rows [pairs][M][2], the records are those of the frames behind
// the first `skip`; row r of d_rows has its predecessor at r - lag, and none where r < lag (skip <= lag: the head of a range, or 0)
hipError_t launch_fbank_flux_stage(const sgx_ctx *c, const sgx_fbank *fb, const float *d_rows, size_t skip, size_t n_frames, uint32_t lag,
                                   float *d_out);   // sgx_fbank.hip
void detach_fbanks(sgx_ctx *c);   // sgx_fbank.hip

#ifdef __HIPCC__
namespace fbank {

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xf, 0xf, true)); }

// The sums of the wave's 64 values of x and of y, each by the halving tree of the definition: for s = 32, 16, 8, 4, 2, 1 lane l < s takes
// a[l] + a[l + s]; the sum is a[0].  One chain for both: the first level is a swap of register halves between x and y (gfx950's
// v_permlane32_swap) and one add, after which lanes 0 .. 31 hold x's 32 sums and lanes 32 .. 63 y's; the level of 16 swaps rows of 16
// lanes, the last four are DPP adds inside a row.  Both partners of a pair compute the same sum (x + y and y + x are the same bits), so
// every lane of a half ends with the half's total.  All 64 lanes must be active.
typedef unsigned int fbank_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void wave_tree2(float ax, float ay, float &sx, float &sy)
{
    const fbank_u32x2 h = __builtin_amdgcn_permlane32_swap(__float_as_uint(ax), __float_as_uint(ay), false, false);   // (x lo, y lo), (x hi, y hi)
    float v = __uint_as_float(h.x) + __uint_as_float(h.y);                                                            // s = 32
    const fbank_u32x2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);     // rows (0, 0, 2, 2), (1, 1, 3, 3)
    v = __uint_as_float(r.x) + __uint_as_float(r.y);                                                                  // s = 16
    v = v + dpp_f32<0x128>(v);   // row_ror:8        s = 8
    v = v + dpp_f32<0x124>(v);   // row_ror:4        s = 4 (lanes l and l + 8 hold the same value by now)
    v = v + dpp_f32<0x4E>(v);    // quad_perm [2, 3, 0, 1]   s = 2
    v = v + dpp_f32<0xB1>(v);    // quad_perm [1, 0, 3, 2]   s = 1
    sx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    sy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
}

// Every filter f = wave, wave + n_waves, ... of a 64 n_waves-thread workgroup over one column: col[j] = the (x, y) pair of stored bin j
// (LDS or memory).  Both components are filtered.  DUP false: dst_a[f] = (out_x, out_y).  DUP true (two mono frames in one column):
// dst_a[f] = (out_x, out_x) where have_a, dst_b[f] = (out_y, out_y) where have_b.  All lanes of the wave must be active.
// A wave takes its filters four at a time (G): the four table entries are scalar loads (the tables are never written while a kernel
// reads them: constant address space), the four first chunks of weights and of the column are requested side by side, and only then
// does the arithmetic start -- one memory latency per four filters instead of two per filter (a mel filter is a few dozen bins: the
// pass is latency, not arithmetic).  Results wait in lane k % 64 for the wave's k-th filter and leave 64 at a time.
typedef unsigned int fbank_u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) fbank_u32x4 *const_u4_ptr;
template <bool DUP>
__device__ __forceinline__ void filter_pass(const float2 *col, const Filter *filters, const float *weights, uint32_t n_filters, bool square,
                                            float2 *dst_a, float2 *dst_b, bool have_a, bool have_b, uint32_t tid, uint32_t n_waves)
{
    constexpr uint32_t G = 4;   // filters a wave takes per trip (eight: inside the spreads of four, 106 scalar registers against 84 .. 89 -- profiles/fbank.txt)
    static_assert(64 % G == 0, "a batch of results never straddles two groups of filters");
    asm volatile("" : "+v"(tid));   // (opaque: inside a persistent kernel's loop over transforms the pass's lane offsets are not to be hoisted out of that loop -- they spill there)
    const uint32_t lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t n_mine = n_filters > wave ? (n_filters - wave + n_waves - 1u) / n_waves : 0u;   // this wave's filters: wave + k n_waves, k < n_mine
    const const_u4_ptr table = (const_u4_ptr)(unsigned long long)filters;
    float kx = 0.0f, ky = 0.0f;
    for (uint32_t k0 = 0; k0 < n_mine; k0 += G) {
        uint32_t first[G], count[G], offset[G];
        float w[G];
        float2 v[G];
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) {
            const bool valid = k0 + g < n_mine;
            const fbank_u32x4 q = table[wave + (size_t)(valid ? k0 + g : k0) * n_waves];
            first[g] = q.x;
            count[g] = valid ? q.y : 0u;
            offset[g] = q.z;
        }
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) {
            w[g] = 0.0f;
            v[g] = make_float2(0.0f, 0.0f);
            if (lane < count[g]) {
                w[g] = weights[(size_t)offset[g] + lane];
                v[g] = col[first[g] + lane];
            }
        }
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) {
            float ax = 0.0f, ay = 0.0f;
            if (lane < count[g]) {
                float2 x = v[g];
                if (square) {
                    x.x = x.x * x.x;
                    x.y = x.y * x.y;
                }
                ax = fmaf(w[g], x.x, ax);
                ay = fmaf(w[g], x.y, ay);
                for (uint32_t i = lane + 64u; i < count[g]; i += 64u) {   // filters of more than 64 bins: the lane's chain goes on
                    const float wi = weights[(size_t)offset[g] + i];
                    float2 xi = col[first[g] + i];
                    if (square) {
                        xi.x = xi.x * xi.x;
                        xi.y = xi.y * xi.y;
                    }
                    ax = fmaf(wi, xi.x, ax);
                    ay = fmaf(wi, xi.y, ay);
                }
            }
            float sx, sy;
            wave_tree2(ax, ay, sx, sy);
            if (lane == ((k0 + g) & 63u)) { kx = sx; ky = sy; }
        }
        const uint32_t k_end = k0 + G < n_mine ? k0 + G : n_mine;
        if ((k_end & 63u) == 0u || k_end == n_mine) {   // (wave-uniform) a full wave of results, or the last ones
            const uint32_t k = ((k_end - 1u) & ~63u) + lane;   // this lane's filter of the wave
            if (k < k_end) {
                const size_t f = wave + (size_t)k * n_waves;
                if (DUP) {
                    if (have_a) dst_a[f] = make_float2(kx, kx);
                    if (have_b) dst_b[f] = make_float2(ky, ky);
                } else {
                    dst_a[f] = make_float2(kx, ky);
                }
            }
        }
    }
}

// ---- the cross pass: per band the sums of |L|^2, |R|^2, Re L conj R, Im L conj R (include/sgx.h: sgx_fbank_cross_batch) -----------------

// The four products of one bin, L = (a, b), R = (c, d), as the header defines them: every product rounded, then one add or subtract --
// never contracted into a fused multiply-add, whatever the build says.  (x0, x1) and (x2, x3) are the elements of the two columns.
__device__ __forceinline__ void cross_terms(float a, float b, float c, float d, float2 &x01, float2 &x23)
{
#pragma clang fp contract(off)
    x01.x = __fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b));   // |L|^2
    x01.y = __fadd_rn(__fmul_rn(c, c), __fmul_rn(d, d));   // |R|^2
    x23.x = __fadd_rn(__fmul_rn(a, c), __fmul_rn(b, d));   // Re L conj R
    x23.y = __fsub_rn(__fmul_rn(b, c), __fmul_rn(a, d));   // Im L conj R
}

// Where the cross pass reads element j from: two float2 columns of products (LDS), or the complex rows where they lie (a column no LDS
// holds: the products are formed at every read -- the same bits, cross_terms is a pure function of the row's words)
struct CrossColumns {
    const float2 *c01, *c23;
    __device__ __forceinline__ void operator()(uint32_t j, float2 &x01, float2 &x23) const { x01 = c01[j]; x23 = c23[j]; }
};
struct CrossRows {
    const float4 *row;   // [M] (L.re, L.im, R.re, R.im)
    __device__ __forceinline__ void operator()(uint32_t j, float2 &x01, float2 &x23) const
    {
        const float4 s = row[j];
        cross_terms(s.x, s.y, s.z, s.w, x01, x23);
    }
};

// filter_pass for the four components at once: one trip over the bank -- the table entries and the weights of a group of filters are
// loaded once, the element comes from two float2 columns, two chain pairs run side by side and two trees close each filter.  Per
// component the order is filter_pass's (64 chains from +0 over i = l, l + 64, ..., then wave_tree2's halving tree), so the bits are the
// definition's.  dst[f] = (out0, out1, out2, out3).  All lanes of the wave must be active.
template <typename Col>
__device__ __forceinline__ void cross_filter_pass(const Col &col, const Filter *filters, const float *weights, uint32_t n_filters, float4 *dst,
                                                  uint32_t tid, uint32_t n_waves)
{
    constexpr uint32_t G = 4;   // filters a wave takes per trip, as filter_pass
    static_assert(64 % G == 0, "a batch of results never straddles two groups of filters");
    asm volatile("" : "+v"(tid));   // (opaque, as in filter_pass)
    const uint32_t lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t n_mine = n_filters > wave ? (n_filters - wave + n_waves - 1u) / n_waves : 0u;   // this wave's filters: wave + k n_waves, k < n_mine
    const const_u4_ptr table = (const_u4_ptr)(unsigned long long)filters;
    float4 kept = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (uint32_t k0 = 0; k0 < n_mine; k0 += G) {
        uint32_t first[G], count[G], offset[G];
        float w[G];
        float2 v01[G], v23[G];
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) {
            const bool valid = k0 + g < n_mine;
            const fbank_u32x4 q = table[wave + (size_t)(valid ? k0 + g : k0) * n_waves];
            first[g] = q.x;
            count[g] = valid ? q.y : 0u;
            offset[g] = q.z;
        }
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) {
            w[g] = 0.0f;
            v01[g] = v23[g] = make_float2(0.0f, 0.0f);
            if (lane < count[g]) {
                w[g] = weights[(size_t)offset[g] + lane];
                col(first[g] + lane, v01[g], v23[g]);
            }
        }
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) {
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
            if (lane < count[g]) {
                a0 = fmaf(w[g], v01[g].x, a0);
                a1 = fmaf(w[g], v01[g].y, a1);
                a2 = fmaf(w[g], v23[g].x, a2);
                a3 = fmaf(w[g], v23[g].y, a3);
                for (uint32_t i = lane + 64u; i < count[g]; i += 64u) {   // filters of more than 64 bins: the lane's chains go on
                    const float wi = weights[(size_t)offset[g] + i];
                    float2 x01, x23;
                    col(first[g] + i, x01, x23);
                    a0 = fmaf(wi, x01.x, a0);
                    a1 = fmaf(wi, x01.y, a1);
                    a2 = fmaf(wi, x23.x, a2);
                    a3 = fmaf(wi, x23.y, a3);
                }
            }
            float s0, s1, s2, s3;
            wave_tree2(a0, a1, s0, s1);
            wave_tree2(a2, a3, s2, s3);
            if (lane == ((k0 + g) & 63u)) kept = make_float4(s0, s1, s2, s3);
        }
        const uint32_t k_end = k0 + G < n_mine ? k0 + G : n_mine;
        if ((k_end & 63u) == 0u || k_end == n_mine) {   // (wave-uniform) a full wave of results, or the last ones
            const uint32_t k = ((k_end - 1u) & ~63u) + lane;   // this lane's filter of the wave
            if (k < k_end) dst[wave + (size_t)k * n_waves] = kept;
        }
    }
}

// ---- the flux pass: per band the sums of a bin's rise and fall against the same bin `lag` frames earlier (include/sgx.h: sgx_flux_batch) --

// Rise and fall of one bin's (l, r) pair, as the header defines them: x = m or rn(m * m), d = rn(x_t - x_{t - lag}) -- one subtract, never
// contracted with the square -- then rise = d < 0 ? +0 : d and fall = d > 0 ? +0 : rn(+0 - d).  Equal words give +0 in both, a NaN
// gives NaN in both (neither comparison holds).
__device__ __forceinline__ float flux_element(float cur, float prev, bool square)
{
#pragma clang fp contract(off)
    if (square) {
        cur = __fmul_rn(cur, cur);
        prev = __fmul_rn(prev, prev);
    }
    return __fsub_rn(cur, prev);
}
__device__ __forceinline__ void flux_terms(float2 cur, float2 prev, bool square, float2 &rise, float2 &fall)
{
    const float dl = flux_element(cur.x, prev.x, square), dr = flux_element(cur.y, prev.y, square);
    rise.x = dl < 0.0f ? 0.0f : dl;
    rise.y = dr < 0.0f ? 0.0f : dr;
    fall.x = dl > 0.0f ? 0.0f : __fsub_rn(0.0f, dl);
    fall.y = dr > 0.0f ? 0.0f : __fsub_rn(0.0f, dr);
}

// The element source of a column no LDS holds: both rows where they lie, rise and fall formed at every read -- the same bits, flux_terms
// is a pure function of the two rows' words.  (A staged column goes through CrossColumns: (rise_l, rise_r) and (fall_l, fall_r).)
struct FluxRows {
    const float2 *cur, *prev;   // [M] (l, r) magnitudes of frame t and of frame t - lag
    bool square;
    __device__ __forceinline__ void operator()(uint32_t j, float2 &rise, float2 &fall) const { flux_terms(cur[j], prev[j], square, rise, fall); }
};

}  // namespace fbank
#endif

}  // namespace sgx
