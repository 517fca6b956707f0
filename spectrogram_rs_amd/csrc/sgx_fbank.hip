// sgx_fbank.hip -- the filterbank stage on rows in device memory: [columns][M][2] magnitudes -> [columns][n_filters][2] weighted sums
// (include/sgx.h: sgx_fbank_mags, and the second kernel of sgx_fbank_batch's workspace route).  The filter pass itself is
// sgx_fbank.hpp's, shared with the fused modes of the 4096-point kernels.  The cross stage (sgx_fbank_cross_spec, and the second kernel of
// sgx_fbank_cross_batch's workspace route): [columns][M][2][2] complex rows -> [columns][n_filters][4] sums of the (L, R) products.
// The flux stage (sgx_flux_mags, and the second kernel of sgx_flux_batch): [frames][pairs][M][2] magnitudes ->
// [frames][pairs][n_filters][4] sums of every bin's rise and fall against the same bin `lag` frames earlier.
#include "sgx_fbank.hpp"

namespace sgx {

struct FbankStageParams {
    const float *mags;             // [columns][M][2]
    const fbank::Filter *filters;
    const float *weights;
    float *out;                    // [columns][n_filters][2]
    uint32_t M, n_filters, square;
};

// One workgroup per column.  STAGED: the column goes through LDS once (overlapping filters read a bin several times); a column that no
// LDS holds is read where it lies, as magnitude_in_kernel does.
template <bool STAGED>
__global__ void __launch_bounds__(256) fbank_stage_kernel(FbankStageParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2 *stage = reinterpret_cast<float2 *>(smem_raw);
    const uint32_t tid = threadIdx.x;
    const size_t col = blockIdx.x;
    const float2 *src = reinterpret_cast<const float2 *>(p.mags) + col * p.M;
    if (STAGED) {
        for (uint32_t i = tid; i < p.M; i += 256u) stage[i] = src[i];
        __syncthreads();
    }
    float2 *dst = reinterpret_cast<float2 *>(p.out) + col * p.n_filters;
    fbank::filter_pass<false>(STAGED ? stage : src, p.filters, p.weights, p.n_filters, p.square != 0, dst, dst, true, false, tid, 4u);
}

hipError_t launch_fbank_stage(const sgx_ctx *c, const sgx_fbank *fb, const float *d_mags, size_t n_columns, float *d_out)
{
    if (n_columns == 0) return hipSuccess;
    FbankStageParams p;
    p.mags = d_mags;
    p.filters = fb->d_filters.get();
    p.weights = fb->d_weights.get();
    p.out = d_out;
    p.M = c->M;
    p.n_filters = fb->n_filters;
    p.square = fb->power == 2 ? 1u : 0u;
    const size_t lds_cap = c->lds_optin < (size_t)160 * 1024 ? c->lds_optin : (size_t)160 * 1024;
    const bool staged = (size_t)c->M * sizeof(float2) <= lds_cap;
    const size_t lds = staged ? (size_t)c->M * sizeof(float2) : 0;
    const auto kernel = staged ? fbank_stage_kernel<true> : fbank_stage_kernel<false>;
    if (lds > 64 * 1024) {   // per launch: the attribute is per device, and a process may hold contexts on several
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const size_t max_chunk = 1u << 30;
    for (size_t done = 0; done < n_columns; done += max_chunk) {
        const size_t chunk = n_columns - done < max_chunk ? n_columns - done : max_chunk;
        FbankStageParams q = p;
        q.mags = d_mags + done * (size_t)c->M * 2;
        q.out = d_out + done * (size_t)fb->n_filters * 2;
        hipLaunchKernelGGL(kernel, dim3((unsigned)chunk), dim3(256), lds, c->stream, q);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

struct FbankCrossStageParams {
    const float *spec;             // [columns][M][2][2]: (L.re, L.im, R.re, R.im) per bin
    const fbank::Filter *filters;
    const float *weights;
    float *out;                    // [columns][n_filters][4]
    uint32_t M, n_filters;
};

// One workgroup per column.  STAGED: the four products of every bin are formed once, on the way into two float2 columns in LDS; a column
// that no LDS holds is read where it lies and the products are formed at every read.
template <bool STAGED>
__global__ void __launch_bounds__(256) fbank_cross_stage_kernel(FbankCrossStageParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2 *c01 = reinterpret_cast<float2 *>(smem_raw), *c23 = c01 + p.M;
    const uint32_t tid = threadIdx.x;
    const size_t col = blockIdx.x;
    const float4 *src = reinterpret_cast<const float4 *>(p.spec) + col * p.M;
    float4 *dst = reinterpret_cast<float4 *>(p.out) + col * p.n_filters;
    if (STAGED) {
        for (uint32_t i = tid; i < p.M; i += 256u) {
            const float4 s = src[i];
            fbank::cross_terms(s.x, s.y, s.z, s.w, c01[i], c23[i]);
        }
        __syncthreads();
        fbank::cross_filter_pass(fbank::CrossColumns{c01, c23}, p.filters, p.weights, p.n_filters, dst, tid, 4u);
    } else {
        fbank::cross_filter_pass(fbank::CrossRows{src}, p.filters, p.weights, p.n_filters, dst, tid, 4u);
    }
}

hipError_t launch_fbank_cross_stage(const sgx_ctx *c, const sgx_fbank *fb, const float *d_spec, size_t n_columns, float *d_out)
{
    if (n_columns == 0) return hipSuccess;
    FbankCrossStageParams p;
    p.spec = d_spec;
    p.filters = fb->d_filters.get();
    p.weights = fb->d_weights.get();
    p.out = d_out;
    p.M = c->M;
    p.n_filters = fb->n_filters;
    const size_t lds_cap = c->lds_optin < (size_t)160 * 1024 ? c->lds_optin : (size_t)160 * 1024;
    const bool staged = (size_t)c->M * 2 * sizeof(float2) <= lds_cap;
    const size_t lds = staged ? (size_t)c->M * 2 * sizeof(float2) : 0;
    const auto kernel = staged ? fbank_cross_stage_kernel<true> : fbank_cross_stage_kernel<false>;
    if (lds > 64 * 1024) {   // per launch: the attribute is per device, and a process may hold contexts on several
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const size_t max_chunk = 1u << 30;
    for (size_t done = 0; done < n_columns; done += max_chunk) {
        const size_t chunk = n_columns - done < max_chunk ? n_columns - done : max_chunk;
        FbankCrossStageParams q = p;
        q.spec = d_spec + done * (size_t)c->M * 4;
        q.out = d_out + done * (size_t)fb->n_filters * 4;
        hipLaunchKernelGGL(kernel, dim3((unsigned)chunk), dim3(256), lds, c->stream, q);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

struct FbankFluxStageParams {
    const float *rows;             // [skip + frames][pairs][M][2]
    const fbank::Filter *filters;
    const float *weights;
    float *out;                    // [frames][pairs][n_filters][4]: (rise_l, rise_r, fall_l, fall_r) per filter
    size_t base;                   // the launch's first (frame, pair) among the call's frames * pairs
    size_t skip;                   // head rows: frame f of the call is row skip + f
    uint32_t M, n_filters, square, pairs, lag;
};

// One workgroup per (frame, pair).  STAGED: rise and fall of every bin are formed once from the two rows, on the way into two float2
// columns in LDS; rows that no LDS holds are read where they lie and the elements are formed at every read.  A frame whose row index is
// below the lag has no predecessor: its records are +0, and no row is read.
template <bool STAGED>
__global__ void __launch_bounds__(256) fbank_flux_stage_kernel(FbankFluxStageParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2 *rise = reinterpret_cast<float2 *>(smem_raw), *fall = rise + p.M;
    const uint32_t tid = threadIdx.x;
    const size_t job = p.base + blockIdx.x, frame = job / p.pairs, pair = job - frame * p.pairs, row = p.skip + frame;
    float4 *dst = reinterpret_cast<float4 *>(p.out) + job * p.n_filters;
    if (row < p.lag) {   // (workgroup-uniform)
        for (uint32_t f = tid; f < p.n_filters; f += 256u) dst[f] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float2 *cur = reinterpret_cast<const float2 *>(p.rows) + (row * p.pairs + pair) * p.M;
    const float2 *prev = reinterpret_cast<const float2 *>(p.rows) + ((row - p.lag) * p.pairs + pair) * p.M;
    if (STAGED) {
        for (uint32_t i = tid; i < p.M; i += 256u) fbank::flux_terms(cur[i], prev[i], p.square != 0, rise[i], fall[i]);
        __syncthreads();
        fbank::cross_filter_pass(fbank::CrossColumns{rise, fall}, p.filters, p.weights, p.n_filters, dst, tid, 4u);
    } else {
        fbank::cross_filter_pass(fbank::FluxRows{cur, prev, p.square != 0}, p.filters, p.weights, p.n_filters, dst, tid, 4u);
    }
}

hipError_t launch_fbank_flux_stage(const sgx_ctx *c, const sgx_fbank *fb, const float *d_rows, size_t skip, size_t n_frames, uint32_t lag,
                                   float *d_out)
{
    if (n_frames == 0) return hipSuccess;
    FbankFluxStageParams p;
    p.rows = d_rows;
    p.filters = fb->d_filters.get();
    p.weights = fb->d_weights.get();
    p.out = d_out;
    p.base = 0;
    p.skip = skip;
    p.M = c->M;
    p.n_filters = fb->n_filters;
    p.square = fb->power == 2 ? 1u : 0u;
    p.pairs = c->pairs;
    p.lag = lag;
    const size_t lds_cap = c->lds_optin < (size_t)160 * 1024 ? c->lds_optin : (size_t)160 * 1024;
    const bool staged = (size_t)c->M * 2 * sizeof(float2) <= lds_cap;   // the cross stage's threshold: two float2 columns
    const size_t lds = staged ? (size_t)c->M * 2 * sizeof(float2) : 0;
    const auto kernel = staged ? fbank_flux_stage_kernel<true> : fbank_flux_stage_kernel<false>;
    if (lds > 64 * 1024) {   // per launch: the attribute is per device, and a process may hold contexts on several
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const size_t jobs = n_frames * c->pairs, max_chunk = 1u << 30;
    for (size_t done = 0; done < jobs; done += max_chunk) {
        const size_t chunk = jobs - done < max_chunk ? jobs - done : max_chunk;
        FbankFluxStageParams q = p;
        q.base = done;
        hipLaunchKernelGGL(kernel, dim3((unsigned)chunk), dim3(256), lds, c->stream, q);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

void detach_fbanks(sgx_ctx *c)
{
    for (sgx_fbank *fb : c->fbanks) fb->ctx = nullptr;
    c->fbanks.clear();
}

}  // namespace sgx
