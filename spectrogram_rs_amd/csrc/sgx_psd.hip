// sgx_psd.hip -- the two kernels of the Welch-averaged spectra (include/sgx.h: sgx_psd_batch, sgx_csd_batch, sgx_psd_mags, sgx_csd_spec)
// over rows in device memory: float32 block partials of 32 frames, then the float64 chain over a column's partials and the one divide.
// The order of both chains is the definition (sgx_psd.hpp); consecutive threads take consecutive elements of a row, so every access is a
// coalesced float2 (psd) or float4 (csd, and its partials and output).
#include "sgx_psd.hpp"

namespace sgx {
namespace psd {

template <int NC> struct VecOf;
template <> struct VecOf<2> { typedef float2 type; };
template <> struct VecOf<4> { typedef float4 type; };
__device__ __forceinline__ void unpack(const float2 &v, float (&s)[2]) { s[0] = v.x; s[1] = v.y; }
__device__ __forceinline__ void unpack(const float4 &v, float (&s)[4]) { s[0] = v.x; s[1] = v.y; s[2] = v.z; s[3] = v.w; }
__device__ __forceinline__ float2 pack(const float (&s)[2]) { return make_float2(s[0], s[1]); }
__device__ __forceinline__ float4 pack(const float (&s)[4]) { return make_float4(s[0], s[1], s[2], s[3]); }

// A thread per (block, element): blockIdx.x / threadIdx.x run over the elements of a row, blockIdx.y strides over the piece's blocks.
template <typename Src>
__global__ void __launch_bounds__(256) psd_block_kernel(BlockPiece p)
{
    constexpr int NC = Src::kComponents;
    typedef typename VecOf<NC>::type Vec;
    const unsigned long long e = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (e >= p.elems) return;
    const Src src{reinterpret_cast<const Vec *>(p.rows), p.elems};
    Vec *partial = reinterpret_cast<Vec *>(p.partial);
    for (unsigned long long lb = blockIdx.y; lb < p.nb; lb += gridDim.y) {
        const unsigned long long b = p.b0 + lb;
        unsigned long long f0 = p.geo.block_first(b), f1 = p.geo.block_end(b);
        if (f0 < p.f_lo) f0 = p.f_lo;
        if (f1 > p.f_hi) f1 = p.f_hi;
        if (f0 >= f1) continue;   // none of this block's frames are among the rows given
        float s[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) s[q] = 0.0f;
        if (p.resume && f0 != p.geo.block_first(b)) unpack(partial[lb * p.elems + e], s);
        block_chain(src, f0 - p.f_lo, f1 - p.f_lo, e, s);
        partial[lb * p.elems + e] = pack(s);
    }
}

// A thread per (column, element): blockIdx.y strides over the columns that blocks [b0, b0 + nb) touch.
template <int NC>
__global__ void __launch_bounds__(256) psd_combine_kernel(CombinePiece p)
{
    typedef typename VecOf<NC>::type Vec;
    const unsigned long long e = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (e >= p.elems) return;
    const Vec *partial = reinterpret_cast<const Vec *>(p.partial);
    const unsigned long long j0 = p.b0 / p.geo.bpc, j1 = (p.b0 + p.nb - 1) / p.geo.bpc;
    for (unsigned long long j = j0 + blockIdx.y; j <= j1; j += gridDim.y) {
        const unsigned long long cb = j * p.geo.bpc, ce = p.geo.column_block_end(j);
        const unsigned long long b_lo = cb < p.b0 ? p.b0 : cb, b_hi = ce < p.b0 + p.nb ? ce : p.b0 + p.nb;
        double S[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) S[q] = b_lo == cb ? 0.0 : p.carry[e * NC + q];
        for (unsigned long long b = b_lo; b < b_hi; ++b) {
            float s[NC];
            unpack(partial[(b - p.b0) * p.elems + e], s);
#pragma unroll
            for (int q = 0; q < NC; ++q) S[q] = __dadd_rn(S[q], (double)s[q]);
        }
        if (b_hi == ce) {
            const double n_j = (double)(p.geo.column_end(j) - p.geo.column_first(j));
            float r[NC];
#pragma unroll
            for (int q = 0; q < NC; ++q) r[q] = (float)__ddiv_rn(S[q], n_j);
            reinterpret_cast<Vec *>(p.out)[j * p.elems + e] = pack(r);
        } else {
#pragma unroll
            for (int q = 0; q < NC; ++q) p.carry[e * NC + q] = S[q];
        }
    }
}

namespace {
// grid.x over a row's elements, grid.y over `n_y` blocks or columns (strided where there are more than a grid holds)
bool grid_for(unsigned long long elems, unsigned long long n_y, dim3 &grid)
{
    const unsigned long long gx = (elems + 255) / 256;
    if (gx == 0 || n_y == 0 || gx > 0x7fffffffull) return false;
    grid = dim3((unsigned)gx, (unsigned)(n_y < 65535 ? n_y : 65535), 1);
    return true;
}
}  // namespace

hipError_t launch_psd_blocks(const sgx_ctx *c, bool cross, const BlockPiece &p)
{
    dim3 grid;
    if (!grid_for(p.elems, p.nb, grid)) return p.nb == 0 ? hipSuccess : hipErrorInvalidValue;
    if (cross) hipLaunchKernelGGL(psd_block_kernel<SpecRows>, grid, dim3(256), 0, c->stream, p);
    else hipLaunchKernelGGL(psd_block_kernel<MagRows>, grid, dim3(256), 0, c->stream, p);
    return hipGetLastError();
}

hipError_t launch_psd_combine(const sgx_ctx *c, bool cross, const CombinePiece &p)
{
    if (p.nb == 0) return hipSuccess;
    const unsigned long long n_cols = (p.b0 + p.nb - 1) / p.geo.bpc - p.b0 / p.geo.bpc + 1;
    dim3 grid;
    if (!grid_for(p.elems, n_cols, grid)) return hipErrorInvalidValue;
    if (cross) hipLaunchKernelGGL(psd_combine_kernel<4>, grid, dim3(256), 0, c->stream, p);
    else hipLaunchKernelGGL(psd_combine_kernel<2>, grid, dim3(256), 0, c->stream, p);
    return hipGetLastError();
}

}  // namespace psd
}  // namespace sgx
