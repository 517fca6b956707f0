// stft_mixed_bands.hip -- the bands instantiations of the mixed-radix kernels' fused column (sgx_bands_batch): the same transforms and
// pixel_passes' sample pass as the kernels that render pixels (stft_mixed.hip), then the rows' (l, r) means stored as float2 instead of
// a colour.  A translation unit of its own so that these instantiations compile beside stft_mixed.hip's, not behind them.
#include "stft_mixed_kernels.hpp"

namespace sgx {
namespace mix {

// stft_mixed_fixed_kernel and stft_mixed_fixed4_kernel (stft_mixed.hip) with the column in its BANDS form
struct BandsColumn {
    template <typename F, bool REAL>
    static __device__ __forceinline__ void run(const Params &p, float2 *s, uint32_t pair, long long row_a, long long row_b, uint32_t tid)
    {
        if constexpr (REAL) pixel_epilogue_real<F::NT, F::P, true>(p, s, row_a, tid);   // P is the WINDOW here
        else pixel_epilogue<F::NT, F::W, true>(p, s, pair, row_a, row_b, tid);
    }
};

template <typename F, int R0A, int R0B, int R1A, int R1B, int R2A, int R2B, bool REAL>
__global__ void __launch_bounds__(F::NT, F::NT <= 256 ? 4 : 8) stft_mixed_fixed_bands_kernel(Params p)
{
    if constexpr (!kOwnText<F>) {
        fixed3_body<F, R0A, R0B, R1A, R1B, R2A, R2B, REAL, BandsColumn>(p);
    } else {   // fixed3_body's text: see kOwnText in stft_mixed_kernels.hpp
        extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
        float2 *s = reinterpret_cast<float2 *>(smem_raw);
        const uint32_t tid = threadIdx.x;
        const uint32_t pair = blockIdx.y;
        long long row_a, row_b;
        Source src;
        frame_source(p, pair, src, row_a, row_b);
        using G0 = FixGeo<F::M0, F::P / F::R0, F::pp(F::M0), F::pp(F::P), F::W, F::PAD, F::NT, true>;
        stage<R0A, R0B, G0, REAL>(s, p, p.tw, G0{}, src, tid);
        stage<R1A, R1B>(s, p, p.tw + F::TW1, FixGeo<F::M1, F::P / F::R1, F::pp(F::M1), F::pp(F::M0), F::W, F::PAD, F::NT, false>{}, src, tid);
        stage<R2A, R2B>(s, p, p.tw, FixGeo<1, F::P / F::R2, 1, F::pp(F::M1), F::W, F::PAD, F::NT, false>{}, src, tid);
        BandsColumn::run<F, REAL>(p, s, pair, row_a, row_b, tid);
    }
}

template <typename F, int R0A, int R0B, int R1A, int R1B, int R2A, int R2B, int R3A, int R3B, bool REAL>
__global__ void __launch_bounds__(F::NT, F::NT == 256 ? 4 : (F::NT == 512 ? 8 : 4)) stft_mixed_fixed4_bands_kernel(Params p)
{
    fixed4_body<F, R0A, R0B, R1A, R1B, R2A, R2B, R3A, R3B, REAL, BandsColumn>(p);
}

// The body of stft_mixed_real2_render_kernel (stft_mixed.hip) with pixel_passes in its BANDS form.  (A copy: see fixed3_body in stft_mixed_kernels.hpp.)
template <typename F, int R0A, int R0B, int R1A, int R1B, int R2A, int R2B>
__global__ void __launch_bounds__(2 * F::NT, real2_waves_per_simd<F>()) stft_mixed_real2_bands_kernel(Params p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2 *s = reinterpret_cast<float2 *>(smem_raw);
    constexpr uint32_t NT = F::NT, IMG = F::pp(F::P), M = F::P - 1, K = F::P / 2, kPer = (K + NT - 1) / NT;
    const uint32_t tid = threadIdx.x, half = tid >= NT ? 1u : 0u, ltid = tid - half * NT;
    float2 *img = s + half * IMG;
    const unsigned long long fa = 2ull * blockIdx.x, f = fa + half;              // rows fa, fa + 1 of this launch
    const unsigned long long fc = f < p.n_frames ? f : p.n_frames - 1;            // no second frame: the last one again, never stored
    Source src;
    src.a = src.b = p.pcm + (size_t)((p.first_frame + fc) * p.H);
    src.cl = src.cr = 0;
    src.data_b = true;
    using G0 = FixGeo<F::M0, F::P / F::R0, F::pp(F::M0), F::pp(F::P), F::W, F::PAD, NT, true>;
    stage<R0A, R0B, G0, 1>(img, p, p.tw, G0{}, src, ltid);
    stage<R1A, R1B>(img, p, p.tw + F::TW1, FixGeo<F::M1, F::P / F::R1, F::pp(F::M1), F::pp(F::M0), F::W, F::PAD, NT, false>{}, src, ltid);
    stage<R2A, R2B>(img, p, p.tw, FixGeo<1, F::P / F::R2, 1, F::pp(F::M1), F::W, F::PAD, NT, false>{}, src, ltid);
    float2 mg[kPer];
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
        const uint32_t k1 = ltid + NT * i;
        mg[i] = k1 < K ? untangle(p, img, k1) : make_float2(0.0f, 0.0f);
    }
    __syncthreads();
    float *col = reinterpret_cast<float *>(s);   // column element j: (frame fa, frame fa + 1) = col[2 j], col[2 j + 1]
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
        const uint32_t k1 = ltid + NT * i;
        if (k1 < K) {
            col[2 * k1 + half] = mg[i].x;
            col[2 * (M - 1 - k1) + half] = mg[i].y;
        }
    }
    __syncthreads();
    pixel_passes<2 * NT, true>(p, s, s + M + 1, M, true, 0u, (long long)fa, (long long)fa + 1, tid);
}

// The instantiations are those launch_mixed's pixel path selects: real-input mode two frames per workgroup (MIX_REAL2_RENDER_PLANS) or
// on a four-stage plan, every other stream on any compile-time plan.  (Real-input mode on a three-stage plan with one frame per
// workgroup -- the 2048-point plan -- has none: the two-kernel route.)
bool bands_kernel_exists(int fixed, bool real, bool two_frames)
{
    if (real && two_frames) {
#define X(Pn, A0, B0, A1, B1, A2, B2, N) if (fixed == Pn) return true;
        MIX_REAL2_RENDER_PLANS(X)
#undef X
        return false;
    }
#define X(Pn, A0, B0, A1, B1, A2, B2, A3, B3, N) if (fixed == Pn) return true;
    MIX_FIXED4_PLANS(X)
#undef X
    if (real) return false;
#define X(Pn, A0, B0, A1, B1, A2, B2, N) if (fixed == Pn) return true;
    MIX_FIXED_PLANS(X)
#undef X
    return false;
}

hipError_t launch_bands_kernel(const Params &p, int fixed, bool real, bool two_frames, dim3 grid, size_t lds, hipStream_t stream)
{
    auto go = [&](auto kernel, unsigned nt, dim3 g) { return launch_kernel(kernel, p, nt, g, lds, stream); };
    if (real && two_frames) {
        switch (fixed) {
#define X(Pn, A0, B0, A1, B1, A2, B2, N) \
    case Pn: return go(stft_mixed_real2_bands_kernel<Fixed3<Pn, A0, B0, A1, B1, A2, B2, N>, A0, B0, A1, B1, A2, B2>, 2 * N, dim3((grid.x + 1) / 2, 1));
            MIX_REAL2_RENDER_PLANS(X)
#undef X
        default: break;
        }
        return hipErrorNotSupported;
    }
    switch (fixed) {
#define X(Pn, A0, B0, A1, B1, A2, B2, A3, B3, N)                                                                                                          \
    case Pn:                                                                                                                                              \
        if (real) return go(stft_mixed_fixed4_bands_kernel<Fixed4<Pn, A0, B0, A1, B1, A2, B2, A3, B3, N>, A0, B0, A1, B1, A2, B2, A3, B3, true>, N, grid);   \
        return go(stft_mixed_fixed4_bands_kernel<Fixed4<Pn, A0, B0, A1, B1, A2, B2, A3, B3, N>, A0, B0, A1, B1, A2, B2, A3, B3, false>, N, grid);
        MIX_FIXED4_PLANS(X)
#undef X
    default: break;
    }
    if (real) return hipErrorNotSupported;
    switch (fixed) {
#define X(Pn, A0, B0, A1, B1, A2, B2, N) \
    case Pn: return go(stft_mixed_fixed_bands_kernel<Fixed3<Pn, A0, B0, A1, B1, A2, B2, N>, A0, B0, A1, B1, A2, B2, false>, N, grid);
        MIX_FIXED_PLANS(X)
#undef X
    default: break;
    }
    return hipErrorNotSupported;
}

}  // namespace mix
}  // namespace sgx
