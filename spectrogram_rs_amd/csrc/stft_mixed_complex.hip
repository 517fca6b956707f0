// stft_mixed_complex.hip -- the complex-row instantiations of the mixed-radix and chirp-z kernels (sgx_stft_batch_complex): the same
// transforms as stft_mixed.hip's row kernels, then the (l, r) split -- or real-input mode's untangle -- stored as complex spectra, (L, R) as
// float4 per bin.  A translation unit of its own, as stft_mixed_bands.hip is.
#include "stft_mixed_kernels.hpp"

namespace sgx {
namespace mix {

// fft.rs:81-98 before the magnitude: a = F[k], b = F[P - k]; L = (a + conj b) / 2, R = (a - conj b) / (2i) -- the difference rotated by
// -90 degrees -- each times 2 / W.  Mono frame pairs: (X, X) rows of frames 2q (L) and 2q+1 (R)
__device__ __forceinline__ void split_store_c64(const Params &p, const float2 *s, uint32_t pair, long long row_a, long long row_b, uint32_t tid, uint32_t nt)
{
    const uint32_t M = p.W - 1;
    const float hs = 0.5f * p.scale;
    const bool st_a = row_a >= 0 && (unsigned long long)row_a < p.n_frames;
    const bool st_b = p.mono_pairs && row_b >= 0 && (unsigned long long)row_b < p.n_frames;
    float4 *out_a = reinterpret_cast<float4 *>(p.mags) + ((size_t)(st_a ? row_a : 0) * p.pairs + pair) * M;
    float4 *out_b = reinterpret_cast<float4 *>(p.mags) + ((size_t)(st_b ? row_b : 0) * p.pairs + pair) * M;
    for (uint32_t j = tid; j < M; j += nt) {
        float2 a, b;
        if (p.chirp) {   // natural order after the inverse stages, one point of padding in 16; F[k] = c[k] y[k]
            const uint32_t k = j + 1, kp = p.P - k;
            a = cmul(s[k + (k >> 4)], p.chirp[k]);
            b = cmul(s[kp + (kp >> 4)], p.chirp[kp]);
        } else {
            const uint32_t w = p.split[j];
            a = s[w & 0xffffu];
            b = s[w >> 16];
        }
        const float sre = a.x + b.x, sim = a.y - b.y;
        const float dre = a.x - b.x, dim = a.y + b.y;
        const float lr = sre * hs, li = sim * hs, rr = dim * hs, ri = -dre * hs;
        if (p.mono_pairs) {
            if (st_a) out_a[j] = make_float4(lr, li, lr, li);
            if (st_b) out_b[j] = make_float4(rr, ri, rr, ri);
        } else {
            out_a[j] = make_float4(lr, li, rr, ri);
        }
    }
}

// Real-input mode (see untangle in stft_mixed_kernels.hpp): S[k] = E[k] + w_2W^k O[k] and S[W - k] = conj(E[k] - w_2W^k O[k]); the row holds (S, S)
__device__ __forceinline__ void untangle_store_c64(const Params &p, const float2 *s, long long row, uint32_t tid, uint32_t nt)
{
    const uint32_t M = p.W - 1, K = p.W / 2;
    const float hs = 0.5f * p.scale;
    float4 *out = reinterpret_cast<float4 *>(p.mags) + (size_t)row * M;
    for (uint32_t k1 = tid; k1 < K; k1 += nt) {   // bin k = k1 + 1 is row element k1, bin W - k element M - 1 - k1 (W even, k = W / 2: the same)
        float2 a, b;
        if (p.chirp) {
            const uint32_t k = k1 + 1, kp = p.P - k;
            a = cmul(s[k + (k >> 4)], p.chirp[k]);
            b = cmul(s[kp + (kp >> 4)], p.chirp[kp]);
        } else {
            const uint32_t w = p.split[k1];
            a = s[w & 0xffffu];
            b = s[w >> 16];
        }
        const float2 t = p.twr[k1];
        const float sre = a.x + b.x, sim = a.y - b.y;     // 2 E
        const float dre = a.x - b.x, dim = a.y + b.y;     // 2 i O
        const float tx = t.x * dim + t.y * dre, ty = t.y * dim - t.x * dre;   // w (dim, -dre) = 2 w O
        const float ux = (sre + tx) * hs, uy = (sim + ty) * hs, vx = (sre - tx) * hs, vy = -((sim - ty) * hs);
        out[k1] = make_float4(ux, uy, ux, uy);
        out[M - 1 - k1] = make_float4(vx, vy, vx, vy);
    }
}

// stft_mixed_kernel (run-time geometry) with the complex store.  (A copy, as the chirp-z kernels below: see fixed3_body in stft_mixed_kernels.hpp.)
__global__ void __launch_bounds__(1024) stft_mixed_complex_kernel(Params p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2 *s = reinterpret_cast<float2 *>(smem_raw);
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    const uint32_t pair = blockIdx.y;
    long long row_a, row_b;
    Source src;
    frame_source(p, pair, src, row_a, row_b);

    for (uint32_t st = 0; st < p.n_stages; ++st) {
        const uint32_t code = p.ra[st] * 8 + p.rb[st];  // uniform
        DynGeo g;
        g.m_ = p.m[st];
        g.count_ = p.P / (p.ra[st] * p.rb[st]);
        g.qs_ = p.q_stride[st];
        g.bs_ = p.blk_stride[st];
        g.W_ = p.real ? (p.W + 1) / 2 : p.W;
        g.nt_ = nt;
        g.inv_m_ = p.inv_m[st];
        g.inv_pad_ = p.inv_pad;
        g.first_ = st == 0;
        const float2 *tw = p.tw + p.tw_off[st];
        switch (code) {
#define X(A, B) case A * 8 + B: stage<A, B, DynGeo, -1>(s, p, tw, g, src, tid); break;
            MIX_STAGE_CASES(X)
#undef X
        default: break;
        }
    }
    if (p.real) untangle_store_c64(p, s, row_a, tid, nt);
    else split_store_c64(p, s, pair, row_a, row_b, tid, nt);
}

// stft_mixed_fixed_kernel / stft_mixed_fixed4_kernel (compile-time plans) without the pixel epilogue, with the complex store
struct ComplexRows {
    template <typename F, bool REAL>
    static __device__ __forceinline__ void run(const Params &p, float2 *s, uint32_t pair, long long row_a, long long row_b, uint32_t tid)
    {
        if constexpr (REAL) untangle_store_c64(p, s, row_a, tid, F::NT);   // P is the WINDOW here
        else split_store_c64(p, s, pair, row_a, row_b, tid, F::NT);
    }
};

template <typename F, int R0A, int R0B, int R1A, int R1B, int R2A, int R2B, bool REAL>
__global__ void __launch_bounds__(F::NT, F::NT <= 256 ? 4 : 8) stft_mixed_fixed_complex_kernel(Params p)
{
    fixed3_body<F, R0A, R0B, R1A, R1B, R2A, R2B, REAL, ComplexRows>(p);
}

template <typename F, int R0A, int R0B, int R1A, int R1B, int R2A, int R2B, int R3A, int R3B, bool REAL>
__global__ void __launch_bounds__(F::NT, F::NT == 256 ? 4 : (F::NT == 512 ? 8 : 4)) stft_mixed_fixed4_complex_kernel(Params p)
{
    fixed4_body<F, R0A, R0B, R1A, R1B, R2A, R2B, R3A, R3B, REAL, ComplexRows>(p);
}

// chirpz3_kernel / chirpz4_kernel with the complex store
template <typename F, int R0A, int R0B, int R1A, int R1B, int R2A, int R2B, bool REAL>
__global__ void __launch_bounds__(F::NT, F::NT >= 256 ? 4 : 2) chirpz3_complex_kernel(Params p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2 *s = reinterpret_cast<float2 *>(smem_raw);
    const uint32_t tid = threadIdx.x;
    const uint32_t pair = blockIdx.y;
    long long row_a, row_b;
    Source src;
    frame_source(p, pair, src, row_a, row_b);
    using G0f = FixGeo<F::M0, F::P / F::R0, F::pp(F::M0), F::pp(F::P), 0, F::PAD, F::NT, true>;
    using G0 = FixGeo<F::M0, F::P / F::R0, F::pp(F::M0), F::pp(F::P), 0, F::PAD, F::NT, false>;
    using G1 = FixGeo<F::M1, F::P / F::R1, F::pp(F::M1), F::pp(F::M0), 0, F::PAD, F::NT, false>;
    using G2 = FixGeo<1, F::P / F::R2, 1, F::pp(F::M1), 0, F::PAD, F::NT, false>;
    stage<R0A, R0B, G0f, REAL>(s, p, p.tw, G0f{REAL ? (p.W + 1) / 2 : p.W}, src, tid);
    stage<R1A, R1B>(s, p, p.tw + F::TW1, G1{}, src, tid);
    stage<R2A, R2B>(s, p, p.tw, G2{}, src, tid);
    for (uint32_t i = tid; i < F::pp(F::P); i += F::NT) s[i] = cmul(s[i], p.bhat[i]);
    __syncthreads();
    stage_inv<R2A, R2B>(s, p.tw, G2{}, tid);
    stage_inv<R1A, R1B>(s, p.tw + F::TW1, G1{}, tid);
    stage_inv<R0A, R0B>(s, p.tw, G0{}, tid);
    if constexpr (REAL) untangle_store_c64(p, s, row_a, tid, F::NT);
    else split_store_c64(p, s, pair, row_a, row_b, tid, F::NT);
}

template <typename F, int R0A, int R0B, int R1A, int R1B, int R2A, int R2B, int R3A, int R3B, bool REAL>
__global__ void __launch_bounds__(F::NT, 4) chirpz4_complex_kernel(Params p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2 *s = reinterpret_cast<float2 *>(smem_raw);
    const uint32_t tid = threadIdx.x;
    const uint32_t pair = blockIdx.y;
    long long row_a, row_b;
    Source src;
    frame_source(p, pair, src, row_a, row_b);
    using G0f = FixGeo<F::M0, F::P / F::R0, F::pp(F::M0), F::pp(F::P), 0, F::PAD, F::NT, true>;
    using G0 = FixGeo<F::M0, F::P / F::R0, F::pp(F::M0), F::pp(F::P), 0, F::PAD, F::NT, false>;
    using G1 = FixGeo<F::M1, F::P / F::R1, F::pp(F::M1), F::pp(F::M0), 0, F::PAD, F::NT, false>;
    using G2 = FixGeo<F::M2, F::P / F::R2, F::pp(F::M2), F::pp(F::M1), 0, F::PAD, F::NT, false>;
    using G3 = FixGeo<1, F::P / F::R3, 1, F::pp(F::M2), 0, F::PAD, F::NT, false>;
    stage<R0A, R0B, G0f, REAL>(s, p, p.tw, G0f{REAL ? (p.W + 1) / 2 : p.W}, src, tid);
    stage<R1A, R1B>(s, p, p.tw + F::TW1, G1{}, src, tid);
    stage<R2A, R2B>(s, p, p.tw + F::TW2, G2{}, src, tid);
    stage<R3A, R3B>(s, p, p.tw, G3{}, src, tid);
    for (uint32_t i = tid; i < F::pp(F::P); i += F::NT) s[i] = cmul(s[i], p.bhat[i]);
    __syncthreads();
    stage_inv<R3A, R3B>(s, p.tw, G3{}, tid);
    stage_inv<R2A, R2B>(s, p.tw + F::TW2, G2{}, tid);
    stage_inv<R1A, R1B>(s, p.tw + F::TW1, G1{}, tid);
    stage_inv<R0A, R0B>(s, p.tw, G0{}, tid);
    if constexpr (REAL) untangle_store_c64(p, s, row_a, tid, F::NT);
    else split_store_c64(p, s, pair, row_a, row_b, tid, F::NT);
}

hipError_t launch_complex_kernel(const Params &p, int fixed, bool real, unsigned threads, dim3 grid, size_t lds, hipStream_t stream)
{
    switch (fixed) {
#define X(Pn, A0, B0, A1, B1, A2, B2, N)                                                                                                      \
    case Pn:                                                                                                                                  \
        if (real) return launch_kernel(stft_mixed_fixed_complex_kernel<Fixed3<Pn, A0, B0, A1, B1, A2, B2, N>, A0, B0, A1, B1, A2, B2, true>, p, N, grid, lds, stream); \
        return launch_kernel(stft_mixed_fixed_complex_kernel<Fixed3<Pn, A0, B0, A1, B1, A2, B2, N>, A0, B0, A1, B1, A2, B2, false>, p, N, grid, lds, stream);
        MIX_FIXED_PLANS(X)
#undef X
#define X(Pn, A0, B0, A1, B1, A2, B2, A3, B3, N)                                                                                                               \
    case Pn:                                                                                                                                                   \
        if (real) return launch_kernel(stft_mixed_fixed4_complex_kernel<Fixed4<Pn, A0, B0, A1, B1, A2, B2, A3, B3, N>, A0, B0, A1, B1, A2, B2, A3, B3, true>, p, N, grid, lds, stream); \
        return launch_kernel(stft_mixed_fixed4_complex_kernel<Fixed4<Pn, A0, B0, A1, B1, A2, B2, A3, B3, N>, A0, B0, A1, B1, A2, B2, A3, B3, false>, p, N, grid, lds, stream);
        MIX_FIXED4_PLANS(X)
#undef X
    default: return launch_kernel(stft_mixed_complex_kernel, p, threads, grid, lds, stream);
    }
}

hipError_t launch_chirpz_complex_kernel(const Params &p, uint32_t L, bool real, dim3 grid, size_t lds, hipStream_t stream)
{
    switch (L) {
#define X(Ln, A0, B0, A1, B1, A2, B2, N)                                                                                                    \
    case Ln:                                                                                                                                \
        if (real) return launch_kernel(chirpz3_complex_kernel<Fixed3<Ln, A0, B0, A1, B1, A2, B2, N>, A0, B0, A1, B1, A2, B2, true>, p, N, grid, lds, stream); \
        return launch_kernel(chirpz3_complex_kernel<Fixed3<Ln, A0, B0, A1, B1, A2, B2, N>, A0, B0, A1, B1, A2, B2, false>, p, N, grid, lds, stream);
        CHIRP_PLANS3(X)
#undef X
#define X(Ln, A0, B0, A1, B1, A2, B2, A3, B3, N)                                                                                                           \
    case Ln:                                                                                                                                               \
        if (real) return launch_kernel(chirpz4_complex_kernel<Fixed4<Ln, A0, B0, A1, B1, A2, B2, A3, B3, N>, A0, B0, A1, B1, A2, B2, A3, B3, true>, p, N, grid, lds, stream); \
        return launch_kernel(chirpz4_complex_kernel<Fixed4<Ln, A0, B0, A1, B1, A2, B2, A3, B3, N>, A0, B0, A1, B1, A2, B2, A3, B3, false>, p, N, grid, lds, stream);
        CHIRP_PLANS4(X)
#undef X
    default: return hipErrorInvalidValue;
    }
}

}  // namespace mix
}  // namespace sgx
