// stft_istft.hip -- sgx_istft_batch: PCM from the complex (L, R) spectra of sgx_stft_batch_complex by weighted overlap-add.
//
// Per frame and channel (include/sgx.h states the definition the tests hold the kernel to):
//   g[n] = 1/2 Re sum_{k=1}^{W-1} L[k] e^{+i pi k n / W},  n in [0, 2W)          (the bins the forward keeps)
//   c_e, c_o = minus the mean of g over the even / odd n of the padding half [W, 2W)   (DC and Nyquist by least squares)
//   f[m] = g[m] + c_{m mod 2},  m in [0, W)
//   x[n] = sum_t w[m] f_t[m] / sum_t w[m]^2,  m = n - t H,  frames t of the call in ascending order; 0 where the envelope is 0
//
// One 2W-point complex inverse per frame carries both channels: Z[k] = L[k] + i R[k], Z[P - k] = conj L[k] + i conj R[k], Z[0] = Z[W] = 0;
// Re z = g_l, Im z = g_r.  Two routes through the composite stages of stft_mixed_kernels.hpp (run-time geometry, DynGeo):
//   route 1, 2W 2-3-5-7-smooth: Z at the digit-reversed positions of the 2W-point plan, stage_inv back to natural order; c_e, c_o from the
//            padding half in the time domain;
//   route 2, any other 2W with 3W - 1 <= 16384: chirp-z, z[n] = conj c[n] sum_k (Z[k] conj c[k]) c[n - k], c[n] = e^{-i pi n^2 / P}, as a
//            circular convolution of L = pow2 >= 3W - 1 points (forward stages, B^, inverse stages) -- only n in [0, W) is formed, so c_e, c_o
//            come from the spectrum through two per-bin weight tables: sum over the even (odd) n in [W, 2W) of g = 1/2 Re sum_k L[k] E[k].
//
// Persistent workgroups: workgroup (x, pair) owns a run of output hops [ta, tb) of one channel pair and first transforms the (W - 1) / H
// frames before the run, so that no sample needs a partner workgroup.  The overlap accumulates in a register ring of RS x threads >= W
// samples per channel; thread tid owns ring slots tid + i threads.  After frame t every sample below (t + 1) H has all its frames: block t
// ([tH, tH + H)) is divided by its envelope, stored, and its slots are cleared.  Each sample's sum runs over its frames in ascending order
// from zero in every workgroup and call, so the output is bit-identical however the sample range is split.  No atomics.
#include "stft_mixed_kernels.hpp"

#include <cmath>

namespace sgx {
namespace istft {

// ring slots per thread and channel at most (istft_kernel<kMaxRing>): 512 threads x 20 = 10 240 samples, the largest W of the composite
// stages (2W <= 20 480)
constexpr uint32_t kMaxRing = 20;

struct IParams {
    mix::Params mp;              // stage geometry (ra, rb, m, tw_off, q_stride, blk_stride, inv_m, inv_pad, tw) of the Q-point plan
    const float4 *spec;          // [n_frames][pairs][W - 1] (L.re, L.im, R.re, R.im)
    float *out;                  // [s1 - s0][C]
    const float *window;         // [W] the context's float32 Hann (w[0] = 0)
    const uint32_t *split;       // route 1: [W - 1] padded position of bin k | of bin P - k << 16
    const float2 *chirp;         // route 2: [P] e^{-i pi n^2 / P}
    const float2 *bhat;          // route 2: [image] FFT_L(b) / L at the padded digit-reversed positions, b[d] = c[|d|], d in (-P, W)
    const float4 *parity;        // route 2: [W - 1] (T_e, T_o), T = -E / (2 |S|): c = sum_k Re(L[k] T[k])
    unsigned long long n_frames, s0, s1, b0, b_end, run;
    uint32_t W, P, H, C, pairs, Q, pos_w, n_stages, chirp_route, mono, vec2;
    float k_e, k_o;              // route 1: -1 / |S_e|, -1 / |S_o|; route 2: 1
};

__device__ __forceinline__ uint32_t padpos(const IParams &p, uint32_t i) { return i + (uint32_t)(((float)i + 0.5f) * p.mp.inv_pad); }

__device__ __forceinline__ mix::DynGeo geo(const IParams &p, uint32_t st, uint32_t nt)
{
    mix::DynGeo g;
    g.m_ = p.mp.m[st];
    g.count_ = p.Q / (p.mp.ra[st] * p.mp.rb[st]);
    g.qs_ = p.mp.q_stride[st];
    g.bs_ = p.mp.blk_stride[st];
    g.W_ = p.Q;
    g.nt_ = nt;
    g.inv_m_ = p.mp.inv_m[st];
    g.inv_pad_ = p.mp.inv_pad;
    g.first_ = false;
    return g;
}

// frame t of the pair -> z[n] = (g_l, g_r)[n] at padpos(n), n in [0, W); returns (c_e,l, c_e,r, c_o,l, c_o,r)
__device__ __forceinline__ float4 inverse_frame(const IParams &p, float2 *s, unsigned long long t, uint32_t pair, uint32_t tid, uint32_t nt)
{
    const uint32_t W = p.W, M = W - 1;
    const float4 *row = p.spec + ((size_t)t * p.pairs + pair) * M;
    float pe_l = 0.0f, pe_r = 0.0f, po_l = 0.0f, po_r = 0.0f;
    __syncthreads();   // the previous frame's reads of the image are done
    if (!p.chirp_route) {
        for (uint32_t j = tid; j < M; j += nt) {
            float4 v = row[j];
            if (p.mono) { v.z = 0.0f; v.w = 0.0f; }
            const uint32_t w = p.split[j];
            s[w & 0xffffu] = make_float2(0.25f * (v.x - v.w), 0.25f * (v.y + v.z));
            s[w >> 16] = make_float2(0.25f * (v.x + v.w), 0.25f * (v.z - v.y));
        }
        if (tid == 0) { s[0] = make_float2(0.0f, 0.0f); s[p.pos_w] = make_float2(0.0f, 0.0f); }
        __syncthreads();
    } else {
        for (uint32_t j = tid; j < M; j += nt) {
            float4 v = row[j];
            if (p.mono) { v.z = 0.0f; v.w = 0.0f; }
            const float4 T = p.parity[j];
            pe_l = fmaf(v.x, T.x, fmaf(-v.y, T.y, pe_l));
            pe_r = fmaf(v.z, T.x, fmaf(-v.w, T.y, pe_r));
            po_l = fmaf(v.x, T.z, fmaf(-v.y, T.w, po_l));
            po_r = fmaf(v.z, T.z, fmaf(-v.w, T.w, po_r));
            const uint32_t k = j + 1, kp = p.P - k;
            const float2 a = make_float2(0.25f * (v.x - v.w), 0.25f * (v.y + v.z));
            const float2 b = make_float2(0.25f * (v.x + v.w), 0.25f * (v.z - v.y));
            const float2 ck = p.chirp[k], ckp = p.chirp[kp];
            s[padpos(p, k)] = mix::cmul(a, make_float2(ck.x, -ck.y));
            s[padpos(p, kp)] = mix::cmul(b, make_float2(ckp.x, -ckp.y));
        }
        if (tid == 0) { s[0] = make_float2(0.0f, 0.0f); s[padpos(p, W)] = make_float2(0.0f, 0.0f); }
        for (uint32_t i = p.P + tid; i < p.Q; i += nt) s[padpos(p, i)] = make_float2(0.0f, 0.0f);
        __syncthreads();
        mix::Source src{};
        for (uint32_t st = 0; st < p.n_stages; ++st) {
            const uint32_t code = p.mp.ra[st] * 8 + p.mp.rb[st];
            const mix::DynGeo g = geo(p, st, nt);
            const float2 *tw = p.mp.tw + p.mp.tw_off[st];
            switch (code) {
#define X(A, B) case A * 8 + B: mix::stage<A, B, mix::DynGeo, 0>(s, p.mp, tw, g, src, tid); break;
                MIX_STAGE_CASES(X)
#undef X
            default: break;
            }
        }
        const uint32_t img = padpos(p, p.Q - 1) + 1;
        for (uint32_t i = tid; i < img; i += nt) s[i] = mix::cmul(s[i], p.bhat[i]);
        __syncthreads();
    }
    for (int st = (int)p.n_stages - 1; st >= 0; --st) {
        const uint32_t code = p.mp.ra[st] * 8 + p.mp.rb[st];
        const mix::DynGeo g = geo(p, (uint32_t)st, nt);
        const float2 *tw = p.mp.tw + p.mp.tw_off[st];
        switch (code) {
#define X(A, B) case A * 8 + B: mix::stage_inv<A, B, mix::DynGeo>(s, tw, g, tid); break;
            MIX_STAGE_CASES(X)
#undef X
        default: break;
        }
    }
    if (!p.chirp_route) {   // the padding half in the time domain: a thread's n = W + tid + k nt all have one parity (nt is even)
        float sl = 0.0f, sr = 0.0f;
        for (uint32_t n = W + tid; n < 2 * W; n += nt) {
            const float2 v = s[padpos(p, n)];
            sl += v.x;
            sr += v.y;
        }
        if ((W + tid) & 1u) { po_l = sl; po_r = sr; } else { pe_l = sl; pe_r = sr; }
    }
    // block sum in a fixed order: the butterfly of a wave (every lane gets the same bits), then the waves in order through the image
    // positions W, W + 1, ... (past the samples the ring reads)
    for (int off = 32; off > 0; off >>= 1) {
        pe_l += __shfl_xor(pe_l, off);
        pe_r += __shfl_xor(pe_r, off);
        po_l += __shfl_xor(po_l, off);
        po_r += __shfl_xor(po_r, off);
    }
    __syncthreads();
    const uint32_t wave = tid >> 6, n_waves = nt >> 6;
    if ((tid & 63u) == 0) {
        s[padpos(p, W + 2 * wave)] = make_float2(pe_l, pe_r);
        s[padpos(p, W + 2 * wave + 1)] = make_float2(po_l, po_r);
    }
    __syncthreads();
    float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (uint32_t i = 0; i < n_waves; ++i) {
        const float2 e = s[padpos(p, W + 2 * i)], o = s[padpos(p, W + 2 * i + 1)];
        c.x += e.x;
        c.y += e.y;
        c.z += o.x;
        c.w += o.y;
    }
    return make_float4(c.x * p.k_e, c.y * p.k_e, c.z * p.k_o, c.w * p.k_o);
}

// the envelope sum_t w[n - tH]^2 of sample n = tH + r (0 <= r < H) over the frames [0, n_frames) that cover it, ascending t
__device__ __forceinline__ float envelope(const IParams &p, unsigned long long t, uint32_t r)
{
    if (r >= p.W) return 0.0f;
    unsigned long long jmax = (p.W - 1 - r) / p.H;
    if (jmax > t) jmax = t;
    const unsigned long long jmin = t >= p.n_frames ? t - (p.n_frames - 1) : 0ull;
    float e = 0.0f;
    for (unsigned long long j = jmax + 1; j-- > jmin;) {
        const float w = p.window[r + (uint32_t)j * p.H];
        e += w * w;
    }
    return e;
}

__device__ __forceinline__ void store(const IParams &p, uint32_t pair, unsigned long long n, float l, float r)
{
    float *o = p.out + (size_t)(n - p.s0) * p.C;
    if (p.mono) o[0] = l;
    else if (p.vec2) *reinterpret_cast<float2 *>(o + 2 * pair) = make_float2(l, r);
    else { o[2 * pair] = l; o[2 * pair + 1] = r; }
}

template <int RS>
__global__ void __launch_bounds__(512) istft_kernel(IParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2 *s = reinterpret_cast<float2 *>(smem_raw);
    const uint32_t tid = threadIdx.x, nt = blockDim.x, pair = blockIdx.y;
    const uint32_t W = p.W, H = p.H, ring = RS * nt;
    const unsigned long long ta = p.b0 + (unsigned long long)blockIdx.x * p.run;
    if (ta >= p.b_end) return;   // uniform
    const unsigned long long tb = ta + p.run < p.b_end ? ta + p.run : p.b_end;
    const unsigned long long kw = (W - 1) / H;
    const unsigned long long t0 = ta > kw ? ta - kw : 0ull;
    float acc_l[RS], acc_r[RS];
#pragma unroll
    for (int i = 0; i < RS; ++i) { acc_l[i] = 0.0f; acc_r[i] = 0.0f; }
    for (unsigned long long t = t0; t < tb; ++t) {
        const uint32_t base = (uint32_t)((t * H) % ring);   // ring slot of sample tH
        if (t < p.n_frames) {   // uniform
            const float4 c = inverse_frame(p, s, t, pair, tid, nt);
#pragma unroll
            for (int i = 0; i < RS; ++i) {
                const uint32_t slot = tid + (uint32_t)i * nt;
                const uint32_t m = slot >= base ? slot - base : slot + ring - base;
                if (m < W) {
                    float2 v = s[padpos(p, m)];
                    if (p.chirp_route) { const float2 cm = p.chirp[m]; v = mix::cmul(v, make_float2(cm.x, -cm.y)); }
                    const float w = p.window[m];
                    const bool odd = m & 1u;
                    acc_l[i] += w * (v.x + (odd ? c.z : c.x));
                    acc_r[i] += w * (v.y + (odd ? c.w : c.y));
                }
            }
        }
        // block t is complete: samples [tH, tH + H)
        const bool emit = t >= ta;
        const unsigned long long n0 = t * H;
#pragma unroll
        for (int i = 0; i < RS; ++i) {
            const uint32_t slot = tid + (uint32_t)i * nt;
            const uint32_t r = slot >= base ? slot - base : slot + ring - base;
            if (r < H) {
                const unsigned long long n = n0 + r;
                if (emit && n >= p.s0 && n < p.s1) {
                    const float e = envelope(p, t, r);
                    store(p, pair, n, e > 0.0f ? acc_l[i] / e : 0.0f, e > 0.0f ? acc_r[i] / e : 0.0f);
                }
                acc_l[i] = 0.0f;
                acc_r[i] = 0.0f;
            }
        }
        if (emit && H > ring)   // hops beyond the ring (H > W): no frame covers [tH + ring, tH + H)
            for (uint32_t r = ring + tid; r < H; r += nt) {
                const unsigned long long n = n0 + r;
                if (n >= p.s0 && n < p.s1) store(p, pair, n, 0.0f, 0.0f);
            }
    }
}

struct ITables {
    TablesPtr<mix::MixTables> plan;   // the Q-point stage plan (route 1: Q = 2W, route 2: Q = L)
    uint32_t route = 0, Q = 0, pos_w = 0;
    DeviceBuffer<float2> d_chirp, d_bhat;   // (route 2 only, as d_parity: else null)
    DeviceBuffer<float4> d_parity;
    float k_e = 0.0f, k_o = 0.0f;
};

// the padded digit-reversed position of bin K of the plan (bin K = k1 + r1 (k2 + r2 (...)) ends at k1 m1 + k2 m2 + ...)
static uint32_t digit_pos(const mix::MixTables *t, uint32_t K)
{
    uint32_t k = K, at = 0;
    for (uint32_t i = 0; i < t->n_stages; ++i) {
        const uint32_t r = t->ra[i] * t->rb[i];
        at += (k % r) * t->m[i];
        k /= r;
    }
    return at + (t->pad_every ? at / t->pad_every : 0u);
}

// float64 radix-2 FFT, e^{-2 pi i k n / N} (table set-up only)
static void fft_host(std::vector<double> &re, std::vector<double> &im)
{
    const size_t n = re.size();
    for (size_t i = 1, j = 0; i < n; ++i) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) { std::swap(re[i], re[j]); std::swap(im[i], im[j]); }
    }
    for (size_t len = 2; len <= n; len <<= 1)
        for (size_t k = 0; k < len / 2; ++k) {
            const double ang = -2.0 * M_PI * (double)k / (double)len, wr = cos(ang), wi = sin(ang);
            for (size_t i = 0; i < n; i += len) {
                const size_t a = i + k, b = a + len / 2;
                const double tr = re[b] * wr - im[b] * wi, ti = re[b] * wi + im[b] * wr;
                re[b] = re[a] - tr;
                im[b] = im[a] - ti;
                re[a] += tr;
                im[a] += ti;
            }
        }
}

// e^{i pi x / W} for an integer x, the angle reduced exactly
static void cis_pi(unsigned long long x, uint32_t W, double &re, double &im)
{
    const double ang = M_PI * (double)(x % (2ull * W)) / (double)W;
    re = cos(ang);
    im = sin(ang);
}

}  // namespace istft

int istft_route(const sgx_ctx *c)
{
    if (c->stft_kernel == kKernelLarge) return 0;
    if (c->W > istft::kMaxRing * 512) return 0;   // (no such W outside kernel 11: mixed_supported and bluestein_supported stop below)
    if (mixed_supported(c->W)) return 1;
    if (bluestein_supported(c->W)) return 2;
    return 0;
}

void TablesDelete::operator()(istft::ITables *t) const { delete t; }

hipError_t istft_init(sgx_ctx *c)
{
    using namespace istft;
    const int route = istft_route(c);
    if (!route) return hipErrorInvalidValue;
    const uint32_t W = c->W, P = c->P;
    TablesPtr<ITables> t(new ITables());
    t->route = (uint32_t)route;
    uint32_t Q = P;
    if (route == 2) { Q = 1; while (Q < 3 * W - 1) Q <<= 1; }
    t->Q = Q;
    hipError_t e = mixed_length_tables(Q, t->plan);
    if (e != hipSuccess) return e;
    const uint32_t cnt_e = W / 2, cnt_o = W - W / 2;   // even / odd n in [W, 2W)
    if (route == 1) {
        t->pos_w = digit_pos(t->plan.get(), W);
        t->k_e = -1.0f / (float)cnt_e;
        t->k_o = -1.0f / (float)cnt_o;
    } else {
        t->k_e = t->k_o = 1.0f;
        std::vector<float2> chirp(P);
        std::vector<double> cr(P), ci(P);
        for (uint32_t n = 0; n < P; ++n) {
            const unsigned long long q = ((unsigned long long)n * n) % (2ull * P);   // n^2 mod 2P: exact
            const double ang = -M_PI * (double)q / (double)P;
            cr[n] = cos(ang);
            ci[n] = sin(ang);
            chirp[n] = make_float2((float)cr[n], (float)ci[n]);
        }
        // b[d] = c[|d|] for d in [-(P - 1), W - 1], wrapped modulo Q
        std::vector<double> br(Q, 0.0), bi(Q, 0.0);
        for (uint32_t d = 0; d < W; ++d) { br[d] = cr[d]; bi[d] = ci[d]; }
        for (uint32_t d = 1; d < P; ++d) { br[Q - d] = cr[d]; bi[Q - d] = ci[d]; }
        fft_host(br, bi);
        std::vector<float2> bhat(t->plan->lds_points, make_float2(0.0f, 0.0f));
        for (uint32_t K = 0; K < Q; ++K) bhat[digit_pos(t->plan.get(), K)] = make_float2((float)(br[K] / (double)Q), (float)(bi[K] / (double)Q));
        // E_S[k] = sum_{n in S} e^{i pi k n / W} over S = {n0, n0 + 2, ...} (cnt terms): e^{i pi k n0 / W} (1 - rho^cnt) / (1 - rho), rho = e^{2 i pi k / W}
        std::vector<float4> par(std::max<uint32_t>(W - 1, 1));
        auto weight = [&](uint32_t k, uint32_t n0, uint32_t cnt, float &tr, float &ti) {
            double ar, ai, qr, qi, rr, ri;
            cis_pi((unsigned long long)k * n0, W, ar, ai);
            cis_pi(2ull * k * cnt, W, qr, qi);
            cis_pi(2ull * k, W, rr, ri);
            const double nr = 1.0 - qr, ni = -qi, dr = 1.0 - rr, di = -ri, dd = dr * dr + di * di;
            const double gr = (nr * dr + ni * di) / dd, gi = (ni * dr - nr * di) / dd;
            const double er = ar * gr - ai * gi, ei = ar * gi + ai * gr;
            tr = (float)(-er / (2.0 * cnt));
            ti = (float)(-ei / (2.0 * cnt));
        };
        const uint32_t n_even = W % 2 ? W + 1 : W, n_odd = W % 2 ? W : W + 1;
        for (uint32_t j = 0; j + 1 < W; ++j) {
            float4 v;
            weight(j + 1, n_even, cnt_e, v.x, v.y);
            weight(j + 1, n_odd, cnt_o, v.z, v.w);
            par[j] = v;
        }
        e = t->d_chirp.upload(chirp);
        if (e == hipSuccess) e = t->d_bhat.upload(bhat);
        if (e == hipSuccess) e = t->d_parity.upload(par);
    }
    if (e == hipSuccess) c->istft = std::move(t);
    return e;
}

hipError_t launch_istft(const sgx_ctx *c, const float *d_spec, size_t n_frames, size_t s0, size_t s1, float *d_pcm)
{
    using namespace istft;
    const ITables *t = c->istft.get();
    const mix::MixTables *pl = t->plan.get();
    IParams p{};
    p.mp.tw = pl->d_tw.get();
    p.mp.inv_pad = pl->pad_every ? 1.0f / (float)pl->pad_every : 0.0f;
    for (uint32_t i = 0; i < pl->n_stages; ++i) {
        p.mp.ra[i] = pl->ra[i];
        p.mp.rb[i] = pl->rb[i];
        p.mp.m[i] = pl->m[i];
        p.mp.tw_off[i] = pl->tw_off[i];
        p.mp.q_stride[i] = pl->q_stride[i];
        p.mp.blk_stride[i] = pl->blk_stride[i];
        p.mp.inv_m[i] = pl->inv_m[i];
    }
    p.spec = reinterpret_cast<const float4 *>(d_spec);
    p.out = d_pcm;
    p.window = c->d_window.get();
    p.split = pl->d_split.get();
    p.chirp = t->d_chirp.get();
    p.bhat = t->d_bhat.get();
    p.parity = t->d_parity.get();
    p.n_frames = n_frames;
    p.s0 = s0;
    p.s1 = s1;
    p.W = c->W;
    p.P = c->P;
    p.H = c->H;
    p.C = c->C;
    p.pairs = c->pairs;
    p.Q = t->Q;
    p.pos_w = t->pos_w;
    p.n_stages = pl->n_stages;
    p.chirp_route = t->route == 2 ? 1u : 0u;
    p.mono = c->C == 1 ? 1u : 0u;
    p.vec2 = reinterpret_cast<uintptr_t>(d_pcm) % 8 == 0 ? 1u : 0u;
    p.k_e = t->k_e;
    p.k_o = t->k_o;
    const uint32_t pairs = c->pairs, H = c->H;
    p.b0 = s0 / H;
    p.b_end = (s1 - 1) / H + 1;
    const unsigned long long n_blocks = p.b_end - p.b0;
    const unsigned long long kw = (c->W - 1) / H;
    // threads: the plan's, at most the kernel's bound of 512 (registers: no spill), and enough for a ring of at most kMaxRing slots per thread
    uint32_t nt = std::min<uint32_t>(pl->threads, 512);
    while (nt < 512 && (c->W + nt - 1) / nt > kMaxRing) nt += 64;
    const uint32_t ring_need = (c->W + nt - 1) / nt;
    const size_t lds = (size_t)pl->lds_points * sizeof(float2);
    if (c->W + 2 * (nt / 64) > t->Q) return hipErrorInvalidValue;   // the block sum's scratch lies at positions W .. W + 2 waves of the image
    auto go = [&](auto kernel) -> hipError_t {
        if (lds > 64 * 1024) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        // persistent workgroups: as many as the device keeps resident (this instantiation's registers, block size and LDS image: asked once
        // and cached), over all pairs; a run at least as long as its warm-up
        const std::array<size_t, 3> key = {(size_t)reinterpret_cast<uintptr_t>(reinterpret_cast<const void *>(kernel)), (size_t)nt, lds};
        int per_cu = 0;
        for (const auto &kv : c->occupancy_cache)
            if (kv.first == key) per_cu = kv.second;
        if (per_cu == 0) {
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, (int)nt, lds) != hipSuccess || per_cu < 1) per_cu = 1;
            c->occupancy_cache.push_back({key, per_cu});
        }
        unsigned long long groups = std::max<unsigned long long>(1ull, (unsigned long long)c->n_cu * (unsigned long long)per_cu / pairs);
        unsigned long long run = (n_blocks + groups - 1) / groups;
        if (run < kw + 1) run = kw + 1;
        groups = (n_blocks + run - 1) / run;
        if (groups > 0x7fffffffull) return hipErrorInvalidValue;
        p.run = run;
        hipLaunchKernelGGL(kernel, dim3((unsigned)groups, pairs), dim3(nt), lds, c->stream, p);
        return hipGetLastError();
    };
    if (ring_need <= 2) return go(istft_kernel<2>);
    if (ring_need <= 4) return go(istft_kernel<4>);
    if (ring_need <= 8) return go(istft_kernel<8>);
    if (ring_need <= 16) return go(istft_kernel<16>);
    if (ring_need <= kMaxRing) return go(istft_kernel<kMaxRing>);
    return hipErrorInvalidValue;
}

}  // namespace sgx
