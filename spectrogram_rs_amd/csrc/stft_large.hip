// stft_large.hip -- STFT for transform lengths that no in-LDS kernel serves (SGX_FLAG_LARGE_TRANSFORM, stft_kernel 11): 2W up to 2^21.
//
// The transform is staged through a device-memory scratch that the context holds (large_plan.hpp: the plan rule, the scratch size).
// Four-step factorisation of an L-point DFT, L = N1 x N2, n = N2 n1 + n2, k = k1 + N1 k2:
//
//   X[k1 + N1 k2] = sum_n2 w_N2^(n2 k2) [ w_L^(n2 k1) sum_n1 x[N2 n1 + n2] w_N1^(n1 k1) ]
//
// The scratch of one transform is an [N1][N2] row-major array, so column n2 of the input and row k1 of the output lie where the
// natural index says: element (r, c) at r N2 + c in every pass.
//
// 2W 2-3-5-7-smooth (L = P = 2W), three launches per chunk:
//   A  cols:  a workgroup gathers adjacent columns (block_shape) of the windowed (l, r) frame straight from the PCM stream (the zero
//             half n >= W is not read), runs their N1-point transforms in LDS, multiplies by w_P^(n2 k1) (a float64-derived [N1][N2]
//             table) and writes them back as rows of the scratch.
//   B  rows:  a workgroup loads whole rows (contiguous), runs their N2-point transforms and writes X in NATURAL order to a
//             second scratch buffer (consecutive lanes: consecutive k1, i.e. consecutive bins).
//   S  split: F[k] and F[P - k] from the natural buffer, hypot and the 2/W scale (fft.rs:81-98), [frames][pairs][M][2] rows.
//   The split has a pass of its own rather than pairing row k1 with its mirror N1 - k1 inside pass B: bin P - k lies in row N1 - k1 at
//   column N2 - 1 - k2, so a mirrored workgroup would still write the output with a stride of N1 bins; the extra pass reads the natural
//   buffer and writes the rows contiguously, one 8-byte (l, r) pair per lane.
//
// Every other W: chirp-z (the identity of stft_bluestein.hip, F[k] = c[k] sum_n (z[n] c[n]) conj(c)[k - n], c[n] = exp(-i pi n^2 / P))
// over L = pow2 >= 3W - 1 (a power of two: the convolution spectrum is then a float64 radix-2 FFT at create time, and the pass count
// is the same as for a smooth L), four launches per chunk, the scratch updated in place:
//   A  cols:  as above on z[n] c[n].
//   B  rows:  forward N2-point rows, times the chirp spectrum B^ / L (stored [k1][k2]), inverse N2-point rows, times w_L^-(m2 k1).
//   C  cols:  inverse N1-point columns: y[m2 + N2 m1] lands at its natural index.
//   S  split: on c[k] y[k].
//
// Sub-transforms are Stockham stages (natural in, natural out, ping-pong between two LDS buffers;
// block_shape: ~kBlockPts / 2 points per workgroup at an odd stride) of radix 4, 2, 3, 5
// and 7 with twiddles from float64-derived tables of the N-th roots.  Pass boundaries are kernel launches on the context's stream.
// Mono streams: every frame its own (s, s) transform.
#include "large_plan.hpp"
#include "sgx_internal.hpp"

#include <algorithm>
#include <cmath>

namespace sgx {

namespace large {

constexpr unsigned kThreads = 256;

struct Geo {
    const float2 *roots;   // [N] e^{-2 pi i m / N}
    uint32_t N, nst;
    uint8_t rad[kMaxStages];
};

struct Params {
    const float *pcm;
    const float *window;
    const float2 *chirp;   // [P] c[n] (chirp-z) or null
    const float2 *tw;      // [N1][N2] w_L^(k1 n2)
    const float2 *bt;      // [N1][N2] B^[k1 + N1 k2] / L (chirp-z) or null
    float2 *scr;           // [chunk][L]
    float2 *nat;           // [chunk][P] natural-order spectrum (direct) or null
    float *mags;
    Geo g1, g2;
    unsigned long long first_frame, t0;   // t0: the chunk's first transform (frame-major, pair-minor) of the call
    uint32_t W, P, L, N1, N2, H, C, pairs, M;
    uint32_t Bc, ld1, Br, ld2;   // sub-transforms per workgroup and their LDS stride (block_shape), columns and rows
    float scale;
};

struct LargeTables {
    Plan pl;
    DeviceBuffer<float2> d_roots1, d_roots2, d_tw, d_chirp, d_bt;   // (d_chirp, d_bt: null unless the plan is chirp-z)
    DeviceBuffer<float2> d_scratch;
    uint32_t chunk = 0;   // transforms per chunk
    Geo g1{}, g2{};
};

__device__ __forceinline__ float2 cmul(float2 a, float2 b)
{
    return make_float2(fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x));
}
__device__ __forceinline__ float2 cmul_conj(float2 a, float2 b)  // a * conj(b)
{
    return make_float2(fmaf(a.x, b.x, a.y * b.y), fmaf(a.y, b.x, -(a.x * b.y)));
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// cos / sin of 2 pi m / R, m = 1 .. R / 2 (R = 3, 5, 7)
template <int R> struct Unit;
template <> struct Unit<3> { static constexpr float c[2] = {1.0f, -0.5f}, s[2] = {0.0f, 0.86602540378443865f}; };
template <> struct Unit<5> { static constexpr float c[3] = {1.0f, 0.30901699437494742f, -0.80901699437494742f},
                                                    s[3] = {0.0f, 0.95105651629515357f, 0.58778525229247313f}; };
template <> struct Unit<7> { static constexpr float c[4] = {1.0f, 0.62348980185873353f, -0.22252093395631440f, -0.90096886790241913f},
                                                    s[4] = {0.0f, 0.78183148246802981f, 0.97492791218182361f, 0.43388373911755812f}; };

// y[q] = sum_r v[r] e^{-+2 pi i r q / R}: pairs (v[r], v[R - r]) share the cosine, their difference takes the sine
template <int R>
__device__ __forceinline__ void dft_odd(float2 *v, bool inv)
{
    float2 sum[R / 2 + 1], dif[R / 2 + 1];
#pragma unroll
    for (int r = 1; r <= R / 2; ++r) { sum[r] = cadd(v[r], v[R - r]); dif[r] = csub(v[r], v[R - r]); }
    float2 y[R];
    y[0] = v[0];
#pragma unroll
    for (int r = 1; r <= R / 2; ++r) y[0] = cadd(y[0], sum[r]);
#pragma unroll
    for (int q = 1; q <= R / 2; ++q) {
        float2 a = v[0], b = make_float2(0.0f, 0.0f);
#pragma unroll
        for (int r = 1; r <= R / 2; ++r) {
            const int m = (r * q) % R, mm = m <= R / 2 ? m : R - m;
            const float cs = Unit<R>::c[mm], sn = m <= R / 2 ? Unit<R>::s[mm] : -Unit<R>::s[mm];
            a.x = fmaf(cs, sum[r].x, a.x);
            a.y = fmaf(cs, sum[r].y, a.y);
            b.x = fmaf(sn, dif[r].x, b.x);
            b.y = fmaf(sn, dif[r].y, b.y);
        }
        // forward: y[q] = a - i b, y[R - q] = a + i b (inverse: the other way round)
        const float2 mi = make_float2(a.x + b.y, a.y - b.x), pi = make_float2(a.x - b.y, a.y + b.x);
        y[q] = inv ? pi : mi;
        y[R - q] = inv ? mi : pi;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = y[r];
}

template <int R>
__device__ __forceinline__ void dft(float2 *v, bool inv)
{
    if constexpr (R == 2) {
        const float2 a = v[0], b = v[1];
        v[0] = cadd(a, b);
        v[1] = csub(a, b);
    } else if constexpr (R == 4) {
        const float2 a0 = cadd(v[0], v[2]), a1 = csub(v[0], v[2]), b0 = cadd(v[1], v[3]), b1 = csub(v[1], v[3]);
        const float2 mi = make_float2(a1.x + b1.y, a1.y - b1.x), pi = make_float2(a1.x - b1.y, a1.y + b1.x);   // a1 - i b1, a1 + i b1
        v[0] = cadd(a0, b0);
        v[2] = csub(a0, b0);
        v[1] = inv ? pi : mi;
        v[3] = inv ? mi : pi;
    } else {
        dft_odd<R>(v, inv);
    }
}

// one Stockham stage over B transforms of N points: src -> dst, Ns = product of the radices before this one
template <int R>
__device__ __forceinline__ void stage(const float2 *src, float2 *dst, uint32_t B, uint32_t ld, const Geo &g, uint32_t Ns, bool inv)
{
    const uint32_t N = g.N, NR = N / R, stride = NR / Ns;
    for (uint32_t idx = threadIdx.x; idx < B * NR; idx += blockDim.x) {
        const uint32_t b = idx / NR, j = idx - b * NR, k = j % Ns;
        const float2 *s = src + (size_t)b * ld;
        float2 v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = s[j + r * NR];
        if (Ns > 1) {
#pragma unroll
            for (int r = 1; r < R; ++r) {
                const float2 w = g.roots[k * r * stride];   // e^{-2 pi i k r / (Ns R)}
                v[r] = inv ? cmul_conj(v[r], w) : cmul(v[r], w);
            }
        }
        dft<R>(v, inv);
        float2 *d = dst + (size_t)b * ld + (j - k) * R + k;
#pragma unroll
        for (int r = 0; r < R; ++r) d[r * Ns] = v[r];
    }
}

// B transforms of g.N points in LDS, ld apart (a: input, b: the other buffer); returns the buffer holding the result
__device__ float2 *sub_fft(float2 *a, float2 *b, uint32_t B, uint32_t ld, const Geo &g, bool inv)
{
    uint32_t Ns = 1;
    for (uint32_t st = 0; st < g.nst; ++st) {
        const uint32_t R = g.rad[st];
        if (R == 4) stage<4>(a, b, B, ld, g, Ns, inv);
        else if (R == 2) stage<2>(a, b, B, ld, g, Ns, inv);
        else if (R == 3) stage<3>(a, b, B, ld, g, Ns, inv);
        else if (R == 5) stage<5>(a, b, B, ld, g, Ns, inv);
        else stage<7>(a, b, B, ld, g, Ns, inv);
        __syncthreads();
        float2 *t = a; a = b; b = t;
        Ns *= R;
    }
    return a;
}

// passes A (FROM_PCM: forward, twiddled) and C (inverse columns of the chirp-z path, in place)
template <bool FROM_PCM>
__global__ void __launch_bounds__(kThreads) large_cols_kernel(Params p)
{
    extern __shared__ float2 lds[];
    const uint32_t N1 = p.N1, N2 = p.N2, Bc = p.Bc, ld = p.ld1;
    const uint32_t c0 = blockIdx.x * Bc, ncol = min(Bc, N2 - c0);
    float2 *buf[2] = {lds, lds + Bc * ld};
    float2 *S = p.scr + (size_t)blockIdx.y * p.L;
    const float *src = nullptr;
    uint32_t C = p.C, cl = 0, cr = 0;
    if constexpr (FROM_PCM) {
        const unsigned long long t = p.t0 + blockIdx.y, frame = p.first_frame + t / p.pairs;
        const uint32_t pair = (uint32_t)(t % p.pairs);
        src = p.pcm + (size_t)(frame * p.H) * C;
        cl = C == 1 ? 0 : 2 * pair;
        cr = C == 1 ? 0 : 2 * pair + 1;
    }
    for (uint32_t idx = threadIdx.x; idx < Bc * N1; idx += blockDim.x) {
        const uint32_t c = idx % Bc, n1 = idx / Bc, n = n1 * N2 + c0 + c;
        float2 v = make_float2(0.0f, 0.0f);
        if (c < ncol) {
            if constexpr (FROM_PCM) {
                if (n < p.W) {   // (l + i r) * hann (fft.rs:53-63); n >= W is the zero padding
                    const float w = p.window[n];
                    v = make_float2(src[(size_t)n * C + cl] * w, src[(size_t)n * C + cr] * w);
                    if (p.chirp) v = cmul(v, p.chirp[n]);
                }
            } else {
                v = S[n];
            }
        }
        buf[0][c * ld + n1] = v;
    }
    __syncthreads();
    const float2 *res = sub_fft(buf[0], buf[1], Bc, ld, p.g1, !FROM_PCM);
    for (uint32_t idx = threadIdx.x; idx < Bc * N1; idx += blockDim.x) {
        const uint32_t c = idx % Bc, k1 = idx / Bc, o = k1 * N2 + c0 + c;
        if (c >= ncol) continue;
        float2 v = res[c * ld + k1];
        if constexpr (FROM_PCM) v = cmul(v, p.tw[o]);
        S[o] = v;
    }
}

// pass B: whole rows; direct: natural-order spectrum into p.nat; chirp-z: the convolution and the inverse rows, in place
__global__ void __launch_bounds__(kThreads) large_rows_kernel(Params p)
{
    extern __shared__ float2 lds[];
    const uint32_t N1 = p.N1, N2 = p.N2, Br = p.Br, ld = p.ld2;
    const uint32_t r0 = blockIdx.x * Br, nrow = min(Br, N1 - r0), live = nrow * N2;
    float2 *buf[2] = {lds, lds + Br * ld};
    float2 *S = p.scr + (size_t)blockIdx.y * p.L + (size_t)r0 * N2;
    for (uint32_t i = threadIdx.x; i < Br * N2; i += blockDim.x) {
        const uint32_t r = i / N2;
        buf[0][r * ld + (i - r * N2)] = i < live ? S[i] : make_float2(0.0f, 0.0f);
    }
    __syncthreads();
    float2 *res = sub_fft(buf[0], buf[1], Br, ld, p.g2, false);
    if (!p.bt) {
        float2 *X = p.nat + (size_t)blockIdx.y * p.P;
        for (uint32_t idx = threadIdx.x; idx < Br * N2; idx += blockDim.x) {
            const uint32_t r = idx % Br, k2 = idx / Br;
            if (r < nrow) X[(size_t)(r0 + r) + (size_t)N1 * k2] = res[r * ld + k2];
        }
        return;
    }
    const float2 *bt = p.bt + (size_t)r0 * N2;
    for (uint32_t i = threadIdx.x; i < live; i += blockDim.x) {
        const uint32_t r = i / N2, o = r * ld + (i - r * N2);
        res[o] = cmul(res[o], bt[i]);
    }
    __syncthreads();
    float2 *other = res == buf[0] ? buf[1] : buf[0];
    res = sub_fft(res, other, Br, ld, p.g2, true);
    const float2 *tw = p.tw + (size_t)r0 * N2;
    for (uint32_t i = threadIdx.x; i < live; i += blockDim.x) {
        const uint32_t r = i / N2;
        S[i] = cmul_conj(res[r * ld + (i - r * N2)], tw[i]);
    }
}

// the L/R split of the natural-order spectrum (fft.rs:81-98), k = 1 .. W-1
__global__ void __launch_bounds__(kThreads) large_split_kernel(Params p)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= p.M) return;
    const uint32_t k = j + 1, P = p.P;
    float2 a, b;
    if (p.chirp) {
        const float2 *y = p.scr + (size_t)blockIdx.y * p.L;
        a = cmul(y[k], p.chirp[k]);
        b = cmul(y[P - k], p.chirp[P - k]);
    } else {
        const float2 *X = p.nat + (size_t)blockIdx.y * P;
        a = X[k];
        b = X[P - k];
    }
    const float sre = a.x + b.x, sim = a.y - b.y;
    const float dre = a.x - b.x, dim = a.y + b.y;
    const float left = sqrtf(fmaf(sre, sre, sim * sim)) * 0.5f * p.scale;
    const float right = sqrtf(fmaf(dre, dre, dim * dim)) * 0.5f * p.scale;
    st_stream(reinterpret_cast<float2 *>(p.mags) + ((size_t)(p.t0 + blockIdx.y) * p.M + j), left, right);
}

// ... the complex rows of sgx_stft_batch_complex: L = (a + conj b) / 2, R = (a - conj b) / (2i), each times 2 / W, as float4 per bin
__global__ void __launch_bounds__(kThreads) large_split_complex_kernel(Params p)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= p.M) return;
    const uint32_t k = j + 1, P = p.P;
    float2 a, b;
    if (p.chirp) {
        const float2 *y = p.scr + (size_t)blockIdx.y * p.L;
        a = cmul(y[k], p.chirp[k]);
        b = cmul(y[P - k], p.chirp[P - k]);
    } else {
        const float2 *X = p.nat + (size_t)blockIdx.y * P;
        a = X[k];
        b = X[P - k];
    }
    const float sre = a.x + b.x, sim = a.y - b.y;
    const float dre = a.x - b.x, dim = a.y + b.y;
    reinterpret_cast<float4 *>(p.mags)[(size_t)(p.t0 + blockIdx.y) * p.M + j] = make_float4(sre * 0.5f * p.scale, sim * 0.5f * p.scale, dim * 0.5f * p.scale, -dre * 0.5f * p.scale);
}

// host: how many N-point sub-transforms a workgroup runs (B, at most `count` of them) and their LDS stride.  About kBlockPts / 2 points
// per workgroup (32 KiB of LDS: five workgroups per CU), one transform of up to kBlockPts points where N is longer; the stride is odd
// (N + 1 for an even N) so that the column gather and the row scatter, whose lanes are one stride apart, hit distinct LDS banks
static void block_shape(uint32_t N, uint32_t count, uint32_t &B, uint32_t &ld)
{
    ld = N | 1u;
    B = (kBlockPts / 2) / ld;
    if (B == 0) { B = 1; ld = N; }
    if (B > count) B = count;
}

// host: e^{-2 pi i m / n} for m < count, in float64, one rounding
static std::vector<float2> roots_of(uint64_t n, size_t count)
{
    std::vector<float2> v(count);
    for (size_t m = 0; m < count; ++m) {
        const double ang = -2.0 * M_PI * (double)m / (double)n;
        v[m] = make_float2((float)std::cos(ang), (float)std::sin(ang));
    }
    return v;
}

// host float64 radix-2 FFT, in place (the chirp spectrum at create time)
static void fft_f64(std::vector<double> &re, std::vector<double> &im)
{
    const size_t n = re.size();
    std::vector<double> wr(n / 2), wi(n / 2);
    for (size_t m = 0; m < n / 2; ++m) {
        const double ang = -2.0 * M_PI * (double)m / (double)n;
        wr[m] = std::cos(ang);
        wi[m] = std::sin(ang);
    }
    for (size_t i = 1, j = 0; i < n; ++i) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) { std::swap(re[i], re[j]); std::swap(im[i], im[j]); }
    }
    for (size_t len = 2; len <= n; len <<= 1) {
        const size_t step = n / len;
        for (size_t i = 0; i < n; i += len)
            for (size_t k = 0; k < len / 2; ++k) {
                const double c = wr[k * step], s = wi[k * step];
                const size_t a = i + k, b = a + len / 2;
                const double tr = re[b] * c - im[b] * s, ti = re[b] * s + im[b] * c;
                re[b] = re[a] - tr; im[b] = im[a] - ti;
                re[a] += tr; im[a] += ti;
            }
    }
}

}  // namespace large

bool large_supported(uint32_t W)
{
    large::Plan pl;
    return large::make_plan(W, pl);
}

void TablesDelete::operator()(large::LargeTables *t) const { delete t; }

hipError_t large_init(sgx_ctx *c)
{
    using namespace large;
    TablesPtr<LargeTables> t(new LargeTables());
    if (!make_plan(c->W, t->pl)) return hipErrorInvalidValue;
    const Plan &pl = t->pl;
    const uint32_t N1 = pl.N1, N2 = pl.N2, L = pl.L, P = pl.P, W = pl.W;
    t->g1.N = N1;
    t->g1.nst = sub_radices(N1, t->g1.rad);
    t->g2.N = N2;
    t->g2.nst = sub_radices(N2, t->g2.rad);
    std::vector<float2> tw((size_t)L);
    for (uint32_t k1 = 0; k1 < N1; ++k1)
        for (uint32_t n2 = 0; n2 < N2; ++n2) {
            const double ang = -2.0 * M_PI * (double)(((uint64_t)k1 * n2) % L) / (double)L;
            tw[(size_t)k1 * N2 + n2] = make_float2((float)std::cos(ang), (float)std::sin(ang));
        }
    hipError_t e = t->d_roots1.upload(roots_of(N1, N1));
    if (e == hipSuccess) e = t->d_roots2.upload(roots_of(N2, N2));
    if (e == hipSuccess) e = t->d_tw.upload(tw);
    if (e == hipSuccess && pl.chirp) {
        std::vector<double> cr(P), ci(P);
        std::vector<float2> chirp(P);
        for (uint32_t n = 0; n < P; ++n) {
            const uint64_t q = ((uint64_t)n * n) % (2ull * P);   // n^2 mod 2P: exact
            const double ang = -M_PI * (double)q / (double)P;
            cr[n] = std::cos(ang);
            ci[n] = std::sin(ang);
            chirp[n] = make_float2((float)cr[n], (float)ci[n]);
        }
        // b[m] = conj(c[|m|]) for m in [-(W-1), P-1], wrapped modulo L; B^ = FFT_L(b) / L, stored [k1][k2]
        std::vector<double> br(L, 0.0), bi(L, 0.0);
        for (uint32_t m = 0; m < P; ++m) { br[m] = cr[m]; bi[m] = -ci[m]; }
        for (uint32_t m = 1; m < W; ++m) { br[L - m] = cr[m]; bi[L - m] = -ci[m]; }
        fft_f64(br, bi);
        std::vector<float2> bt((size_t)L);
        for (uint32_t k1 = 0; k1 < N1; ++k1)
            for (uint32_t k2 = 0; k2 < N2; ++k2) {
                const size_t k = (size_t)k1 + (size_t)N1 * k2;
                bt[(size_t)k1 * N2 + k2] = make_float2((float)(br[k] / (double)L), (float)(bi[k] / (double)L));
            }
        e = t->d_chirp.upload(chirp);
        if (e == hipSuccess) e = t->d_bt.upload(bt);
    }
    t->g1.roots = t->d_roots1.get();
    t->g2.roots = t->d_roots2.get();
    // the scratch: as many transforms as fit kScratchBytes (at least one; 2 at 2W = 2^21)
    const size_t per = scratch_per_transform(pl);
    size_t chunk = kScratchBytes / per;
    if (chunk < 1) chunk = 1;
    if (chunk > 65535) chunk = 65535;
    t->chunk = (uint32_t)chunk;
    if (e == hipSuccess) e = t->d_scratch.alloc(chunk * per / sizeof(float2));   // (per: whole complex points)
    if (e == hipSuccess) c->large = std::move(t);
    return e;
}

hipError_t launch_large(const sgx_ctx *c, const StftCall &call)
{
    using namespace large;
    if (call.kind != Out::kMags && call.kind != Out::kComplex) return hipErrorInvalidValue;
    const bool complex_rows = call.kind == Out::kComplex;
    const float *d_pcm = call.pcm;
    float *d_mags = static_cast<float *>(call.out);
    const uint32_t channels = call.channels, pairs = call.pairs;
    const size_t first_frame = call.first, n_frames = call.n, total_frames = call.total;
    (void)total_frames;   // every frame its own transform: no frame pairing
    if (n_frames == 0) return hipSuccess;
    const LargeTables *t = c->large.get();
    const Plan &pl = t->pl;
    Params p{};
    p.pcm = d_pcm;
    p.window = c->d_window.get();
    p.chirp = t->d_chirp.get();
    p.tw = t->d_tw.get();
    p.bt = t->d_bt.get();
    p.scr = t->d_scratch.get();
    p.nat = pl.chirp ? nullptr : t->d_scratch.get() + (size_t)t->chunk * pl.L;
    p.mags = d_mags;
    p.g1 = t->g1;
    p.g2 = t->g2;
    p.first_frame = first_frame;
    p.W = pl.W;
    p.P = pl.P;
    p.L = pl.L;
    p.N1 = pl.N1;
    p.N2 = pl.N2;
    p.H = c->H;
    p.C = channels;
    p.pairs = pairs;
    p.M = pl.W - 1;
    p.scale = 2.0f / (float)pl.W;
    block_shape(pl.N1, pl.N2, p.Bc, p.ld1);
    block_shape(pl.N2, pl.N1, p.Br, p.ld2);
    const uint32_t Bc = p.Bc, Br = p.Br;
    const size_t lds_cols = 2 * (size_t)p.Bc * p.ld1 * sizeof(float2), lds_rows = 2 * (size_t)p.Br * p.ld2 * sizeof(float2);
    const unsigned gx_cols = (pl.N2 + Bc - 1) / Bc, gx_rows = (pl.N1 + Br - 1) / Br, gx_split = (p.M + kThreads - 1) / kThreads;
    const unsigned long long n_tr = (unsigned long long)n_frames * pairs;
    for (unsigned long long done = 0; done < n_tr; done += t->chunk) {
        const unsigned m = (unsigned)std::min<unsigned long long>(t->chunk, n_tr - done);
        p.t0 = done;
        hipLaunchKernelGGL(large_cols_kernel<true>, dim3(gx_cols, m), dim3(kThreads), lds_cols, c->stream, p);
        hipLaunchKernelGGL(large_rows_kernel, dim3(gx_rows, m), dim3(kThreads), lds_rows, c->stream, p);
        if (pl.chirp) hipLaunchKernelGGL(large_cols_kernel<false>, dim3(gx_cols, m), dim3(kThreads), lds_cols, c->stream, p);
        if (complex_rows) hipLaunchKernelGGL(large_split_complex_kernel, dim3(gx_split, m), dim3(kThreads), 0, c->stream, p);
        else hipLaunchKernelGGL(large_split_kernel, dim3(gx_split, m), dim3(kThreads), 0, c->stream, p);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace sgx
