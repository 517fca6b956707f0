// stft_mixed_kernels.hpp -- the device code, plan tables and launch helper that the mixed-radix translation units share: stft_mixed.hip (rows
// and pixels, and all host code), stft_mixed_bands.hip, stft_mixed_complex.hip and stft_istft.hip each instantiate kernels of their own from it.
//
// The family: STFT for windows whose padded length P = 2W is not a power of two but has only the prime
// factors 2, 3, 5 and 7: a mixed-radix FFT of exactly P points, in place in LDS.
//
// The reference sizes its window from a duration: FastFourierTransform::new(sample_rate, 0.05)
// (gpu_spectrogram.rs:323, simple_spectrogram.rs:217) gives W = 2400 at 48 kHz (P = 4800 = 2^6 3 5^2) and
// W = 2205 at 44.1 kHz (P = 4410 = 2 3^2 5 7^2); FFTW takes any length (fft.rs:20-24).  The chirp-z kernel
// (stft_bluestein.hip) serves every length with two power-of-two transforms of >= 3W points; for the smooth
// lengths the application actually produces, this kernel does a quarter of that arithmetic.
//
// Decimation in frequency, one stage per radix R of the current block length Ns (m = Ns / R):
//   y_k = (sum_q x[q m + j] w_R^{q k}) * w_Ns^{j k},  stored at k m + j      (k < R, j < m)
// after which sub-block k is the length-m problem of the bins = k (mod R).  Bin K ends at pos[K] (mixed-radix
// digit reversal, a host table); the split reads F[k] and F[P - k] through it.
//
// Round 2: a stage's radix is a PRODUCT of two prime-ish factors (R = RA RB <= 28: 4800 = 20 x 15 x 16, 4410 =
// 21 x 15 x 14), its R-point DFT done in registers (RB transforms of RA points, constant twiddles, RA transforms of
// RB points), so a transform makes three trips through LDS instead of six; the first stage reads the windowed
// samples straight from the stream (no staging trip for the input), the last (m = 1) has no twiddles; a stage's
// twiddles w_Ns^{j k}, k = 1 .. R-1, lie side by side in a per-stage table (16-byte reads instead of R-1 gathers
// from the full circle); the LDS image is padded by one point per R_last points (the last stage reads at a lane stride of R
// points); the split reads both positions of a bin from one packed word.  Measured at W = 2400, hop 93, stereo
// (SQ counters, profiles/r02_mixed_radix.txt): the first version kept the LDS array busy 62 % of the launch, 58 %
// of that in bank conflicts, and the address unit 58 %.
//
// The lengths the usual device rates produce (and the powers of two without a tuned kernel) run instantiations whose
// whole plan is a compile-time constant (stft_mixed_fixed_kernel / stft_mixed_fixed4_kernel, MIX_FIXED_PLANS): the same
// stage() over FixGeo instead of DynGeo; half the registers, workgroups of 512 / 1024 threads, +24 % to +64 %.
//
// Round 4: REAL-INPUT MODE -- a mono stream in the default mode (every frame its own transform; include/sgx.h, "Mono streams") runs the
// W-point plan on z[m] = x[2m] + i x[2m+1] and an untangling epilogue (untangle_store / pixel_epilogue_real) instead of the 2W-point plan
// on (s, s): half the transform per frame.  The chirp-z kernels below (lengths with a prime factor above 7) take the same mode.
#pragma once
#include <algorithm>
#include <vector>

#include <hip/hip_fp16.h>

#include "mix_codelets.hpp"
#include "pixel_passes.hpp"
#include "sgx_internal.hpp"

namespace sgx {

namespace mix {

constexpr int kMaxStages = 8;
constexpr uint32_t kMaxRadix = 28;

struct MixTables {
    DeviceBuffer<uint32_t> d_split;  // [M] padded position of bin k | padded position of bin P - k << 16   (k = j + 1)
    DeviceBuffer<float2> d_tw;       // per stage: [m][R - 1] w_Ns^{j k}
    uint32_t n_stages = 0, pad_every = 0, lds_points = 0, threads = 0;
    int fixed = 0;                // P when the host's plan is the compile-time one of a fixed kernel (MIX_FIXED_PLANS), else 0
    // real-input mode (a mono stream, every frame its own transform): the plan of the W-point transform of z[m] = x[2m] + i x[2m+1]
    // with its own d_split ([W / 2]: positions of Z[k] and Z[W - k], k = j + 1) and the untangling twiddles w_2W^k
    TablesPtr<MixTables> half;
    DeviceBuffer<float2> d_twr;
    uint32_t ra[kMaxStages] = {}, rb[kMaxStages] = {}, m[kMaxStages] = {}, tw_off[kMaxStages] = {};
    uint32_t q_stride[kMaxStages] = {}, blk_stride[kMaxStages] = {};   // padded LDS positions: see stage()
    float inv_m[kMaxStages] = {};
};

struct Params {
    const float *pcm;
    const float *window;
    const float2 *tw;
    const uint32_t *split;
    float *mags;
    unsigned long long first_frame, pair_base, n_frames, total_frames;
    uint32_t mono_pairs, W, P, H, C, pairs, n_stages, vec2;
    uint32_t real;       // real-input mode: P = W points, the first stage reads sample PAIRS, the epilogue untangles (untangle_store)
    const float2 *twr;   // [W / 2] w_2W^k, k = j + 1
    uint32_t out_f16;   // magnitudes are stored as (l, r) half pairs, 4 B per bin (the F16F16 ring of gpu_spectrogram.rs:218-226)
    float scale, inv_pad;
    // fused pixel stage (fixed plans only): magnitudes never leave LDS
    uint32_t render, R, n_samples, interp;
    const RowEntry *rows;
    const SampleEntry *samples;
    const uint2 *pal;          // [256] {threshold to leave level i, RGBA of level i}
    float guess_a, guess_b;    // level ~ floor(log2(power + 1e-7) a + b - 1/2), then one compare (wg::seed_within_one holds)
    uint8_t *rgba;             // [F][pairs][R][4]
    // chirp-z through the same stages (lengths with a prime factor above 7): the transform length is a compile-time power of two,
    // P stays 2 W, the first stage multiplies by the chirp, the split reads natural-order positions and multiplies again
    const float2 *chirp;       // [P] exp(-i pi n^2 / P), or null
    const float2 *bhat;        // [LDS image] FFT_L(conj chirp) / L at the padded digit-reversed positions, zero in the padding
    uint32_t ra[kMaxStages], rb[kMaxStages], m[kMaxStages], tw_off[kMaxStages], q_stride[kMaxStages], blk_stride[kMaxStages];
    float inv_m[kMaxStages];
};

typedef float v2f_a4 __attribute__((ext_vector_type(2), aligned(4)));   // an 8-byte word at a 4-byte aligned address

struct Source {   // where the first stage finds (l + i r) * hann (fft.rs:53-63); zeros from W on (fft.rs:65-69)
    const float *a, *b;
    uint32_t cl, cr;
    bool data_b;
};

// LDS positions.  The last stage (m = 1) reads R consecutive points per lane -- a lane stride of R points, 32-way bank
// conflicts when R is even -- so the image carries one point of padding per D = R_last points: position(i) = i + i / D.
// Every earlier stage's m is a multiple of R_last, hence of D, which makes the R accesses of a butterfly an arithmetic
// sequence:
//   position(blk m R + j + q m) = blk * blk_stride + j + j / D + q * q_stride      (one add per access)
// with blk_stride = m R (1 + 1 / D) and q_stride = m (1 + 1 / D) from the host (last stage: R + 1 and 1); j / D by one float
// multiply (inv_pad = 0 when the image is not padded).
// A stage's geometry: read from the launch parameters (any supported length), or compile-time constants (the two lengths
// the application itself produces: every index multiply, LDS offset and "is this row inside the window" test folds
// away, and rows of the first stage that lie in the zero padding prune the butterfly at compile time).
struct DynGeo {
    uint32_t m_, count_, qs_, bs_, W_, nt_;
    float inv_m_, inv_pad_;
    bool first_;
    __device__ __forceinline__ uint32_t m() const { return m_; }
    __device__ __forceinline__ uint32_t count() const { return count_; }
    __device__ __forceinline__ uint32_t qs() const { return qs_; }
    __device__ __forceinline__ uint32_t W() const { return W_; }
    __device__ __forceinline__ uint32_t nt() const { return nt_; }
    __device__ __forceinline__ bool first() const { return first_; }
    __device__ __forceinline__ uint32_t blk_of(uint32_t b) const { return (uint32_t)(((float)b + 0.5f) * inv_m_); }  // b / m: exact for every supported length (tests/test_host_logic.py)
    __device__ __forceinline__ uint32_t base_of(uint32_t blk, uint32_t j) const { return blk * bs_ + j + (uint32_t)(((float)j + 0.5f) * inv_pad_); }
};
template <uint32_t M, uint32_t COUNT, uint32_t QS, uint32_t BS, uint32_t WN, uint32_t PAD, uint32_t NT, bool FIRST>
struct FixGeo {
    uint32_t w_rt = 0;   // WN = 0: the number of non-zero inputs is a run-time value (chirp-z)
    __device__ __forceinline__ constexpr uint32_t m() const { return M; }
    __device__ __forceinline__ constexpr uint32_t count() const { return COUNT; }
    __device__ __forceinline__ constexpr uint32_t qs() const { return QS; }
    __device__ __forceinline__ constexpr uint32_t W() const { return WN ? WN : w_rt; }
    __device__ __forceinline__ constexpr uint32_t nt() const { return NT; }
    __device__ __forceinline__ constexpr bool first() const { return FIRST; }
    __device__ __forceinline__ uint32_t blk_of(uint32_t b) const { return b / M; }
    __device__ __forceinline__ uint32_t base_of(uint32_t blk, uint32_t j) const { return blk * BS + j + (PAD ? j / (PAD ? PAD : 1u) : 0u); }
};

// REAL: 1 / 0 at compile time, -1 = p.real (the run-time plan).  Real-input mode: complex sample n of the first stage is
// (x[2n] hann[2n], x[2n + 1] hann[2n + 1]) of the one mono frame, g.W() = ceil(W / 2) of them; p.vec2 = both as 8-byte words.
template <int RA, int RB, typename Geo, int REAL = 0>
__device__ __forceinline__ void stage(float2 *s, const Params &p, const float2 *tw, const Geo g, const Source &src, uint32_t tid)
{
    constexpr int R = RA * RB;
    const bool real = REAL < 0 ? p.real != 0 : REAL != 0;
    const uint32_t m = g.m(), qs = g.qs();
    const uint32_t q_nz = g.first() ? (g.W() + m - 1) / m : (uint32_t)R;   // first stage: rows q >= q_nz lie wholly in the padding
    for (uint32_t b = tid; b < g.count(); b += g.nt()) {
        const uint32_t blk = g.first() ? 0u : g.blk_of(b);
        const uint32_t j = b - blk * m;
        float2 *at = s + g.base_of(blk, j);
        float2 x[R];
        if (g.first()) {   // blk = 0: sample n = q m + j; a lane past the window loads sample W - 1 and drops it
#pragma unroll
            for (int q = 0; q < R; ++q) {
                x[q] = make_float2(0.0f, 0.0f);
                if ((uint32_t)q < q_nz) {   // uniform
                    const uint32_t n = q * m + j, nc = n < g.W() ? n : g.W() - 1;
                    if (real) {   // uniform
                        float2 x2, w2;
                        if (p.vec2) {   // an even W: whole pairs.  The samples' 8-byte words are 4-byte aligned at odd hops / stream offsets:
                                        // loads of two dwords need dword alignment only (v2f_a4 tells the compiler as much)
                            const v2f_a4 xv = *reinterpret_cast<const v2f_a4 *>(src.a + 2 * nc);
                            x2 = make_float2(xv.x, xv.y);
                            w2 = *reinterpret_cast<const float2 *>(p.window + 2 * nc);
                        } else {   // an odd W ends on half a pair
                            const bool whole = 2 * nc + 1 < p.W;
                            x2 = make_float2(src.a[2 * nc], whole ? src.a[2 * nc + 1] : 0.0f);
                            w2 = make_float2(p.window[2 * nc], whole ? p.window[2 * nc + 1] : 0.0f);
                        }
                        if (n < g.W()) x[q] = p.chirp ? cmul(make_float2(x2.x * w2.x, x2.y * w2.y), p.chirp[nc]) : make_float2(x2.x * w2.x, x2.y * w2.y);
                        continue;
                    }
                    const float w = p.window[nc];
                    float l, r;
                    if (p.vec2) {   // uniform
                        const float2 lr = *reinterpret_cast<const float2 *>(src.a + (nc * p.C + src.cl));
                        l = lr.x;
                        r = lr.y;
                    } else {
                        l = src.a[nc * p.C + src.cl];
                        r = src.data_b ? src.b[nc * p.C + src.cr] : 0.0f;
                    }
                    if (n < g.W()) x[q] = p.chirp ? cmul(make_float2(l * w, r * w), p.chirp[nc]) : make_float2(l * w, r * w);
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < R; ++q) x[q] = at[q * qs];
        }
        dft_composite<RA, RB>(x);
        at[0] = x[0];
        if (m == 1 || j == 0) {
#pragma unroll
            for (int k = 1; k < R; ++k) at[k * qs] = x[k];
        } else {
            const float2 *twj = tw + (size_t)j * (R - 1);
#pragma unroll
            for (int k = 1; k < R; ++k) at[k * qs] = cmul(x[k], twj[k - 1]);
        }
    }
    __syncthreads();
}

// The inverse of stage() on the same positions: x[q m + j] = sum_k (y_k conj(w_Ns^{j k})) conj(w_R^{q k}), unnormalised, through
// the forward butterfly: IDFT(v) = conj(DFT(conj(v))).
template <int RA, int RB, typename Geo>
__device__ __forceinline__ void stage_inv(float2 *s, const float2 *tw, const Geo g, uint32_t tid)
{
    constexpr int R = RA * RB;
    const uint32_t m = g.m(), qs = g.qs();
    for (uint32_t b = tid; b < g.count(); b += g.nt()) {
        const uint32_t blk = g.blk_of(b);
        const uint32_t j = b - blk * m;
        float2 *at = s + g.base_of(blk, j);
        float2 x[R];
        const float2 y0 = at[0];
        x[0] = make_float2(y0.x, -y0.y);
        if (m == 1 || j == 0) {
#pragma unroll
            for (int k = 1; k < R; ++k) { const float2 y = at[k * qs]; x[k] = make_float2(y.x, -y.y); }
        } else {
            const float2 *twj = tw + (size_t)j * (R - 1);
#pragma unroll
            for (int k = 1; k < R; ++k) { const float2 y = at[k * qs]; x[k] = cmul(make_float2(y.x, -y.y), twj[k - 1]); }
        }
        dft_composite<RA, RB>(x);
#pragma unroll
        for (int q = 0; q < R; ++q) at[q * qs] = make_float2(x[q].x, -x[q].y);
    }
    __syncthreads();
}

#define MIX_STAGE_CASES(X) X(7, 4) X(7, 3) X(7, 2) X(5, 5) X(5, 4) X(5, 3) X(5, 2) X(4, 4) X(4, 3) X(4, 2) X(3, 3) X(3, 2) \
                           X(7, 1) X(5, 1) X(4, 1) X(3, 1) X(2, 1)

// (l, r) of one frame -- or, for a mono stream, frames 2q and 2q+1 by GLOBAL index (see sgx_kernels.hip)
__device__ __forceinline__ void frame_source(const Params &p, uint32_t pair, Source &src, long long &row_a, long long &row_b)
{
    row_b = -1;
    src.data_b = true;
    if (p.mono_pairs) {
        const unsigned long long fa = 2 * (p.pair_base + blockIdx.x), fb = fa + 1;
        row_a = (long long)fa - (long long)p.first_frame;
        row_b = row_a + 1;
        src.data_b = fb < p.total_frames;
        src.a = p.pcm + (size_t)(fa * p.H);
        src.b = src.data_b ? src.a + p.H : src.a;
        src.cl = src.cr = 0;
    } else {
        row_a = (long long)blockIdx.x;
        src.a = src.b = p.pcm + (size_t)((p.first_frame + blockIdx.x) * p.H) * p.C;
        src.cl = p.C == 1 ? 0 : 2 * pair;
        src.cr = p.C == 1 ? 0 : 2 * pair + 1;
    }
}

// |re + i im| * hs through the hardware square root (1 ulp; the tuned kernels' choice: the correctly rounded sqrtf is a dozen more
// vector instructions per bin -- 12-14 % of this kernel's instruction count, round 4), hs = scale / 2 (an exact halving)
__device__ __forceinline__ float mag_of(float re, float im, float hs) { return __builtin_amdgcn_sqrtf(fmaf(re, re, im * im)) * hs; }

// split + magnitude + scale (fft.rs:81-98); k = 1 .. W-1 kept
__device__ __forceinline__ void split_store(const Params &p, const float2 *s, uint32_t pair, long long row_a, long long row_b, uint32_t tid, uint32_t nt)
{
    const uint32_t M = p.W - 1;
    const bool st_a = row_a >= 0 && (unsigned long long)row_a < p.n_frames;
    const bool st_b = p.mono_pairs && row_b >= 0 && (unsigned long long)row_b < p.n_frames;
    const size_t off_a = ((size_t)(st_a ? row_a : 0) * p.pairs + pair) * M, off_b = ((size_t)(st_b ? row_b : 0) * p.pairs + pair) * M;
    float2 *out_a = reinterpret_cast<float2 *>(p.mags) + off_a, *out_b = reinterpret_cast<float2 *>(p.mags) + off_b;
    __half2 *half_a = reinterpret_cast<__half2 *>(p.mags) + off_a, *half_b = reinterpret_cast<__half2 *>(p.mags) + off_b;
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
        const float left = mag_of(sre, sim, 0.5f * p.scale), right = mag_of(dre, dim, 0.5f * p.scale);
        if (p.out_f16) {   // round to nearest even, as the conversion pass of the kernels without a native half store
            if (p.mono_pairs) {
                if (st_a) half_a[j] = __floats2half2_rn(left, left);
                if (st_b) half_b[j] = __floats2half2_rn(right, right);
            } else {
                half_a[j] = __floats2half2_rn(left, right);
            }
        } else if (p.mono_pairs) {
            if (st_a) st_stream(out_a + j, left, left);
            if (st_b) st_stream(out_b + j, right, right);
        } else {
            st_stream(out_a + j, left, right);
        }
    }
}

// Real-input mode: the image holds Z = FFT_W(z), z[m] = x[2m] + i x[2m+1] of ONE real frame x.  With E / O the transforms of the
// even / odd samples, 2 E[k] = Z[k] + conj Z[W-k], 2 O[k] = -i (Z[k] - conj Z[W-k]), the frame's 2W-point spectrum is
// S[k] = E[k] + w_2W^k O[k] and S[W-k] = conj(E[k] - w_2W^k O[k]): one (k, W-k) pair of the image gives bins k and W-k, k = 1 .. W/2
// (the same identity as stft4096_real.hip; W even: k = W/2 is its own partner and both formulas give the same magnitude).
__device__ __forceinline__ float2 untangle(const Params &p, const float2 *s, uint32_t k1)
{
    float2 a, b;
    if (p.chirp) {   // chirp-z: natural order, one point of padding in 16; Z[k] = c[k] y[k] (P = W here)
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
    const float ux = sre + tx, uy = sim + ty, vx = sre - tx, vy = sim - ty;
    return make_float2(mag_of(ux, uy, 0.5f * p.scale), mag_of(vx, vy, 0.5f * p.scale));
}

__device__ __forceinline__ void untangle_store(const Params &p, const float2 *s, long long row, uint32_t tid, uint32_t nt)
{
    const uint32_t M = p.W - 1, K = p.W / 2;
    float2 *out = reinterpret_cast<float2 *>(p.mags) + (size_t)row * M;
    __half2 *half = reinterpret_cast<__half2 *>(p.mags) + (size_t)row * M;
    for (uint32_t k1 = tid; k1 < K; k1 += nt) {   // bin k = k1 + 1 is row element k1, bin W - k element M - 1 - k1
        const float2 m = untangle(p, s, k1);
        if (p.out_f16) {
            half[k1] = __floats2half2_rn(m.x, m.x);
            half[M - 1 - k1] = __floats2half2_rn(m.y, m.y);
        } else {
            st_stream(out + k1, m.x, m.x);
            st_stream(out + (M - 1 - k1), m.y, m.y);
        }
    }
}

// ... and the pixel stage on it: the column (s, s) of the one frame, then pixel_passes as below (the launch asks for LDS for the column
// and its samples, which the W-point image alone would not hold).
template <uint32_t NT, uint32_t WN, bool BANDS = false>   // BANDS: the column's float means, no colour (pixel_passes)
__device__ __forceinline__ void pixel_epilogue_real(const Params &p, float2 *s, long long row, uint32_t tid)
{
    constexpr uint32_t M = WN - 1, K = WN / 2, kPer = (K + NT - 1) / NT;
    float2 mg[kPer];
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
        const uint32_t k1 = tid + NT * i;
        mg[i] = k1 < K ? untangle(p, s, k1) : make_float2(0.0f, 0.0f);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
        const uint32_t k1 = tid + NT * i;
        if (k1 < K) {
            s[k1] = make_float2(mg[i].x, mg[i].x);
            s[M - 1 - k1] = make_float2(mg[i].y, mg[i].y);
        }
    }
    __syncthreads();
    pixel_passes<NT, BANDS>(p, s, s + M + 1, M, false, 0u, row, -1, tid);
}

// The pixel stage on the transform's own LDS image (magnitude_in -> color_for -> put_pixel, simple_spectrogram.rs:141-161), as
// the two-pass kernel of sgx_kernels.hip does it on magnitudes from HBM: every thread first takes its bins' magnitudes
// into registers (all reads of the transform happen before anything is written over it), the column goes to s[0 .. M), the
// interpolated samples behind it, then one thread per row.  A mono stream carries two frames per transform: .x / .y of a
// bin are the two columns, each an (s, s) pixel.  256-level palettes without the diverging branch whose thresholds pass
// the seed proof only (mixed_can_fuse_render); everything else takes the two-kernel route.
template <uint32_t NT, uint32_t WN, bool BANDS = false>
__device__ __forceinline__ void pixel_epilogue(const Params &p, float2 *s, uint32_t pair, long long row_a, long long row_b, uint32_t tid)
{
    constexpr uint32_t M = WN - 1, kPer = (M + NT - 1) / NT;
    float2 mg[kPer];
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
        const uint32_t j = tid + NT * i;
        mg[i] = make_float2(0.0f, 0.0f);
        if (j < M) {
            const uint32_t w = p.split[j];
            const float2 a = s[w & 0xffffu], b = s[w >> 16];
            const float sre = a.x + b.x, sim = a.y - b.y;
            const float dre = a.x - b.x, dim = a.y + b.y;
            mg[i] = make_float2(mag_of(sre, sim, 0.5f * p.scale), mag_of(dre, dim, 0.5f * p.scale));
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
        const uint32_t j = tid + NT * i;
        if (j < M) s[j] = mg[i];
    }
    __syncthreads();
    pixel_passes<NT, BANDS>(p, s, s + M + 1, M, p.mono_pairs != 0, pair, row_a, row_b, tid);
}

// The two lengths the application produces (0.05 s at 48 and 44.1 kHz), three stages each, everything about the plan a
// compile-time constant.  PAD = R2 (even) -> position(i) = i + i / R2; the host checks that its own plan for the length is
// exactly this one before it launches these (mixed_init).
template <int P_, int R0A, int R0B, int R1A, int R1B, int R2A, int R2B, int NT_>
struct Fixed3 {
    static constexpr uint32_t P = P_, W = (P_ + 1) / 2, NT = NT_;   // W: the non-zero inputs (real-input mode runs odd P)
    static constexpr uint32_t R0 = R0A * R0B, R1 = R1A * R1B, R2 = R2A * R2B;
    static constexpr uint32_t M0 = P / R0, M1 = M0 / R1, M2 = 1;
    static constexpr uint32_t PAD = R2 % 2 == 0 ? R2 : 0;   // an odd lane stride needs no padding
    static constexpr uint32_t pp(uint32_t i) { return i + (PAD ? i / (PAD ? PAD : 1) : 0); }
    static constexpr uint32_t TW1 = M0 * (R0 - 1);   // offset of the second stage's twiddle rows
    static_assert(M1 == R2 && M0 % R2 == 0 && R0 * R1 * R2 == P, "plan shape");
};

template <int P_, int R0A, int R0B, int R1A, int R1B, int R2A, int R2B, int R3A, int R3B, int NT_>
struct Fixed4 {
    static constexpr uint32_t P = P_, W = (P_ + 1) / 2, NT = NT_;   // W: the non-zero inputs (real-input mode runs odd P)
    static constexpr uint32_t R0 = R0A * R0B, R1 = R1A * R1B, R2 = R2A * R2B, R3 = R3A * R3B;
    static constexpr uint32_t M0 = P / R0, M1 = M0 / R1, M2 = M1 / R2;
    static constexpr uint32_t PAD = R3 % 2 == 0 ? R3 : 0;
    static constexpr uint32_t pp(uint32_t i) { return i + (PAD ? i / (PAD ? PAD : 1) : 0); }
    static constexpr uint32_t TW1 = M0 * (R0 - 1), TW2 = TW1 + M1 * (R1 - 1);
    static_assert(M2 == R3 && M1 % R3 == 0 && M0 % R3 == 0 && R0 * R1 * R2 * R3 == P, "plan shape");
};

// The kernels of a compile-time plan -- these, the bands ones (stft_mixed_bands.hip) and the complex-row ones (stft_mixed_complex.hip) -- are
// wrappers around their shape's body (fixed3_body, fixed4_body) with an epilogue E: what becomes of the finished transform.  A wrapper
// keeps its name, template parameters and launch bounds, and tools/isa_unchanged.py holds its code to what it was, by symbol.  That check
// is also why the other shapes (run-time geometry, two frames per workgroup, chirp-z) are still copies: DESIGN.md, "Complex rows".
template <typename F, int R0A, int R0B, int R1A, int R1B, int R2A, int R2B, bool REAL, typename E>
__device__ __forceinline__ void fixed3_body(const Params &p)
{
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
    E::template run<F, REAL>(p, s, pair, row_a, row_b, tid);
}

// The one plan whose kernels keep the body's text in themselves: through fixed3_body the 2205-point kernels at 192 threads come out with
// two instructions of their last stage in another order (profiles/r08_shared_bodies.txt), and every kernel is to compile to what it was.
template <typename F>
constexpr bool kOwnText = F::P == 2205 && F::NT == 192;

// The launch bound of the kernels that take TWO frames per workgroup (stft_mixed_real2_render_kernel, stft_mixed_real2_bands_kernel): the
// waves per SIMD the LDS lets stay resident -- two images, or the column with ~2300 samples behind it -- so that the register budget is
// no tighter than the occupancy the kernel can have anyway
template <typename F>
constexpr unsigned real2_waves_per_simd()
{
    constexpr size_t lds = (size_t)(2 * F::pp(F::P) > F::P + 2304 ? 2 * F::pp(F::P) : F::P + 2304) * sizeof(float2);
    constexpr size_t wgs = 160 * 1024 / lds < 1 ? 1 : 160 * 1024 / lds;
    constexpr size_t waves = wgs * (2 * F::NT / 64) / 4;
    return waves < 1 ? 1u : (waves > 8 ? 8u : (unsigned)waves);
}

template <typename F, int R0A, int R0B, int R1A, int R1B, int R2A, int R2B, int R3A, int R3B, bool REAL, typename E>
__device__ __forceinline__ void fixed4_body(const Params &p)
{
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
    stage<R2A, R2B>(s, p, p.tw + F::TW2, FixGeo<F::M2, F::P / F::R2, F::pp(F::M2), F::pp(F::M1), F::W, F::PAD, F::NT, false>{}, src, tid);
    stage<R3A, R3B>(s, p, p.tw, FixGeo<1, F::P / F::R3, 1, F::pp(F::M2), F::W, F::PAD, F::NT, false>{}, src, tid);
    E::template run<F, REAL>(p, s, pair, row_a, row_b, tid);
}

// L, the stages, threads (W 86 .. 5461; shorter windows keep the radix-4 ladder of stft_bluestein.hip)
#define CHIRP_PLANS3(X) X(512, 4, 1, 4, 2, 4, 4, 128) X(1024, 4, 1, 4, 4, 4, 4, 256) X(2048, 4, 2, 4, 4, 4, 4, 256) X(4096, 4, 4, 4, 4, 4, 4, 256)
#define CHIRP_PLANS4(X) X(8192, 4, 1, 4, 2, 4, 4, 4, 4, 512) X(16384, 4, 1, 4, 4, 4, 4, 4, 4, 1024)

// P, the three stages (RA, RB), threads.  0.05 s at 48 / 44.1 / 32 / 16 / 8 / 88.2 kHz.  512 threads where a stage has more than
// 256 butterflies (62-64 registers: eight waves per SIMD; same-device A/B at 4800 points: 256 threads 1.41 ms per 100 000
// stereo frames, 320 1.31, 512 1.33; at 4410: 1.21 / 1.17 / 1.14).
#define MIX_FIXED_PLANS(X) X(4800, 5, 4, 5, 3, 4, 4, 512) X(4410, 7, 3, 5, 3, 7, 2, 512) X(3200, 5, 4, 5, 2, 4, 4, 512) \
                           X(1600, 5, 4, 5, 1, 4, 4, 512) X(800, 5, 2, 5, 1, 4, 4, 256) X(8820, 7, 3, 7, 3, 5, 4, 512) \
                           X(2048, 4, 2, 4, 4, 4, 4, 256) X(1024, 4, 1, 4, 4, 4, 4, 256) \
                           X(2400, 5, 3, 5, 2, 4, 4, 256) X(2205, 7, 3, 5, 3, 7, 1, 192) \
                           X(4096, 4, 4, 4, 4, 4, 4, 256) X(512, 4, 1, 4, 2, 4, 4, 128)
// (2400, 2205, 4096, 512: the W-point transforms of real-input mode at 48 and 44.1 kHz and at W 4096 / 512; every plan is instantiated for both modes.  Same-device
// A/B, mono, 262 144 frames at hop 93, rows / PCM -> pixels: 2400 points at 192 threads 2.07 / 3.86 ms, 256 2.03 / 3.25, 320 2.17 / 3.07,
// 512 2.23 / 2.77; 2205 points at 160 2.02 / 4.31, 192 1.97 / 3.89, 256 1.99 / 3.46, 320 2.22 / 3.27 -- the transform wants one
// butterfly per thread, the pixel stage behind it every thread it can get: real-input mode to pixels runs these two plans wider)
#define MIX_REAL_RENDER_PLANS(X) X(2400, 5, 3, 5, 2, 4, 4, 512) X(2205, 7, 3, 5, 3, 7, 1, 320)
// ... and every three-stage plan with TWO frames per workgroup (threads per FRAME here):
// stft_mixed_real2_render_kernel
#define MIX_REAL2_RENDER_PLANS(X) X(2400, 5, 3, 5, 2, 4, 4, 256) X(2205, 7, 3, 5, 3, 7, 1, 192) X(4800, 5, 4, 5, 3, 4, 4, 512) \
                                  X(4410, 7, 3, 5, 3, 7, 2, 512) X(4096, 4, 4, 4, 4, 4, 4, 256) X(1024, 4, 1, 4, 4, 4, 4, 256) \
                                  X(512, 4, 1, 4, 2, 4, 4, 128) X(1600, 5, 4, 5, 1, 4, 4, 256) X(800, 5, 2, 5, 1, 4, 4, 128) \
                                  X(3200, 5, 4, 5, 2, 4, 4, 256) X(8820, 7, 3, 7, 3, 5, 4, 512)
// four stages: 0.05 s at 96 / 192 / 176.4 kHz, and the 8192-point power of two
#define MIX_FIXED4_PLANS(X) X(9600, 4, 3, 5, 2, 5, 1, 4, 4, 1024) X(19200, 5, 3, 5, 1, 4, 4, 4, 4, 1024) \
                            X(17640, 5, 3, 7, 2, 4, 3, 7, 1, 1024) X(8192, 4, 1, 4, 2, 4, 4, 4, 4, 512)

// Every launch of the family goes through here: `lds` bytes of dynamic LDS for the transform's image, nt threads.  An image above the
// 64 KiB a kernel may have by default (a CU has 160) has to be asked for as a function attribute first.  Returns that call's error, else
// hipSuccess; an error of the launch itself is left for the caller's hipGetLastError.
template <typename K>
hipError_t launch_kernel(K kernel, const Params &p, unsigned nt, dim3 grid, size_t lds, hipStream_t stream)
{
    if (lds > 64 * 1024) {  // per launch: the attribute is per device, and a process may hold contexts on several
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, grid, dim3(nt), lds, stream, p);
    return hipSuccess;
}

// the bands instantiations (stft_mixed_bands.hip): the kernel of the plan `fixed` that launch_mixed would run to pixels (real-input mode,
// two frames per workgroup, as it chose them), writing the (l, r) means instead; hipErrorNotSupported when no bands kernel has that plan
hipError_t launch_bands_kernel(const Params &p, int fixed, bool real, bool two_frames, dim3 grid, size_t lds, hipStream_t stream);
bool bands_kernel_exists(int fixed, bool real, bool two_frames);
// the complex-row instantiations (stft_mixed_complex.hip, sgx_stft_batch_complex): the row kernel launch_mixed / launch_chirpz would run
hipError_t launch_complex_kernel(const Params &p, int fixed, bool real, unsigned threads, dim3 grid, size_t lds, hipStream_t stream);
hipError_t launch_chirpz_complex_kernel(const Params &p, uint32_t L, bool real, dim3 grid, size_t lds, hipStream_t stream);

}  // namespace mix

}  // namespace sgx
