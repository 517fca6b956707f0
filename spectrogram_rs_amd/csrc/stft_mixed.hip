// stft_mixed.hip -- the mixed-radix and chirp-z kernels that write rows of magnitudes or the fused pixel column, and the host code of the
// family: plans, tables, routes and launches.  The transform itself -- stages, epilogues, plan tables -- is stft_mixed_kernels.hpp.
#include "stft_mixed_kernels.hpp"

namespace sgx {

namespace mix {

__global__ void __launch_bounds__(1024) stft_mixed_kernel(Params p)
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
    if (p.real) untangle_store(p, s, row_a, tid, nt);
    else split_store(p, s, pair, row_a, row_b, tid, nt);
}

struct RowsOrPixels {   // rows of magnitudes, or with p.render the fused pixel column
    template <typename F, bool REAL>
    static __device__ __forceinline__ void run(const Params &p, float2 *s, uint32_t pair, long long row_a, long long row_b, uint32_t tid)
    {
        if constexpr (REAL) {   // P is the WINDOW here
            if (p.render) pixel_epilogue_real<F::NT, F::P>(p, s, row_a, tid);
            else untangle_store(p, s, row_a, tid, F::NT);
        } else if (p.render) {
            pixel_epilogue<F::NT, F::W>(p, s, pair, row_a, row_b, tid);
        } else {
            split_store(p, s, pair, row_a, row_b, tid, F::NT);
        }
    }
};

template <typename F, int R0A, int R0B, int R1A, int R1B, int R2A, int R2B, bool REAL>
__global__ void __launch_bounds__(F::NT, F::NT <= 256 ? 4 : 8) stft_mixed_fixed_kernel(Params p)
{
    if constexpr (!kOwnText<F>) {
        fixed3_body<F, R0A, R0B, R1A, R1B, R2A, R2B, REAL, RowsOrPixels>(p);
    } else {
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
        if constexpr (REAL) {   // the epilogue too: RowsOrPixels' text
            if (p.render) pixel_epilogue_real<F::NT, F::P>(p, s, row_a, tid);
            else untangle_store(p, s, row_a, tid, F::NT);
        } else if (p.render) {
            pixel_epilogue<F::NT, F::W>(p, s, pair, row_a, row_b, tid);
        } else {
            split_store(p, s, pair, row_a, row_b, tid, F::NT);
        }
    }
}

// Real-input mode from PCM to pixels, TWO frames per workgroup (the two application plans, MIX_REAL2_RENDER_PLANS): each half of the
// workgroup transforms one frame on its own W-point image; then the pixel stage runs ONCE, with every thread, over both columns -- .x / .y
// of a bin, as for a frame pair -- where a mono column alone would carry the same value in both components and do every sum twice.
// (Launch bound: real2_waves_per_simd, stft_mixed_kernels.hpp.)
template <typename F, int R0A, int R0B, int R1A, int R1B, int R2A, int R2B>
__global__ void __launch_bounds__(2 * F::NT, real2_waves_per_simd<F>()) stft_mixed_real2_render_kernel(Params p)
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
    pixel_passes<2 * NT>(p, s, s + M + 1, M, true, 0u, (long long)fa, (long long)fa + 1, tid);
}

template <typename F, int R0A, int R0B, int R1A, int R1B, int R2A, int R2B, int R3A, int R3B, bool REAL>
__global__ void __launch_bounds__(F::NT, F::NT == 256 ? 4 : (F::NT == 512 ? 8 : 4)) stft_mixed_fixed4_kernel(Params p)
{
    fixed4_body<F, R0A, R0B, R1A, R1B, R2A, R2B, R3A, R3B, REAL, RowsOrPixels>(p);
}

// ---- chirp-z (Bluestein) through the same stages: F[k] = c[k] sum_{n<W} (z[n] c[n]) conj(c)[k - n], c[n] = exp(-i pi n^2 / P), as a
// circular convolution of length L = pow2 >= P + W - 1 (stft_bluestein.hip has the derivation and the first implementation, a
// radix-4 ladder): forward stages (the first one reads z[n] hann[n] c[n] from the stream, rows past W are zero), pointwise
// product with B^ = FFT_L(conj chirp) / L stored at the image's own positions, the stages inverted in reverse order (natural
// order back at position n + n / 16), split with the second chirp factor.
template <typename F, int R0A, int R0B, int R1A, int R1B, int R2A, int R2B, bool REAL>
__global__ void __launch_bounds__(F::NT, F::NT >= 256 ? 4 : 2) chirpz3_kernel(Params p)
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
    stage<R0A, R0B, G0f, REAL>(s, p, p.tw, G0f{REAL ? (p.W + 1) / 2 : p.W}, src, tid);   // (real-input mode: ceil(W / 2) sample pairs)
    stage<R1A, R1B>(s, p, p.tw + F::TW1, G1{}, src, tid);
    stage<R2A, R2B>(s, p, p.tw, G2{}, src, tid);
    for (uint32_t i = tid; i < F::pp(F::P); i += F::NT) s[i] = cmul(s[i], p.bhat[i]);
    __syncthreads();
    stage_inv<R2A, R2B>(s, p.tw, G2{}, tid);
    stage_inv<R1A, R1B>(s, p.tw + F::TW1, G1{}, tid);
    stage_inv<R0A, R0B>(s, p.tw, G0{}, tid);
    if constexpr (REAL) untangle_store(p, s, row_a, tid, F::NT);
    else split_store(p, s, pair, row_a, row_b, tid, F::NT);
}

template <typename F, int R0A, int R0B, int R1A, int R1B, int R2A, int R2B, int R3A, int R3B, bool REAL>
__global__ void __launch_bounds__(F::NT, 4) chirpz4_kernel(Params p)
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
    if constexpr (REAL) untangle_store(p, s, row_a, tid, F::NT);
    else split_store(p, s, pair, row_a, row_b, tid, F::NT);
}

struct ChirpTables {
    DeviceBuffer<float2> d_chirp, d_bhat, d_tw;
    uint32_t L = 0, lds_points = 0;
    // real-input mode (a mono stream, every frame its own transform): the chirp-z transform of W points over ceil(W / 2) sample pairs
    // -- a convolution of half the length -- and the untangling twiddles w_2W^k
    TablesPtr<ChirpTables> half;
    DeviceBuffer<float2> d_twr;
};

}  // namespace mix

bool mixed_supported(uint32_t W)
{
    uint32_t n = 2 * W;
    if (W < 4 || n > 20480) return false;  // the transform lives in LDS: 8 bytes per point, all 160 KB of a CU at most
                                           // (192 kHz x 0.05 s: 2W = 19 200)
    for (uint32_t f : {2u, 3u, 5u, 7u})
        while (n % f == 0) n /= f;
    return n == 1;
}

namespace mix {

// The stage plan: P's factors 7, 5, 3, 4 (pairs of twos) and a last 2, grouped into stages of one or two factors with
// a product <= kMaxRadix -- fewest stages, then the smallest largest radix (registers), then the smallest sum.
// Stages with an odd factor come first (largest first), powers of two last (smallest first).  tests/test_host_logic.py restates it.
struct Plan { std::vector<std::pair<uint32_t, uint32_t>> stages; };

static void plan_search(std::vector<uint32_t> &rest, std::vector<std::pair<uint32_t, uint32_t>> &cur,
                        std::vector<std::pair<uint32_t, uint32_t>> &best, uint64_t &best_key)
{
    if (rest.empty()) {
        uint64_t mx = 0, sum = 0;
        for (auto &g : cur) { mx = std::max<uint64_t>(mx, g.first * g.second); sum += g.first * g.second; }
        const uint64_t key = ((uint64_t)cur.size() << 40) | (mx << 20) | sum;
        if (key < best_key) { best_key = key; best = cur; }
        return;
    }
    const uint32_t f = rest.back();   // the smallest remaining factor goes alone or with any other
    rest.pop_back();
    cur.push_back({f, 1});
    plan_search(rest, cur, best, best_key);
    cur.pop_back();
    for (size_t i = 0; i < rest.size(); ++i) {
        if (i > 0 && rest[i] == rest[i - 1]) continue;
        const uint32_t g = rest[i];
        if (f * g > kMaxRadix || (f == 2 && g == 2)) continue;
        rest.erase(rest.begin() + (long)i);
        cur.push_back({std::max(f, g), std::min(f, g)});
        plan_search(rest, cur, best, best_key);
        cur.pop_back();
        rest.insert(rest.begin() + (long)i, g);
    }
    rest.push_back(f);
}

static bool make_plan(uint32_t P, Plan &plan)
{
    std::vector<uint32_t> factors;   // descending
    uint32_t n = P;
    for (uint32_t f : {7u, 5u})
        while (n % f == 0) { factors.push_back(f); n /= f; }
    std::vector<uint32_t> threes;
    while (n % 3 == 0) { threes.push_back(3); n /= 3; }
    while (n % 4 == 0) { factors.push_back(4); n /= 4; }
    factors.insert(factors.end(), threes.begin(), threes.end());
    if (n % 2 == 0) { factors.push_back(2); n /= 2; }
    if (n != 1) return false;
    std::sort(factors.begin(), factors.end(), std::greater<uint32_t>());
    std::vector<std::pair<uint32_t, uint32_t>> cur, best;
    uint64_t best_key = ~0ull;
    plan_search(factors, cur, best, best_key);
    auto odd = [](const std::pair<uint32_t, uint32_t> &g) { return ((g.first * g.second) & (g.first * g.second - 1)) != 0; };
    std::stable_sort(best.begin(), best.end(), [&](const auto &a, const auto &b) {
        if (odd(a) != odd(b)) return odd(a);
        if (odd(a)) return a.first * a.second > b.first * b.second;
        return a.first * a.second < b.first * b.second;   // powers of two: the largest last (its padding is the thinnest)
    });
    plan.stages = best;
    return !best.empty() && best.size() <= (size_t)kMaxStages;
}

}  // namespace mix

// Tables of a P-point plan.  real: P is the WINDOW of real-input mode -- the split table pairs Z[k] with Z[P - k], k = 1 .. P / 2, and
// the untangling twiddles w_2P^k come with it.  hipErrorInvalidValue: no plan for P (the caller of the real-input half goes without).
static hipError_t build_tables(uint32_t P, bool real, TablesPtr<mix::MixTables> &out)
{
    using namespace mix;
    TablesPtr<MixTables> t(new MixTables());
    const uint32_t M = real ? P / 2 : P / 2 - 1;
    Plan plan;
    if (!make_plan(P, plan)) return hipErrorInvalidValue;
    t->n_stages = (uint32_t)plan.stages.size();
    std::vector<uint32_t> radix(t->n_stages);
    std::vector<float2> tw;
    uint32_t ns = P;
    for (uint32_t i = 0; i < t->n_stages; ++i) {
        t->ra[i] = plan.stages[i].first;
        t->rb[i] = plan.stages[i].second;
        radix[i] = t->ra[i] * t->rb[i];
        t->m[i] = ns / radix[i];
        t->inv_m[i] = 1.0f / (float)t->m[i];
        t->tw_off[i] = (uint32_t)tw.size();
        if (t->m[i] > 1)
            for (uint32_t j = 0; j < t->m[i]; ++j)
                for (uint32_t k = 1; k < radix[i]; ++k) tw.push_back(unit_root2((unsigned long long)j * k, ns));
        ns = t->m[i];
    }
    // one point of padding per R_last points (see stage()) when R_last is even and the padding costs no resident
    // workgroup (it cannot be afforded at the largest lengths: P = 20480 fills the 160 KB by itself)
    const size_t kLds = 160 * 1024;
    const uint32_t r_last = radix[t->n_stages - 1];
    auto resident_of = [&](uint32_t points) {
        return (unsigned)std::max<size_t>(1, std::min<size_t>(8, kLds / ((size_t)points * sizeof(float2))));
    };
    auto threads_of = [&](uint32_t points) {
        // the widest stage's butterflies in one round where the resident workgroups leave room (16 waves per CU at this
        // kernel's register budget), whole waves  (measured at 4800 points: 256 threads 1.72 ms, 192 2.13, 320 2.11)
        unsigned widest = 0;
        for (uint32_t i = 0; i < t->n_stages; ++i) widest = std::max(widest, P / radix[i]);
        unsigned cap = std::max((1024u / resident_of(points)) / 64 * 64, 64u);
        return std::max(std::min(cap, (widest + 63) / 64 * 64), 64u);
    };
    uint32_t best_d = 0;
    // (round 4: "no resident workgroup" counts up to four -- the registers hold no more than four 256-thread workgroups of the run-time
    // geometry or 512-thread ones of a compile-time plan anyway.  Same-device A/B: 4000 points +15 %, 3600 +-0, 3888 -4 %, and the
    // 4096-point plan of real-input mode at W 4096 becomes the compile-time one: 41 -> 68 M frames/s.  gpurun_out/r4_km_pad.log)
    if (r_last % 2 == 0 && (size_t)(P + P / r_last) * sizeof(float2) <= kLds && resident_of(P + P / r_last) >= std::min(resident_of(P), 4u)) best_d = r_last;
    t->pad_every = best_d;
    t->lds_points = best_d ? P + P / best_d : P;
    auto padpos = [&](uint32_t i) { return i + (t->pad_every ? i / t->pad_every : 0u); };
    for (uint32_t i = 0; i < t->n_stages; ++i) {
        t->q_stride[i] = t->m[i] == 1 ? 1u : padpos(t->m[i]);          // m > 1 is a multiple of R_last, hence of D
        t->blk_stride[i] = padpos(t->m[i] * radix[i]);
    }
    t->threads = threads_of(t->lds_points);
    auto is_plan = [&](uint32_t Pn, std::initializer_list<uint32_t> ab) {   // the compiled plan of a fixed kernel == the host's
        if (P != Pn || t->n_stages * 2 != ab.size()) return false;
        uint32_t i = 0, off = 0;
        for (auto it = ab.begin(); it != ab.end(); ++i) {
            const uint32_t a = *it++, b = *it++;
            if (t->ra[i] != a || t->rb[i] != b || (t->m[i] > 1 && t->tw_off[i] != off)) return false;
            off += t->m[i] * (a * b - 1);
        }
        const uint32_t rl = radix[t->n_stages - 1];
        return t->pad_every == (rl % 2 == 0 ? rl : 0u);
    };
#define X(Pn, A0, B0, A1, B1, A2, B2, N) if (is_plan(Pn, {A0, B0, A1, B1, A2, B2})) t->fixed = Pn;
    MIX_FIXED_PLANS(X)
#undef X
#define X(Pn, A0, B0, A1, B1, A2, B2, A3, B3, N) if (is_plan(Pn, {A0, B0, A1, B1, A2, B2, A3, B3})) t->fixed = Pn;
    MIX_FIXED4_PLANS(X)
#undef X
    // bin K = k1 + r1 (k2 + r2 (k3 + ...)) ends at k1 m1 + k2 m2 + ...
    std::vector<uint32_t> pos(P);
    for (uint32_t K = 0; K < P; ++K) {
        uint32_t k = K, at = 0;
        for (uint32_t i = 0; i < t->n_stages; ++i) {
            at += (k % radix[i]) * t->m[i];
            k /= radix[i];
        }
        pos[K] = padpos(at);
    }
    std::vector<uint32_t> split(M);
    for (uint32_t j = 0; j < M; ++j) split[j] = pos[j + 1] | (pos[P - (j + 1)] << 16);   // positions < 21 120 < 2^16
    hipError_t e = t->d_split.upload_at_least_one(split);   // (the kernels take both pointers whatever the lengths)
    if (e == hipSuccess) e = t->d_tw.upload_at_least_one(tw);
    if (e == hipSuccess && real) {
        std::vector<float2> twr(std::max<uint32_t>(M, 1));
        for (uint32_t j = 0; j < M; ++j) {
            const uint32_t k = j + 1;   // w_2P^k, k <= P / 2: the first quadrant of the circle, its end exact
            const double ang = -M_PI * (double)k / (double)P;
            twr[j] = 2 * k == P ? make_float2(0.0f, -1.0f) : make_float2((float)cos(ang), (float)sin(ang));
        }
        e = t->d_twr.upload(twr);
    }
    if (e == hipSuccess) out = std::move(t);
    return e;
}

void TablesDelete::operator()(mix::MixTables *t) const { delete t; }
void TablesDelete::operator()(mix::ChirpTables *t) const { delete t; }

hipError_t mixed_init(sgx_ctx *c)
{
    TablesPtr<mix::MixTables> t;
    hipError_t e = build_tables(c->P, false, t);
    if (e != hipSuccess) return e;
    if (c->C == 1 && c->W >= 8) {   // a mono stream: the W-point plan of real-input mode, where W has one
        e = build_tables(c->W, true, t->half);
        if (e != hipSuccess && e != hipErrorInvalidValue) return e;
    }
    c->mix = std::move(t);
    return hipSuccess;
}

hipError_t mixed_length_tables(uint32_t n, TablesPtr<mix::MixTables> &out) { return build_tables(n, false, out); }

uint32_t mixed_fixed_plan(const sgx_ctx *c) { return c->mix ? (uint32_t)c->mix->fixed : 0u; }

// a mono stream whose frames each get their own transform (the default; SGX_FLAG_COMPLEX_MONO: as (s, s) through the 2W-point plan)
bool mixed_real_serves(const sgx_ctx *c, uint32_t channels)
{
    const mix::MixTables *t = c->mix.get();
    return t && t->half && channels == 1 && !(c->cfg.flags & SGX_FLAG_PAIRED_FRAMES) && !(c->cfg.flags & SGX_FLAG_COMPLEX_MONO);
}

// real-input mode from PCM to pixels: a compile-time W-point plan, the palette conditions of the fused pixel stage, W / 2 bin pairs in
// registers (ten per thread at most); the launch sizes its LDS for the column and its samples
// (the palette conditions: the bands instantiations have no palette and fuse without them)
static bool fused_palette(const sgx_ctx *c)
{
    return !c->pal.stereo && !c->pal.segments && c->pal.n == 256 && c->d_pal_seed.get() && wg4096_seed_is_within_one(c);
}

static bool real_two_frames(int fixed)   // real-input mode to pixels or bands: two frames per workgroup at this plan
{
#define X(Pn, A0, B0, A1, B1, A2, B2, N) if (fixed == Pn) return true;
    MIX_REAL2_RENDER_PLANS(X)
#undef X
    return false;
}

// the threads of a compile-time plan (0: `fixed` names none); real_render: as real-input mode runs it to a column, two plans wider
static unsigned plan_threads(int fixed, bool real_render = false)
{
    unsigned nt = 0;
#define X(Pn, A0, B0, A1, B1, A2, B2, N) if (fixed == Pn) nt = N;
    MIX_FIXED_PLANS(X)
    if (real_render) { MIX_REAL_RENDER_PLANS(X) }
#undef X
#define X(Pn, A0, B0, A1, B1, A2, B2, A3, B3, N) if (fixed == Pn) nt = N;
    MIX_FIXED4_PLANS(X)
#undef X
    return nt;
}

// the column and its interpolated samples on the transform's LDS image; ten bins per thread in registers at most
static bool real_column_fits(const sgx_ctx *c, const mix::MixTables *t)
{
    const unsigned nt = t->half ? plan_threads(t->half->fixed, true) : 0;
    return nt && c->W / 2 <= nt * 10u && ((size_t)c->M + 1 + c->tab.samples.size()) * sizeof(float2) <= 160 * 1024;
}

static bool mixed_column_fits(const sgx_ctx *c, const mix::MixTables *t)
{
    const unsigned nt = t ? plan_threads(t->fixed) : 0;
    return nt && (size_t)c->M + 1 + c->tab.samples.size() <= t->lds_points && c->M <= nt * 10u;
}

static bool real_fuses_render(const sgx_ctx *c, const mix::MixTables *t) { return fused_palette(c) && real_column_fits(c, t); }

static bool real_fuses_bands(const sgx_ctx *c, const mix::MixTables *t)
{
    return real_column_fits(c, t) && mix::bands_kernel_exists(t->half->fixed, true, real_two_frames(t->half->fixed));
}

bool mixed_can_fuse_render(const sgx_ctx *c)
{
    const mix::MixTables *t = c->mix.get();
    // (a mono stream that real-input mode cannot take to pixels goes the two-kernel route on real-input ROWS, not through the 2W-point
    // plan as an (s, s) frame: the pixels of a context are those of its rows)
    if (mixed_real_serves(c, c->C)) return real_fuses_render(c, t);
    return fused_palette(c) && mixed_column_fits(c, t);
}

bool mixed_can_fuse_bands(const sgx_ctx *c)
{
    const mix::MixTables *t = c->mix.get();
    if (mixed_real_serves(c, c->C)) return real_fuses_bands(c, t);
    return mixed_column_fits(c, t) && mix::bands_kernel_exists(t->fixed, false, false);
}

// The frames p.first_frame .. + p.n_frames in launches of at most 2^30 workgroups (gridDim.x is limited to 2^31 - 1).  launch(grid) starts
// one with p as this leaves it and returns the error of setting it up.  A mono stream under SGX_FLAG_PAIRED_FRAMES: one workgroup per frame
// PAIR (2q, 2q+1) by global index, every launch addressing the whole range's rows.  Otherwise one per frame and channel pair, every launch
// on its own rows: mags_stride floats and rgba_stride bytes per frame (either pointer may be null).
// p is the caller's, changed in place before every launch (mono_pairs, pair_base and mags, or first_frame, n_frames, mags and rgba), so
// `launch` must hold p by reference; c is read for the paired-frames flag only.
template <typename Launch>
static hipError_t launch_chunks(const sgx_ctx *c, mix::Params &p, float *d_mags, size_t mags_stride, uint8_t *d_rgba, size_t rgba_stride, Launch launch)
{
    const size_t first_frame = p.first_frame, n_frames = p.n_frames, max_chunk = 1u << 30;
    if (paired_mono(c, p.C)) {
        p.mono_pairs = 1;
        p.mags = d_mags;
        const unsigned long long q0 = first_frame / 2, q1 = (first_frame + n_frames + 1) / 2;
        for (unsigned long long q = q0; q < q1; q += max_chunk) {
            const unsigned long long chunk = q1 - q < max_chunk ? q1 - q : max_chunk;
            p.pair_base = q;
            hipError_t e = launch(dim3((unsigned)chunk, 1));
            if (e == hipSuccess) e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    for (size_t done = 0; done < n_frames; done += max_chunk) {
        const size_t chunk = n_frames - done < max_chunk ? n_frames - done : max_chunk;
        p.first_frame = first_frame + done;
        p.n_frames = chunk;
        p.mags = d_mags ? d_mags + done * mags_stride : nullptr;
        if (d_rgba) p.rgba = d_rgba + done * rgba_stride;
        hipError_t e = launch(dim3((unsigned)chunk, p.pairs));
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// d_rgba: the fused column -- RGBA pixels, or with `bands` float2 (l, r) means per row (sgx_bands_batch)
hipError_t launch_mixed(const sgx_ctx *c, const StftCall &call)
{
    if (call.kind == Out::kPeak) return hipErrorInvalidValue;
    const float *d_pcm = call.pcm;
    const uint32_t channels = call.channels, pairs = call.pairs;
    const size_t first_frame = call.first, n_frames = call.n, total_frames = call.total;
    const bool band_means = call.kind == Out::kBands, half_rows = call.kind == Out::kMagsF16, complex_rows = call.kind == Out::kComplex;
    uint8_t *d_rgba = band_means || call.kind == Out::kRgba ? static_cast<uint8_t *>(call.out) : nullptr;
    float *d_mags = d_rgba ? nullptr : static_cast<float *>(call.out);
    using namespace mix;
    if (n_frames == 0) return hipSuccess;
    const MixTables *t = c->mix.get();
    // a mono stream, every frame its own transform (the default): real-input mode on the W-point plan, where there is one
    const bool real = mixed_real_serves(c, channels) && (!d_rgba || (band_means ? real_fuses_bands(c, t) : real_fuses_render(c, t)));
    if (real) t = t->half.get();
    Params p{};
    if (d_rgba) {
        p.render = 1;
        p.rgba = d_rgba;
        p.R = c->R;
        p.n_samples = (uint32_t)c->tab.samples.size();
        p.interp = c->cfg.interp;
        p.rows = c->d_rows.get();
        p.samples = c->d_samples.get();
        p.pal = c->d_pal_seed.get();
        if (!band_means) lut_seed_coefficients(c, p.guess_a, p.guess_b);
    }
    p.pcm = d_pcm;
    p.window = c->d_window.get();
    p.tw = t->d_tw.get();
    p.split = t->d_split.get();
    p.W = c->W;
    p.P = real ? c->W : c->P;
    p.real = real ? 1u : 0u;
    p.twr = t->d_twr.get();
    p.H = c->H;
    p.C = channels;
    p.pairs = pairs;
    p.scale = 2.0f / (float)c->W;
    p.n_stages = t->n_stages;
    p.out_f16 = half_rows ? 1u : 0u;
    p.inv_pad = t->pad_every ? 1.0f / (float)t->pad_every : 0.0f;
    for (uint32_t i = 0; i < t->n_stages; ++i) {
        p.ra[i] = t->ra[i];
        p.rb[i] = t->rb[i];
        p.m[i] = t->m[i];
        p.tw_off[i] = t->tw_off[i];
        p.inv_m[i] = t->inv_m[i];
        p.q_stride[i] = t->q_stride[i];
        p.blk_stride[i] = t->blk_stride[i];
    }
    p.first_frame = first_frame;
    p.n_frames = n_frames;
    p.total_frames = total_frames;
    // (l, r) of a channel pair as one 8-byte word: even channel count and an 8-byte aligned stream
    p.vec2 = (channels >= 2 && channels % 2 == 0 && reinterpret_cast<uintptr_t>(d_pcm) % 8 == 0) ? 1u : 0u;
    if (real) p.vec2 = c->W % 2 == 0 ? 1u : 0u;   // sample PAIRS of one channel as 8-byte words (any hop, any alignment: see stage())
    size_t lds = (size_t)t->lds_points * sizeof(float2);
    if (real && d_rgba) lds = std::max(lds, ((size_t)c->M + 1 + c->tab.samples.size()) * sizeof(float2));   // the column and its samples
    const bool two_frames = real && d_rgba && real_two_frames(t->fixed);   // real-input mode to pixels at the application plans: two frames (two images) per workgroup
    if (two_frames) lds = std::max(lds, 2 * (size_t)t->lds_points * sizeof(float2));
    const unsigned threads = t->threads;
    auto go = [&](auto kernel, unsigned nt, dim3 grid) { return launch_kernel(kernel, p, nt, grid, lds, c->stream); };
    auto launch = [&](dim3 grid) -> hipError_t {
        if (band_means) return launch_bands_kernel(p, t->fixed, real, two_frames, grid, lds, c->stream);
        // complex rows (sgx_stft_batch_complex): the same plan's kernel with the complex store
        if (complex_rows) return launch_complex_kernel(p, t->fixed, real, threads, grid, lds, c->stream);
        if (two_frames)
            switch (t->fixed) {
#define X(Pn, A0, B0, A1, B1, A2, B2, N)                                                                                                  \
    case Pn:                                                                                                                              \
        return go(stft_mixed_real2_render_kernel<Fixed3<Pn, A0, B0, A1, B1, A2, B2, N>, A0, B0, A1, B1, A2, B2>, 2 * N, dim3((grid.x + 1) / 2, 1));
                MIX_REAL2_RENDER_PLANS(X)
#undef X
            default: break;
            }
        if (real && d_rgba)
            switch (t->fixed) {
#define X(Pn, A0, B0, A1, B1, A2, B2, N) \
    case Pn: return go(stft_mixed_fixed_kernel<Fixed3<Pn, A0, B0, A1, B1, A2, B2, N>, A0, B0, A1, B1, A2, B2, true>, N, grid);
                MIX_REAL_RENDER_PLANS(X)
#undef X
            default: break;
            }
        switch (t->fixed) {
#define X(Pn, A0, B0, A1, B1, A2, B2, N)                                                                                      \
    case Pn:                                                                                                                  \
        if (real) return go(stft_mixed_fixed_kernel<Fixed3<Pn, A0, B0, A1, B1, A2, B2, N>, A0, B0, A1, B1, A2, B2, true>, N, grid); \
        return go(stft_mixed_fixed_kernel<Fixed3<Pn, A0, B0, A1, B1, A2, B2, N>, A0, B0, A1, B1, A2, B2, false>, N, grid);
            MIX_FIXED_PLANS(X)
#undef X
#define X(Pn, A0, B0, A1, B1, A2, B2, A3, B3, N)                                                                                               \
    case Pn:                                                                                                                                   \
        if (real) return go(stft_mixed_fixed4_kernel<Fixed4<Pn, A0, B0, A1, B1, A2, B2, A3, B3, N>, A0, B0, A1, B1, A2, B2, A3, B3, true>, N, grid); \
        return go(stft_mixed_fixed4_kernel<Fixed4<Pn, A0, B0, A1, B1, A2, B2, A3, B3, N>, A0, B0, A1, B1, A2, B2, A3, B3, false>, N, grid);
            MIX_FIXED4_PLANS(X)
#undef X
        default: return go(stft_mixed_kernel, threads, grid);
        }
    };
    return launch_chunks(c, p, d_mags, (size_t)pairs * c->M * (half_rows ? 1 : (complex_rows ? 4 : 2)), d_rgba, (size_t)pairs * c->R * (band_means ? 8 : 4), launch);
}

// ---- chirp-z through the composite stages (see chirpz3_kernel) --------------------------------------------------------

namespace mix {

// host float64 radix-2 FFT (table set-up only)
static void fft_host(std::vector<double> &re, std::vector<double> &im)
{
    const size_t n = re.size();
    for (size_t i = 1, j = 0; i < n; ++i) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) { std::swap(re[i], re[j]); std::swap(im[i], im[j]); }
    }
    for (size_t len = 2; len <= n; len <<= 1) {
        const double ang = -2.0 * M_PI / (double)len;
        for (size_t i = 0; i < n; i += len)
            for (size_t k = 0; k < len / 2; ++k) {
                const double wr = cos(ang * (double)k), wi = sin(ang * (double)k);
                const size_t a = i + k, b = i + k + len / 2;
                const double tr = re[b] * wr - im[b] * wi, ti = re[b] * wi + im[b] * wr;
                re[b] = re[a] - tr; im[b] = im[a] - ti;
                re[a] += tr; im[a] += ti;
            }
    }
}

static uint32_t chirp_length(uint32_t W)
{
    uint32_t L = 1;
    while (L < 3 * W - 1) L <<= 1;   // P + W - 1
    return L;
}

// P points out of nz non-zero inputs: any power of two >= P + nz - 1 that has a plan
static uint32_t conv_length(uint32_t P, uint32_t nz)
{
    uint32_t L = 512;
    while (L < P + nz - 1) L <<= 1;
    return L;
}

}  // namespace mix

bool chirpz_supported(uint32_t W)
{
    if (W < 4 || 3ull * W - 1 > 16384) return false;
    const uint32_t L = mix::chirp_length(W);
    return L == 512 || L == 1024 || L == 2048 || L == 4096 || L == 8192 || L == 16384;
}

// Tables of the chirp-z transform of P points out of nz non-zero inputs (2W and W for an (l, r) frame; real: W and ceil(W / 2) sample
// pairs, with the untangling twiddles w_2P^k).  hipErrorInvalidValue: no plan for the convolution length.
static hipError_t build_chirp(uint32_t P, uint32_t nz, bool real, TablesPtr<mix::ChirpTables> &out)
{
    using namespace mix;
    const uint32_t L = real ? conv_length(P, nz) : chirp_length(nz);
    std::vector<uint32_t> radix;
#define X(Ln, A0, B0, A1, B1, A2, B2, N) if (L == Ln) radix = {A0 * B0, A1 * B1, A2 * B2};
    CHIRP_PLANS3(X)
#undef X
#define X(Ln, A0, B0, A1, B1, A2, B2, A3, B3, N) if (L == Ln) radix = {A0 * B0, A1 * B1, A2 * B2, A3 * B3};
    CHIRP_PLANS4(X)
#undef X
    if (radix.empty()) return hipErrorInvalidValue;
    TablesPtr<ChirpTables> t(new ChirpTables());
    t->L = L;
    t->lds_points = L + L / 16;
    auto padpos = [](uint32_t i) { return i + i / 16; };
    // per-stage twiddle rows [m][R - 1] and the digit reversal, exactly as mixed_init lays them out for the dynamic plan
    std::vector<float2> tw;
    std::vector<uint32_t> ms(radix.size());
    uint32_t ns = L;
    for (size_t i = 0; i < radix.size(); ++i) {
        ms[i] = ns / radix[i];
        if (ms[i] > 1)
            for (uint32_t j = 0; j < ms[i]; ++j)
                for (uint32_t k = 1; k < radix[i]; ++k) tw.push_back(unit_root2((unsigned long long)j * k, ns));
        ns = ms[i];
    }
    std::vector<float2> chirp(P), bhat(t->lds_points, make_float2(0.0f, 0.0f));
    std::vector<double> cr(P), ci(P);
    for (uint32_t n = 0; n < P; ++n) {
        const unsigned long long q = ((unsigned long long)n * n) % (2ull * P);  // n^2 mod 2P: exact
        const double ang = -M_PI * (double)q / (double)P;
        cr[n] = cos(ang); ci[n] = sin(ang);
        chirp[n] = make_float2((float)cr[n], (float)ci[n]);
    }
    // b[m] = conj(c[|m|]) for m in [-(nz-1), P-1], wrapped modulo L
    std::vector<double> br(L, 0.0), bi(L, 0.0);
    for (uint32_t m = 0; m < P; ++m) { br[m] = cr[m]; bi[m] = -ci[m]; }
    for (uint32_t m = 1; m < nz; ++m) { br[L - m] = cr[m]; bi[L - m] = -ci[m]; }
    fft_host(br, bi);
    for (uint32_t K = 0; K < L; ++K) {   // bin K = k1 + r1 (k2 + r2 (...)) ends at k1 m1 + k2 m2 + ...
        uint32_t k = K, at = 0;
        for (size_t i = 0; i < radix.size(); ++i) {
            at += (k % radix[i]) * ms[i];
            k /= radix[i];
        }
        bhat[padpos(at)] = make_float2((float)(br[K] / (double)L), (float)(bi[K] / (double)L));
    }
    hipError_t e = t->d_chirp.upload(chirp);
    if (e == hipSuccess) e = t->d_bhat.upload(bhat);
    if (e == hipSuccess) e = t->d_tw.upload(tw);
    if (e == hipSuccess && real) {
        std::vector<float2> twr(std::max<uint32_t>(P / 2, 1));
        for (uint32_t j = 0; j < P / 2; ++j) {
            const uint32_t k = j + 1;   // w_2P^k, k <= P / 2
            const double ang = -M_PI * (double)k / (double)P;
            twr[j] = 2 * k == P ? make_float2(0.0f, -1.0f) : make_float2((float)cos(ang), (float)sin(ang));
        }
        e = t->d_twr.upload(twr);
    }
    if (e == hipSuccess) out = std::move(t);
    return e;
}

hipError_t chirpz_init(sgx_ctx *c)
{
    TablesPtr<mix::ChirpTables> t;
    hipError_t e = build_chirp(c->P, c->W, false, t);
    if (e != hipSuccess) return e;
    if (c->C == 1) {   // a mono stream: real-input mode
        e = build_chirp(c->W, (c->W + 1) / 2, true, t->half);
        if (e != hipSuccess && e != hipErrorInvalidValue) return e;
    }
    c->chz = std::move(t);
    return hipSuccess;
}

bool chirpz_real_serves(const sgx_ctx *c, uint32_t channels)
{
    const mix::ChirpTables *t = c->chz.get();
    return t && t->half && channels == 1 && !(c->cfg.flags & SGX_FLAG_PAIRED_FRAMES) && !(c->cfg.flags & SGX_FLAG_COMPLEX_MONO);
}

hipError_t launch_chirpz(const sgx_ctx *c, const StftCall &call)
{
    using namespace mix;
    if (call.kind != Out::kMags && call.kind != Out::kComplex) return hipErrorInvalidValue;
    const bool complex_rows = call.kind == Out::kComplex;
    const float *d_pcm = call.pcm;
    float *d_mags = static_cast<float *>(call.out);
    const uint32_t channels = call.channels, pairs = call.pairs;
    const size_t first_frame = call.first, n_frames = call.n, total_frames = call.total;
    if (n_frames == 0) return hipSuccess;
    const ChirpTables *t = c->chz.get();
    const bool real = chirpz_real_serves(c, channels);   // a mono stream, every frame its own transform (the default)
    if (real) t = t->half.get();
    Params p{};
    p.pcm = d_pcm;
    p.window = c->d_window.get();
    p.tw = t->d_tw.get();
    p.chirp = t->d_chirp.get();
    p.bhat = t->d_bhat.get();
    p.twr = t->d_twr.get();
    p.real = real ? 1u : 0u;
    p.W = c->W;
    p.P = real ? c->W : c->P;
    p.H = c->H;
    p.C = channels;
    p.pairs = pairs;
    p.scale = 2.0f / (float)c->W;
    p.first_frame = first_frame;
    p.n_frames = n_frames;
    p.total_frames = total_frames;
    p.vec2 = (channels >= 2 && channels % 2 == 0 && reinterpret_cast<uintptr_t>(d_pcm) % 8 == 0) ? 1u : 0u;
    if (real) p.vec2 = c->W % 2 == 0 ? 1u : 0u;   // sample PAIRS of one channel as 8-byte words
    const size_t lds = (size_t)t->lds_points * sizeof(float2);
    auto go = [&](auto kernel, unsigned nt, dim3 grid) { return launch_kernel(kernel, p, nt, grid, lds, c->stream); };
    auto launch = [&](dim3 grid) -> hipError_t {
        // complex rows (sgx_stft_batch_complex): the same plan's kernel with the complex store
        if (complex_rows) return launch_chirpz_complex_kernel(p, t->L, real, grid, lds, c->stream);
        switch (t->L) {
#define X(Ln, A0, B0, A1, B1, A2, B2, N)                                                                             \
    case Ln:                                                                                                         \
        if (real) return go(chirpz3_kernel<Fixed3<Ln, A0, B0, A1, B1, A2, B2, N>, A0, B0, A1, B1, A2, B2, true>, N, grid); \
        return go(chirpz3_kernel<Fixed3<Ln, A0, B0, A1, B1, A2, B2, N>, A0, B0, A1, B1, A2, B2, false>, N, grid);
            CHIRP_PLANS3(X)
#undef X
#define X(Ln, A0, B0, A1, B1, A2, B2, A3, B3, N)                                                                                      \
    case Ln:                                                                                                                          \
        if (real) return go(chirpz4_kernel<Fixed4<Ln, A0, B0, A1, B1, A2, B2, A3, B3, N>, A0, B0, A1, B1, A2, B2, A3, B3, true>, N, grid); \
        return go(chirpz4_kernel<Fixed4<Ln, A0, B0, A1, B1, A2, B2, A3, B3, N>, A0, B0, A1, B1, A2, B2, A3, B3, false>, N, grid);
            CHIRP_PLANS4(X)
#undef X
        default: return hipErrorInvalidValue;
        }
    };
    return launch_chunks(c, p, d_mags, (size_t)pairs * c->M * (complex_rows ? 4 : 2), nullptr, 0, launch);
}

}  // namespace sgx
