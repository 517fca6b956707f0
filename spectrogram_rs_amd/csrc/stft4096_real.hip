// stft4096_real.hip -- K1R: a mono stream at W = 2048 (H = 256: the tuned form; any other hop too) with EVERY frame its own transform, at the
// price of half a transform.
//
// The reference duplicates a mono sample into (s, s) and runs one 4096-point complex transform per frame
// (audio_input_list_model.rs:67-69, fft.rs:47-99): F = (1 + i) S with S the spectrum of the real windowed frame, and both output
// columns are |S[k]| 2 / W (fft.rs:81-98).  The headline kernel (stft4096_wg.hip) halves that work by packing frames 2j and 2j+1
// into the real and imaginary part of ONE transform -- and pays with a shared rounding floor: the quieter frame of a pair carries
// the louder one's float32 noise (tests/test_gpu_parity.py::test_onsets_*).  This kernel halves the work the other way: the
// 4096-point spectrum of a REAL sequence is a 2048-point complex transform of z[m] = x[2m] + i x[2m+1] plus one butterfly per bin,
//
//     S[k]        = E[k] + w_4096^k O[k],          E[k] = (Z[k] + conj Z[2048-k]) / 2,   O[k] = (Z[k] - conj Z[2048-k]) / 2i
//     S[2048 - k] = conj(E[k] - w_4096^k O[k]),    k = 0 .. 1023   (+ the self-paired k = 1024)
//
// so every frame is transformed on its own -- the reference's dataflow, north_star's tolerance against the frame's OWN peak on any
// input -- for the arithmetic of half a 4096-point transform.  Two frames share a workgroup only as two independent problems.
//
// Shape: K1's, so that K1's measured choices carry over (256 threads, three in-register passes, two LDS exchanges of one padded
// 34 816-byte image, partner exchange, persistent workgroups, four per CU, the same wave priorities).  A workgroup iteration does
// frames fa = first + 2 job (A) and fa + 1 (B), 2048 points each (zero padding: only m < 1024 is non-zero, never materialised):
//
//   sample index  m = t + 256 a            (a < 4 non-zero rows; x[2m], x[2m+1] arrive as ONE 8-byte load per lane)
//   pass 1  thread t, BOTH frames : 8-point DFT over a with 4 non-zero inputs = two 4-point FFTs -> q1; twiddle w_2048^{t q1}
//   pass 2  thread (F, q1, t0)    : t = t0 + 16 t1; 16-point FFT over t1 -> q2; twiddle w_256^{t0 q2} (K1's LDS table)
//   pass 3  thread (F, u = q1 + 8 q2): 16-point FFT over t0 -> q3;  Z_F[k], k = u + 128 q3
//   untangle  Z[k] with Z[2048-k] (thread 128 - u, register 15 - q3, through LDS as K1's split) -> |S[k]|, |S[2048-k]|:
//           every thread stores 16 bins of its frame's row, 8 ascending and 8 descending runs of 512 contiguous bytes per wave
//
// H = 256 = HALF a row of z.  With c[i] = (x[2i], x[2i+1]) the stream as 8-byte columns, frame f reads c[128 f + t + 256 a]: a thread's
// eight rows of a frame pair are R[j] = c[128 fa + t + 128 j], j = 0 .. 7 (even j: frame A, odd j: frame B), and the next pair's are
// R[j + 2]: the window slides in registers.  Of the two new values R[9] = c[128 fa + 1152 + t] is the thread's own load (ONE 8-byte
// load per thread and iteration, requested a whole iteration ahead, in front of the stores); R[8] = c[128 fa + 1024 + t] is what
// thread t - 128 loaded for this iteration (t >= 128) or what thread t + 128 holds as its R[7] (t < 128): every thread publishes
// the one its opposite number needs in 2 KB of LDS beside the partner exchange (same barrier) and reads the other's.  Every sample
// is fetched from memory exactly once.
// (The first version let both frames slide on their own and fetched every sample twice; the output stream keeps evicting the
// input from L2, the second fetch went to HBM, and the launch took exactly the 5.9 % longer that 18 424 B / frame are more than
// 17 400: 3.72 ms per 1e6 frames against the paired kernel's 3.50.)
#include <cmath>
#include <type_traits>

#include "run_claim.hpp"
#include "stft4096_wg.hpp"

namespace sgx {

namespace wgr {

using wg::kBufComplex;
using wg::kLdsBytes;
using wg::kLdsBytesRender;
using wg::kM;
using wg::kS1;
using wg::kS2;
using wg::kW;
using wg::lds_barrier;
using wg::lds_read_alone;
using wg::lds_cfloat2;
using wg::lds_ptr;
using wg::pcm_rsrc;
using wg::u32x2;
using wg::u32x4;

typedef float f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float cl_fma(float a, float c, float u) { return fmaf(a, c, u); }
__device__ __forceinline__ f2v cl_fma(f2v a, float c, f2v u) { return __builtin_elementwise_fma(a, f2v{c, c}, u); }

#include "fft_codelets.inc"

using wg::Params;   // the 4096-point kernels' parameter block: tw1 = [8][256] w_2048^{t q1}, + twu, stream_samples (stft4096_wg.hpp)

__device__ __forceinline__ float2 cmulf(float2 a, float2 b)
{
    return make_float2(fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x));
}

// a raw buffer descriptor over one output row (uniform base); `present` false: zero records, every store through it is dropped by
// the range check -- a frame outside the requested range costs no branch in the store section.  (gfx950 checks lane offset + SCALAR
// offset against the record count -- tools/bufrange.hip, profiles/r05_bufrange.txt: a store with records 0 and soffset 2048 writes
// nothing, a load whose soffset alone passes the records reads 0 -- and test_rows_past_the_requested_count_are_never_written holds
// every two-frames-per-iteration kernel to it with sentinel rows behind and in front of the caller's range.)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t out_rsrc(char *base, long long byte, bool present)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)byte);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((unsigned long long)byte >> 32));
    const int records = __builtin_amdgcn_readfirstlane(present ? 0x7fffffff : 0);
    return __builtin_amdgcn_make_buffer_rsrc(base + (long long)(((unsigned long long)hi << 32) | lo), 0, records, 0x00020000);
}

// 8-point forward DFT of (z0, z1, z2, z3, 0, 0, 0, 0): even bins = FFT4(z), odd bins = FFT4(z_a w_8^a); bin q1 in (yr, yi)[q1]
__device__ __forceinline__ void fft8_half_zero(const float (&zr)[4], const float (&zi)[4], float (&yr)[8], float (&yi)[8])
{
    constexpr float kH = 0.70710678118654752440f;
    auto fft4 = [](float a0r, float a0i, float a1r, float a1i, float a2r, float a2i, float a3r, float a3i, float *outr, float *outi) {
        const float s0r = a0r + a2r, s0i = a0i + a2i, s1r = a0r - a2r, s1i = a0i - a2i;
        const float s2r = a1r + a3r, s2i = a1i + a3i, s3r = a1r - a3r, s3i = a1i - a3i;
        outr[0] = s0r + s2r; outi[0] = s0i + s2i;          // bin 0
        outr[4] = s0r - s2r; outi[4] = s0i - s2i;          // bin 2
        outr[2] = s1r + s3i; outi[2] = s1i - s3r;          // bin 1: s1 - i s3
        outr[6] = s1r - s3i; outi[6] = s1i + s3r;          // bin 3: s1 + i s3
    };
    fft4(zr[0], zi[0], zr[1], zi[1], zr[2], zi[2], zr[3], zi[3], yr, yi);                       // even q1 at [0], [2], [4], [6]
    const float y1r = (zr[1] + zi[1]) * kH, y1i = (zi[1] - zr[1]) * kH;                          // z1 (1 - i) / sqrt 2
    const float y3r = (zi[3] - zr[3]) * kH, y3i = -(zr[3] + zi[3]) * kH;                         // z3 (-1 - i) / sqrt 2
    fft4(zr[0], zi[0], y1r, y1i, zi[2], -zr[2], y3r, y3i, yr + 1, yi + 1);                       // odd q1 at [1], [3], [5], [7]
}

constexpr int kRowsF32 = 0, kRowsF16 = 1, kPixels = 2;   // what a launch writes: float rows, half-pair rows, RGBA columns (fused pixel path)
constexpr int kBands = 3;   // the fused column's (l, r) row means as float2, no colour (sgx_bands_batch; PIX wg::kPixBandsCubic / kPixBandsCosine)
constexpr int kPeak = 5;    // kBands held as a running maximum over groups of frames (sgx_bands_peak_batch; PIX wg::kPixPeakCubic / kPixPeakCosine)
constexpr int kFbank = 6;   // a filterbank over the pair's columns (sgx_fbank_batch; PIX wg::kPixFbank): the column in LDS, one filter pass (sgx_fbank.hpp)
constexpr int kRowsC64 = 4;   // complex rows (sgx_stft_batch_complex): (S, S) per bin, 16 bytes, every bin pair stored as soon as it is untangled

// PIX (kPixels only): the pixel code of the instantiation, wg::kPixCubic / kPixCosine / kPixGeneric (stft4096_wg.hpp)
// SLIDE: H = 256, the window slides in registers (above).  Else: any hop (a frame starts on any sample): the eight columns of the
// next frame pair are requested where the sliding form requests its one, straight into R -- dead since pass 1 -- and every sample is
// fetched 2048 / H times, through L2.
// TR (the sliding instantiation): the two LDS transposes as real / imaginary planes, written with ds_write_addtid_b32 and read back in
// 16-byte pieces, as in stft4096_wg.hip (there: why pass 1 then runs column t = (tid >> 4) + 16 (tid & 15)).  Image 1: rows 8 F + q1 of 272
// words; image 2: rows q2 of 280 words -- its readers are the threads (F, u = q1 + 8 q2), and with that lane order 280 is the stride whose
// 16-byte reads are conflict-free (tools/lds_b128_conflicts.py).  The imaginary plane starts 4 480 words in, for both.
constexpr int kPlaneIm = 4480;                                        // words
constexpr int kBufComplexTR = kPlaneIm;                               // 2 * 4 480 words = 35 840 B: 1 KB more than the b64 images
static_assert(kBufComplexTR >= kBufComplex && 16 * 280 <= kPlaneIm, "the planes hold both images");
constexpr size_t kLdsBytesR = (size_t)(kBufComplexTR + 256) * sizeof(float2);
constexpr size_t kLdsBytesRenderR = kLdsBytesR + 256 * sizeof(uint2);
static_assert(4 * kLdsBytesRenderR <= 160 * 1024, "four workgroups per CU");
// rows ra and rb (STRIDE words each) of both planes, this wave's 64 words: LDS address = M0 + offset + 4 * lane.  M0 is set inside the
// statement (it cannot be declared clobbered -- a reserved register to clang: stft4096_wg.hip -- so the ISA check also refuses every implicit reader of M0 beside these statements) and one wait state separates a scalar write of M0 from an
// add-TID instruction (tools/isa_check_addtid.py looks at every build).
template <int STRIDE>
__device__ __forceinline__ void addtid_rows(float2 a, float2 b, uint32_t m0_wave, int ra, int rb)
{
    asm volatile("s_mov_b32 m0, %4\n\t"
                 "s_nop 0\n\t"
                 "ds_write_addtid_b32 %0 offset:%5\n\t"
                 "ds_write_addtid_b32 %1 offset:%6\n\t"
                 "ds_write_addtid_b32 %2 offset:%7\n\t"
                 "ds_write_addtid_b32 %3 offset:%8"
                 :
                 : "v"(a.x), "v"(a.y), "v"(b.x), "v"(b.y), "s"(m0_wave), "i"(4 * STRIDE * ra), "i"(4 * STRIDE * ra + 4 * kPlaneIm), "i"(4 * STRIDE * rb), "i"(4 * STRIDE * rb + 4 * kPlaneIm)
                 : "memory");
}
__device__ __forceinline__ void read_planes(const float4 *rd4, float (&xr)[16], float (&xi)[16])
{
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float4 r = rd4[c], i = rd4[c + kPlaneIm / 4];
        xr[4 * c] = r.x; xr[4 * c + 1] = r.y; xr[4 * c + 2] = r.z; xr[4 * c + 3] = r.w;
        xi[4 * c] = i.x; xi[4 * c + 1] = i.y; xi[4 * c + 2] = i.z; xi[4 * c + 3] = i.w;
    }
}
__device__ __forceinline__ float lane_xor8(float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x128, 0xf, 0xf, true)); }   // row_ror:8

#if SGX_STAMPS
// diagnostic build only (tools/k1r_phases.py): per-phase wave cycles (s_memtime), summed over all waves and iterations; SGX_STAMP: sgx_internal.hpp
__device__ unsigned long long g_phase_cycles_r[24];
// tools/k1r_finish.py: per workgroup {wall clock at entry, at exit, block index, jobs done}, plain stores of thread 0.  The wall clock is the
// constant-rate counter all CUs share (the cycle counter of the phase stamps is per CU and not comparable between them).
// -DSGX_STAMPS=2 keeps these and compiles the phase stamps away, so that the iteration is the product's.
constexpr int kFinishBlocks = 4096;
__device__ unsigned long long g_finish_r[4 * kFinishBlocks];
#if SGX_STAMPS == 2
#undef SGX_STAMP
#define SGX_STAMP(i)
#endif
#endif

template <int MODE, int PIX, bool SLIDE>
__global__ void __launch_bounds__(256, 4) stft4096_real_kernel(Params p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2 *buf = reinterpret_cast<float2 *>(smem_raw);
    constexpr bool TR = SLIDE;
    float2 *tw2 = buf + (TR ? kBufComplexTR : kBufComplex);
    uint2 *pal = reinterpret_cast<uint2 *>(tw2 + 256);          // kPixels only: [256] {threshold, RGBA} (wg::pixel_for)
    constexpr bool F16 = MODE == kRowsF16;
    constexpr bool C64 = MODE == kRowsC64;
    constexpr bool FUSED = MODE == kPixels || MODE == kBands || MODE == kPeak || MODE == kFbank;  // the column goes through LDS to the pixel passes (kFbank: to the filter pass)

    const int tid = threadIdx.x;
#if SGX_STAMPS
    if (tid == 0 && blockIdx.x < kFinishBlocks) g_finish_r[4 * blockIdx.x] = wall_clock64();
#endif
    const int t_p1 = TR ? (tid >> 4) + 16 * (tid & 15) : tid;     // pass-1 column of this thread
    float *plane = reinterpret_cast<float *>(smem_raw);
    const uint32_t m0_wave = __builtin_amdgcn_readfirstlane((uint32_t)(tid >> 6) * 272u);   // TR: byte offset of this wave inside a plane row (64 + 4 words per wave)
    // TR read sides: image 1, thread (g2 = tid >> 4, t0 = tid & 15): the words of writers 16 t0 .. + 15 of row g2; image 2, thread (F, u):
    // the words of writers 16 (8 F + q1) .. + 15 of row q2
    const float4 *rd4_1 = reinterpret_cast<const float4 *>(plane + 272 * (tid >> 4) + 68 * ((tid & 15) >> 2) + 16 * (tid & 3));
    const float4 *rd4_2 = reinterpret_cast<const float4 *>(plane + 280 * ((tid & 127) >> 3) + 68 * ((8 * (tid >> 7) + (tid & 7)) >> 2) + 16 * (tid & 3));
    tw2[tid] = p.tw2[tid];
    uint32_t row_words[4] = {0u, 0u, 0u, 0u};  // FUSED: the table words of this thread's rows tid + 256 i
    if (FUSED && MODE != kFbank) {
        if (MODE == kPixels) pal[tid] = make_uint2(__float_as_uint(tid < 255 ? p.lut_thr[tid] : __builtin_nanf("")), *reinterpret_cast<const uint32_t *>(&p.lut_rgba[tid]));
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if ((uint32_t)tid + 256u * i < p.R) row_words[i] = p.rows[tid + 256 * i];
    }

    // per-thread constants, resident for the life of the (persistent) workgroup
    // the output scale |S| 2 / W rides on the window as 1 / 2048 (the untangle's two halves and 2 / W = 1 / 1024): a power of two
    // commutes with every rounding below
    float win[8];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        win[2 * a] = p.window[2 * t_p1 + 512 * a] * (1.0f / 2048.0f);
        win[2 * a + 1] = p.window[2 * t_p1 + 512 * a + 1] * (1.0f / 2048.0f);
    }
    float2 tw1[8];
#pragma unroll
    for (int q = 1; q < 8; ++q) tw1[q] = p.tw1[q * 256 + t_p1];
    const int F = tid >> 7, u = tid & 127;        // pass-3 / output role: frame of the pair, bins u + 128 q3
    float2 twu[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) twu[q] = p.twu[q * 128 + u];
    const int g2 = tid >> 4, t0_2 = tid & 15;      // pass-2 role: g2 = 8 F + q1
    const int cbase2 = (g2 >> 3) * 128 + (g2 & 7); // its image-2 column is cbase2 + 8 q2
    __syncthreads();

    // The rows launches run their jobs in RUNS: the static one, [blockIdx.x * jobs_per_block, + jobs_per_block), and then -- where the launch
    // carries a claim counter (run_claim.hpp) -- chunks of the pool until a claim index falls past it.  The workgroups of this launch do not
    // run at one speed (profiles/k1r_claimed_tail.txt), and with static runs alone the launch waits for the slowest.  The fused modes and
    // the sensitivity build keep the static split (kPeak's run alignment is built on it).
#ifdef SGX_VARIANT_SKIP_LAST_JOB
    constexpr bool CLAIM = false;
#else
    constexpr bool CLAIM = !FUSED;
#endif
    const bool claiming = CLAIM && p.claim_counter != nullptr;
    unsigned long long *claim_word = reinterpret_cast<unsigned long long *>(tw2 + 256);   // LDS, behind the tables: the claim of the run after this one
    unsigned long long job_begin = (unsigned long long)blockIdx.x * p.jobs_per_block;
    unsigned long long job_end = job_begin + p.jobs_per_block;
    // The static run of a rows launch dealt by slot (run_claim.hpp: the n-th workgroup placed on a CU runs at the n-th slot's rate, and its
    // run is sized for it): the deal rides in the LUT and seed words, and slot_run is compares, selects and three scalar multiplications.
    if (CLAIM && p.slot_n_cu != 0u) {
        SlotDeal deal{};
        deal.per[0] = p.slot_per0;
        deal.per[1] = p.slot_per1;
        deal.per[2] = ((unsigned long long)p.slot_per2_hi << 32) | p.slot_per2_lo;
        deal.per[3] = ((unsigned long long)p.slot_per3_hi << 32) | p.slot_per3_lo;
        deal.n_cu = p.slot_n_cu;
        deal.leftover = p.slot_leftover;
        const JobRun run = slot_run(deal, blockIdx.x);
        // (scalar by statement: the compiler forms the 64-bit products in vector registers, and a run held there stays in two of them for
        // the whole loop -- every register of the iteration renumbered)
        auto uniform = [](unsigned long long v) { return ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)v); };
        job_begin = uniform(run.begin);
        job_end = uniform(run.end);
    }
    if (job_end > p.n_jobs) job_end = p.n_jobs;
#ifdef SGX_VARIANT_SKIP_LAST_JOB   // the sensitivity build of tests/test_gpu_cu_counts.py: a run of more than one job omits its last (omits work only)
    if (job_end > job_begin + 1) --job_end;
#endif
    if (job_begin >= job_end && !claiming) return;

    // Columns from `col0` of the stream on, as a raw buffer (uniform base + one 32-bit lane offset); its record count is what the
    // stream still holds from there, so a column past the end reads as zero: a pair's second frame that the stream does not hold, or
    // the rows requested ahead at the end of a run, need no branch (their results are never stored).
    // (the loads below are 8-byte words at 4-byte aligned addresses when the hop is odd or the stream starts on an odd sample: buffer
    // loads of more than one dword need dword alignment only)
    auto samples_from = [&](unsigned long long first) {                      // first: sample index
        const unsigned long long left = first < p.stream_samples ? (p.stream_samples - first) * 4 : 0;
        const unsigned long long addr = (unsigned long long)(p.pcm + (first < p.stream_samples ? first : 0));
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)addr), hi = __builtin_amdgcn_readfirstlane((uint32_t)(addr >> 32));
        const int records = __builtin_amdgcn_readfirstlane((int)(left < 0x7fffffffull ? left : 0x7fffffffull));
        return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((unsigned long long)hi << 32) | lo), 0, records, 0x00020000);
    };
    auto columns_from = [&](unsigned long long col0) { return samples_from(2 * col0); };
    auto column = [&](__amdgpu_buffer_rsrc_t r, int byte_offset) {
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, t_p1 * 8, byte_offset, 0);
        return make_float2(__uint_as_float(v.x), __uint_as_float(v.y));
    };
    float2 R[8];        // R[j] = c[128 fa + tid + 128 j]: rows a = j / 2 of frame A (even j) and frame B (odd j)
    float2 L;           // the next R[7] = c[128 fa + 1152 + tid]   (SLIDE)
    auto load_pair = [&](unsigned long long fa_) {   // !SLIDE: all eight columns of the pair (fa_, fa_ + 1); any hop
        const __amdgpu_buffer_rsrc_t r0 = samples_from(fa_ * p.H), r1 = samples_from((fa_ + 1) * p.H);
#pragma unroll
        for (int a = 0; a < 4; ++a) { R[2 * a] = column(r0, 2048 * a); R[2 * a + 1] = column(r1, 2048 * a); }
    };
    float2 *xch = buf + 2304;         // [256] the iteration's loads, beside the partner rows (image 2 is dead by then)
    char *out = reinterpret_cast<char *>(p.mags);
    constexpr int kBin = C64 ? 16 : (F16 ? 4 : 8);   // bytes per output bin
#if SGX_STAMPS
    unsigned long long st_acc[20] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long st_last = __builtin_readcyclecounter();
    unsigned long long jobs_done = 0;
#endif
    for (;;) {   // the runs of this workgroup
        {
            const __amdgpu_buffer_rsrc_t r0 = columns_from(128 * (p.first_frame + 2 * job_begin));
            if (SLIDE) {
#pragma unroll
                for (int j = 0; j < 8; ++j) R[j] = column(r0, 1024 * j);
                L = column(r0, 9216);         // c[128 fa + 1152 + tid]
            } else {
                load_pair(p.first_frame + 2 * job_begin);
                L = R[7];
            }
            // The claim of the NEXT run is requested here, behind the requests for this run's window and in front of the wait for them: the two
            // round trips overlap, and thread 0 parks the index in LDS, where the end of the run finds it behind a barrier.  Requested at
            // the end of the run instead, the whole workgroup would wait for a round trip to L2 behind its own row stores.
            // One returning add, relaxed, agent scope (a workgroup reads nothing another one writes); request and wait in ONE statement:
            // the compiler's own atomic waits for the result where it is issued -- it reduces over the wave first -- with the window
            // still unrequested, and a request of our own whose wait came later would leave it a register it believes complete.
            if (claiming && tid == 0) {
                unsigned long long claimed;
                asm volatile("global_atomic_add_x2 %0, %1, %2, off sc0\n\t"
                             "s_waitcnt vmcnt(0)"
                             : "=&v"(claimed)
                             : "v"(p.claim_counter), "v"(1ull)
                             : "memory");
                *claim_word = claimed;
            }
            // the window is waited for HERE (an empty asm that reads it), so that the loop header carries no pending load of the entry path:
            // merged with the back edge -- where the same registers are long complete -- it made the compiler wait at the top of EVERY
            // iteration with vmcnt(2), i.e. for the sixteen row stores just issued to be acknowledged by memory
#pragma unroll
            for (int j = 0; j < 8; ++j) asm volatile("" ::"v"(R[j].x), "v"(R[j].y));
            asm volatile("" ::"v"(L.x), "v"(L.y));
            // (the resident constants too: the compiler schedules their loads BEHIND the window's, and a constant still pending at the
            // loop entry became a vmcnt(10) .. vmcnt(5) at its first use inside the loop -- in every iteration)
#pragma unroll
            for (int q = 1; q < 8; ++q) asm volatile("" ::"v"(tw1[q].x), "v"(tw1[q].y));
#pragma unroll
            for (int q = 0; q < 8; ++q) asm volatile("" ::"v"(twu[q].x), "v"(twu[q].y), "v"(win[q]));
            // (L as well: in flight at the loop entry it made the wait at its first use -- the exchange write, two thirds into the
            // iteration -- a vmcnt(1): all sixteen row stores of the PREVIOUS iteration acknowledged.  Every later L is complete before the
            // back edge: the copy from Ln behind the stores waits for it with vmcnt(16), the stores still in flight.)
        }
        for (unsigned long long job = job_begin; job < job_end; ++job) {
            SGX_STAMP(19)
            const unsigned long long fa = p.first_frame + 2 * job;             // frame A; B = fa + 1
            const unsigned long long la = 2 * job, lb = la + 1;                // their rows in the output
            const bool have_b = lb < p.n_frames;                                // (a B outside the range is computed and dropped)

            // ---- Hann (fft.rs:53-63) and pass 1 for both frames
            float yr[8], yi[8];
            {
                float zr[4], zi[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) { zr[a] = R[2 * a].x * win[2 * a]; zi[a] = R[2 * a].y * win[2 * a + 1]; }
                fft8_half_zero(zr, zi, yr, yi);
            }
            float vr[8], vi[8];
            {
                float zr[4], zi[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) { zr[a] = R[2 * a + 1].x * win[2 * a]; zi[a] = R[2 * a + 1].y * win[2 * a + 1]; }
                fft8_half_zero(zr, zi, vr, vi);
            }
            SGX_STAMP(0)    // Hann + pass 1 (two frames)
            lds_barrier();  // the previous iteration's partner reads are complete
            SGX_STAMP(1)    // barrier 0
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float2 ya = make_float2(yr[q], yi[q]), yb = make_float2(vr[q], vi[q]);
                if (TR) {
                    addtid_rows<272>(q == 0 ? ya : cmulf(ya, tw1[q]), q == 0 ? yb : cmulf(yb, tw1[q]), m0_wave, q, 8 + q);
                } else {
                    buf[q * kS1 + tid] = q == 0 ? ya : cmulf(ya, tw1[q]);
                    buf[(8 + q) * kS1 + tid] = q == 0 ? yb : cmulf(yb, tw1[q]);
                }
            }
            __builtin_amdgcn_s_setprio(0);  // (wave priorities: stft4096_wg.hip)
            SGX_STAMP(2)    // twiddles + image-1 writes
            lds_barrier();
            SGX_STAMP(3)    // barrier 1

            // ---- pass 2: thread (g2 = 8 F + q1, t0): 16-point FFT over t1, then twiddle w_256^{t0 q2}
            float xr[16], xi[16];
            if (TR) {
                read_planes(rd4_1, xr, xi);
            } else {
#pragma unroll
                for (int t1 = 0; t1 < 16; ++t1) {
                    const float2 v = buf[g2 * kS1 + t0_2 + 16 * t1];
                    xr[t1] = v.x; xi[t1] = v.y;
                }
            }
            fft16(xr, xi);
            SGX_STAMP(4)    // image-1 reads + FFT16
            lds_barrier();  // everyone has read image 1
            SGX_STAMP(5)    // barrier 2
            if (TR) {
                lds_cfloat2 *tw2p = lds_ptr(tw2 + t0_2);
#pragma unroll
                for (int q2 = 0; q2 < 16; q2 += 2) {
                    const int pa = FFT16_OUT[q2], pb = FFT16_OUT[q2 + 1];
                    const float2 va = make_float2(xr[pa], xi[pa]), vb = make_float2(xr[pb], xi[pb]);
                    addtid_rows<280>(q2 == 0 ? va : cmulf(va, lds_read_alone(tw2p, q2 * 16)), cmulf(vb, lds_read_alone(tw2p, (q2 + 1) * 16)), m0_wave, q2, q2 + 1);
                }
            } else {
#pragma unroll
                for (int q2 = 0; q2 < 16; ++q2) {
                    const int pos = FFT16_OUT[q2];
                    const float2 v = make_float2(xr[pos], xi[pos]);
                    buf[t0_2 * kS2 + cbase2 + 8 * q2] = q2 == 0 ? v : cmulf(v, tw2[q2 * 16 + t0_2]);
                }
            }
            SGX_STAMP(6)    // pass-2 twiddles + image-2 writes
            lds_barrier();
            SGX_STAMP(7)    // barrier 3

            // ---- pass 3: thread (F, u): 16-point FFT over t0 -> Z[u + 128 q3]
            if (TR) {
                read_planes(rd4_2, xr, xi);
            } else {
#pragma unroll
                for (int t0 = 0; t0 < 16; ++t0) {
                    const float2 v = buf[t0 * kS2 + tid];
                    xr[t0] = v.x; xi[t0] = v.y;
                }
            }
            fft16(xr, xi);

            // ---- rows: the load of the NEXT iteration (its R[9]), ahead of this iteration's stores (vmcnt retires in issue order), into a
            // second register pair -- L is still needed for the exchange.  Unconditional (a conditional request keeps the old value alive
            // around the loop); past the end of the stream it reads zeros.  (Requested at the TOP of the iteration instead -- a whole
            // iteration to return in -- it sits right behind the previous iteration's sixteen stores: 5-7 % slower, same device.)
            float2 Ln = make_float2(0.0f, 0.0f);
            if (SLIDE && !FUSED) Ln = column(columns_from(128 * (fa + 2) + 1152), 0);
            if (!SLIDE) load_pair(fa + 2);     // (R is dead since pass 1; past the end of the stream: zeros, never stored)

            if (FUSED) __builtin_amdgcn_s_setprio(1);   // the pixel passes are long: 3 only from the row pass (the pixel stores) on
            else __builtin_amdgcn_s_setprio(3);
            SGX_STAMP(8)    // image-2 reads + FFT16 + next column requested
            lds_barrier();  // everyone has read image 2
            SGX_STAMP(9)    // barrier 4
            // partner exchange: publish q3 = 8..15
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int pos = FFT16_OUT[8 + j];
                buf[j * 256 + tid] = make_float2(xr[pos], xi[pos]);
            }
            // the next R[6] = c[128 fa + 1024 + tid] of the thread half a row away: its L (lower half publishes) or its R[7] (upper half)
            if (SLIDE && !TR) {
                xch[tid].x = tid < 128 ? L.x : R[7].x;
                xch[tid].y = tid < 128 ? L.y : R[7].y;
            }
            SGX_STAMP(10)   // partner + window-exchange writes
            lds_barrier();
            SGX_STAMP(11)   // barrier 5
            if (SLIDE) {
                // (TR: column t + 128 is lane ^ 8 of the same wave -- no trip through LDS)
                const float2 Y = TR ? make_float2(lane_xor8((tid & 8) ? R[7].x : L.x), lane_xor8((tid & 8) ? R[7].y : L.y)) : xch[(tid + 128) & 255];
                // ---- slide the window by two half rows, here: L is dead from now on (the Hann products of this iteration were taken at its top)
#pragma unroll
                for (int j = 0; j < 6; ++j) R[j] = R[j + 2];
                R[6] = Y;
                R[7] = L;
            }

            // ---- untangle + magnitude: bins k = u + 128 q3 and 2048 - k.  Z[2048 - k] is register 15 - q3 of thread 128 - u (row 7 - q3);
            // thread 0 holds its own partners one row up (register 16 - q3), and spends its q3 = 0 slot -- DC and Nyquist are not outputs
            // (fft.rs:81) -- on the self-paired bin 1024: Z = P = its register 8, twiddle -i (twu[0][0])
            const int pcol = F * 128 + (u == 0 ? 256 : 128 - u);
            float m1[8], m2[8];
            // rows: every bin pair is stored as soon as it is computed (stft4096_wg.hip does the same for (l, r) rows):
            // sixteen stores spread over the untangle instead of one burst behind it
            constexpr bool kInterleave = (!FUSED && SLIDE) || C64;   // (C64: at any hop -- four arrays of eight would stay live otherwise)   // (same device, 1e6 frames: H 256 3.64 / 3.87 / 3.84 -> 3.56 / 3.82 / 3.81 ms; any other hop -- eight column loads in flight around the stores -- 4.02 -> 4.29: the burst stays there)
            const long long row = (long long)(F == 0 ? la : lb) * (long long)kM * kBin - kBin;      // byte of the (absent) bin 0
            const __amdgpu_buffer_rsrc_t r = out_rsrc(out, !FUSED ? row : 0, !FUSED && (F == 0 || have_b));
            const int l1 = kBin * u, l2 = kBin * (1152 - u);                                        // bins u + 128 q3 ; 2048 - u - 128 q3 = (1152 - u) + 128 (7 - q3)
            auto store_pair = [&](const int q3) {
                // bin k at byte kBin (k - 1).  Thread 0's q3 = 0 slot: bin 1024 from m1, and a second copy of it where its m2 would go.
                const float a = m1[q3], b = (q3 == 0 && u == 0) ? m1[0] : m2[q3];
                const int o1 = (q3 == 0 && u == 0) ? kBin * 1024 : l1;
                const int o2 = (q3 == 0 && u == 0) ? kBin * 128 : l2;                               // 128 + 128 * 7 = 1024
                const int s1 = kBin * 128 * q3, s2 = kBin * 128 * (7 - q3);
                if (F16) {
                    const __half2 ha = __floats2half2_rn(a, a), hb = __floats2half2_rn(b, b);
                    __builtin_amdgcn_raw_buffer_store_b32(*reinterpret_cast<const uint32_t *>(&ha), r, o1 + (s1 & 2047), s1 & ~2047, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(*reinterpret_cast<const uint32_t *>(&hb), r, o2 + (s2 & 2047), s2 & ~2047, 0);
                } else {
                    __builtin_amdgcn_raw_buffer_store_b64(u32x2{__float_as_uint(a), __float_as_uint(a)}, r, o1 + (s1 & 2047), s1 & ~2047, 0);
                    __builtin_amdgcn_raw_buffer_store_b64(u32x2{__float_as_uint(b), __float_as_uint(b)}, r, o2 + (s2 & 2047), s2 & ~2047, 0);
                }
            };
            float2 pvs[8];
            if (kInterleave) {
#pragma unroll
                for (int q3 = 0; q3 < 8; ++q3) pvs[q3] = buf[(7 - q3) * 256 + pcol];
            }
#pragma unroll
            for (int q3 = 0; q3 < 8; ++q3) {
                const int pos = FFT16_OUT[q3];
                float zr_ = xr[pos], zi_ = xi[pos];
                float2 pv = kInterleave ? pvs[q3] : buf[(7 - q3) * 256 + pcol];
                if (q3 == 0) {
                    const float2 own = buf[F * 128];              // thread 0 of the frame: its register 8 as published
                    const int p8 = FFT16_OUT[8];
                    zr_ = u == 0 ? xr[p8] : zr_; zi_ = u == 0 ? xi[p8] : zi_;
                    pv.x = u == 0 ? own.x : pv.x; pv.y = u == 0 ? own.y : pv.y;
                }
                const float er = zr_ + pv.x, ei = zi_ - pv.y;    // Z + conj P   = 2 E
                const float orr = zi_ + pv.y, oi = pv.x - zr_;    // -i (Z - conj P) = 2 O
                const float wr = fmaf(twu[q3].x, orr, -(twu[q3].y * oi)), wi = fmaf(twu[q3].x, oi, twu[q3].y * orr);
                const float ar = er + wr, ai = ei + wi, br = er - wr, bi = ei - wi;
                if constexpr (C64) {
                    // S[k] = (ar, ai) and S[2048 - k] = conj(br + i bi), both already times 2 / W; thread 0's q3 = 0 slot: bin 1024 twice
                    const bool self = q3 == 0 && u == 0;
                    const float cr2 = self ? ar : br, ci2 = self ? ai : -bi;
                    const int o1 = self ? kBin * 1024 : l1, o2 = self ? kBin * 128 : l2;
                    const int s1 = kBin * 128 * q3, s2 = kBin * 128 * (7 - q3);
                    __builtin_amdgcn_raw_buffer_store_b128(u32x4{__float_as_uint(ar), __float_as_uint(ai), __float_as_uint(ar), __float_as_uint(ai)}, r, o1 + s1, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b128(u32x4{__float_as_uint(cr2), __float_as_uint(ci2), __float_as_uint(cr2), __float_as_uint(ci2)}, r, o2 + s2, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    continue;
                }
                m1[q3] = __builtin_amdgcn_sqrtf(fmaf(ar, ar, ai * ai));   // |S[k]| 2 / W      (the scale rides on the window)
                m2[q3] = __builtin_amdgcn_sqrtf(fmaf(br, br, bi * bi));   // |S[2048 - k]| 2 / W
                if (kInterleave) {
                    store_pair(q3);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }

            // ---- store row [M][2] (or half pairs): straight-line code: the wait for the prefetched rows below is then vmcnt(stores issued since)
            if (!FUSED) {
                if (!kInterleave) {
#pragma unroll
                    for (int q3 = 0; q3 < 8; ++q3) store_pair(q3);
                }
            } else {
                // ---- fused pixel columns (simple_spectrogram.rs:141-161): the pair's magnitudes go to LDS as float2 per bin -- (frame A,
                // frame B), each half written by its own frame's threads -- and K1's two pixel passes render both columns
                float2 *mpair = buf;                           // the padded column [bin] (wg::kColSlots)
                float2 *vbuf = mpair + wg::kColSlots;          // [sample slot]
                float *mcol = reinterpret_cast<float *>(buf) + F;
                lds_barrier();  // partner and exchange reads done: the image can be overwritten
                SGX_STAMP(13)   // (pixels) barrier 6
                // the sample pass's table words (nine per thread, the same in every iteration but eighteen registers nobody has to spare across
                // the transform) are requested as the column writes free m1 / m2, one word behind each pair of writes: their L1 / L2 latency
                // falls on the rest of the writes and on the barrier instead of on the head of the pass
                constexpr bool kEarlyWords = PIX != wg::kPixGeneric && MODE != kFbank;   // (the generic instantiation -- interpolator and LUT walk at run time -- has no register left: one spill)
                wg::SampleWords sw;
                const __amdgpu_buffer_rsrc_t rt_words = wg::pcm_rsrc(reinterpret_cast<const float *>(p.samples));
                int tid_w = tid;
                asm volatile("" : "+v"(tid_w));   // (opaque: the nine table offsets are not to be hoisted out of the loop over the transforms)
#pragma unroll
                for (int q3 = 0; q3 < 8; ++q3) {
                    const bool self = q3 == 0 && u == 0;       // thread 0's bin-1024 slot: m1 twice
                    const int k1 = self ? 1024 : u + 128 * q3, k2 = self ? 1024 : 2048 - u - 128 * q3;
                    mcol[2 * k1] = m1[q3];
                    mcol[2 * k2] = self ? m1[0] : m2[q3];
                    if (q3 == 0 && u == 1) {                   // this thread holds bin 1 (m1[0]) and bin 2047 (m2[0]): the repeats around the column
                        mcol[0] = m1[0];
                        mcol[2 * (kM + 1)] = mcol[2 * (kM + 2)] = m2[0];
                    }
                    if (kEarlyWords) {
                        sw.se[q3] = wg::sample_word(rt_words, p, (uint32_t)tid_w + 256u * q3);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                if (kEarlyWords) sw.se[8] = wg::sample_word(rt_words, p, (uint32_t)tid_w + 2048u);
                static_assert(wg::kSampleSteps == 9 && wg::kSampleEarly == 9, "one word per column-write step and one behind them");
                SGX_STAMP(14)   // (pixels) column writes
                lds_barrier();
                SGX_STAMP(15)   // (pixels) barrier 7
                if constexpr (MODE == kFbank) {
                    // one filter pass over the pair's column (frame A in .x, frame B in .y), a wave per filter: element j of a row is bin j + 1
                    float2 *sums = reinterpret_cast<float2 *>(p.rgba);
                    __builtin_amdgcn_s_setprio(3);
                    fbank::filter_pass<true>(mpair + 1, reinterpret_cast<const fbank::Filter *>(p.rows), reinterpret_cast<const float *>(p.samples), p.R,
                                             p.interp == 2u, sums + la * (size_t)p.R, sums + lb * (size_t)p.R, true, have_b, (uint32_t)tid, 4u);
                    // the next iteration's load behind the pass, straight into L (dead since the slide): requested in front of it, it is two
                    // more registers alive through the pass and two spills
                    if (SLIDE) L = column(columns_from(128 * (fa + 2) + 1152), 0);
                } else {
                if (kEarlyWords) wg::sample_pass_with<PIX>(p, mpair, vbuf, tid, sw);
                else wg::sample_pass<PIX>(p, mpair, vbuf, tid);
                // the fused pixel path requests the next iteration's load HERE, straight into L (dead since the slide): requested in front
                // of the exchange like the rows' it is two more live registers through the sample pass -- two spills, and a spill reload
                // is a vector-memory load the compiler waits for with vmcnt(0), this load included (same device: 3.79 -> 3.68 ms)
                [[maybe_unused]] wg::PeakDst peak_a{}, peak_b{};
                [[maybe_unused]] wg::PeakOld<true> peak_old{};
                if constexpr (MODE == kPeak) {
                    // the column's rows as they are, requested in front of the barrier -- and in front of the next transform's load, which comes
                    // from HBM: the counter retires in order, and behind that load the row pass would wait for it too
                    peak_a = wg::peak_dst(p, la);
                    peak_b = have_b ? wg::peak_dst_next(p, peak_a, lb) : peak_a;
                    peak_old = wg::peak_prefetch<true>(p, peak_a, tid);
                }
                if (SLIDE) L = column(columns_from(128 * (fa + 2) + 1152), 0);
                SGX_STAMP(16)   // (pixels) sample pass
                lds_barrier();
                SGX_STAMP(17)   // (pixels) barrier 8
                __builtin_amdgcn_s_setprio(3);
                if constexpr (MODE == kPeak) {
                    wg::row_pass_peak<true>(p, row_words, vbuf, peak_a, peak_b, peak_old, have_b, tid);
                } else if constexpr (MODE == kBands) {
                    float2 *bands = reinterpret_cast<float2 *>(p.rgba);
                    wg::row_pass_bands<true>(p, row_words, vbuf, bands + la * (size_t)p.R, bands + lb * (size_t)p.R, true, have_b, tid);
                } else {
                    uchar4 *rgba = reinterpret_cast<uchar4 *>(p.rgba);
                    wg::row_pass<true, PIX>(p, row_words, vbuf, rgba + la * (size_t)p.R, rgba + lb * (size_t)p.R, true, have_b, pal, tid);
                }
                }
            }
            if (SLIDE && !FUSED) {
                // `Ln` is pinned behind the row stores: its copy into L needs the load complete, and scheduled in front of the stores (where
                // the compiler had put it) that is a vmcnt(0) in the middle of the iteration; here it is vmcnt(stores since).  (The load
                // straight into L behind the slide, no second pair: 4 % slower on the same device.)
                asm volatile("" : "+v"(Ln.x), "+v"(Ln.y));
                L = Ln;
            }
            SGX_STAMP(18)   // rows: 16 stores issued + wait for the next column; pixels: the row pass (sums, dB, LUT, pixel stores)
        }
#if SGX_STAMPS
        jobs_done += job_end - job_begin;
#endif
        if (!claiming) break;
        lds_barrier();   // (a run may be empty: no barrier of the loop stands between the write above and this read)
        const unsigned long long word = *claim_word;
        const unsigned long long chunk_i = ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(word >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)word);
        lds_barrier();   // everyone has read it: thread 0 may park the next one
        if (chunk_i >= p.claim_chunks) break;
        job_begin = p.claim_pool_begin + chunk_i * p.claim_chunk;
        job_end = job_begin + p.claim_chunk < p.n_jobs ? job_begin + p.claim_chunk : p.n_jobs;
    }
#if SGX_STAMPS
    if (tid == 0 && blockIdx.x < kFinishBlocks) {
        g_finish_r[4 * blockIdx.x + 1] = wall_clock64();
        g_finish_r[4 * blockIdx.x + 2] = blockIdx.x;
        g_finish_r[4 * blockIdx.x + 3] = jobs_done;
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int i = 0; i < 20; ++i) atomicAdd(&g_phase_cycles_r[i], st_acc[i]);
        atomicAdd(&g_phase_cycles_r[20], jobs_done);
    }
#endif
}

struct RealTables {
    DeviceBuffer<float2> d_tw1, d_tw2, d_twu;
    DeviceBuffer<unsigned long long> d_claim;   // [1] the claim counter of a rows launch with a claimed tail: zeroed on the stream in front of every such launch
};

}  // namespace wgr

#if SGX_STAMPS
extern "C" __attribute__((visibility("default"))) int sgx_debug_phase_cycles_r(unsigned long long *h_out, int reset)
{
    hipError_t e = hipMemcpyFromSymbol(h_out, HIP_SYMBOL(wgr::g_phase_cycles_r), sizeof(unsigned long long) * 24);
    if (e == hipSuccess && reset) {
        unsigned long long zero[24] = {0};
        e = hipMemcpyToSymbol(HIP_SYMBOL(wgr::g_phase_cycles_r), zero, sizeof(zero));
    }
    return e == hipSuccess ? 0 : -1;
}
// the first n_blocks records of g_finish_r (four words each), as the last launch of the kernel left them
extern "C" __attribute__((visibility("default"))) int sgx_debug_finish_r(unsigned long long *h_out, int n_blocks)
{
    if (n_blocks < 0 || n_blocks > wgr::kFinishBlocks) return -1;
    return hipMemcpyFromSymbol(h_out, HIP_SYMBOL(wgr::g_finish_r), sizeof(unsigned long long) * 4 * (size_t)n_blocks) == hipSuccess ? 0 : -1;
}
#endif

void TablesDelete::operator()(wgr::RealTables *t) const { delete t; }

hipError_t real4096_init(sgx_ctx *c)
{
    using namespace wgr;
    TablesPtr<RealTables> t(new RealTables());
    std::vector<float2> tw1(8 * 256), tw2(256), twu(8 * 128);
    for (int q = 0; q < 8; ++q)
        for (int tt = 0; tt < 256; ++tt) tw1[q * 256 + tt] = unit_root2((unsigned long long)tt * q, 2048);
    for (int q = 0; q < 16; ++q)
        for (int t0 = 0; t0 < 16; ++t0) tw2[q * 16 + t0] = unit_root2((unsigned long long)t0 * q, 256);
    for (int q3 = 0; q3 < 8; ++q3)
        for (int uu = 0; uu < 128; ++uu) twu[q3 * 128 + uu] = unit_root2((unsigned long long)(uu + 128 * q3), 4096);
    twu[0] = unit_root2(1024, 4096);   // thread 0, q3 = 0: the self-paired bin 1024
    hipError_t e = t->d_tw1.upload(tw1);
    if (e == hipSuccess) e = t->d_tw2.upload(tw2);
    if (e == hipSuccess) e = t->d_twu.upload(twu);
    if (e == hipSuccess) e = t->d_claim.alloc(1);
    if (e == hipSuccess) c->real = std::move(t);
    return e;
}

// the streams this kernel serves: one channel, W = 2048 (H = 256 slides its window in registers)
bool real4096_serves(const sgx_ctx *c, const float *d_pcm, uint32_t channels)
{
    (void)d_pcm;   // any hop, any (4-byte) alignment of the stream: see samples_from
    return channels == 1 && c->real && c->W == (uint32_t)wgr::kW;
}

namespace wg {

// the deal of a rows launch of n_jobs jobs in `blocks` workgroups: (16, 0) static, else (static share in sixteenths, jobs per chunk); w: the slot
// weights of the static runs (run_claim.hpp), all 64 for the equal deal
struct RowsClaim { uint32_t sixteenths, chunk; uint32_t w[4]; };
static RowsClaim rows_claim(const sgx_ctx *c, Out kind, unsigned long long n_jobs, unsigned long long blocks)
{
    const bool rows = kind == Out::kMags || kind == Out::kMagsF16 || kind == Out::kComplex;
#ifdef SGX_VARIANT_SKIP_LAST_JOB   // (the sensitivity build compiles the equal static split only)
    const bool compiled = false;
#else
    const bool compiled = true;
#endif
    RowsClaim rc{16u, 0u, {64u, 64u, 64u, 64u}};
    if (!rows || !compiled || n_jobs == 0) return rc;
    // the weights: the context's (sgx_set_run_weights) anywhere, else the measured ones where the slots are the measured ones
    const bool forced_w = c->run_weights[0] != 0u;
    const unsigned *w = forced_w ? c->run_weights : slot_weights_measured(blocks, (unsigned long long)c->n_cu, c->n_cu != c->n_cu_device, c->H) ? slot_weights_auto(kind == Out::kComplex) : kSlotWeightsEqual;
    for (int s = 0; s < 4; ++s) rc.w[s] = w[s];
    if (c->claim_sixteenths == 16u && c->claim_chunk == 0u) return rc;
    if (c->claim_chunk != 0u) {
        rc.sixteenths = c->claim_sixteenths;
        rc.chunk = c->claim_chunk;
        return rc;
    }
    // (the complex rows -- twice the bytes per job -- lose with a pool of equal runs, +0.2 ... +3.5 %, profiles/k1r_claimed_tail.txt, and gain nothing
    // from one behind weighted runs, profiles/k1r_slot_weights.txt: their weights stand alone)
    if (kind == Out::kComplex || !run_claim_engages(n_jobs, blocks)) return rc;
    const bool weighted = !slot_weights_equal(rc.w);
    rc.sixteenths = weighted ? kSlotAutoSixteenths : kClaimAutoSixteenths;
    rc.chunk = weighted ? kSlotAutoChunk : kClaimAutoChunk;
    return rc;
}

// p: as launch_wg4096 (stft4096_wg.hip) fills it for a one-channel stream -- stream, window, tw2, output, the pixel tables; the
// transform's own tables and the job split are set here
hipError_t launch_real4096(const sgx_ctx *c, Params p, Out kind)
{
    using namespace wgr;
    if (p.n_frames == 0) return hipSuccess;
    const RealTables *t = c->real.get();
    const bool hold_peak = kind == Out::kPeak;
    p.tw1 = t->d_tw1.get();
    p.tw2 = t->d_tw2.get();
    p.twu = t->d_twu.get();
    p.stream_samples = p.total_frames ? (p.total_frames - 1) * (unsigned long long)c->H + (unsigned long long)kW : 0;   // what the stream's frames cover (the caller may hold more)
    p.n_jobs = (p.n_frames + 1) / 2;
    RunSplit runs = run_split(c, p.n_jobs, 4);   // persistent workgroups, four per CU, each a contiguous run of frame pairs
    if (hold_peak) {   // sgx_bands_peak_batch: a run is 2 per frames
        runs = runs_of(p.n_jobs, peak_align_run(runs.per, 2, p.peak_group));
        p.peak_run = 2 * runs.per;
    }
    p.jobs_per_block = runs.per;
    // The rows launches deal only a share of the jobs statically and let the workgroups claim the rest in chunks (run_claim.hpp): where the
    // context forces it (sgx_set_run_claim), else where the static run that is left is still long.  Otherwise nothing here differs from
    // the static launch: no counter, no memset.
    const RowsClaim rc = rows_claim(c, kind, p.n_jobs, runs.blocks);
    const bool pooled = rc.sixteenths != 16u || rc.chunk != 0u;
    RunClaim split{};
    if (!slot_weights_equal(rc.w)) {
        // static runs sized by slot: the deal rides in the LUT and seed words (Params), the kernel forms its run from them (slot_run)
        const SlotDeal deal = slot_deal(p.n_jobs, runs.blocks, (unsigned long long)c->n_cu, rc.sixteenths, rc.chunk, rc.w);
        p.slot_per0 = deal.per[0];
        p.slot_per1 = deal.per[1];
        p.slot_per2_lo = (uint32_t)deal.per[2];
        p.slot_per2_hi = (uint32_t)(deal.per[2] >> 32);
        p.slot_per3_lo = (uint32_t)deal.per[3];
        p.slot_per3_hi = (uint32_t)(deal.per[3] >> 32);
        p.slot_n_cu = (uint32_t)c->n_cu;
        p.slot_leftover = (uint32_t)deal.leftover;
        split = deal.claim;
    } else if (pooled) {
        split = run_claim(p.n_jobs, runs.blocks, rc.sixteenths, rc.chunk);
        p.jobs_per_block = split.per;
    }
    if (pooled) {
        // zero on the stream in front of every launch: a replayed or an aborted launch leaves nothing behind that the next one reads
        const hipError_t e = hipMemsetAsync(t->d_claim.get(), 0, sizeof(unsigned long long), c->stream);
        if (e != hipSuccess) return e;
        p.claim_counter = t->d_claim.get();
        p.claim_pool_begin = split.pool_begin;
        p.claim_chunks = split.n_chunks;
        p.claim_chunk = (uint32_t)split.chunk;
    }
    const size_t lds_claim = p.claim_counter ? sizeof(unsigned long long) : 0;   // the parked claim index, behind the tables
    const dim3 grid((unsigned)runs.blocks), block(256);
    auto launch = [&](auto slide_c) {
        constexpr bool S_ = decltype(slide_c)::value;
        const size_t lds_rows = (S_ ? kLdsBytesR : kLdsBytes) + lds_claim;
        constexpr size_t lds_render = S_ ? kLdsBytesRenderR : kLdsBytesRender;
        if (hold_peak) {
            if (p.interp == SGX_INTERP_COSINE) hipLaunchKernelGGL((stft4096_real_kernel<kPeak, kPixPeakCosine, S_>), grid, block, lds_rows, c->stream, p);
            else hipLaunchKernelGGL((stft4096_real_kernel<kPeak, kPixPeakCubic, S_>), grid, block, lds_rows, c->stream, p);
        } else if (kind == Out::kFbank) {   // (no palette either)
            hipLaunchKernelGGL((stft4096_real_kernel<kFbank, kPixFbank, S_>), grid, block, lds_rows, c->stream, p);
        } else if (kind == Out::kBands) {   // (no palette: the row-image LDS size)
            if (p.interp == SGX_INTERP_COSINE) hipLaunchKernelGGL((stft4096_real_kernel<kBands, kPixBandsCosine, S_>), grid, block, lds_rows, c->stream, p);
            else hipLaunchKernelGGL((stft4096_real_kernel<kBands, kPixBandsCubic, S_>), grid, block, lds_rows, c->stream, p);
        } else if (kind == Out::kRgba) {
            if (!p.seed_pm1) hipLaunchKernelGGL((stft4096_real_kernel<kPixels, kPixGeneric, S_>), grid, block, lds_render, c->stream, p);
            else if (p.interp == SGX_INTERP_COSINE) hipLaunchKernelGGL((stft4096_real_kernel<kPixels, kPixCosine, S_>), grid, block, lds_render, c->stream, p);
            else hipLaunchKernelGGL((stft4096_real_kernel<kPixels, kPixCubic, S_>), grid, block, lds_render, c->stream, p);
        } else if (kind == Out::kComplex) {
            hipLaunchKernelGGL((stft4096_real_kernel<kRowsC64, kPixNone, S_>), grid, block, lds_rows, c->stream, p);
        } else if (kind == Out::kMagsF16) {
            hipLaunchKernelGGL((stft4096_real_kernel<kRowsF16, kPixNone, S_>), grid, block, lds_rows, c->stream, p);
        } else {
            hipLaunchKernelGGL((stft4096_real_kernel<kRowsF32, kPixNone, S_>), grid, block, lds_rows, c->stream, p);
        }
    };
    if (c->H == 256) launch(std::true_type{});
    else launch(std::false_type{});
    const hipError_t e = hipGetLastError();
    return e == hipSuccess && hold_peak ? launch_peak_combine(c, p, runs.blocks) : e;
}

}  // namespace wg

}  // namespace sgx

// Diagnostic: how the rows launches of the real-input 4096-point kernel deal their jobs (run_claim.hpp).  (16, 0): the static split; (0, 0): the
// automatic rule; else the claimed tail at any size, `static_sixteenths` of the jobs dealt statically and the rest in chunks of `chunk_jobs`.
// The results do not depend on it, bit for bit.
int sgx_set_run_claim(sgx_ctx *c, uint32_t static_sixteenths, uint32_t chunk_jobs)
{
    if (!c) return SGX_ERR_INVALID_ARG;
    if (!sgx::run_claim_valid(static_sixteenths, chunk_jobs)) {
        c->err = "sgx_set_run_claim: a share of 0 .. 16 sixteenths with a chunk of 1 .. 2^20 jobs, (16, 0) for the static split or (0, 0) for the automatic rule";
        return SGX_ERR_INVALID_ARG;
    }
    c->claim_sixteenths = static_sixteenths;
    c->claim_chunk = chunk_jobs;
    return SGX_OK;
}

// the split a float or half rows call of n_frames frames runs under, now: (16, 0) where it is the static one (complex rows: only a forced split)
int sgx_run_claim(const sgx_ctx *c, size_t n_frames, uint32_t *static_sixteenths, uint32_t *chunk_jobs)
{
    if (!c || !static_sixteenths || !chunk_jobs) return SGX_ERR_INVALID_ARG;
    sgx::wg::RowsClaim rc{16u, 0u, {64u, 64u, 64u, 64u}};
    if (sgx::real4096_serves(c, nullptr, c->C) && !(c->cfg.flags & (SGX_FLAG_PAIRED_FRAMES | SGX_FLAG_COMPLEX_MONO))) {
        const unsigned long long n_jobs = ((unsigned long long)n_frames + 1) / 2;
        rc = sgx::wg::rows_claim(c, sgx::Out::kMags, n_jobs, sgx::run_split(c, n_jobs, 4).blocks);
    }
    *static_sixteenths = rc.sixteenths;
    *chunk_jobs = rc.chunk;
    return SGX_OK;
}

// Diagnostic: the slot weights of those launches' static runs (run_claim.hpp: the n-th workgroup placed on a CU runs w[n] / 64 of the equal
// run).  Null or all zero: the automatic weights.  Forced weights apply at any CU limit.  The results do not depend on them, bit for bit.
int sgx_set_run_weights(sgx_ctx *c, const uint32_t *w)
{
    if (!c) return SGX_ERR_INVALID_ARG;
    const bool automatic = !w || (w[0] == 0u && w[1] == 0u && w[2] == 0u && w[3] == 0u);
    if (!automatic && !sgx::run_weights_valid(w)) {
        c->err = "sgx_set_run_weights: four weights of at least 1 each that sum to 256, or all zero (a null pointer) for the automatic ones";
        return SGX_ERR_INVALID_ARG;
    }
    for (int s = 0; s < 4; ++s) c->run_weights[s] = automatic ? 0u : w[s];
    return SGX_OK;
}

// the weights a float rows call of n_frames frames runs under, now: (64, 64, 64, 64) where its static runs are equal
int sgx_run_weights(const sgx_ctx *c, size_t n_frames, uint32_t *w)
{
    if (!c || !w) return SGX_ERR_INVALID_ARG;
    sgx::wg::RowsClaim rc{16u, 0u, {64u, 64u, 64u, 64u}};
    if (sgx::real4096_serves(c, nullptr, c->C) && !(c->cfg.flags & (SGX_FLAG_PAIRED_FRAMES | SGX_FLAG_COMPLEX_MONO))) {
        const unsigned long long n_jobs = ((unsigned long long)n_frames + 1) / 2;
        rc = sgx::wg::rows_claim(c, sgx::Out::kMags, n_jobs, sgx::run_split(c, n_jobs, 4).blocks);
    }
    for (int s = 0; s < 4; ++s) w[s] = rc.w[s];
    return SGX_OK;
}
