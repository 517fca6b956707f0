// stft4096_wg.hpp -- declarations shared by the two workgroup-per-transform kernels
// (stft4096_wg.hip: scalar codelets; stft4096_wgp.hip: packed (re, im) codelets).
#pragma once
#include <hip/hip_fp16.h>

#include "sgx_fbank.hpp"
#include "sgx_internal.hpp"

namespace sgx {
namespace wg {

constexpr int kW = 2048, kP = 4096, kM = 2047;
// Sliding the sample window in registers (2 new rows per mono transform instead of 9 loads): every
// sample is fetched once per workgroup.  It pins 7 VGPRs across the FFT passes (the scalar kernel
// then spills 3 registers) but the launch is bound by total HBM traffic, and dropping the overlap
// re-reads (3.3 -> 1.0 KB per frame) was worth +5 % (same-device A/B, 1e6 frames).
constexpr bool kSlideWindow = true;
constexpr int kS1 = 272;            // row stride (complex) of the pass-1 -> pass-2 image [q1][t]
constexpr int kS2 = 257;            // row stride (complex) of the pass-2 -> pass-3 image [t0][q1 + 16 q2]
constexpr int kBufComplex = 16 * kS1;  // 4352 complex = 34 816 B (also holds 16*257 and 9*256)
constexpr size_t kLdsBytes = (size_t)(kBufComplex + 256) * sizeof(float2);
constexpr size_t kLdsBytesRender = kLdsBytes + 256 * sizeof(uint2);   // + the palette table of pixel_for: {threshold to leave index i, RGBA of index i}

struct PackedSample {
    int32_t i0;   // cubic: floor(index) = x1; cosine: low.  The taps are the slots i0 .. i0 + 3 (cubic) / i0 + 1, i0 + 2 (cosine) of the padded column
    float w;      // cubic: mu;           cosine: o' (the cosine-eased offset)
};

struct Params {
    const float *pcm;
    const float2 *tw1;   // [16][256]  w_4096^{t q1}
    const float2 *tw2;   // [16][16]   w_256^{t0 q2} at [q2][t0]
    const float *window; // [2048]
    // The filterbank mode (sgx_fbank_batch, kPixFbank) has no sample stage, no row tables and no palette either, and rides the same way:
    // `rows` is the bank's filter table (fbank::Filter [n_filters]), `samples` its weights, `n_samples` their count, `R` the filter
    // count, `interp` the power (1 or 2) and `rgba` the output, float2 [F][pairs][n_filters].
    // Peak-hold columns (sgx_bands_peak_batch, the kPixPeak* instantiations; `rgba` is then float2 [columns][pairs][R]) write no rows
    // and carry no palette: their three values ride in those words, so that the argument block of every other instantiation -- and
    // with it their code objects -- stays as it is.
    union {
        float *mags;
        float2 *peak_partial;            // [workgroups][2][R]: columns that leave a workgroup's run at its front (slot 0) or at its back (slot 1)
    };
    unsigned long long first_frame, n_frames, n_jobs, jobs_per_block;
    unsigned long long pair_base;  // mono: global index of the first frame PAIR (first_frame / 2)
    unsigned long long total_frames;  // frames the stream holds (a pair's second frame is transformed whenever it exists)
    uint32_t H, C, pair_l, pair_r, pairs, pair;
    uint32_t out_f16;          // magnitudes are stored as (l, r) half pairs, 4 B per bin (the F16F16 ring of gpu_spectrogram.rs:218-226)
    // fused pixel path (RENDER): magnitudes never leave LDS
    // The rows launches of the real-input kernel read none of the pixel fields: a launch with a claimed tail (run_claim.hpp) carries its
    // four values in those words, for the same reason as the peak-hold columns above.  claim_counter null: the static split.
    union {
        const uint32_t *rows;      // [R]  first slot | count << 16
        unsigned long long *claim_counter;   // one device word, zero at the launch: the next chunk of the pool
    };
    union {
        const PackedSample *samples;   // one entry per LDS slot: the rows' samples in lin_space order, plus pad slots (see wg4096_init)
        unsigned long long claim_pool_begin;   // first job of the pool; jobs_per_block is then the static run
    };
    union {
        uint32_t n_samples;        // slots per column (sum of the rows' counts + pads)
        uint32_t claim_chunk;      // jobs per chunk
    };
    // A rows launch of the real-input kernel whose static runs are dealt by slot (run_claim.hpp, SlotDeal) carries the deal in the LUT and
    // seed words: the four run lengths (slots 2 and 3 as two 32-bit halves each), the blocks per slot and the leftover count.  The slot
    // bases are not carried -- there are 44 such bytes, not 72 -- but formed from the lengths in front of the run loop (slot_run).
    // slot_n_cu 0: the equal deal, blockIdx.x * jobs_per_block.
    union {
        const float *lut_thr;            // [255]
        unsigned long long peak_group;   // frames per column, at most n_frames
        unsigned long long slot_per0;
    };
    union {
        const uchar4 *lut_rgba;          // [256]
        unsigned long long peak_run;     // frames per workgroup: its run is [blockIdx.x * peak_run, + peak_run) of the call's frames
        unsigned long long slot_per1;
    };
    union {
        uint8_t *rgba;             // [F][pairs][R][4]
        unsigned long long claim_chunks;   // chunks of the pool: a claim index from here on ends the workgroup
    };
    union { uint32_t R; uint32_t slot_per2_lo; };
    union { uint32_t interp; uint32_t slot_per2_hi; };
    union { float guess_a; uint32_t slot_per3_lo; };    // LUT index ~ floor(log2(power + 1e-7) * a + b), then exact fix-up
    union { float guess_b; uint32_t slot_per3_hi; };
    union { uint32_t seed_pm1; uint32_t slot_n_cu; };         // the host has shown that this seed is never off by more than one (seed_within_one): one compare pair fixes it
    union { uint32_t single_rows; uint32_t slot_leftover; };  // bit i: every row of block i (rows 256 i .. 256 i + 255) averages exactly one sample
    uint32_t block_max_cnt;    // byte i: the largest sample count of a row of block i.  No kernel reads it (docs/history/retired_switches.md): it keeps the argument layout
    // the real-input kernel (stft4096_real.hip: every mono frame its own transform; tw1 is then [8][256] w_2048^{t q1})
    const float2 *twu;         // [8][128] w_4096^{u + 128 q3} at [q3][u]; [0][0] holds w_4096^{1024} = -i
    unsigned long long stream_samples;   // samples the frames of the stream cover: columns past them read as zero
};
static_assert(sizeof(Params) == 216, "the kernel argument of every instantiation: its size is part of their code objects");

// sgx_bands_peak_batch: the jobs of a workgroup's run, `per` of `fpj` (1 or 2) frames each, rounded up to whole columns of `group` frames
// where that lengthens the run by at most 1/32 -- the runs are resident side by side, so a longer run is a longer launch, and finishing
// the columns that cross a boundary (peak_combine_kernel) costs far less than that for all but the smallest groups
inline unsigned long long peak_align_run(unsigned long long per, unsigned fpj, unsigned long long group)
{
    const unsigned long long unit = group % fpj == 0 ? group : group * fpj, run = per * fpj;
    if (unit > run / 32) return per;
    return (run + unit - 1) / unit * unit / fpj;
}
hipError_t launch_peak_combine(const sgx_ctx *c, const Params &p, unsigned long long blocks);   // stft4096_wg.hip

// stft4096_real.hip
hipError_t launch_real4096(const sgx_ctx *c, Params p, Out kind);   // kPeak: p.peak_group, p.peak_partial

// Which two mono frames share a transform: always (2j, 2j+1).
//   kPairAdjacentRow : H = 256: frame 2j+1's rows are frame 2j's rows shifted by one (9 rows feed both)
//   kPairAdjacent    : any other hop (16 row loads)
// (Tried and rejected, same-device A/B on 1e6 frames: pairing (f, f+16) plus a per-row lane rotation
// so that both rows' stores are 128-byte aligned: -10 %, the extra row loads cost more than the
// alignment buys; 16-byte stores via a DPP lane-pair exchange: -8 %.  The launch is bound by total
// HBM traffic, not by store alignment or store instruction count.)
constexpr int kPairAdjacentRow = 0, kPairAdjacent = 1;

struct WgTables {
    DeviceBuffer<float2> d_tw1, d_tw2;
    DeviceBuffer<uint32_t> d_rows;        // packed row table for the fused pixel path
    DeviceBuffer<PackedSample> d_samples;
    uint32_t n_samples = 0;
    uint32_t single_rows = 0;          // Params::single_rows
    uint32_t block_max_cnt = 0;        // Params::block_max_cnt
    bool fusable = false;
    DeviceBuffer<float> d_planes;          // more than two channels: (l, r) pair planes of the sample range of a call, grown on demand
    DeviceBuffer<float2> d_peak_partial;   // sgx_bands_peak_batch: [workgroups][2][R] partial columns (peak_dst), grown on demand
};

__device__ __forceinline__ void lds_barrier()
{
    // LDS-only workgroup barrier: outstanding global stores are NOT waited for
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// An 8-byte LDS read that stays one: the compiler merges two reads off one base register into a ds_read2_b64, which occupies the LDS
// pipe for 8 cycles where two ds_read_b64 take 2 each (MI355X_MICROARCH.md, LDS table).  The empty statement makes the base a new value
// for every read (no instruction; the register allocator keeps it in place).
typedef float lds_f2v __attribute__((ext_vector_type(2)));
typedef const lds_f2v __attribute__((address_space(3))) lds_cfloat2;   // (an LDS pointer by type: behind the statement nothing else says so)
__device__ __forceinline__ lds_cfloat2 *lds_ptr(const float2 *p) { return (lds_cfloat2 *)p; }
__device__ __forceinline__ float2 lds_read_alone(lds_cfloat2 *&base, int idx)
{
    asm("" : "+v"(base));
    const lds_f2v v = base[idx];
    return make_float2(v.x, v.y);
}

// one row of [M][2] floats; rowm8 = row base - 8 bytes (bin k lives at byte 8 k of rowm8): a uniform
// (SGPR) row base plus one 32-bit lane offset, immediate offsets per segment
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// A raw buffer descriptor over one output row: base = the row's bin-0 address (uniform), no stride, no bounds
// in the way (2 GB window).  Stores through it take an SGPR descriptor + one 32-bit lane offset + a scalar
// segment offset + an immediate: no per-lane 64-bit address arithmetic at all.
// `present` false: zero records, every store through the descriptor is dropped by the range check (lane offset + scalar offset against
// the records: tools/bufrange.hip) -- a row outside the requested range costs no branch, and the stores of an iteration are
// straight-line code whose count the compiler's vmcnt waits can rely on
__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(char *mags, long long row_byte, bool present = true)
{
    const uint32_t olo = __builtin_amdgcn_readfirstlane((uint32_t)row_byte);
    const uint32_t ohi = __builtin_amdgcn_readfirstlane((uint32_t)((unsigned long long)row_byte >> 32));
    const int records = __builtin_amdgcn_readfirstlane(present ? 0x7fffffff : 0);
    return __builtin_amdgcn_make_buffer_rsrc(mags + (long long)(((unsigned long long)ohi << 32) | olo), 0, records, 0x00020000);
}

// the same kind of descriptor over the sample stream from a wave-uniform address on (a frame's first sample)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t pcm_rsrc(const float *base)
{
    const unsigned long long a = (unsigned long long)base;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((unsigned long long)hi << 32) | lo), 0, 0x7fffffff, 0x00020000);
}

// one row of [M][2] floats; row_byte = byte offset of the row's (absent) bin 0, bin k lives 8 k bytes on
// Cache policy of the magnitude stores (A/B on one device, 1e6 frames): an (l, r) stream re-reads 7/8 of every frame's
// samples through L2, and marking the output non-temporal keeps them there: 6.00 -> 5.57 ms.  A mono stream slides its
// window in registers and re-reads nothing: there the same bit costs 10-40 %, sc1 30 %.
constexpr int kAuxNt = 2;   // the `nt` bit of a buffer store
template <bool DUP>  // DUP: mono, the row holds (m, m); else (va, vb) = (left, right)
__device__ __forceinline__ void store_row(char *mags, long long row_byte, int col, const float (&va)[8], const float (&vb)[8], bool present = true)
{
    const __amdgpu_buffer_rsrc_t r = row_rsrc(mags, row_byte, present);
    const int lane_off = col * 8;
    // k = 0 (DC) is not part of the output (fft.rs:81): thread 0's first store carries a lane offset beyond the descriptor's 2 GB and is
    // dropped by the range check (tools/bufrange.hip) -- eight store instructions in straight-line code for every wave, so that the
    // compiler's count of the stores issued since the prefetch (its vmcnt waits) is exact
    const int lane_off0 = col != 0 ? lane_off : (int)0x80000000;
#pragma unroll
    for (int q3 = 0; q3 < 8; ++q3) {
        const u32x2 d = {__float_as_uint(va[q3]), __float_as_uint(DUP ? va[q3] : vb[q3])};
        __builtin_amdgcn_raw_buffer_store_b64(d, r, (q3 == 0 ? lane_off0 : lane_off) + 2048 * (q3 & 1), 4096 * (q3 >> 1), DUP ? 0 : kAuxNt);
    }
}

// ---- fused pixel column: magnitude_in -> color_for -> put_pixel (simple_spectrogram.rs:141-161) ---------------
// Two passes over LDS, both balanced whatever the rows' sample counts (a row of the log axis averages 1 sample
// at the bottom and 11 at the top: one thread per ROW leaves the wave that owns the top rows with twice the work
// of the others, and walks the sample table in a dependent loop of L1 loads):
//   sample pass  one thread per magnitude_in SAMPLE (2 173 per column at 48 kHz / 1024 rows): coalesced table
//                read, interpolation of BOTH channels (stereo) or BOTH mono columns of the transform -- the
//                column lives in LDS as float2 per bin either way -- result to LDS
//   row pass     one thread per row: sum of its samples in lin_space order (Complex::sum), the divide, dB
//                thresholds, LUT, pixel store (coalesced: consecutive lanes, consecutive image rows).  A row's slots
//                start at an odd distance from the previous row's where the count is even (pad slots, host table
//                only): 32 consecutive rows of 8 samples then touch 32 different bank pairs instead of 4
// The column in LDS (round 4): P[k] = bin k (k = 1 .. 2047, i.e. data[k - 1] of interpolated_frequency_sample.rs), with the end bins
// REPEATED around it -- P[0] = bin 1, P[2048] = P[2049] = bin 2047 -- so that the saturating index arithmetic of :89-105
// (x0 = max(x1 - 1, 0), x2 / x3 = min(x1 + 1 / 2, M - 1)) is a plain read of four CONTIGUOUS slots P[x1 .. x1 + 3] for every sample:
// no clamped variant, no branch per sample, two ds_read2_b64 per cubic sample (one per cosine sample: P[lo + 1], P[lo + 2]).
constexpr int kColSlots = 2050;                                 // slots of the padded column
constexpr int kMaxFusedSamples = kBufComplex - kColSlots;       // float2 per sample behind it (2302)
// which pixel code an instantiation carries: the launch-uniform switches -- the interpolator, the LUT search -- are compile-time,
// each instantiation holds one path's code and live ranges
constexpr int kPixNone = 0, kPixCubic = 1, kPixCosine = 2, kPixGeneric = 3, kPixRowsF16 = 4;   // kPixRowsF16: no pixels either -- half-pair rows (stft4096_wg.hip)
// the fused column without the colour (sgx_bands_batch): the row pass stores the (l, r) means as float2, lowest row first; no palette
constexpr int kPixBandsCubic = 5, kPixBandsCosine = 6;
// the bands column held as a running maximum over groups of frames (sgx_bands_peak_batch): the row pass of the bands instantiations,
// its store a load / max / store on a column that only this workgroup writes
constexpr int kPixPeakCubic = 8, kPixPeakCosine = 9;
constexpr bool pix_peak(int pix) { return pix == kPixPeakCubic || pix == kPixPeakCosine; }
constexpr bool pix_bands(int pix) { return pix == kPixBandsCubic || pix == kPixBandsCosine || pix_peak(pix); }
constexpr bool pix_cosine(int pix) { return pix == kPixCosine || pix == kPixBandsCosine || pix == kPixPeakCosine; }   // the interpolator is compile-time
// a filterbank over the column (sgx_fbank_batch): the magnitudes go to LDS as for the bands, then one filter pass (sgx_fbank.hpp) -- no sample
// stage, no row pass; the bank's tables ride in the words of the row and sample tables (Params)
constexpr int kPixFbank = 10;
// a filterbank over the four products of the (L, R) pair (sgx_fbank_cross_batch): the split's L and R never become magnitudes -- every
// thread forms |L|^2, |R|^2, Re and Im of L conj R of its eight bins (fbank::cross_terms) into two float2 columns of kColSlots slots in
// the transform's buffer (2 x 2050 x 8 B of its 34 816), then one cross pass (sgx_fbank.hpp).  The bank rides as for kPixFbank; `rgba`
// is the output, float4 [F][pairs][n_filters].  (l, r) streams and pair planes only.
constexpr int kPixFbankCross = 11;
static_assert(2 * kColSlots <= kBufComplex, "the two product columns lie in the transform's buffer");
// no pixels: the complex rows of sgx_stft_batch_complex, (L, R) as 16 bytes per bin, stored inside the split (stft4096_wg.hip)
constexpr int kPixRowsC64 = 7;
//   // kPixGeneric: interpolator at run time, LUT seed + walk (SGX_FLAG_LUT_WALK / proof failed)

// (The repeats are written by the ONE thread that holds bin 1 / bin 2047, in the one unrolled step where it does -- a test of the
// bin index in every step of every thread kept sixteen compares' worth of values alive and spilled 14 registers.)

template <bool COSINE>
__device__ __forceinline__ float2 interp_sample2(const float2 *P, int i0, float w)
{
    float2 v;
    if (COSINE) {
        // :79-86  data[low] * (1 - o') + data[high] * o',  high = min(low + 1, M - 1)
        const float w1 = 1.0f - w;
        lds_cfloat2 *q = lds_ptr(P + i0);
        const float2 a = lds_read_alone(q, 1), b = lds_read_alone(q, 2);
        v.x = a.x * w1 + b.x * w;
        v.y = a.y * w1 + b.y * w;
    } else {
        // :89-105
        const float mu = w, mu2 = mu * mu, mu3 = mu * mu2;
        lds_cfloat2 *q = lds_ptr(P + i0);
        // both components at once: the same operations in the same order on (x, y) pairs -- v_pk_add_f32 / v_pk_mul_f32 round each half
        // as the scalar instructions do (no contraction: -ffp-contract=off), and the taps arrive from LDS as register pairs.  (The cosine
        // taps, the row sums and the two mono powers packed the same way cost more than they saved: not taken)
        asm("" : "+v"(q)); const lds_f2v y0 = q[0];
        asm("" : "+v"(q)); const lds_f2v y1 = q[1];
        asm("" : "+v"(q)); const lds_f2v y2 = q[2];
        asm("" : "+v"(q)); const lds_f2v y3 = q[3];
        const lds_f2v a0 = ((y3 - y2) - y0) + y1;
        const lds_f2v a1 = (y0 - y1) - a0;
        const lds_f2v a2 = y2 - y0;
        const lds_f2v r = ((a0 * mu3) + (a1 * mu2)) + ((a2 * mu) + y1);
        v.x = r.x; v.y = r.y;
    }
    return v;
}

template <bool COSINE>
__device__ __forceinline__ void sample_pass_for(const Params &p, const float2 *P, float2 *vbuf, int tid)
{
    // the table word of the next step is requested before this step's gathers: one L1 latency per step is
    // overlapped instead of exposed (two registers; deeper unrolling costs more registers than these kernels have)
    // (the table through a buffer descriptor: a uniform base + a 32-bit lane offset, no per-lane 64-bit pointer to keep)
    const __amdgpu_buffer_rsrc_t rt = pcm_rsrc(reinterpret_cast<const float *>(p.samples));
    auto item = [&](uint32_t i) {
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rt, (int)((i < p.n_samples ? i : 0u) * 8u), 0, 0);
        return PackedSample{(int32_t)v.x, __uint_as_float(v.y)};
    };
    // the nine steps unrolled (kMaxFusedSamples / 256 rounded up), a thread's table words requested kAhead steps ahead: their L1 / L2
    // latencies overlap each other instead of following one another (all nine at once: 18 registers, 52 bytes of scratch; it beat
    // three ahead and the one-step-ahead loop of rounds 1-4 on both interpolators)
    constexpr int kSteps = (kMaxFusedSamples + 255) / 256, kAhead = 9;
    PackedSample se[kSteps];
    asm volatile("" : "+v"(tid));   // (opaque: the unrolled steps' table offsets and slot addresses are not to be hoisted out of the transform loop -- they spill)
#pragma unroll
    for (int k = 0; k < kAhead && k < kSteps; ++k) se[k] = item(tid + 256 * k);
#pragma unroll
    for (int k = 0; k < kSteps; ++k) {
        if (k + kAhead < kSteps) se[k + kAhead] = item(tid + 256 * (k + kAhead));
        const uint32_t s = tid + 256 * k;
        if (s < p.n_samples) vbuf[s] = interp_sample2<COSINE>(P, se[k].i0, se[k].w);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// The same pass with the table words requested EARLY (stft4096_real.hip): a thread's nine words are asked for in front of
// the barrier and the column writes that precede the pass, so that their L1 / L2 latency falls on those instead of on the head of the pass
// (stamped build: the pass was 22 % of config 3's iteration, most of it the wait for the words it had just requested).
constexpr int kSampleSteps = (kMaxFusedSamples + 255) / 256;
constexpr int kSampleEarly = 9;   // words requested early (in front of the column writes: 17 spilled registers at the 128-register cap; behind each pair of them, as stft4096_real.hip does: none)
struct SampleWords { PackedSample se[kSampleEarly]; };
__device__ __forceinline__ PackedSample sample_word(const __amdgpu_buffer_rsrc_t &rt, const Params &p, uint32_t i)
{
    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rt, (int)((i < p.n_samples ? i : 0u) * 8u), 0, 0);
    return PackedSample{(int32_t)v.x, __uint_as_float(v.y)};
}
__device__ __forceinline__ void sample_request(const Params &p, int tid, SampleWords &w)
{
    const __amdgpu_buffer_rsrc_t rt = pcm_rsrc(reinterpret_cast<const float *>(p.samples));
    asm volatile("" : "+v"(tid));   // (opaque: see sample_pass_for)
#pragma unroll
    for (int k = 0; k < kSampleEarly; ++k) w.se[k] = sample_word(rt, p, tid + 256 * k);
}
template <int PIX>
__device__ __forceinline__ void sample_pass_with(const Params &p, const float2 *P, float2 *vbuf, int tid, const SampleWords &w)
{
    const __amdgpu_buffer_rsrc_t rt = pcm_rsrc(reinterpret_cast<const float *>(p.samples));
    asm volatile("" : "+v"(tid));
    PackedSample se[kSampleSteps];
#pragma unroll
    for (int k = 0; k < kSampleSteps; ++k) se[k] = k < kSampleEarly ? w.se[k] : sample_word(rt, p, tid + 256 * k);   // the rest: now, all at once
#pragma unroll
    for (int k = 0; k < kSampleSteps; ++k) {
        const uint32_t s = tid + 256 * k;
        if (s < p.n_samples) {
            if (pix_cosine(PIX) || (PIX == kPixGeneric && p.interp == SGX_INTERP_COSINE)) vbuf[s] = interp_sample2<true>(P, se[k].i0, se[k].w);
            else vbuf[s] = interp_sample2<false>(P, se[k].i0, se[k].w);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int PIX>
__device__ __forceinline__ void sample_pass(const Params &p, const float2 *P, float2 *vbuf, int tid)
{
    if (pix_cosine(PIX) || (PIX == kPixGeneric && p.interp == SGX_INTERP_COSINE)) sample_pass_for<true>(p, P, vbuf, tid);
    else sample_pass_for<false>(p, P, vbuf, tid);
}

// colorscheme.rs:59-61 as a threshold count: the LUT index is the number of thresholds the power has reached, the
// thresholds being the exact switch points of the host's float32 evaluation (sgx_tables.cpp).  v_log_f32 only SEEDS the
// count.  pal[i] = {the smallest power whose index is i + 1 (NaN for i = 255: no power leaves the last index), RGBA of i}.
//   seed_pm1 (the usual case; the only code of kPixCubic / kPixCosine): the host has checked, threshold by threshold, that the
//     exact value u the seed approximates lies within half an index of the count at every switch point (seed_within_one), so
//     floor(u - 1/2) is the count or one below it: ONE 16-byte LDS access brings that entry's threshold and both candidate
//     colours, one compare picks.  No loop, no second (dependent) LDS access for the colour.  (A NaN power: the seed is 0 and
//     the compare fails -> index 0, as the walk below gives.)
//   otherwise (unreachable levels, SGX_FLAG_LUT_WALK; kPixGeneric): walk from the seed, as the first version of this kernel did.
template <int PIX>
__device__ __forceinline__ uint32_t pixel_from_power(const Params &p, float power, const uint2 *pal)
{
    const float u = fmaf(__builtin_amdgcn_logf(power + 1e-7f), p.guess_a, p.guess_b);
    if (PIX != kPixGeneric || p.seed_pm1) {
        int idx = (int)floorf(u - 0.5f);
        idx = idx < 0 ? 0 : (idx > 254 ? 254 : idx);
        const uint2 e0 = pal[idx], e1 = pal[idx + 1];
        return power >= __uint_as_float(e0.x) ? e1.y : e0.y;      // RGBA, alpha = 1.0 -> 255
    }
    int idx = (int)floorf(u);
    idx = idx < 0 ? 0 : (idx > 255 ? 255 : idx);
    while (idx < 255 && power >= __uint_as_float(pal[idx].x)) ++idx;
    while (idx > 0 && !(power >= __uint_as_float(pal[idx - 1].x))) --idx;
    return pal[idx].y;
}

template <int PIX>
__device__ __forceinline__ uint32_t pixel_for(const Params &p, float l, float r, const uint2 *pal)
{
    return pixel_from_power<PIX>(p, (l * l) + (r * r), pal);      // colorscheme.rs:59
}

bool seed_within_one(const std::vector<float> &lut_thr, double guess_a, double guess_b);

// MONO: .x / .y of a sample are the two columns (frames) of the transform, each a (s, s) pixel; else one (l, r) pixel.
// A thread renders the same four rows tid + 256 i of every column: the loop over i is unrolled, the rows' table words are registers
// by name.  p.single_rows bit i: EVERY row of block i (rows 256 i .. 256 i + 255) is one sample -- 743 of the 1024 rows at 48 kHz,
// blocks 0 and 1 whole -- and the block runs without the sample loop, the count test and the divide.
// (Tried, same-device A/B: the thread's sample-table words and row words requested before the two barriers and the
// loops unrolled (9 samples, 4 rows side by side, thresholds read four at a time): 182 -> 131 M frames/s -- these
// kernels sit at the 128-VGPR cap of four waves per SIMD and every extra live value becomes scratch traffic.)
template <bool MONO, int PIX>
__device__ __forceinline__ void row_pass(const Params &p, const uint32_t (&row_words)[4], const float2 *vbuf, uchar4 *dst_a, uchar4 *dst_b,
                                         bool have_a, bool have_b, const uint2 *pal, int tid)
{
    uint32_t *out_a = reinterpret_cast<uint32_t *>(dst_a), *out_b = reinterpret_cast<uint32_t *>(dst_b);
#pragma unroll 1
    for (int i_row = 0; i_row < 4; ++i_row) {
        const uint32_t py = tid + 256 * i_row;
        if (py >= p.R) break;
        const uint32_t re = i_row == 0 ? row_words[0] : i_row == 1 ? row_words[1] : i_row == 2 ? row_words[2] : row_words[3];
        const uint32_t first = re & 0xffffu, cnt = re >> 16;
        float l, r;
        if (p.single_rows & (1u << i_row)) {          // (launch-uniform)
            const float2 v = vbuf[first];
            l = v.x;                                   // (0 + x and x / 1.0 are x -- but for the sign of a zero, and only l * l + r * r is used)
            r = v.y;
        } else {
            float sl = 0.0f, sr = 0.0f;
            for (uint32_t i = 0; i < cnt; ++i) {
                const float2 v = vbuf[first + i];
                sl = sl + v.x;
                sr = sr + v.y;
            }
            l = sl;
            r = sr;
            if (cnt > 1) {  // x / 1.0 == x: only rows that average several samples divide (:72)
                const float nf = (float)cnt;
                l = sl / nf;
                r = sr / nf;
            }
        }
        const uint32_t y = p.R - 1 - py;  // simple_spectrogram.rs:150
        if (MONO) {  // mono -> (s, s): both channels carry the same magnitude
            if (have_a) out_a[y] = pixel_for<PIX>(p, l, l, pal);
            if (have_b) out_b[y] = pixel_for<PIX>(p, r, r, pal);
        } else {
            out_a[y] = pixel_for<PIX>(p, l, r, pal);
        }
        // one row at a time: without this fence the scheduler interleaves the four unrolled rows, and the kernels -- at the 128-VGPR cap
        // of four waves per SIMD -- spill 15 to 34 registers
        asm volatile("" ::: "memory");
    }
}

// The row pass of the bands instantiations: FrequencySample::magnitude_in (interpolated_frequency_sample.rs:60-75) as magnitude_in_kernel
// (sgx_kernels.hip) computes it -- the sum from zero in lin_space order, then the divide (x / 1.0 is x) -- stored as one float2 per row at
// dst[py], py = 0 the LOWEST row: a wave's 64 consecutive rows are one contiguous 512-byte run.  MONO: .x / .y are the two frames of the
// transform, each stored as (s, s); else (l, r).
template <bool MONO>
__device__ __forceinline__ void row_pass_bands(const Params &p, const uint32_t (&row_words)[4], const float2 *vbuf, float2 *dst_a, float2 *dst_b,
                                               bool have_a, bool have_b, int tid)
{
#pragma unroll 1
    for (int i_row = 0; i_row < 4; ++i_row) {
        const uint32_t py = tid + 256 * i_row;
        if (py >= p.R) break;
        const uint32_t re = i_row == 0 ? row_words[0] : i_row == 1 ? row_words[1] : i_row == 2 ? row_words[2] : row_words[3];
        const uint32_t first = re & 0xffffu, cnt = re >> 16;
        float l, r;
        if (p.single_rows & (1u << i_row)) {          // (launch-uniform) one sample: 0 + x (the sign of a zero as the sum gives it), / 1.0 = x
            const float2 v = vbuf[first];
            l = 0.0f + v.x;
            r = 0.0f + v.y;
        } else {
            float sl = 0.0f, sr = 0.0f;
            for (uint32_t i = 0; i < cnt; ++i) {
                const float2 v = vbuf[first + i];
                sl = sl + v.x;
                sr = sr + v.y;
            }
            l = sl;
            r = sr;
            if (cnt > 1) {
                const float nf = (float)cnt;
                l = sl / nf;
                r = sr / nf;
            }
        }
        if (MONO) {
            if (have_a) dst_a[py] = make_float2(l, l);
            if (have_b) dst_b[py] = make_float2(r, r);
        } else {
            dst_a[py] = make_float2(l, r);
        }
        asm volatile("" ::: "memory");   // one row at a time (see row_pass)
    }
}

// Peak-hold columns (sgx_bands_peak_batch).  A workgroup's frames are the contiguous run [run0, run1) of the call's frames; frame f
// belongs to column f / peak_group.  A column that lies inside the run is accumulated in place in the output; one that leaves the run
// at its front or at its back is accumulated in this workgroup's slot 0 or 1 of p.peak_partial, and peak_combine_kernel takes the
// maximum over the workgroups it spans.  Either way the column is written by this workgroup alone, a row always by the same thread:
// the first frame stores, every later one loads, takes the maximum and stores -- program order of one thread, no atomics.  (The
// running column does not fit in LDS beside the transform at four workgroups per CU -- 4 x (kLdsBytes + 8 KB) > 160 KB -- nor in
// registers across the transform; it lives in L2: 8 KB per workgroup.)
struct PeakDst {
    float2 *col;   // the (pair's) column this frame accumulates into
    bool first;    // no frame of this run has been stored there yet
    unsigned long long end;   // the column's frames end here
};
// (workgroup-uniform: scalar code.  The column of a frame by division -- a 64-bit one is a hundred scalar instructions in every wave
// and every transform, so the 32-bit one wherever frame and group fit; a state carried across the frames instead costs these kernels,
// at the 128-VGPR cap, a spilled register)
__device__ __forceinline__ PeakDst peak_dst(const Params &p, unsigned long long f)
{
    const unsigned long long run0 = (unsigned long long)blockIdx.x * p.peak_run;
    unsigned long long run1 = run0 + p.peak_run;
    if (run1 > p.n_frames) run1 = p.n_frames;
    const unsigned long long j = ((f | p.peak_group) >> 32) == 0 ? (unsigned long long)((uint32_t)f / (uint32_t)p.peak_group) : f / p.peak_group;
    const unsigned long long c0 = j * p.peak_group;
    unsigned long long c1 = c0 + p.peak_group;
    if (c1 > p.n_frames) c1 = p.n_frames;
    PeakDst d;
    if (c0 >= run0 && c1 <= run1) d.col = reinterpret_cast<float2 *>(p.rgba) + (j * p.pairs + p.pair) * (size_t)p.R;
    else d.col = p.peak_partial + ((size_t)blockIdx.x * 2 + (c0 >= run0 ? 1 : 0)) * (size_t)p.R;
    d.first = f == (c0 > run0 ? c0 : run0);
    d.end = c1;
    return d;
}
// the frame behind the one `a` was found for: in the same column where that goes on (no second division), else found on its own
__device__ __forceinline__ PeakDst peak_dst_next(const Params &p, const PeakDst &a, unsigned long long f)
{
    if (f >= a.end) return peak_dst(p, f);
    PeakDst d = a;
    d.first = false;
    return d;
}

// What column `d` holds in this thread's four rows, requested in front of the barrier that precedes the row pass: four L2 round trips
// side by side under the barrier instead of one after the other inside the pass.  MONO: a row holds (m, m), one word is enough.
template <bool MONO>
struct PeakOld {   // (named words, not arrays: the row pass picks one by a run-time row number, and an indexed array is a stack object)
    float x0, x1, x2, x3, y0, y1, y2, y3;   // y: (l, r) streams only
};
template <bool MONO>
__device__ __forceinline__ void peak_prefetch_row(const Params &p, const PeakDst &d, uint32_t py, float &x, float &y)
{
    x = y = 0.0f;
    if (!d.first && py < p.R) {   // (d.first: workgroup-uniform)
        if (MONO) {
            x = reinterpret_cast<const float *>(d.col + py)[0];
        } else {
            const float2 v = d.col[py];
            x = v.x;
            y = v.y;
        }
    }
}
template <bool MONO>
__device__ __forceinline__ PeakOld<MONO> peak_prefetch(const Params &p, const PeakDst &d, int tid)
{
    PeakOld<MONO> o;
    asm volatile("" : "+v"(tid));   // (opaque: the four row addresses are not to be hoisted out of the transform loop -- they spill)
    peak_prefetch_row<MONO>(p, d, tid, o.x0, o.y0);
    peak_prefetch_row<MONO>(p, d, tid + 256, o.x1, o.y1);
    peak_prefetch_row<MONO>(p, d, tid + 512, o.x2, o.y2);
    peak_prefetch_row<MONO>(p, d, tid + 768, o.x3, o.y3);
    return o;
}

__device__ __forceinline__ void peak_update(float2 *col, uint32_t py, bool first, float l, float r)
{
    if (!first) {   // (workgroup-uniform)
        const float2 old = col[py];
        l = l > old.x ? l : old.x;
        r = r > old.y ? r : old.y;
    }
    col[py] = make_float2(l, r);
}

// row_pass_bands with the peak-hold store; `old`: peak_prefetch of column a.  MONO: .x / .y are frames a and b of the transform;
// where both accumulate into the same column their maximum is taken in registers and the column is updated once, else b's column
// (another one: a run's columns follow each other) is read here.
template <bool MONO>
__device__ __forceinline__ void row_pass_peak(const Params &p, const uint32_t (&row_words)[4], const float2 *vbuf, PeakDst a, PeakDst b,
                                              const PeakOld<MONO> &old, bool have_b, int tid)
{
    const bool same = MONO && have_b && a.col == b.col;
    // (the prefetched words move down one row per trip: picked by the row number they became an indexed stack object)
    float ox = old.x0, ox1 = old.x1, ox2 = old.x2, ox3 = old.x3;
    [[maybe_unused]] float oy = old.y0, oy1 = old.y1, oy2 = old.y2, oy3 = old.y3;
#pragma unroll 1
    for (int i_row = 0; i_row < 4; ++i_row) {
        const uint32_t py = tid + 256 * i_row;
        if (py >= p.R) break;
        const uint32_t re = i_row == 0 ? row_words[0] : i_row == 1 ? row_words[1] : i_row == 2 ? row_words[2] : row_words[3];
        const uint32_t first = re & 0xffffu, cnt = re >> 16;
        float l, r;
        if (p.single_rows & (1u << i_row)) {          // (launch-uniform) one sample: 0 + x (the sign of a zero as the sum gives it), / 1.0 = x
            const float2 v = vbuf[first];
            l = 0.0f + v.x;
            r = 0.0f + v.y;
        } else {
            float sl = 0.0f, sr = 0.0f;
            for (uint32_t i = 0; i < cnt; ++i) {
                const float2 v = vbuf[first + i];
                sl = sl + v.x;
                sr = sr + v.y;
            }
            l = sl;
            r = sr;
            if (cnt > 1) {
                const float nf = (float)cnt;
                l = sl / nf;
                r = sr / nf;
            }
        }
        if constexpr (MONO) {
            float m = same && r > l ? r : l;          // frame a, or both frames
            if (!a.first) m = m > ox ? m : ox;
            a.col[py] = make_float2(m, m);
            if (have_b && !same) peak_update(b.col, py, b.first, r, r);
        } else {
            if (!a.first) {
                l = l > ox ? l : ox;
                r = r > oy ? r : oy;
            }
            a.col[py] = make_float2(l, r);
            oy = oy1; oy1 = oy2; oy2 = oy3;
        }
        ox = ox1; ox1 = ox2; ox2 = ox3;
        asm volatile("" ::: "memory");   // one row at a time (see row_pass)
    }
}

// the same row as IEEE half pairs (round to nearest even): bin k at byte 4 k of rowm4
template <bool DUP>
__device__ __forceinline__ void store_row_f16(char *mags, long long row_byte, int col, const float (&va)[8], const float (&vb)[8], bool present = true)
{
    const __amdgpu_buffer_rsrc_t r = row_rsrc(mags, row_byte, present);
    const int lane_off = col * 4;
    const int lane_off0 = col != 0 ? lane_off : (int)0x80000000;   // k = 0 (DC): dropped by the range check (see store_row)
#pragma unroll
    for (int q3 = 0; q3 < 8; ++q3) {
        const __half2 h = __floats2half2_rn(va[q3], DUP ? va[q3] : vb[q3]);
        __builtin_amdgcn_raw_buffer_store_b32(*reinterpret_cast<const uint32_t *>(&h), r, (q3 == 0 ? lane_off0 : lane_off) + 1024 * (q3 & 3), 4096 * (q3 >> 2), 0);
    }
}

}  // namespace wg
}  // namespace sgx
