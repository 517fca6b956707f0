// sgx_internal.hpp -- context layout and kernel launchers shared by the C-ABI translation units.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <array>
#include <memory>
#include <string>
#include <vector>

#include "../../include/sgx.h"
#include "device_buffer.hpp"
#include "unit_root.hpp"

namespace sgx {

// interpolated_frequency_sample.rs:89-105 on an (l, r) / (frame A, frame B) pair: both components in packed f32 instructions --
// v_pk_add_f32 / v_pk_mul_f32 round each half as the scalar instructions do (the library is built with -ffp-contract=off), so the bits
// are those of the two scalar evaluations; on the fused mono path 4-5 % of config 3's cubic leg (profiles/r05_pixel_lds.txt)
#ifdef __HIPCC__
typedef float sgx_f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float2 cubic_pair(float2 y0, float2 y1, float2 y2, float2 y3, float mu, float mu2, float mu3)
{
    const sgx_f2v Y0 = {y0.x, y0.y}, Y1 = {y1.x, y1.y}, Y2 = {y2.x, y2.y}, Y3 = {y3.x, y3.y};
    const sgx_f2v a0 = ((Y3 - Y2) - Y0) + Y1;
    const sgx_f2v a1 = (Y0 - Y1) - a0;
    const sgx_f2v a2 = Y2 - Y0;
    const sgx_f2v r = ((a0 * mu3) + (a1 * mu2)) + ((a2 * mu) + Y1);
    return make_float2(r.x, r.y);
}
#endif

// The grid over the balance t = l / (|l| + |r|) that shortens the search for its colour segment: a monotone cell number,
// the same IEEE double operations on the host (table) and on the device (lookup).
constexpr int kTCells = 512;
__host__ __device__ inline int sgx_t_cell(double t)
{
    const double x = (t + 1.0) * (double)(kTCells / 2);
    return x >= (double)kTCells ? kTCells - 1 : (x > 0.0 ? (int)x : 0);
}

// One row of the pixel column (py = 0 is the LOWEST frequency; it is written at image row R-1-py).
struct RowEntry {
    uint32_t first;  // index of the row's first entry in the sample table
    uint32_t count;  // n = max(1, floor(i1 - i0))           interpolated_frequency_sample.rs:63-64
    float count_f;   // n as f32, the divisor of the mean     :72
    uint32_t pad;
};

// One sample of magnitude_in's lin_space.  Everything that depends only on the configuration is
// evaluated once on the host with the reference's f32 operation order; the kernel is left with
// gathers and exactly-rounded adds / multiplies.
//   cubic  (:89-105): i0 = x1 (floor(index)), w = {mu, mu^2, mu^3}
//   cosine (:79-86) : i0 = low, i1 = high,    w = {1 - o', o'}
struct SampleEntry {
    int32_t i0;
    union { int32_t i1; float w0; };
    float w1;
    float w2;
};
static_assert(sizeof(SampleEntry) == 16, "SampleEntry must be 16 bytes");

struct Tables {
    std::vector<float> window;      // [W]      fft.rs:61
    std::vector<float2> twiddle;    // [P]      e^{-2 pi i j / P}, the full circle
    std::vector<float> edges;       // [R+1]    log_scaling.rs:114-119
    std::vector<RowEntry> rows;     // [R]
    std::vector<SampleEntry> samples;
};

struct Palette {
    std::vector<uint8_t> rgb;       // [n][3]
    uint32_t n = 0;
    int stereo = 0;
    std::vector<float> lut_thr;     // [n-1]   smallest power whose LUT index is >= i+1 (mono)
    std::vector<float> alpha_thr;   // [255]   smallest power whose alpha byte is >= i+1 (stereo)
    // continuous gradient given as a callback (sgx_set_gradient_fn): rgb[] then holds one colour per
    // constant SEGMENT of the colour function instead of one per uniform LUT step
    bool segments = false;
    sgx_gradient_fn fn = nullptr;
    void *fn_user = nullptr;
    std::vector<double> t_thr;      // stereo + segments: smallest t (as double) at which segment i+1 starts
    std::vector<uint16_t> t_cell;   // [kTCells + 1]: t_cell[c] = how many switch points fall in cells below c of the grid over t in [-1, 1] (sgx_t_cell)
    uint8_t nan_rgb[3] = {0, 0, 0}; // colour of t = NaN (l = r = 0 in the diverging branch)
};

void build_tables(uint32_t W, uint32_t R, uint32_t sample_rate_u32, double f_min, double f_max, uint32_t interp,
                  Tables &out);
void build_range_tables(uint32_t W, uint32_t sample_rate_u32, uint32_t interp, const float *range_f0, const float *range_f1,
                        uint32_t n_ranges, std::vector<RowEntry> &rows, std::vector<SampleEntry> &samples);
void build_palette_thresholds(float min_db, float max_db, uint32_t lut_mode, Palette &pal);
void build_palette_segments(float min_db, float max_db, Palette &pal);
int lut_index_host(double t, uint32_t n, uint32_t mode);
uint8_t alpha_u8_host(float alpha);
float bounded_db_host(float min_db, float max_db, float power);

// sgx_info.stft_kernel (ABI: the numbers stay): generic radix-4 ladder, tuned 4096 workgroup-per-transform, Bluestein / chirp-z (2W with a
// prime factor above 7), mixed radix (2W = 2^a 3^b 5^c 7^d), tuned 4800 (W = 2400; more than two channels run the mixed-radix kernels),
// tuned 16384 (32 x 32 x 16: stft16384_w.hip), multi-pass (stft_large.hip).  Retired numbers: docs/history/stft_kernel_numbers.md
enum StftKernel : int { kKernelGeneric = 0, kKernelWg4096 = 2, kKernelChirp = 4, kKernelMixed = 6, kKernelW4800 = 9, kKernelW16384 = 10, kKernelLarge = 11 };

// The table structs of the transform families, each defined in its family's translation unit (or the header its units share).  The
// context owns one of each that it runs; `delete t` is defined where the type is complete.
namespace wg { struct WgTables; }
namespace wgr { struct RealTables; }
namespace mix { struct MixTables; struct ChirpTables; }
namespace w48 { struct W48Tables; }
namespace blu { struct BluTables; }
namespace w16k { struct TablesW; }
namespace large { struct LargeTables; }
namespace istft { struct ITables; }
struct TablesDelete {
    void operator()(wg::WgTables *t) const;       // stft4096_wg.hip
    void operator()(wgr::RealTables *t) const;    // stft4096_real.hip
    void operator()(mix::MixTables *t) const;     // stft_mixed.hip
    void operator()(mix::ChirpTables *t) const;   // stft_mixed.hip
    void operator()(w48::W48Tables *t) const;     // stft4800_wg.hip
    void operator()(blu::BluTables *t) const;     // stft_bluestein.hip
    void operator()(w16k::TablesW *t) const;      // stft16384_w.hip
    void operator()(large::LargeTables *t) const; // stft_large.hip
    void operator()(istft::ITables *t) const;     // stft_istft.hip
};
template <typename T> using TablesPtr = std::unique_ptr<T, TablesDelete>;

// unit_root (unit_root.hpp) as the float2 the twiddle tables hold
inline float2 unit_root2(unsigned long long e, unsigned long long n) { const UnitRoot w = unit_root(e, n); return make_float2(w.re, w.im); }

}  // namespace sgx

struct sgx_ctx {
    sgx_config cfg{};
    uint32_t W = 0, P = 0, M = 0, H = 0, C = 0, pairs = 0, R = 0, sr_u32 = 0, logP = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t rebind_event = nullptr;   // sgx_set_stream: recorded on the stream the context leaves, waited for by the one it moves to (made by the first rebinding)
    sgx::StftKernel stft_kernel = sgx::kKernelGeneric;   // what sgx_create chose; sgx_info.stft_kernel reports the number

    sgx::Tables tab;
    sgx::Palette pal;

    // device tables
    sgx::DeviceBuffer<float> d_window;
    sgx::DeviceBuffer<float2> d_twiddle;
    sgx::DeviceBuffer<sgx::RowEntry> d_rows;
    sgx::DeviceBuffer<sgx::SampleEntry> d_samples;
    sgx::DeviceBuffer<float> d_lut_thr;    // [n-1]
    sgx::DeviceBuffer<float> d_alpha_thr;  // [255]
    sgx::DeviceBuffer<uchar4> d_lut_rgba;  // [n]
    sgx::DeviceBuffer<uint2> d_pal_seed;   // [256] {threshold to leave level i (NaN for 255), RGBA of level i}: 256-level palettes, mono branch (else null)
    sgx::DeviceBuffer<double> d_t_thr;     // [n-1], segment palettes with a diverging scheme only
    sgx::DeviceBuffer<uint16_t> d_t_cell;  // [kTCells + 1] (or null)
    // Each family's tables and scratch, or null where the context does not run the family.  The context's constness does not reach through
    // these pointers: a family's scratch is working storage, which a launch on a `const sgx_ctx *` may regrow (DeviceBuffer::grow).
    sgx::TablesPtr<sgx::wg::WgTables> wg;         // the workgroup-per-transform 4096-point kernel
    sgx::TablesPtr<sgx::blu::BluTables> blu;      // the Bluestein (non-power-of-two) kernel
    sgx::TablesPtr<sgx::mix::MixTables> mix;      // the mixed-radix (2, 3, 5, 7-smooth lengths) kernel
    sgx::TablesPtr<sgx::w48::W48Tables> w4800;    // the tuned 4800-point kernel (W = 2400: the application's window at 48 kHz)
    sgx::TablesPtr<sgx::wgr::RealTables> real;    // the real-input 4096-point kernel (independent mono frames at W 2048 / H 256)
    sgx::TablesPtr<sgx::mix::ChirpTables> chz;    // chirp-z through the mixed-radix kernel's stages (or null: the radix-4 ladder of stft_bluestein.hip)
    sgx::TablesPtr<sgx::w16k::TablesW> w16k;      // the 16384-point kernel, 32 x 32 x 16 (stft16384_w.hip)
    sgx::TablesPtr<sgx::large::LargeTables> large;   // plan, tables and scratch of the multi-pass transform (stft_large.hip)
    sgx::TablesPtr<sgx::istft::ITables> istft;    // the inverse STFT (stft_istft.hip): built by the first sgx_istft_batch, not by sgx_create

    // workspaces (grown on demand, kept)
    sgx::DeviceBuffer<float> d_ws_mags;   // whole frames of magnitudes (ensure_workspace)
    sgx::DeviceBuffer<float> d_one_in, d_one_out;
    sgx::DeviceBuffer<unsigned long long> d_cksum;
    // cached tables of the last sgx_magnitude_in range set
    std::vector<float> bands_key;
    sgx::DeviceBuffer<sgx::RowEntry> d_band_rows;
    sgx::DeviceBuffer<sgx::SampleEntry> d_band_samples;
    sgx::DeviceBuffer<float> d_levels;  // sgx_spectrum_levels: the bands' (l, r) means, [n_bars][2], grown on demand
    sgx::DeviceBuffer<double> d_psd_carry;   // sgx_psd_batch / sgx_csd_batch: the running float64 row [pairs][M][4] of a column that spans chunks, grown on demand

    unsigned long long palette_gen = 0;  // bumped by every palette upload (sgx_view rebuilds its palette texture on a change)

    // device limits, read once at sgx_create (not on the per-tick latency path)
    int n_cu = 256;          // the count in force: every persistent grid and job split follows it (sgx_set_cu_limit; default n_cu_device)
    int n_cu_device = 256;   // hipDeviceAttributeMultiprocessorCount
    // sgx_set_run_claim: how the rows launches of the real-input 4096-point kernel deal their jobs (run_claim.hpp).  (0, 0): the automatic rule
    uint32_t claim_sixteenths = 0, claim_chunk = 0;
    // sgx_set_run_weights: the slot weights of those launches' static runs (run_claim.hpp).  All zero: the automatic ones
    uint32_t run_weights[4] = {0, 0, 0, 0};
    size_t lds_optin = 64 * 1024;   // hipDeviceAttributeSharedMemPerBlockOptin: the largest LDS image a workgroup may ask for
    // resident workgroups per CU of a kernel instantiation at a block size and LDS image (hipOccupancyMaxActiveBlocksPerMultiprocessor, cached)
    mutable std::vector<std::pair<std::array<size_t, 3>, int>> occupancy_cache;
    // objects that hold a pointer into this context (sgx_view): sgx_destroy detaches them, their calls then fail cleanly
    std::vector<struct sgx_view *> views;
    std::vector<struct sgx_image *> images;   // sgx_image.hip: the image rings created on this context
    std::vector<struct sgx_fbank *> fbanks;   // sgx_fbank.hpp: the filterbanks created on this context

    std::string err;

    ~sgx_ctx();   // sgx_api.hip: frees every buffer above.  sgx_destroy has set the device and waited for the stream.
};

namespace sgx {

// ---- one transform call, as every family's launcher takes it --------------------------------------------------------------
// What the call writes: magnitude pairs [F][pairs][M][2] floats, the same as half pairs (4 B per bin), the complex rows of
// sgx_stft_batch_complex [F][pairs][M][2][2] floats, or the fused column: RGBA pixels [F][pairs][R][4] bytes, the rows' (l, r) means as
// float2 [F][pairs][R] (sgx_bands_batch), or those held as a maximum over groups of frames, float2 [ceil(F / group)][pairs][R]; or the
// weighted sums of a filterbank over the magnitudes, float2 [F][pairs][n_filters] (sgx_fbank_batch), or over the four products of the
// (L, R) pair, float4 [F][pairs][n_filters] (sgx_fbank_cross_batch); or the means over groups of frames of the squared magnitudes, float2
// [ceil(F / group)][pairs][M] (sgx_psd_batch), and of the four products, float4 [ceil(F / group)][pairs][M] (sgx_csd_batch).  No family
// writes the last two itself: their route is the rows into the workspace and the kernels of sgx_psd.hip over them.
enum class Out { kMags, kMagsF16, kComplex, kRgba, kBands, kPeak, kFbank, kFbankCross, kPsd, kCsd };
// `total`: frames the stream holds (mono transforms carry frame pairs and pair by global index).  channels and pairs are the CALL's, not the
// context's: sgx_process_one runs a two-channel frame (2, 1) on a context of any channel count.  peak_group (kPeak): 1 .. n.  bank (kFbank,
// kFbankCross): the filterbank whose sums the call writes.
struct StftCall {
    const float *pcm;
    uint32_t channels, pairs;
    size_t first, n, total;
    void *out;
    Out kind;
    size_t peak_group;
    const struct sgx_fbank *bank = nullptr;
};
// Each X_init builds its family's tables into the context; on an error it leaves nothing behind.  Each launcher takes its tables from the
// context, returns hipSuccess or the launch error, and hipErrorInvalidValue for an Out (or a channel count) its family has no kernel for.
hipError_t launch_generic(const sgx_ctx *c, const StftCall &call);     // sgx_kernels.hip: kMags, kComplex
hipError_t launch_wg4096(const sgx_ctx *c, const StftCall &call);      // stft4096_wg.hip (and stft4096_real.hip): every Out (kFbank, kFbankCross: where wg4096_can_fuse_fbank / _cross)
hipError_t launch_w16384(const sgx_ctx *c, const StftCall &call);      // stft16384_w.hip: kMags, kComplex
hipError_t launch_w4800(const sgx_ctx *c, const StftCall &call);       // stft4800_wg.hip: kMags, kMagsF16, kComplex of one or two channels
hipError_t launch_mixed(const sgx_ctx *c, const StftCall &call);       // stft_mixed.hip: every Out but kPeak
hipError_t launch_chirpz(const sgx_ctx *c, const StftCall &call);      // stft_mixed.hip: kMags, kComplex
hipError_t launch_bluestein(const sgx_ctx *c, const StftCall &call);   // stft_bluestein.hip: kMags, kComplex
hipError_t launch_large(const sgx_ctx *c, const StftCall &call);       // stft_large.hip: kMags, kComplex

// a mono stream whose frames share transforms two by two (SGX_FLAG_PAIRED_FRAMES; the literal (s, s) transform of SGX_FLAG_COMPLEX_MONO never pairs)
inline bool paired_mono(const sgx_ctx *c, uint32_t channels)
{
    return channels == 1 && (c->cfg.flags & SGX_FLAG_PAIRED_FRAMES) && !(c->cfg.flags & SGX_FLAG_COMPLEX_MONO);
}
// Frame pairs of the tuned kernels read the partner frame through the first frame's buffer descriptor, H * 4 bytes on as its scalar offset:
// that offset plus the window must stay inside the descriptor's 2^31 - 1 records (beyond them the loads return zero, and from H = 2^30 the
// 32-bit offset has wrapped).  A context with such a hop runs every frame as its own transform: a property of the context, not of the call.
inline bool descriptor_pairs_fit(uint32_t H, uint32_t W) { return 4ull * ((unsigned long long)H + W) <= 0x7fffffffull; }
// Persistent workgroups, `per_cu` to a CU at most, each with a contiguous run of `per` jobs (neighbouring frames share most of their samples:
// the overlap is re-read from L1 / L2, not from HBM).  runs_of: the workgroups that runs of `per` jobs need.
struct RunSplit { unsigned long long per, blocks; };
inline RunSplit runs_of(unsigned long long n_jobs, unsigned long long per) { return {per, (n_jobs + per - 1) / per}; }
inline RunSplit run_split(const sgx_ctx *c, unsigned long long n_jobs, unsigned per_cu)
{
    const unsigned long long blocks = (unsigned long long)c->n_cu * per_cu, per = (n_jobs + blocks - 1) / blocks;
    return runs_of(n_jobs, per < 1 ? 1 : per);
}
inline bool fast4096_supported(const sgx_ctx *c) { return c->W == 2048; }   // the tuned 4096-point kernels (stft4096_wg.hip)
hipError_t wg4096_init(sgx_ctx *c);
bool wg4096_can_fuse_render(const sgx_ctx *c);
bool wg4096_can_fuse_bands(const sgx_ctx *c);   // the fused column without the colour (sgx_bands_batch): no palette condition
bool wg4096_can_fuse_peak(const sgx_ctx *c);    // sgx_bands_peak_batch in one kernel (plus the combine pass)
hipError_t launch_deinterleave_pairs(const sgx_ctx *c, const float *d_pcm, float *d_planes, size_t plane_floats, size_t first_sample, size_t n_samples,
                                     uint32_t channels, uint32_t pairs);   // deinterleave.hip
bool wg4096_seed_is_within_one(const sgx_ctx *c);
void lut_seed_coefficients(const sgx_ctx *c, float &a, float &b);
namespace wg { bool seed_within_one(const std::vector<float> &thr, double guess_a, double guess_b); }   // stft4096_wg.hip: is floor(log2(p + 1e-7) a + b) within one of the threshold count for every power?   // LUT level ~ floor(log2(power + 1e-7) a + b): the seed of the threshold count
// stft16384_w.hip: W = 8192 as 32 x 32 x 16 in one 512-thread workgroup, 32 points per thread
bool w16384_supported(const sgx_ctx *c);
hipError_t w16384_init(sgx_ctx *c);
// stft4096_real.hip: independent mono frames at W 2048 / H 256 as 2048-point complex transforms of the real frame
hipError_t real4096_init(sgx_ctx *c);
bool real4096_serves(const sgx_ctx *c, const float *d_pcm, uint32_t channels);   // (launched from stft4096_wg.hip: launch_wg4096)
// W = 2400 (48 kHz x 0.05 s): persistent 320-thread workgroups, 16 x 20 x 15 (stft4800_wg.hip); rows and half rows of one or two channels -- more
// channels and the fused PCM-to-pixel path go to the composite-radix kernel, whose tables such a context carries too
bool w4800_supported(const sgx_ctx *c);
hipError_t w4800_init(sgx_ctx *c);
bool mixed_supported(uint32_t W);
hipError_t mixed_init(sgx_ctx *c);
hipError_t mixed_length_tables(uint32_t n, TablesPtr<mix::MixTables> &out);   // the stage plan and tables of an n-point transform alone, for a caller that keeps them itself (stft_istft.hip)
uint32_t mixed_fixed_plan(const sgx_ctx *c);   // the length whose compile-time plan serves this context, or 0 (run-time geometry)
bool mixed_real_serves(const sgx_ctx *c, uint32_t channels);   // real-input mode: a mono stream, every frame its own W-point transform
// chirp-z through the composite stages of the mixed-radix kernel (stft_mixed_kernels.hpp): L = 512 .. 16384, i.e. W = 86 .. 5461
bool chirpz_supported(uint32_t W);
hipError_t chirpz_init(sgx_ctx *c);
bool chirpz_real_serves(const sgx_ctx *c, uint32_t channels);   // real-input mode, as mixed_real_serves
bool mixed_can_fuse_render(const sgx_ctx *c);   // one kernel from PCM to pixels at this length, palette and row table
bool mixed_can_fuse_bands(const sgx_ctx *c);    // one kernel from PCM to the rows' (l, r) means at this length and row table
bool bluestein_supported(uint32_t W);
hipError_t bluestein_init(sgx_ctx *c);
// stft_large.hip: lengths no in-LDS kernel serves (SGX_FLAG_LARGE_TRANSFORM), W up to 2^20: four-step passes through a scratch the
// context holds (allocated here, at create time), direct for a 2-3-5-7-smooth 2W, chirp-z otherwise
bool large_supported(uint32_t W);
hipError_t large_init(sgx_ctx *c);
// stft_istft.hip: the inverse of sgx_stft_batch_complex by weighted overlap-add; route 1 = the composite stages of 2W points,
// 2 = chirp-z through a power-of-two plan, 0 = none (the lengths only kernel 11 serves)
int istft_route(const sgx_ctx *c);
hipError_t istft_init(sgx_ctx *c);
hipError_t launch_istft(const sgx_ctx *c, const float *d_spec, size_t n_frames, size_t s0, size_t s1, float *d_pcm);
hipError_t launch_to_half(const sgx_ctx *c, const float *d_in, void *d_out, size_t n_pairs);
hipError_t launch_render(const sgx_ctx *c, const float *d_mags, size_t n_columns, uint8_t *d_rgba);
hipError_t launch_magnitude_in(const sgx_ctx *c, const float *d_mags, size_t n_columns, const RowEntry *d_rows,
                               const SampleEntry *d_samples, uint32_t n_ranges, float *d_out);
// sgx_bands_peak_batch, the workspace route: output column k = the maximum of the source columns it covers (sgx_kernels.hip: PeakParams)
inline size_t peak_columns(size_t n_src, size_t group, size_t sub)
{
    const size_t spc = (group + sub - 1) / sub, full = n_src / group, rem = n_src - full * group;
    return full * spc + (rem + sub - 1) / sub;
}
hipError_t launch_bands_peak(const sgx_ctx *c, const float *d_src, size_t n_src, size_t group, size_t sub, float *d_dst, bool accumulate);
hipError_t launch_render_bands(const sgx_ctx *c, const float *d_bands, size_t n_columns, uint8_t *d_rgba);
void detach_views(sgx_ctx *c);   // sgx_view.hip: every live view of the context forgets it
void detach_images(sgx_ctx *c);   // sgx_image.hip
sgx_ctx *image_context(const struct sgx_image *im);
sgx_ctx *view_context(const struct sgx_view *v);   // sgx_view.hip: the context a view was created on (nullptr once that context is gone)
hipError_t launch_white_noise(const sgx_ctx *c, float *d_out, uint64_t first, size_t n, uint32_t channels, uint32_t seed);
hipError_t launch_checksum(const sgx_ctx *c, const uint32_t *d_words, size_t n_words, uint64_t base_word,
                           unsigned long long *d_acc);

}  // namespace sgx

#ifdef __HIPCC__
// a (left, right) magnitude pair of an output row: written once, never read by the kernel
__device__ __forceinline__ void st_stream(float2 *p, float a, float b)
{
    *p = make_float2(a, b);
}

// Diagnostic builds only (-DSGX_STAMPS=1: tools/k1_phases.py, k1r_phases.py, k16_phases.py): a kernel that keeps `st_acc[]` and `st_last` adds
// the wave cycles since the previous stamp to phase i.  A default build compiles the stamps away.
#if SGX_STAMPS
#define SGX_STAMP(i) { const unsigned long long now_ = __builtin_readcyclecounter(); st_acc[i] += now_ - st_last; st_last = now_; }
#else
#define SGX_STAMP(i)
#endif
#endif
