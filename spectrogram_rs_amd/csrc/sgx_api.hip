// sgx_api.hip -- the C ABI declared in include/sgx.h: context lifetime, table upload, dispatch.
// Host code only (kernels live in sgx_kernels.hip and stft4096.hip).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>

#include "sgx_fbank.hpp"
#include "sgx_gradients.inc"
#include "sgx_maxima.hpp"
#include "sgx_psd.hpp"
#include "sgx_quantile.hpp"
#include "sgx_rolloff.hpp"
#include "sgx_internal.hpp"

namespace {

// the shortest power-of-two window that rides the composite-radix stages (sgx_create): W 512 gains, W 256 and below lose
constexpr uint32_t kPow2MixedMin = 512;

thread_local std::string g_create_error;

const char *kVersion = "sgx 0.4 (hip gfx950)";

int fail(sgx_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg;
    else g_create_error = msg;
    return code;
}

int fail_hip(sgx_ctx *c, hipError_t e, const char *what)
{
    char buf[512];
    std::snprintf(buf, sizeof(buf), "%s: %s (%s)", what, hipGetErrorString(e), hipGetErrorName(e));
    return fail(c, SGX_ERR_HIP, buf);
}

#define SGX_HIP(ctx, call)                                          \
    do {                                                            \
        hipError_t e__ = (call);                                    \
        if (e__ != hipSuccess) return fail_hip((ctx), e__, #call);  \
    } while (0)

// Rust `f as usize` for f32: truncate, saturate, NaN -> 0
uint32_t f32_as_u32(float v)
{
    if (!(v > 0.0f)) return 0;
    if (v >= 4294967296.0f) return 0xffffffffu;
    return (uint32_t)v;
}

const unsigned char *builtin_gradient(const char *name)
{
    if (!name) return nullptr;
    if (!std::strcmp(name, "viridis")) return SGX_GRADIENT_VIRIDIS;
    if (!std::strcmp(name, "magma")) return SGX_GRADIENT_MAGMA;
    if (!std::strcmp(name, "inferno")) return SGX_GRADIENT_INFERNO;
    if (!std::strcmp(name, "plasma")) return SGX_GRADIENT_PLASMA;
    return nullptr;
}

// colorous' B-spline gradients (RED_YELLOW_BLUE ... ORANGES, colorscheme.rs:130-148).  [third-party] colorous 1.0.12 ports
// d3-scale-chromatic, whose ramp(scheme) is d3-interpolate's interpolateRgbBasis over the scheme's largest ColorBrewer
// class: a uniform cubic B-spline per channel, the end anchors reflected (v[-1] = 2 v[0] - v[1]).  The anchors are
// generated from matplotlib's copy of ColorBrewer (tools/gen_gradients.py); the rounding to bytes (nearest, clamped) is
// d3's `rgb` formatting and is as unverifiable offline as the rest of colorous: PARITY UNPINNED, and replaceable by the
// integrator's own eval_continuous through sgx_set_gradient_fn.
const sgx_brewer *brewer_gradient(const char *name)
{
    if (!name) return nullptr;
    for (const sgx_brewer &g : SGX_BREWER)
        if (!std::strcmp(name, g.name)) return &g;
    return nullptr;
}

void brewer_eval(double t, uint8_t out[3], void *user)
{
    const sgx_brewer *g = static_cast<const sgx_brewer *>(user);
    const int n = g->n - 1;
    int i;
    if (!(t > 0.0)) { t = 0.0; i = 0; }          // t <= 0 and NaN
    else if (t >= 1.0) { t = 1.0; i = n - 1; }
    else i = (int)std::floor(t * (double)n);
    const double t1 = (t - (double)i / (double)n) * (double)n, t2 = t1 * t1, t3 = t2 * t1;
    for (int ch = 0; ch < 3; ++ch) {
        const double v1 = g->rgb[i][ch], v2 = g->rgb[i + 1][ch];
        const double v0 = i > 0 ? (double)g->rgb[i - 1][ch] : 2.0 * v1 - v2;
        const double v3 = i < n - 1 ? (double)g->rgb[i + 2][ch] : 2.0 * v2 - v1;
        const double v = ((1.0 - 3.0 * t1 + 3.0 * t2 - t3) * v0 + (4.0 - 6.0 * t2 + 3.0 * t3) * v1 +
                          (1.0 + 3.0 * t1 + 3.0 * t2 - 3.0 * t3) * v2 + t3 * v3) / 6.0;
        const double r = std::floor(v + 0.5);
        out[ch] = (uint8_t)(r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r));
    }
}

// colorous' closed-form gradients (colorscheme.rs:140-143).  [third-party] colorous 1.0.12 ports d3-scale-chromatic:
//   TURBO, CIVIDIS: a quintic per channel in t clamped to [0, 1] (d3's interpolateTurbo / interpolateCividis, Horner with
//     the signs as published), bytes by rounding to nearest, clamped;
//   CUBEHELIX, COOL (and WARM): d3's interpolateCubehelixLong between two (h, s, l) triples -- h, s, l each linear in t,
//     no shortest-arc on the hue, gamma 1 -- followed by d3-color's Cubehelix -> sRGB matrix.  The default CUBEHELIX,
//     (300, 0.5, 0) -> (-240, 0.5, 1), is Green's (2011) helix with start 0.5, -1.5 rotations, hue 1, gamma 1: the curve
//     matplotlib's `cubehelix` colormap traces (checked in tests/test_host_logic.py against matplotlib._cm.cubehelix).
//     Bytes of the cubehelix family by TRUNCATION (Rust's saturating `as u8`), not d3's Math.round: the one place where
//     something the reference holds decides -- screenshots/colorscheme-cool.png shows background() = eval_continuous(0.0)
//     (colorscheme.rs:41-44) as (109, 63, 169) where the curve is (109.70, 63.81, 169.91), the axes = eval_continuous(1.0) as
//     (175, 239, 90) for (175.23, 239.78, 90.54), and 599 of the curve's 623 truncated colours verbatim against 364 of its
//     rounded ones (tests/golden/screenshot_colours.npz, tests/test_host_logic.py).
// The endpoint triples and, for Turbo / Cividis / the splines, the byte rule (round to nearest, clamp) are data of this
// file: PARITY UNPINNED (the crate is not vendored in the reference), replaceable through sgx_set_gradient_fn.
struct sgx_poly { const char *name; double r[6], g[6], b[6]; };
const sgx_poly SGX_POLY[] = {
    {"turbo", {34.61, 1172.33, -10793.56, 33300.12, -38394.49, 14825.05}, {23.31, 557.33, 1225.33, -3574.96, 1073.77, 707.56},
     {27.2, 3211.1, -15327.97, 27814.0, -22569.18, 6838.66}},
    {"cividis", {-4.54, -35.34, 2381.73, -6402.7, 7024.72, -2710.57}, {32.49, 170.73, 52.82, -131.46, 176.58, -67.37},
     {81.24, 442.36, -2482.43, 6167.24, -6614.94, 2475.67}},
};
struct sgx_helix { const char *name; double h0, s0, l0, h1, s1, l1; };
const sgx_helix SGX_HELIX[] = {
    {"cubehelix", 300.0, 0.5, 0.0, -240.0, 0.5, 1.0},
    {"cool", 260.0, 0.75, 0.35, 80.0, 1.5, 0.8},
    {"warm", -100.0, 0.75, 0.35, 80.0, 1.5, 0.8},
};

uint8_t byte_round(double v)
{
    const double r = std::floor(v + 0.5);
    if (!(r > 0.0)) return 0;   // negative and NaN
    return (uint8_t)(r > 255.0 ? 255.0 : r);
}

uint8_t byte_trunc(double v)     // Rust `as u8` on a float: toward zero, saturating, NaN -> 0
{
    if (!(v > 0.0)) return 0;
    return (uint8_t)(v >= 255.0 ? 255.0 : v);
}

void poly_eval(double t, uint8_t out[3], void *user)
{
    const sgx_poly *g = static_cast<const sgx_poly *>(user);
    t = !(t > 0.0) ? 0.0 : (t > 1.0 ? 1.0 : t);   // clamp; NaN -> 0
    const double *cs[3] = {g->r, g->g, g->b};
    for (int ch = 0; ch < 3; ++ch) {
        const double *c = cs[ch];
        double v = c[5];
        for (int k = 4; k >= 0; --k) v = c[k] + t * v;
        out[ch] = byte_round(v);
    }
}

void helix_eval(double t, uint8_t out[3], void *user)
{
    const sgx_helix *g = static_cast<const sgx_helix *>(user);
    t = !(t > 0.0) ? 0.0 : (t > 1.0 ? 1.0 : t);
    const double h = (g->h0 + t * (g->h1 - g->h0) + 120.0) * (M_PI / 180.0);
    const double s = g->s0 + t * (g->s1 - g->s0), l = g->l0 + t * (g->l1 - g->l0);
    const double a = s * l * (1.0 - l), ch = std::cos(h), sh = std::sin(h);
    out[0] = byte_trunc(255.0 * (l + a * (-0.14861 * ch + 1.78277 * sh)));
    out[1] = byte_trunc(255.0 * (l + a * (-0.29227 * ch + -0.90649 * sh)));
    out[2] = byte_trunc(255.0 * (l + a * (1.97294 * ch)));
}

// name -> (evaluator, its data) for every continuous gradient this library evaluates itself
bool continuous_gradient(const char *name, sgx_gradient_fn *fn, void **user)
{
    if (!name) return false;
    if (const sgx_brewer *b = brewer_gradient(name)) { *fn = brewer_eval; *user = const_cast<sgx_brewer *>(b); return true; }
    for (const sgx_poly &g : SGX_POLY)
        if (!std::strcmp(name, g.name)) { *fn = poly_eval; *user = const_cast<sgx_poly *>(&g); return true; }
    for (const sgx_helix &g : SGX_HELIX)
        if (!std::strcmp(name, g.name)) { *fn = helix_eval; *user = const_cast<sgx_helix *>(&g); return true; }
    return false;
}

int upload_palette(sgx_ctx *c)
{
    if (c->pal.segments) sgx::build_palette_segments(c->cfg.min_db, c->cfg.max_db, c->pal);
    else sgx::build_palette_thresholds(c->cfg.min_db, c->cfg.max_db, c->cfg.lut_index_mode, c->pal);
    std::vector<uchar4> rgba(c->pal.n);
    for (uint32_t i = 0; i < c->pal.n; ++i)
        rgba[i] = make_uchar4(c->pal.rgb[3 * i], c->pal.rgb[3 * i + 1], c->pal.rgb[3 * i + 2], 255);
    SGX_HIP(c, hipSetDevice(c->device));
    // ordering against kernels that may still read the old tables
    SGX_HIP(c, hipStreamSynchronize(c->stream));
    SGX_HIP(c, c->d_lut_rgba.upload(rgba));
    SGX_HIP(c, c->d_lut_thr.upload(c->pal.lut_thr));
    SGX_HIP(c, c->d_alpha_thr.upload(c->pal.alpha_thr));
    SGX_HIP(c, c->d_t_thr.upload(c->pal.t_thr));
    c->pal.t_cell.clear();
    if (c->pal.segments && c->pal.stereo && c->pal.t_thr.size() < 65535) {
        // t_cell[c] = switch points in cells below c: a balance in cell c has passed at least t_cell[c] of them and at most t_cell[c + 1]
        c->pal.t_cell.assign(sgx::kTCells + 1, 0);
        for (double thr : c->pal.t_thr)
            for (int cell = sgx::sgx_t_cell(thr) + 1; cell <= sgx::kTCells; ++cell) ++c->pal.t_cell[cell];
    }
    SGX_HIP(c, c->d_t_cell.upload(c->pal.t_cell));
    std::vector<uint2> seed;
    if (!c->pal.stereo && c->pal.n == 256 && c->pal.lut_thr.size() == 255) {
        seed.resize(256);
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t thr_bits = 0x7fc00000u, word = 0;   // NaN: no power leaves the last level
            if (i < 255) std::memcpy(&thr_bits, &c->pal.lut_thr[i], 4);
            std::memcpy(&word, &rgba[i], 4);
            seed[i] = make_uint2(thr_bits, word | 0xff000000u);
        }
    }
    SGX_HIP(c, c->d_pal_seed.upload(seed));   // (null where the palette has no seed table: fused_palette asks)
    ++c->palette_gen;
    return SGX_OK;
}

using sgx::Out;
using sgx::StftCall;

// ---- the host dispatch: which family serves a call, and the bounded workspace of the routes that take two kernels -------------------

enum class Family { kGeneric, kWg4096, kBluestein, kChirpz, kMixed, kW4800, kW16384, kLarge };
// `fused`: one launch of `family` writes the call's Out.  Otherwise `family` writes the rows (Out::kMags) into the workspace and a second
// kernel makes the Out of them.  real_input: the rows are the family's real-input mode (sgx_info.render_path bit 3).
struct Route { Family family; bool fused, real_input; };

// The one place that answers: on this context, a call of `channels` channels for `kind` -- which family launches, and is the Out fused?
//
// Channel counts.  The rows' family goes by the CALL's channel count: sgx_process_one passes 2 on any context, so on a W 2400 context that
// is mono (real-input mode) or has more than two channels its one (l, r) frame runs the tuned 4800-point kernel.  The fused columns go by
// the CONTEXT's channel count (wg4096_can_fuse_*, mixed_can_fuse_* read c->C: the tables they test were built for it).  Only the batch entry
// points ask for a column, and their channel count is the context's, so one `channels` serves both here; the queries (sgx_query,
// sgx_bands_fused, sgx_bands_peak_fused) pass c->C.
// `bank` (Out::kFbank, Out::kFbankCross): the filterbank of the call; its size decides with the context.
Route stft_route(const sgx_ctx *c, uint32_t channels, Out kind, const sgx_fbank *bank = nullptr)
{
    const bool mixed = c->stft_kernel == sgx::kKernelMixed || c->stft_kernel == sgx::kKernelW4800;
    // The W 2400 rows of one or two channels come from the 4800-point kernel, unless real-input mode takes the stream (a mono stream, every
    // frame its own transform: 2400 points instead of 4800 on (s, s)); more channels run the mixed-radix kernels
    const bool rows_from_w4800 = c->stft_kernel == sgx::kKernelW4800 && channels <= 2 && !sgx::mixed_real_serves(c, channels);
    Route rows{Family::kGeneric, true, false};
    switch (c->stft_kernel) {
    case sgx::kKernelW16384: rows.family = Family::kW16384; break;   // (a mono stream whose frames are not paired: as an (s, s) plane through the two-channel instantiation)
    case sgx::kKernelLarge: rows.family = Family::kLarge; break;     // lengths no in-LDS kernel serves (SGX_FLAG_LARGE_TRANSFORM)
    case sgx::kKernelW4800:
    case sgx::kKernelMixed:
        rows.family = rows_from_w4800 ? Family::kW4800 : Family::kMixed;
        rows.real_input = sgx::mixed_real_serves(c, channels);
        break;
    case sgx::kKernelChirp:
        rows.family = c->chz ? Family::kChirpz : Family::kBluestein;
        rows.real_input = sgx::chirpz_real_serves(c, channels);
        break;
    case sgx::kKernelWg4096:
        rows.family = Family::kWg4096;
        rows.real_input = !sgx::paired_mono(c, channels) && !(c->cfg.flags & SGX_FLAG_COMPLEX_MONO) && sgx::real4096_serves(c, nullptr, channels);
        break;
    case sgx::kKernelGeneric: break;
    }
    const bool may_fuse = !(c->cfg.flags & SGX_FLAG_NO_FUSED_RENDER);
    bool fused = false;
    switch (kind) {
    case Out::kMags:
    case Out::kComplex: return rows;
    case Out::kMagsF16:   // the tuned and the mixed-radix kernels store half pairs themselves; the others convert float32 rows
        fused = rows.family == Family::kWg4096 || rows.family == Family::kW4800 || rows.family == Family::kMixed;
        break;
    case Out::kRgba:      // (the pixels of a W 2400 stream come from the mixed-radix kernel whichever kernel its rows come from)
        fused = may_fuse && rows.family == Family::kWg4096 && sgx::wg4096_can_fuse_render(c);
        if (may_fuse && mixed && sgx::mixed_can_fuse_render(c)) {
            rows.family = Family::kMixed;
            fused = true;
        }
        break;
    case Out::kBands:     // Only the transform decides, not the palette: the column has no colour.  It must hold the bits of the context's rows, so
                          // a fused kernel serves only where the rows come from the same transform: not where they come from the 4800-point kernel
        fused = may_fuse && ((rows.family == Family::kWg4096 && sgx::wg4096_can_fuse_bands(c)) ||
                             (rows.family == Family::kMixed && sgx::mixed_can_fuse_bands(c)));
        break;
    case Out::kPeak:      // in one kernel where sgx_bands_batch runs the 4096-point kernels and the frames are not paired
        fused = stft_route(c, channels, Out::kBands).fused && rows.family == Family::kWg4096 && sgx::wg4096_can_fuse_peak(c);
        break;
    case Out::kFbank:     // in one kernel at W 2048 where every frame is its own transform and the bank is within the stated size
        fused = may_fuse && rows.family == Family::kWg4096 && sgx::wg4096_can_fuse_fbank(c, bank);
        break;
    case Out::kFbankCross:   // likewise, on a stream of (l, r) pairs
        fused = may_fuse && rows.family == Family::kWg4096 && sgx::wg4096_can_fuse_fbank_cross(c, bank);
        break;
    case Out::kPsd:       // the means over groups of frames: no family accumulates them itself (no fused mode has been measured
    case Out::kCsd:       // against this route: DESIGN.md), so the rows go through the workspace on every context
        fused = false;
        break;
    }
    rows.fused = fused;
    return rows;
}

hipError_t launch_family(const sgx_ctx *c, Family f, const StftCall &call)
{
    switch (f) {
    case Family::kGeneric: return sgx::launch_generic(c, call);
    case Family::kWg4096: return sgx::launch_wg4096(c, call);
    case Family::kBluestein: return sgx::launch_bluestein(c, call);
    case Family::kChirpz: return sgx::launch_chirpz(c, call);
    case Family::kMixed: return sgx::launch_mixed(c, call);
    case Family::kW4800: return sgx::launch_w4800(c, call);
    case Family::kW16384: return sgx::launch_w16384(c, call);
    case Family::kLarge: return sgx::launch_large(c, call);
    }
    return hipErrorInvalidValue;
}

// frames [first, first + n) of the context's own stream layout into `out`, by the family `r` names
hipError_t run_call(const sgx_ctx *c, const Route &r, const float *d_pcm, size_t first, size_t n, size_t total, void *out, Out kind, size_t peak_group = 0)
{
    return launch_family(c, r.family, StftCall{d_pcm, c->C, c->pairs, first, n, total, out, kind, peak_group});
}

// The bounded workspace: the routes that take two kernels keep the magnitudes of a chunk of frames in it (L2 / Infinity-Cache sized chunks,
// reused), grown on demand and kept.  ensure_workspace counts frames of magnitudes.
constexpr size_t kWorkspaceBytes = (size_t)192u << 20;
size_t mags_bytes_per_frame(const sgx_ctx *c) { return (size_t)c->pairs * c->M * 2 * sizeof(float); }

size_t workspace_chunk(size_t bytes_per_frame, size_t n)
{
    const size_t chunk = kWorkspaceBytes / bytes_per_frame;
    return chunk < 1 ? 1 : (chunk > n ? n : chunk);
}

int ensure_workspace(sgx_ctx *c, size_t frames)
{
    const hipError_t e = c->d_ws_mags.grow(c->stream, frames * (mags_bytes_per_frame(c) / sizeof(float)));
    return e == hipSuccess ? SGX_OK : fail_hip(c, e, "hipMalloc(render workspace)");
}

// n frames in chunks whose magnitudes fit the workspace: body(done, m) runs frames [done, done + m) of the call and returns an SGX code.
// rows_per_frame 2: chunks whose complex rows fit (16 B per bin: two magnitude rows' bytes, half as many frames)
template <typename Body>
int in_workspace_chunks(sgx_ctx *c, size_t n, Body body, size_t rows_per_frame = 1)
{
    const size_t chunk = workspace_chunk(mags_bytes_per_frame(c) * rows_per_frame, n);
    int rc = ensure_workspace(c, chunk * rows_per_frame);
    for (size_t done = 0; rc == SGX_OK && done < n; done += chunk) rc = body(done, n - done < chunk ? n - done : chunk);
    return rc;
}

// The rows of frames [first, first + m) into the workspace (the caller has grown it to m frames), for the second kernel of a two-kernel route
// (kind: Out::kMags, or Out::kComplex for the complex rows)
hipError_t rows_to_workspace(const sgx_ctx *c, const float *d_pcm, size_t first, size_t m, size_t total, Out kind = Out::kMags)
{
    return run_call(c, stft_route(c, c->C, kind), d_pcm, first, m, total, c->d_ws_mags.get(), kind);
}

// What sgx_bands_batch runs on frames [first, first + m): the fused kernel of its route, or the rows into the workspace (m frames fit: the
// caller's chunk) and magnitude_in over the context's own row and sample tables.
int run_bands(sgx_ctx *c, const char *who, const Route &r, const float *d_pcm, size_t first, size_t m, size_t total, float *d_bands)
{
    if (r.fused) {
        // one kernel from PCM to bands: the magnitudes stay in LDS, 8 B per row leave the kernel
        const hipError_t e = run_call(c, r, d_pcm, first, m, total, d_bands, Out::kBands);
        return e == hipSuccess ? SGX_OK : fail_hip(c, e, (std::string(who) + ": fused launch").c_str());
    }
    // two kernels, as sgx_render_batch
    hipError_t e = rows_to_workspace(c, d_pcm, first, m, total);
    if (e != hipSuccess) return fail_hip(c, e, (std::string(who) + ": stft launch").c_str());
    e = sgx::launch_magnitude_in(c, c->d_ws_mags.get(), m * c->pairs, c->d_rows.get(), c->d_samples.get(), c->R, d_bands);
    if (e != hipSuccess) return fail_hip(c, e, (std::string(who) + ": magnitude_in launch").c_str());
    return SGX_OK;
}

// The opening of the six batch calls.  SGX_OK with n == 0: nothing to do (no frames in range: None, fft.rs:72 -- answered before the buffers
// are looked at); another code: the error, recorded; else frames [first_frame, first_frame + n) of the stream's `total` are to be computed.
int begin_batch(sgx_ctx *c, const char *who, size_t n_samples, size_t first_frame, size_t max_frames, const void *d_pcm, const void *d_out,
                size_t *n_out, size_t &total, size_t &n)
{
    total = n = 0;
    if (n_out) *n_out = 0;
    if (!c) return SGX_ERR_INVALID_ARG;
    total = sgx_num_frames(c, n_samples);
    if (first_frame >= total || max_frames == 0) return SGX_OK;
    if (!d_pcm || !d_out) return fail(c, SGX_ERR_INVALID_ARG, std::string(who) + ": null buffer");
    SGX_HIP(c, hipSetDevice(c->device));
    n = total - first_frame < max_frames ? total - first_frame : max_frames;
    return SGX_OK;
}

// sgx_stft_batch and sgx_stft_batch_complex: one dispatch, so that both outputs of a context come from the same kernel family
int stft_batch(sgx_ctx *c, const char *who, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames, float *d_out, Out kind,
               size_t *n_out)
{
    size_t total, n;
    const int rc = begin_batch(c, who, n_samples, first_frame, max_frames, d_pcm, d_out, n_out, total, n);
    if (rc != SGX_OK || n == 0) return rc;
    const hipError_t e = run_call(c, stft_route(c, c->C, kind), d_pcm, first_frame, n, total, d_out, kind);
    if (e != hipSuccess) return fail_hip(c, e, (std::string(who) + ": kernel launch").c_str());
    if (n_out) *n_out = n;
    return SGX_OK;
}

// ---- Welch-averaged spectra per bin (sgx_psd.hpp): the means over columns of `group` frames of n frames' rows, into d_out ---------------
// rows(f, m) answers the device pointer to the rows of frames [f, f + m) of the call, or null with its error recorded.  own_rows: it
// writes them to the front of the workspace, at most as many frames as this function asks for at once (the batch calls); else they lie in
// the caller's buffer (the stage calls) and the workspace holds block partials only.  A row and a block's partial row are the same size
// (psd: [pairs][M][2] floats, csd: [pairs][M][4]), so the workspace's budget is counted in rows of either.
//
// The call's blocks are taken in ranges.  A range holds whole blocks, and whole columns where a column's blocks fit one range; a longer
// column is taken alone, range by range, its float64 sums carried in the context's one carry row.  A row so long that the workspace does
// not hold a block of rows beside one partial row is taken a few frames at a time, each piece continuing the block's chain where the last
// one stopped.  The bits do not depend on any of it: the order of both chains is the header's.
template <typename Rows>
int psd_reduce(sgx_ctx *c, const char *who, bool cross, size_t n, size_t group, bool own_rows, Rows rows, float *d_out)
{
    namespace psd = sgx::psd;
    const psd::Geometry geo = psd::geometry(n, group);
    const size_t rpf = cross ? 2 : 1, row_floats = mags_bytes_per_frame(c) / sizeof(float) * rpf;
    const size_t elems = (size_t)c->pairs * c->M, nc = cross ? 4 : 2;
    // (the whole workspace per range: ranges of 96, 48, 24 and 12 MiB ran at 0.82, 0.58, 0.30 and 0.19 of this rate: profiles/psd.txt)
    const size_t cap = kWorkspaceBytes / (row_floats * sizeof(float));
    const size_t fpb = geo.g < psd::kBlock ? (size_t)geo.g : (size_t)psd::kBlock;   // frames per block, at most
    const size_t all = (size_t)geo.blocks();
    size_t per = cap, piece = SIZE_MAX;   // blocks per range; frames per piece of a range
    if (own_rows) {
        if (cap >= fpb + 1) per = cap / (fpb + 1);
        else { per = 1; piece = cap > 1 ? cap - 1 : 1; }
    }
    if (per < 1) per = 1;
    if (per > all) per = all;
    const bool carried = geo.bpc > per;
    if (!carried) per -= per % (size_t)geo.bpc;
    size_t row_slots = 0;
    if (own_rows) {
        row_slots = piece != SIZE_MAX ? piece : per * fpb;
        if (row_slots > n) row_slots = n;
    }
    int rc = ensure_workspace(c, (row_slots + per) * rpf);
    if (rc != SGX_OK) return rc;
    if (carried) {
        const hipError_t e = c->d_psd_carry.grow(c->stream, elems * nc);
        if (e != hipSuccess) return fail_hip(c, e, "hipMalloc(psd carry row)");
    }
    float *partial = c->d_ws_mags.get() + row_slots * row_floats;
    for (size_t b = 0; b < all;) {
        const size_t j = b / (size_t)geo.bpc;
        size_t m = all - b < per ? all - b : per;
        if (carried && m > (size_t)geo.column_block_end(j) - b) m = (size_t)geo.column_block_end(j) - b;
        const size_t f_lo = (size_t)geo.block_first(b), f_hi = (size_t)geo.block_end(b + m - 1);
        for (size_t f = f_lo; f < f_hi;) {
            const size_t k = f_hi - f < piece ? f_hi - f : piece;
            const float *src = rows(f, k);
            if (!src) return SGX_ERR_HIP;
            const hipError_t e = psd::launch_psd_blocks(c, cross, psd::BlockPiece{src, partial, geo, elems, b, m, f, f + k, f != f_lo ? 1u : 0u});
            if (e != hipSuccess) return fail_hip(c, e, (std::string(who) + ": block launch").c_str());
            f += k;
        }
        const hipError_t e = psd::launch_psd_combine(c, cross, psd::CombinePiece{partial, d_out, c->d_psd_carry.get(), geo, elems, b, m});
        if (e != hipSuccess) return fail_hip(c, e, (std::string(who) + ": combine launch").c_str());
        b += m;
    }
    return SGX_OK;
}

// sgx_psd_batch and sgx_csd_batch: the rows (or the complex rows) of a range of frames by their own route into the workspace, then the two
// kernels of sgx_psd.hip
int psd_batch(sgx_ctx *c, const char *who, bool cross, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames, size_t group,
              float *d_out, size_t *n_out)
{
    if (n_out) *n_out = 0;
    if (c && group == 0) return fail(c, SGX_ERR_INVALID_ARG, std::string(who) + ": group is 0");
    if (c && cross && c->C < 2) return fail(c, SGX_ERR_UNSUPPORTED, std::string(who) + ": a mono context has no (l, r) pair (L = R: the means are x0, x0, x0, 0)");
    size_t total, n;
    int rc = begin_batch(c, who, n_samples, first_frame, max_frames, d_pcm, d_out, n_out, total, n);
    if (rc != SGX_OK || n == 0) return rc;
    if (cross && ((uintptr_t)d_out & 15u)) return fail(c, SGX_ERR_INVALID_ARG, std::string(who) + ": the output must be 16-byte aligned");
    const Out rows_kind = cross ? Out::kComplex : Out::kMags;
    rc = psd_reduce(c, who, cross, n, group, true, [&](size_t f, size_t m) -> const float * {
        const hipError_t e = rows_to_workspace(c, d_pcm, first_frame + f, m, total, rows_kind);
        if (e != hipSuccess) { fail_hip(c, e, (std::string(who) + ": stft launch").c_str()); return nullptr; }
        return c->d_ws_mags.get();
    }, d_out);
    if (rc != SGX_OK) return rc;
    if (n_out) *n_out = (size_t)sgx::psd::geometry(n, group).columns();
    return SGX_OK;
}

// sgx_psd_mags and sgx_csd_spec: the same two kernels over the caller's rows
int psd_stage(sgx_ctx *c, const char *who, bool cross, const float *d_rows, size_t n_frames, size_t group, float *d_out, size_t *n_out)
{
    if (n_out) *n_out = 0;
    if (!c) return SGX_ERR_INVALID_ARG;
    if (group == 0) return fail(c, SGX_ERR_INVALID_ARG, std::string(who) + ": group is 0");
    if (n_frames == 0) return SGX_OK;
    if (!d_rows || !d_out) return fail(c, SGX_ERR_INVALID_ARG, std::string(who) + ": null buffer");
    if (cross && (((uintptr_t)d_rows | (uintptr_t)d_out) & 15u)) return fail(c, SGX_ERR_INVALID_ARG, std::string(who) + ": buffers must be 16-byte aligned");
    SGX_HIP(c, hipSetDevice(c->device));
    const size_t row_floats = mags_bytes_per_frame(c) / sizeof(float) * (cross ? 2 : 1);
    const int rc = psd_reduce(c, who, cross, n_frames, group, false, [&](size_t f, size_t) { return d_rows + f * row_floats; }, d_out);
    if (rc != SGX_OK) return rc;
    if (n_out) *n_out = (size_t)sgx::psd::geometry(n_frames, group).columns();
    return SGX_OK;
}

// sgx_maxima_batch and sgx_maxima_mags: what both calls refuse before anything is enqueued
int check_maxima(sgx_ctx *c, const char *who, uint32_t k, float floor, const float *d_max)
{
    if (k < 1 || k > sgx::maxima::kMaxK) return fail(c, SGX_ERR_INVALID_ARG, std::string(who) + ": k must be 1 .. 64");
    if (!(floor >= 0.0f) || std::isinf(floor)) return fail(c, SGX_ERR_INVALID_ARG, std::string(who) + ": floor must be finite and >= 0");
    if ((uintptr_t)d_max & 15u) return fail(c, SGX_ERR_INVALID_ARG, std::string(who) + ": d_max must be 16-byte aligned");
    return SGX_OK;
}

// sgx_rolloff_batch and sgx_rolloff_mags: what both calls refuse before anything is enqueued; the shares, read from the host array
int check_rolloff(sgx_ctx *c, const char *who, uint32_t power, const float *h_p, uint32_t n_p, const float *d_out, sgx::rolloff::Shares &shares)
{
    if (power != 1 && power != 2) return fail(c, SGX_ERR_INVALID_ARG, std::string(who) + ": power must be 1 or 2");
    if (n_p < 1 || n_p > sgx::rolloff::kMaxShares) return fail(c, SGX_ERR_INVALID_ARG, std::string(who) + ": n_p must be 1 .. 8");
    if (!h_p) return fail(c, SGX_ERR_INVALID_ARG, std::string(who) + ": h_p is null");
    shares = sgx::rolloff::Shares{};
    for (uint32_t i = 0; i < n_p; ++i) {
        if (!(h_p[i] > 0.0f && h_p[i] <= 1.0f)) return fail(c, SGX_ERR_INVALID_ARG, std::string(who) + ": every p must lie in (0, 1]");
        shares.p[i] = h_p[i];
    }
    if ((uintptr_t)d_out & 15u) return fail(c, SGX_ERR_INVALID_ARG, std::string(who) + ": d_out must be 16-byte aligned");
    return SGX_OK;
}

// sgx_quantile_batch and sgx_quantile_mags: what both calls refuse before anything is enqueued
int check_quantile(sgx_ctx *c, const char *who, size_t group, const double *q, uint32_t n_q)
{
    if (group == 0) return fail(c, SGX_ERR_INVALID_ARG, std::string(who) + ": group is 0");
    if (n_q < 1 || n_q > sgx::quantile::kMaxQ) return fail(c, SGX_ERR_INVALID_ARG, std::string(who) + ": n_q must be 1 .. 16");
    if (!q) return fail(c, SGX_ERR_INVALID_ARG, std::string(who) + ": q is null");
    for (uint32_t i = 0; i < n_q; ++i)
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) return fail(c, SGX_ERR_INVALID_ARG, std::string(who) + ": every q must lie in [0, 1]");
    return SGX_OK;
}

// the frames of rows the workspace holds, at least 1: the longest column sgx_quantile_batch selects
size_t quantile_cap(const sgx_ctx *c)
{
    const size_t cap = kWorkspaceBytes / mags_bytes_per_frame(c);
    return cap < 1 ? 1 : cap;
}

}  // namespace

// Every table, workspace and family struct is a member that frees itself: nothing is listed here.  (Out of line so that a translation unit
// that only reads the context's layout needs neither the runtime nor the families' deleters.)
sgx_ctx::~sgx_ctx() = default;

extern "C" {

const char *sgx_version(void) { return kVersion; }

int sgx_config_init(sgx_config *cfg)
{
    if (!cfg) return SGX_ERR_INVALID_ARG;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = sizeof(sgx_config);
    cfg->sample_rate = 48000.0f;
    cfg->period = 0.0f;
    cfg->stride = 0.0f;
    cfg->window_samples = 2048;  // fourier/mod.rs:7
    cfg->hop_samples = 256;      // BASELINE config A
    cfg->channels = 1;
    cfg->rows = 1024;            // simple_spectrogram.rs:34-35
    cfg->f_min = 32.0;           // simple_spectrogram.rs:107
    cfg->f_max = 22030.0;
    cfg->min_db = -70.0f;        // colorscheme.rs:16-17
    cfg->max_db = -10.0f;
    cfg->interp = SGX_INTERP_CUBIC;
    cfg->lut_index_mode = SGX_LUT_FLOOR_N;
    cfg->device = -1;
    cfg->flags = 0;
    return SGX_OK;
}

int sgx_create(const sgx_config *cfg, sgx_ctx **out_ctx)
{
    if (out_ctx) *out_ctx = nullptr;
    if (!cfg || !out_ctx) return fail(nullptr, SGX_ERR_INVALID_ARG, "sgx_create: null argument");
    if (cfg->struct_size != sizeof(sgx_config))
        return fail(nullptr, SGX_ERR_INVALID_ARG, "sgx_create: struct_size mismatch (call sgx_config_init first)");

    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0)
        return fail(nullptr, SGX_ERR_NO_DEVICE,
                    std::string("sgx_create: no HIP device (this library has no CPU fallback): ") +
                        (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));

    sgx_ctx *c = new (std::nothrow) sgx_ctx();
    if (!c) return fail(nullptr, SGX_ERR_NOMEM, "sgx_create: out of host memory");
    c->cfg = *cfg;
    // Mono streams (include/sgx.h): every frame its own transform unless SGX_FLAG_PAIRED_FRAMES asks for frame pairs; the literal
    // (s, s) transform of SGX_FLAG_COMPLEX_MONO implies no pairing.  (Bit 16, the SGX_FLAG_INDEPENDENT_FRAMES of rounds 1-5 -- "never
    // pair", the default since round 4 -- is accepted and means nothing.)
    c->cfg.flags &= ~16u;
    if (c->cfg.flags & SGX_FLAG_COMPLEX_MONO) c->cfg.flags &= ~SGX_FLAG_PAIRED_FRAMES;

    // fft.rs:19 / audio_transform.rs:35: f32 product, truncating cast
    c->W = cfg->window_samples ? cfg->window_samples : f32_as_u32(cfg->period * cfg->sample_rate);
    c->H = cfg->hop_samples ? cfg->hop_samples : f32_as_u32(cfg->stride * cfg->sample_rate);
    c->P = 2 * c->W;
    c->M = c->W - 1;
    c->C = cfg->channels;
    c->pairs = c->C <= 2 ? 1 : c->C / 2;
    c->R = cfg->rows;
    c->sr_u32 = f32_as_u32(cfg->sample_rate);  // SampleRate(sample_rate as u32), simple_spectrogram.rs:138

    auto bail = [&](int code, const std::string &msg) {
        sgx_destroy(c);
        return fail(nullptr, code, msg);
    };
    if (c->W < 4) return bail(SGX_ERR_INVALID_ARG, "sgx_create: window must be at least 4 samples");
    if (c->H < 1) return bail(SGX_ERR_INVALID_ARG, "sgx_create: hop must be at least 1 sample");
    if (c->C < 1 || (c->C > 2 && (c->C & 1))) return bail(SGX_ERR_INVALID_ARG, "sgx_create: channels must be 1, 2 or an even number");
    if (c->R < 1 || c->R > 65536) return bail(SGX_ERR_INVALID_ARG, "sgx_create: rows out of range");
    if (!(cfg->f_min > 0.0) || !(cfg->f_max > cfg->f_min)) return bail(SGX_ERR_INVALID_ARG, "sgx_create: need 0 < f_min < f_max");
    if (!(cfg->max_db > cfg->min_db)) return bail(SGX_ERR_INVALID_ARG, "sgx_create: need min_db < max_db");
    if (cfg->interp > SGX_INTERP_COSINE) return bail(SGX_ERR_INVALID_ARG, "sgx_create: unknown interpolation");
    if (cfg->lut_index_mode > SGX_LUT_ROUND_NM1) return bail(SGX_ERR_INVALID_ARG, "sgx_create: unknown lut_index_mode");
    if (c->sr_u32 == 0) return bail(SGX_ERR_INVALID_ARG, "sgx_create: sample_rate must be at least 1 Hz");
    const bool pow2 = (c->P & (c->P - 1)) == 0 && c->P <= 16384;
    const bool in_lds = pow2 || sgx::bluestein_supported(c->W) || sgx::mixed_supported(c->W);
    const bool large = !in_lds && (cfg->flags & SGX_FLAG_LARGE_TRANSFORM) && sgx::large_supported(c->W);
    if (!in_lds && !large)
        return bail(SGX_ERR_UNSUPPORTED,
                    "sgx_create: transform length 2W = " + std::to_string(c->P) +
                        " is not supported by this build (up to 20480 with prime factors 2, 3, 5, 7 only, or any 2W with 3W - 1 <= 16384" +
                        (sgx::large_supported(c->W) ? std::string("; SGX_FLAG_LARGE_TRANSFORM serves it as a multi-pass transform)")
                                                    : std::string(")")));
    c->logP = 0;
    while ((1u << c->logP) < c->P) ++c->logP;

    c->device = cfg->device;
    if (c->device < 0) {
        e = hipGetDevice(&c->device);
        if (e != hipSuccess) return bail(SGX_ERR_HIP, std::string("hipGetDevice: ") + hipGetErrorString(e));
    }
    if (c->device >= n_dev) return bail(SGX_ERR_INVALID_ARG, "sgx_create: device ordinal out of range");
    e = hipSetDevice(c->device);
    if (e != hipSuccess) return bail(SGX_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    {   // device limits the launchers need: read once, here
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, c->device) == hipSuccess && v > 0) c->n_cu = c->n_cu_device = v;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeSharedMemPerBlockOptin, c->device) == hipSuccess && v > 0) c->lds_optin = (size_t)v;
        else if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device) == hipSuccess && v > 0) c->lds_optin = (size_t)v;
    }

    sgx::build_tables(c->W, c->R, c->sr_u32, cfg->f_min, cfg->f_max, cfg->interp, c->tab);
    if ((e = c->d_window.upload(c->tab.window)) != hipSuccess ||
        (e = c->d_twiddle.upload(c->tab.twiddle)) != hipSuccess ||
        (e = c->d_rows.upload(c->tab.rows)) != hipSuccess ||
        (e = c->d_samples.upload(c->tab.samples)) != hipSuccess ||
        (e = c->d_one_in.alloc((size_t)c->W * 2)) != hipSuccess ||
        (e = c->d_one_out.alloc((size_t)c->M * 2)) != hipSuccess ||
        (e = c->d_cksum.alloc(1)) != hipSuccess)
        return bail(SGX_ERR_HIP, std::string("sgx_create: table upload: ") + hipGetErrorString(e));

    // default palette: ColorScheme::new_mono(colorous::MAGMA, "magma"), simple_spectrogram.rs:95
    c->pal.rgb.assign(SGX_GRADIENT_MAGMA, SGX_GRADIENT_MAGMA + 256 * 3);
    c->pal.n = 256;
    c->pal.stereo = 0;
    int rc = upload_palette(c);
    if (rc != SGX_OK) { std::string m = c->err; return bail(rc, m); }

    c->stft_kernel = sgx::kKernelGeneric;
    if (cfg->flags & (2u | 8u | 32u | 128u | 2048u))   // the flag bits of superseded A/B kernels: wave-per-transform, packed arithmetic, the first three 16384-point designs
        return bail(SGX_ERR_UNSUPPORTED, "sgx_create: flag bits 2, 8, 32 (removed in round 5), 128 and 2048 (SGX_FLAG_RESIDUE_16K, SGX_FLAG_CHANNEL_PLANES: removed in "
                                         "round 6) selected superseded A/B kernels (their measurements: profiles/r01_*, r02_*, r03_k16_ablation.txt, r05_k16.txt, r06_k16.txt)");
    if (c->C > 32768u) return bail(SGX_ERR_INVALID_ARG, "sgx_create: at most 32768 channels (the kernels address a sample row with 32-bit byte offsets)");
    // powers of two from W = 512 on that have no tuned kernel ride the composite-radix stages too (compile-time plans 4 x 16 x 16,
    // 8 x 16 x 16, 4 x 8 x 16 x 16): same-device A/B against the radix-4 ladder of the generic kernel, mono / stereo:
    // W 512 +29 % / +44 %, W 1024 +48 % / +90 %, W 4096 +83 % / +117 %; W 256: -14 %, W 128: -53 % (run-time geometry)
    const bool pow2_mixed = pow2 && c->W >= kPow2MixedMin && c->W != 2048 && c->W != 8192 && sgx::mixed_supported(c->W) && !(cfg->flags & SGX_FLAG_FORCE_GENERIC);
    if (large) {
        // no in-LDS kernel serves this length (SGX_FLAG_LARGE_TRANSFORM): four-step passes through a scratch allocated here
        e = sgx::large_init(c);
        if (e != hipSuccess) return bail(SGX_ERR_HIP, std::string("sgx_create: multi-pass transform tables and scratch: ") + hipGetErrorString(e));
        c->stft_kernel = sgx::kKernelLarge;
    } else if (pow2_mixed || (!pow2 && sgx::mixed_supported(c->W) && !((cfg->flags & SGX_FLAG_FORCE_GENERIC) && sgx::bluestein_supported(c->W)))) {
        // a length FFTW would factor: mixed-radix transform of exactly 2W points (SGX_FLAG_FORCE_GENERIC: chirp-z instead)
        e = sgx::mixed_init(c);
        if (e != hipSuccess) return bail(SGX_ERR_HIP, std::string("sgx_create: mixed-radix tables: ") + hipGetErrorString(e));
        c->stft_kernel = sgx::kKernelMixed;
        if (!(cfg->flags & (SGX_FLAG_FORCE_GENERIC | SGX_FLAG_MIXED_GENERIC)) && sgx::w4800_supported(c)) {
            e = sgx::w4800_init(c);
            if (e != hipSuccess) return bail(SGX_ERR_HIP, std::string("sgx_create: 4800-point kernel tables: ") + hipGetErrorString(e));
            c->stft_kernel = sgx::kKernelW4800;
        }
    } else if (!pow2) {
        e = sgx::bluestein_init(c);
        if (e != hipSuccess) return bail(SGX_ERR_HIP, std::string("sgx_create: Bluestein tables: ") + hipGetErrorString(e));
        if (!(cfg->flags & SGX_FLAG_FORCE_GENERIC) && sgx::chirpz_supported(c->W)) {   // (SGX_FLAG_FORCE_GENERIC: the radix-4 ladder, the A/B reference)
            e = sgx::chirpz_init(c);
            if (e != hipSuccess) return bail(SGX_ERR_HIP, std::string("sgx_create: chirp-z tables: ") + hipGetErrorString(e));
        }
        c->stft_kernel = sgx::kKernelChirp;
    } else if (!(cfg->flags & SGX_FLAG_FORCE_GENERIC) && sgx::fast4096_supported(c)) {
        e = sgx::wg4096_init(c);
        if (e != hipSuccess) return bail(SGX_ERR_HIP, std::string("sgx_create: tuned kernel tables: ") + hipGetErrorString(e));
        if (c->C == 1) {
            e = sgx::real4096_init(c);
            if (e != hipSuccess) return bail(SGX_ERR_HIP, std::string("sgx_create: real-input kernel tables: ") + hipGetErrorString(e));
        }
        c->stft_kernel = sgx::kKernelWg4096;
    } else if (!(cfg->flags & SGX_FLAG_FORCE_GENERIC) && sgx::w16384_supported(c)) {
        e = sgx::w16384_init(c);
        if (e != hipSuccess) return bail(SGX_ERR_HIP, std::string("sgx_create: 16384-point kernel tables: ") + hipGetErrorString(e));
        c->stft_kernel = sgx::kKernelW16384;
    }
    *out_ctx = c;
    return SGX_OK;
}

// The order holds the rule of device_buffer.hpp: the context's device current, its stream drained, and only then anything freed.
void sgx_destroy(sgx_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    sgx::detach_views(c);
    sgx::detach_fbanks(c);
    sgx::detach_images(c);   // views that outlive their context keep their own buffers and answer SGX_ERR_INVALID_ARG from now on
    if (c->rebind_event) (void)hipEventDestroy(c->rebind_event);
    delete c;
}

const char *sgx_last_error(const sgx_ctx *c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int sgx_query(const sgx_ctx *c, sgx_info *out)
{
    if (!c || !out) return SGX_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof(*out));
    out->struct_size = sizeof(sgx_info);
    out->window_samples = c->W;
    out->fft_length = c->P;
    out->num_frequencies = c->M;
    out->hop_samples = c->H;
    out->channels = c->C;
    out->pairs = c->pairs;
    out->rows = c->R;
    out->sample_rate_u32 = c->sr_u32;
    out->total_samples_per_column = (uint32_t)c->tab.samples.size();
    out->stft_kernel = (uint32_t)c->stft_kernel;
    // render_path from the routes the calls themselves take: bit 0 the fused pixels (bit 1: their LUT search needs no walk), bit 2 a compile-time
    // plan of the composite-radix stages, bit 3 real-input rows
    const Route rows = stft_route(c, c->C, Out::kMags), pixels = stft_route(c, c->C, Out::kRgba);
    out->render_path = 0;
    if (pixels.fused) out->render_path = pixels.family == Family::kMixed ? 3u : 1u | (sgx::wg4096_seed_is_within_one(c) ? 2u : 0u);
    if (rows.family == Family::kChirpz || ((rows.family == Family::kMixed || rows.family == Family::kW4800) && sgx::mixed_fixed_plan(c))) out->render_path |= 4u;
    if (rows.real_input) out->render_path |= 8u;
    out->mags_bytes_per_frame = mags_bytes_per_frame(c);
    out->rgba_bytes_per_frame = (uint64_t)c->pairs * c->R * 4;
    return SGX_OK;
}

size_t sgx_num_frames(const sgx_ctx *c, size_t n_samples)
{
    if (!c || n_samples < c->W) return 0;
    return (n_samples - c->W) / c->H + 1;
}

int sgx_set_stream(sgx_ctx *c, void *stream)
{
    if (!c) return SGX_ERR_INVALID_ARG;
    const hipStream_t next = reinterpret_cast<hipStream_t>(stream);
    if (next == c->stream) return SGX_OK;   // (a wrapper that binds before every call: nothing to do, no runtime call)
    // The context's buffers (workspace, planes, scratch, peak partials, tables) may still be in use by what it enqueued on the stream it
    // leaves: the new stream's work is ordered behind that, on the device -- the host does not wait
    SGX_HIP(c, hipSetDevice(c->device));
    if (!c->rebind_event) SGX_HIP(c, hipEventCreateWithFlags(&c->rebind_event, hipEventDisableTiming));
    SGX_HIP(c, hipEventRecord(c->rebind_event, c->stream));
    SGX_HIP(c, hipStreamWaitEvent(next, c->rebind_event, 0));
    c->stream = next;
    return SGX_OK;
}

int sgx_set_cu_limit(sgx_ctx *c, uint32_t n)
{
    if (!c) return SGX_ERR_INVALID_ARG;
    if (n > (uint32_t)c->n_cu_device) {
        c->err = "sgx_set_cu_limit: more compute units than the device has";
        return SGX_ERR_INVALID_ARG;
    }
    // Only grids and job splits read the count.  The one buffer sized by it, the 4096-point kernels' peak partials, is checked by DeviceBuffer::grow at
    // every launch: a limit raised again regrows it.
    c->n_cu = n ? (int)n : c->n_cu_device;
    return SGX_OK;
}

uint32_t sgx_cu_limit(const sgx_ctx *c) { return c ? (uint32_t)c->n_cu : 0u; }

int sgx_sync(sgx_ctx *c)
{
    if (!c) return SGX_ERR_INVALID_ARG;
    SGX_HIP(c, hipSetDevice(c->device));
    SGX_HIP(c, hipStreamSynchronize(c->stream));
    return SGX_OK;
}

int sgx_stft_batch(sgx_ctx *c, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames,
                   float *d_mags, size_t *n_out)
{
    return stft_batch(c, "sgx_stft_batch", d_pcm, n_samples, first_frame, max_frames, d_mags, Out::kMags, n_out);
}

int sgx_stft_batch_complex(sgx_ctx *c, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames,
                           float *d_spec, size_t *n_out)
{
    return stft_batch(c, "sgx_stft_batch_complex", d_pcm, n_samples, first_frame, max_frames, d_spec, Out::kComplex, n_out);
}

int sgx_istft_supported(const sgx_ctx *c)
{
    if (!c) return SGX_ERR_INVALID_ARG;
    return sgx::istft_route(c) ? 1 : 0;
}

int sgx_istft_batch(sgx_ctx *c, const float *d_spec, size_t n_frames, size_t first_sample, size_t max_samples, float *d_pcm,
                    size_t *n_out)
{
    if (n_out) *n_out = 0;
    if (!c) return SGX_ERR_INVALID_ARG;
    if (!sgx::istft_route(c))
        return fail(c, SGX_ERR_UNSUPPORTED, "sgx_istft_batch: no inverse for transform length 2W = " + std::to_string(c->P) +
                                                " (the multi-pass lengths of SGX_FLAG_LARGE_TRANSFORM are not served)");
    if (n_frames == 0 || max_samples == 0) return SGX_OK;
    if (n_frames - 1 > (SIZE_MAX - c->W) / c->H) return fail(c, SGX_ERR_INVALID_ARG, "sgx_istft_batch: n_frames out of range");
    const size_t total = (n_frames - 1) * (size_t)c->H + c->W;   // samples n < (n_frames - 1) H + W exist
    if (first_sample >= total) return SGX_OK;
    size_t n = total - first_sample;
    if (n > max_samples) n = max_samples;
    if (!d_spec || !d_pcm) return fail(c, SGX_ERR_INVALID_ARG, "sgx_istft_batch: null buffer");
    SGX_HIP(c, hipSetDevice(c->device));
    hipError_t e;
    if (!c->istft && (e = sgx::istft_init(c)) != hipSuccess) return fail_hip(c, e, "sgx_istft_batch: tables");
    e = sgx::launch_istft(c, d_spec, n_frames, first_sample, first_sample + n, d_pcm);
    if (e != hipSuccess) return fail_hip(c, e, "sgx_istft_batch: kernel launch");
    if (n_out) *n_out = n;
    return SGX_OK;
}

int sgx_stft_batch_f16(sgx_ctx *c, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames,
                       void *d_mags_f16, size_t *n_out)
{
    size_t total, n;
    int rc = begin_batch(c, "sgx_stft_batch_f16", n_samples, first_frame, max_frames, d_pcm, d_mags_f16, n_out, total, n);
    if (rc != SGX_OK || n == 0) return rc;
    const Route r = stft_route(c, c->C, Out::kMagsF16);
    if (r.fused) {
        // half pairs straight from the kernel's split (no float32 round trip)
        const hipError_t e = run_call(c, r, d_pcm, first_frame, n, total, d_mags_f16, Out::kMagsF16);
        if (e != hipSuccess) return fail_hip(c, e, "sgx_stft_batch_f16: kernel launch");
    } else {
        // kernels without a native half store: float32 into the bounded workspace, then one conversion pass
        const size_t per_frame = (size_t)c->pairs * c->M;  // (l, r) pairs per frame
        rc = in_workspace_chunks(c, n, [&](size_t done, size_t m) {
            hipError_t e = rows_to_workspace(c, d_pcm, first_frame + done, m, total);
            if (e == hipSuccess)
                e = sgx::launch_to_half(c, c->d_ws_mags.get(), static_cast<char *>(d_mags_f16) + done * per_frame * 4, m * per_frame);
            return e == hipSuccess ? (int)SGX_OK : fail_hip(c, e, "sgx_stft_batch_f16: kernel launch");
        });
        if (rc != SGX_OK) return rc;
    }
    if (n_out) *n_out = n;
    return SGX_OK;
}

int sgx_process_one(sgx_ctx *c, const float *h_lr, size_t n_avail, float *h_out)
{
    if (!c) return SGX_ERR_INVALID_ARG;
    if (n_avail < c->W) return 0;  // None (fft.rs:72)
    if (!h_lr || !h_out) return fail(c, SGX_ERR_INVALID_ARG, "sgx_process_one: null buffer");
    SGX_HIP(c, hipSetDevice(c->device));
    SGX_HIP(c, hipMemcpyAsync(c->d_one_in.get(), h_lr, (size_t)c->W * 2 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    // one (l, r) frame whatever the context's channel count: the family goes by the call's two channels (stft_route)
    hipError_t e = launch_family(c, stft_route(c, 2, Out::kMags).family, StftCall{c->d_one_in.get(), 2, 1, 0, 1, 1, c->d_one_out.get(), Out::kMags, 0});
    if (e != hipSuccess) return fail_hip(c, e, "sgx_process_one: kernel launch");
    SGX_HIP(c, hipMemcpyAsync(h_out, c->d_one_out.get(), (size_t)c->M * 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SGX_HIP(c, hipStreamSynchronize(c->stream));
    return 1;
}

int sgx_render_mags(sgx_ctx *c, const float *d_mags, size_t n_columns, uint8_t *d_rgba)
{
    if (!c) return SGX_ERR_INVALID_ARG;
    if (n_columns == 0) return SGX_OK;
    if (!d_mags || !d_rgba) return fail(c, SGX_ERR_INVALID_ARG, "sgx_render_mags: null buffer");
    SGX_HIP(c, hipSetDevice(c->device));
    hipError_t e = sgx::launch_render(c, d_mags, n_columns, d_rgba);
    if (e != hipSuccess) return fail_hip(c, e, "sgx_render_mags: kernel launch");
    return SGX_OK;
}

int sgx_render_batch(sgx_ctx *c, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames,
                     uint8_t *d_rgba, size_t *n_out)
{
    size_t total, n;
    int rc = begin_batch(c, "sgx_render_batch", n_samples, first_frame, max_frames, d_pcm, d_rgba, n_out, total, n);
    if (rc != SGX_OK || n == 0) return rc;
    const Route r = stft_route(c, c->C, Out::kRgba);
    if (r.fused) {
        // one kernel from PCM to pixels: the magnitudes never leave LDS (the 4096-point kernels: 5 120 B of HBM traffic per frame; the
        // application's own window lengths: the pixel stage runs on the mixed-radix transform's LDS image)
        const hipError_t e = run_call(c, r, d_pcm, first_frame, n, total, d_rgba, Out::kRgba);
        if (e != hipSuccess) return fail_hip(c, e, "sgx_render_batch: fused launch");
    } else {
        // two kernels; magnitudes stay in the bounded, reused workspace
        rc = in_workspace_chunks(c, n, [&](size_t done, size_t m) {
            hipError_t e = rows_to_workspace(c, d_pcm, first_frame + done, m, total);
            if (e != hipSuccess) return fail_hip(c, e, "sgx_render_batch: stft launch");
            e = sgx::launch_render(c, c->d_ws_mags.get(), m * c->pairs, d_rgba + done * (size_t)c->pairs * c->R * 4);
            return e == hipSuccess ? (int)SGX_OK : fail_hip(c, e, "sgx_render_batch: render launch");
        });
        if (rc != SGX_OK) return rc;
    }
    if (n_out) *n_out = n;
    return SGX_OK;
}

int sgx_bands_batch(sgx_ctx *c, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames, float *d_bands, size_t *n_out)
{
    size_t total, n;
    int rc = begin_batch(c, "sgx_bands_batch", n_samples, first_frame, max_frames, d_pcm, d_bands, n_out, total, n);
    if (rc != SGX_OK || n == 0) return rc;
    const Route r = stft_route(c, c->C, Out::kBands);
    if (r.fused) rc = run_bands(c, "sgx_bands_batch", r, d_pcm, first_frame, n, total, d_bands);
    else   // two kernels: the magnitudes of a chunk of frames in the bounded workspace
        rc = in_workspace_chunks(c, n, [&](size_t done, size_t m) {
            return run_bands(c, "sgx_bands_batch", r, d_pcm, first_frame + done, m, total, d_bands + done * (size_t)c->pairs * c->R * 2);
        });
    if (rc != SGX_OK) return rc;
    if (n_out) *n_out = n;
    return SGX_OK;
}

// ---- filterbanks: weighted sums of bin magnitudes or powers over sparse filters (sgx_fbank.hpp) ----------------------------------------

int sgx_mel_weights(double sample_rate, uint32_t window_samples, uint32_t n_mels, double f_min, double f_max, uint32_t scale, uint32_t norm,
                    uint32_t *h_first, uint32_t *h_count, float *h_weights, size_t *n_weights)
{
    return sgx::fbank::mel_weights(sample_rate, window_samples, n_mels, f_min, f_max, scale, norm, h_first, h_count, h_weights, n_weights);
}

int sgx_fbank_create(sgx_ctx *c, uint32_t n_filters, const uint32_t *h_first, const uint32_t *h_count, const float *h_weights, uint32_t power,
                     void **out)
{
    if (out) *out = nullptr;
    if (!c) return SGX_ERR_INVALID_ARG;
    if (!out) return fail(c, SGX_ERR_INVALID_ARG, "sgx_fbank_create: null argument");
    std::vector<sgx::fbank::Filter> table;
    size_t n_weights = 0;
    const char *why = "";
    if (sgx::fbank::validate(c->M, n_filters, h_first, h_count, h_weights, power, &table, &n_weights, &why) != SGX_OK)
        return fail(c, SGX_ERR_INVALID_ARG, std::string("sgx_fbank_create: ") + why);
    sgx_fbank *fb = new (std::nothrow) sgx_fbank();
    if (!fb) return fail(c, SGX_ERR_NOMEM, "sgx_fbank_create: out of host memory");
    fb->ctx = c;
    fb->n_filters = n_filters;
    fb->power = power;
    fb->n_weights = n_weights;
    // The uploads go onto the context's stream, from copies the bank keeps: the calls that read the tables follow on the same stream, and
    // nothing is waited for.
    fb->h_filters = std::move(table);
    fb->h_weights.assign(h_weights, h_weights + n_weights);
    if (fb->h_weights.empty()) fb->h_weights.push_back(0.0f);
    hipError_t e = hipSetDevice(c->device);
    const size_t table_bytes = fb->h_filters.size() * sizeof(fb->h_filters[0]), weight_bytes = fb->h_weights.size() * sizeof(float);
    if (e == hipSuccess) e = fb->d_filters.alloc(fb->h_filters.size());
    if (e == hipSuccess) e = fb->d_weights.alloc(fb->h_weights.size());
    if (e == hipSuccess) e = hipMemcpyAsync(fb->d_filters.get(), fb->h_filters.data(), table_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(fb->d_weights.get(), fb->h_weights.data(), weight_bytes, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) {
        delete fb;
        return fail_hip(c, e, "sgx_fbank_create: table upload");
    }
    c->fbanks.push_back(fb);
    *out = fb;
    return SGX_OK;
}

void sgx_fbank_destroy(void *bank)
{
    sgx_fbank *fb = static_cast<sgx_fbank *>(bank);
    if (!fb) return;
    if (sgx_ctx *c = fb->ctx) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);   // a call that reads the tables may still be in flight
        for (size_t i = 0; i < c->fbanks.size(); ++i)
            if (c->fbanks[i] == fb) { c->fbanks.erase(c->fbanks.begin() + (long)i); break; }
    }
    delete fb;
}

uint32_t sgx_fbank_filters(const void *bank) { return bank ? static_cast<const sgx_fbank *>(bank)->n_filters : 0u; }

int sgx_fbank_fused(const void *bank)
{
    const sgx_fbank *fb = static_cast<const sgx_fbank *>(bank);
    if (!fb || !fb->ctx) return SGX_ERR_INVALID_ARG;
    return stft_route(fb->ctx, fb->ctx->C, Out::kFbank, fb).fused ? 1 : 0;
}

int sgx_fbank_mags(void *bank, const float *d_mags, size_t n_columns, float *d_out)
{
    sgx_fbank *fb = static_cast<sgx_fbank *>(bank);
    if (!fb || !fb->ctx) return SGX_ERR_INVALID_ARG;
    sgx_ctx *c = fb->ctx;
    if (n_columns == 0) return SGX_OK;
    if (!d_mags || !d_out) return fail(c, SGX_ERR_INVALID_ARG, "sgx_fbank_mags: null buffer");
    SGX_HIP(c, hipSetDevice(c->device));
    const hipError_t e = sgx::launch_fbank_stage(c, fb, d_mags, n_columns, d_out);
    if (e != hipSuccess) return fail_hip(c, e, "sgx_fbank_mags: kernel launch");
    return SGX_OK;
}

int sgx_fbank_batch(void *bank, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames, float *d_out, size_t *n_out)
{
    sgx_fbank *fb = static_cast<sgx_fbank *>(bank);
    if (n_out) *n_out = 0;
    if (!fb || !fb->ctx) return SGX_ERR_INVALID_ARG;
    sgx_ctx *c = fb->ctx;
    size_t total, n;
    int rc = begin_batch(c, "sgx_fbank_batch", n_samples, first_frame, max_frames, d_pcm, d_out, n_out, total, n);
    if (rc != SGX_OK || n == 0) return rc;
    const Route r = stft_route(c, c->C, Out::kFbank, fb);
    if (r.fused) {
        // one kernel from PCM to the bank's sums: the magnitudes stay in LDS, 8 B per filter leave the kernel
        const hipError_t e = launch_family(c, r.family, StftCall{d_pcm, c->C, c->pairs, first_frame, n, total, d_out, Out::kFbank, 0, fb});
        if (e != hipSuccess) return fail_hip(c, e, "sgx_fbank_batch: fused launch");
    } else {
        // two kernels: the rows of a chunk of frames in the bounded workspace, by the rows' own route, then the stage kernel over them
        rc = in_workspace_chunks(c, n, [&](size_t done, size_t m) {
            hipError_t e = rows_to_workspace(c, d_pcm, first_frame + done, m, total);
            if (e != hipSuccess) return fail_hip(c, e, "sgx_fbank_batch: stft launch");
            e = sgx::launch_fbank_stage(c, fb, c->d_ws_mags.get(), m * c->pairs, d_out + done * (size_t)c->pairs * fb->n_filters * 2);
            return e == hipSuccess ? (int)SGX_OK : fail_hip(c, e, "sgx_fbank_batch: filter launch");
        });
        if (rc != SGX_OK) return rc;
    }
    if (n_out) *n_out = n;
    return SGX_OK;
}

// ---- the cross sums of a bank: |L|^2, |R|^2, Re and Im of L conj R per band (sgx_fbank.hpp: cross_filter_pass) ---------------------------

int sgx_fbank_cross_fused(const void *bank)
{
    const sgx_fbank *fb = static_cast<const sgx_fbank *>(bank);
    if (!fb || !fb->ctx) return SGX_ERR_INVALID_ARG;
    return stft_route(fb->ctx, fb->ctx->C, Out::kFbankCross, fb).fused ? 1 : 0;
}

int sgx_fbank_cross_spec(void *bank, const float *d_spec, size_t n_columns, float *d_out)
{
    sgx_fbank *fb = static_cast<sgx_fbank *>(bank);
    if (!fb || !fb->ctx) return SGX_ERR_INVALID_ARG;
    sgx_ctx *c = fb->ctx;
    if (n_columns == 0) return SGX_OK;
    if (!d_spec || !d_out) return fail(c, SGX_ERR_INVALID_ARG, "sgx_fbank_cross_spec: null buffer");
    if (((uintptr_t)d_spec | (uintptr_t)d_out) & 15u) return fail(c, SGX_ERR_INVALID_ARG, "sgx_fbank_cross_spec: buffers must be 16-byte aligned");
    SGX_HIP(c, hipSetDevice(c->device));
    const hipError_t e = sgx::launch_fbank_cross_stage(c, fb, d_spec, n_columns, d_out);
    if (e != hipSuccess) return fail_hip(c, e, "sgx_fbank_cross_spec: kernel launch");
    return SGX_OK;
}

int sgx_fbank_cross_batch(void *bank, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames, float *d_out, size_t *n_out)
{
    sgx_fbank *fb = static_cast<sgx_fbank *>(bank);
    if (n_out) *n_out = 0;
    if (!fb || !fb->ctx) return SGX_ERR_INVALID_ARG;
    sgx_ctx *c = fb->ctx;
    if (c->C < 2) return fail(c, SGX_ERR_UNSUPPORTED, "sgx_fbank_cross_batch: a mono context has no (l, r) pair (L = R: the sums are x0, x0, x0, 0)");
    size_t total, n;
    int rc = begin_batch(c, "sgx_fbank_cross_batch", n_samples, first_frame, max_frames, d_pcm, d_out, n_out, total, n);
    if (rc != SGX_OK || n == 0) return rc;
    if ((uintptr_t)d_out & 15u) return fail(c, SGX_ERR_INVALID_ARG, "sgx_fbank_cross_batch: d_out must be 16-byte aligned");
    const Route r = stft_route(c, c->C, Out::kFbankCross, fb);
    if (r.fused) {
        // one kernel from PCM to the four sums: L and R stay in registers, their products in LDS, 16 B per filter leave the kernel
        const hipError_t e = launch_family(c, r.family, StftCall{d_pcm, c->C, c->pairs, first_frame, n, total, d_out, Out::kFbankCross, 0, fb});
        if (e != hipSuccess) return fail_hip(c, e, "sgx_fbank_cross_batch: fused launch");
    } else {
        // two kernels: the complex rows of a chunk of frames in the bounded workspace, by the rows' own route, then the cross stage over them
        rc = in_workspace_chunks(c, n, [&](size_t done, size_t m) {
            hipError_t e = rows_to_workspace(c, d_pcm, first_frame + done, m, total, Out::kComplex);
            if (e != hipSuccess) return fail_hip(c, e, "sgx_fbank_cross_batch: stft launch");
            e = sgx::launch_fbank_cross_stage(c, fb, c->d_ws_mags.get(), m * c->pairs, d_out + done * (size_t)c->pairs * fb->n_filters * 4);
            return e == hipSuccess ? (int)SGX_OK : fail_hip(c, e, "sgx_fbank_cross_batch: filter launch");
        }, 2);
        if (rc != SGX_OK) return rc;
    }
    if (n_out) *n_out = n;
    return SGX_OK;
}

// ---- the flux of a bank: per band the sums of every bin's rise and fall against the same bin `lag` frames earlier (sgx_fbank.hpp) -------
static_assert(sgx::flux::kWorkspaceBytes == kWorkspaceBytes, "flux_host.hpp counts rows of the one workspace");

uint32_t sgx_flux_max_lag(const void *bank)
{
    const sgx_fbank *fb = static_cast<const sgx_fbank *>(bank);
    return fb && fb->ctx ? sgx::flux::max_lag(mags_bytes_per_frame(fb->ctx)) : 0u;
}

int sgx_flux_mags(void *bank, const float *d_mags, size_t n_frames, uint32_t lag, float *d_out)
{
    sgx_fbank *fb = static_cast<sgx_fbank *>(bank);
    if (!fb || !fb->ctx) return SGX_ERR_INVALID_ARG;
    sgx_ctx *c = fb->ctx;
    if (lag == 0 || lag > sgx::flux::kMaxLag) return fail(c, SGX_ERR_INVALID_ARG, "sgx_flux_mags: lag must be 1 .. 64");
    if (n_frames == 0) return SGX_OK;
    if (!d_mags || !d_out) return fail(c, SGX_ERR_INVALID_ARG, "sgx_flux_mags: null buffer");
    if ((uintptr_t)d_out & 15u) return fail(c, SGX_ERR_INVALID_ARG, "sgx_flux_mags: d_out must be 16-byte aligned");
    SGX_HIP(c, hipSetDevice(c->device));
    const hipError_t e = sgx::launch_fbank_flux_stage(c, fb, d_mags, 0, n_frames, lag, d_out);
    if (e != hipSuccess) return fail_hip(c, e, "sgx_flux_mags: kernel launch");
    return SGX_OK;
}

int sgx_flux_batch(void *bank, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames, uint32_t lag, float *d_out,
                         size_t *n_out)
{
    namespace flux = sgx::flux;
    sgx_fbank *fb = static_cast<sgx_fbank *>(bank);
    if (n_out) *n_out = 0;
    if (!fb || !fb->ctx) return SGX_ERR_INVALID_ARG;
    sgx_ctx *c = fb->ctx;
    if (lag == 0 || lag > flux::kMaxLag) return fail(c, SGX_ERR_INVALID_ARG, "sgx_flux_batch: lag must be 1 .. 64");
    // a frame and its predecessor lie in the workspace together, or the call does not run
    const size_t cap = flux::row_cap(mags_bytes_per_frame(c));
    if (lag > flux::max_lag(mags_bytes_per_frame(c)))
        return fail(c, SGX_ERR_UNSUPPORTED, "sgx_flux_batch: lag " + std::to_string(lag) + " exceeds the cap of " +
                                                std::to_string(flux::max_lag(mags_bytes_per_frame(c))) +
                                                " frames (sgx_flux_max_lag); sgx_flux_mags takes any lag over rows the caller holds");
    size_t total, n;
    int rc = begin_batch(c, "sgx_flux_batch", n_samples, first_frame, max_frames, d_pcm, d_out, n_out, total, n);
    if (rc != SGX_OK || n == 0) return rc;
    if ((uintptr_t)d_out & 15u) return fail(c, SGX_ERR_INVALID_ARG, "sgx_flux_batch: d_out must be 16-byte aligned");
    // ranges: the rows of a range's frames and of the `back` frames before them by the rows' own route into the workspace (the head is
    // recomputed, not carried: a row is a pure function of its frame index), then the stage kernel over the frames behind the head
    rc = ensure_workspace(c, flux::rows_needed(first_frame, n, lag, cap));
    if (rc != SGX_OK) return rc;
    const size_t end = first_frame + n;
    for (size_t a = first_frame; a < end;) {
        const flux::Range r = flux::range_at(a, end, lag, cap);
        hipError_t e = rows_to_workspace(c, d_pcm, r.a - r.back, r.back + r.m, total);
        if (e != hipSuccess) return fail_hip(c, e, "sgx_flux_batch: stft launch");
        e = sgx::launch_fbank_flux_stage(c, fb, c->d_ws_mags.get(), r.back, r.m, lag, d_out + (a - first_frame) * (size_t)c->pairs * fb->n_filters * 4);
        if (e != hipSuccess) return fail_hip(c, e, "sgx_flux_batch: filter launch");
        a += r.m;
    }
    if (n_out) *n_out = n;
    return SGX_OK;
}

int sgx_bands_peak_fused(const sgx_ctx *c)
{
    if (!c) return SGX_ERR_INVALID_ARG;
    return stft_route(c, c->C, Out::kPeak).fused ? 1 : 0;
}

int sgx_bands_peak_batch(sgx_ctx *c, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames, size_t group,
                         float *d_peak, size_t *n_out)
{
    if (n_out) *n_out = 0;
    if (c && group == 0) return fail(c, SGX_ERR_INVALID_ARG, "sgx_bands_peak_batch: group is 0");
    size_t total, n;
    int rc = begin_batch(c, "sgx_bands_peak_batch", n_samples, first_frame, max_frames, d_pcm, d_peak, n_out, total, n);
    if (rc != SGX_OK || n == 0) return rc;
    const size_t g = group < n ? group : n;              // (one column: any group from n on)
    const size_t n_cols = (n - 1) / g + 1;
    const Route peak = stft_route(c, c->C, Out::kPeak);
    if (peak.fused) {
        // one kernel from PCM to peak columns: every persistent workgroup keeps the running maximum of its current column (in L2),
        // the columns that span several workgroups are finished by one combine launch
        const hipError_t e = run_call(c, peak, d_pcm, first_frame, n, total, d_peak, Out::kPeak, g);
        if (e != hipSuccess) return fail_hip(c, e, "sgx_bands_peak_batch: fused launch");
        if (n_out) *n_out = n_cols;
        return SGX_OK;
    }
    // The workspace route: chunks of frames through sgx_bands_batch's own route into the bounded workspace, bands_peak_kernel reduces
    // each chunk.  The workspace's budget (kWorkspaceBytes) holds, per frame of a chunk: its band column; on the two-kernel bands route its
    // magnitudes in front; and behind the columns the sub-columns of a two-level reduction (kSubNum / kSubDen of a column and two more: below).
    const size_t col = (size_t)c->pairs * c->R * 2, col_bytes = col * sizeof(float);
    const Route bands = stft_route(c, c->C, Out::kBands);
    const size_t mags_bytes = bands.fused ? 0 : mags_bytes_per_frame(c);
    constexpr size_t kBudget = kWorkspaceBytes, kSubNum = 9, kSubDen = 64, kTwoLevelMin = 64;
    const size_t per_frame = col_bytes + mags_bytes + (col_bytes * kSubNum + kSubDen - 1) / kSubDen;
    size_t chunk = kBudget > 2 * col_bytes ? (kBudget - 2 * col_bytes) / per_frame : 0;
    if (chunk < 1) chunk = 1;
    if (chunk > n) chunk = n;
    if (g <= chunk) chunk -= chunk % g;                  // whole columns per chunk; else a column accumulates over several chunks
    const size_t sub_cap = chunk * kSubNum / kSubDen + 2;
    const size_t ws_bytes = chunk * (col_bytes + mags_bytes) + sub_cap * col_bytes;
    const size_t ws_unit = mags_bytes_per_frame(c);   // (ensure_workspace counts frames of magnitudes)
    rc = ensure_workspace(c, (ws_bytes + ws_unit - 1) / ws_unit);
    if (rc != SGX_OK) return rc;
    float *ws_bands = c->d_ws_mags.get() + chunk * (mags_bytes / sizeof(float)), *ws_sub = ws_bands + chunk * col;
    for (size_t done = 0; done < n;) {
        const size_t j = done / g;                       // the column this chunk starts in: at its first frame unless g > chunk
        size_t m = n - done < chunk ? n - done : chunk;
        if (g > chunk && m > (j + 1) * g - done) m = (j + 1) * g - done;
        rc = run_bands(c, "sgx_bands_peak_batch", bands, d_pcm, first_frame + done, m, total, ws_bands);
        if (rc != SGX_OK) return rc;
        const size_t ge = g < m ? g : m;                 // frames per column inside this chunk
        const bool accumulate = done != j * g;
        float *dst = d_peak + j * col;
        // long columns in two levels, about sqrt(ge) sub-columns of sqrt(ge) frames each: one thread per row and column would read
        // thousands of frames in sequence on a handful of threads.  Sub-columns: m / sub + m / ge + 1 at most, with
        // sub >= 8 and ge >= 64 that is 9 m / 64 + 1 -- what the workspace reserves; checked all the same.
        size_t sub = ge;
        if (ge >= kTwoLevelMin) {
            sub = (size_t)std::ceil(std::sqrt((double)ge));
            if (sgx::peak_columns(m, ge, sub) > sub_cap) sub = ge;
        }
        hipError_t e;
        if (sub < ge) {
            e = sgx::launch_bands_peak(c, ws_bands, m, ge, sub, ws_sub, false);
            const size_t spc = (ge + sub - 1) / sub;
            if (e == hipSuccess) e = sgx::launch_bands_peak(c, ws_sub, sgx::peak_columns(m, ge, sub), spc, spc, dst, accumulate);
        } else {
            e = sgx::launch_bands_peak(c, ws_bands, m, ge, ge, dst, accumulate);
        }
        if (e != hipSuccess) return fail_hip(c, e, "sgx_bands_peak_batch: bands_peak launch");
        done += m;
    }
    if (n_out) *n_out = n_cols;
    return SGX_OK;
}

// ---- Welch-averaged spectra per bin: the mean over groups of frames of |X|^2, and of the four (L, R) products (sgx_psd.hpp) --------------

int sgx_psd_fused(const sgx_ctx *c)
{
    if (!c) return SGX_ERR_INVALID_ARG;
    return stft_route(c, c->C, Out::kPsd).fused ? 1 : 0;
}

int sgx_csd_fused(const sgx_ctx *c)
{
    if (!c) return SGX_ERR_INVALID_ARG;
    return stft_route(c, c->C, Out::kCsd).fused ? 1 : 0;
}

int sgx_psd_batch(sgx_ctx *c, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames, size_t group, float *d_psd,
                  size_t *n_out)
{
    return psd_batch(c, "sgx_psd_batch", false, d_pcm, n_samples, first_frame, max_frames, group, d_psd, n_out);
}

int sgx_csd_batch(sgx_ctx *c, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames, size_t group, float *d_csd,
                  size_t *n_out)
{
    return psd_batch(c, "sgx_csd_batch", true, d_pcm, n_samples, first_frame, max_frames, group, d_csd, n_out);
}

int sgx_psd_mags(sgx_ctx *c, const float *d_mags, size_t n_frames, size_t group, float *d_psd, size_t *n_out)
{
    return psd_stage(c, "sgx_psd_mags", false, d_mags, n_frames, group, d_psd, n_out);
}

int sgx_csd_spec(sgx_ctx *c, const float *d_spec, size_t n_frames, size_t group, float *d_csd, size_t *n_out)
{
    return psd_stage(c, "sgx_csd_spec", true, d_spec, n_frames, group, d_csd, n_out);
}

// ---- the K strongest spectral maxima of every row (sgx_maxima.hpp): the rows through the workspace, the selection kernel over them ------

int sgx_maxima_mags(sgx_ctx *c, const float *d_mags, size_t n_columns, uint32_t k, float floor, float *d_max)
{
    if (!c) return SGX_ERR_INVALID_ARG;
    const int rc = check_maxima(c, "sgx_maxima_mags", k, floor, d_max);
    if (rc != SGX_OK) return rc;
    if (n_columns == 0) return SGX_OK;
    if (!d_mags || !d_max) return fail(c, SGX_ERR_INVALID_ARG, "sgx_maxima_mags: null buffer");
    SGX_HIP(c, hipSetDevice(c->device));
    const hipError_t e = sgx::maxima::launch_maxima(c, d_mags, n_columns * c->pairs, k, floor, d_max);
    if (e != hipSuccess) return fail_hip(c, e, "sgx_maxima_mags: kernel launch");
    return SGX_OK;
}

int sgx_maxima_batch(sgx_ctx *c, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames, uint32_t k, float floor,
                     float *d_max, size_t *n_out)
{
    if (n_out) *n_out = 0;
    if (c) {
        const int bad = check_maxima(c, "sgx_maxima_batch", k, floor, d_max);
        if (bad != SGX_OK) return bad;
    }
    size_t total, n;
    int rc = begin_batch(c, "sgx_maxima_batch", n_samples, first_frame, max_frames, d_pcm, d_max, n_out, total, n);
    if (rc != SGX_OK || n == 0) return rc;
    // two kernels: the rows of a chunk of frames in the bounded workspace, by the rows' own route, then the selection kernel over them
    rc = in_workspace_chunks(c, n, [&](size_t done, size_t m) {
        hipError_t e = rows_to_workspace(c, d_pcm, first_frame + done, m, total);
        if (e != hipSuccess) return fail_hip(c, e, "sgx_maxima_batch: stft launch");
        e = sgx::maxima::launch_maxima(c, c->d_ws_mags.get(), m * c->pairs, k, floor, d_max + done * (size_t)c->pairs * 2 * k * 4);
        return e == hipSuccess ? (int)SGX_OK : fail_hip(c, e, "sgx_maxima_batch: selection launch");
    });
    if (rc != SGX_OK) return rc;
    if (n_out) *n_out = n;
    return SGX_OK;
}

// ---- where a row's cumulative sum crosses shares of its total (sgx_rolloff.hpp): the rows through the workspace, the kernel over them ----

int sgx_rolloff_mags(sgx_ctx *c, const float *d_mags, size_t n_columns, uint32_t power, const float *h_p, uint32_t n_p, float *d_out)
{
    if (!c) return SGX_ERR_INVALID_ARG;
    sgx::rolloff::Shares shares;
    const int rc = check_rolloff(c, "sgx_rolloff_mags", power, h_p, n_p, d_out, shares);
    if (rc != SGX_OK) return rc;
    if (n_columns == 0) return SGX_OK;
    if (!d_mags || !d_out) return fail(c, SGX_ERR_INVALID_ARG, "sgx_rolloff_mags: null buffer");
    SGX_HIP(c, hipSetDevice(c->device));
    const hipError_t e = sgx::rolloff::launch_rolloff(c, d_mags, n_columns * c->pairs, power, shares, n_p, d_out);
    if (e != hipSuccess) return fail_hip(c, e, "sgx_rolloff_mags: kernel launch");
    return SGX_OK;
}

int sgx_rolloff_batch(sgx_ctx *c, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames, uint32_t power,
                      const float *h_p, uint32_t n_p, float *d_out, size_t *n_out)
{
    if (n_out) *n_out = 0;
    sgx::rolloff::Shares shares;
    if (c) {
        const int bad = check_rolloff(c, "sgx_rolloff_batch", power, h_p, n_p, d_out, shares);
        if (bad != SGX_OK) return bad;
    }
    size_t total, n;
    int rc = begin_batch(c, "sgx_rolloff_batch", n_samples, first_frame, max_frames, d_pcm, d_out, n_out, total, n);
    if (rc != SGX_OK || n == 0) return rc;
    // two kernels: the rows of a chunk of frames in the bounded workspace, by the rows' own route, then the cumulative kernel over them
    rc = in_workspace_chunks(c, n, [&](size_t done, size_t m) {
        hipError_t e = rows_to_workspace(c, d_pcm, first_frame + done, m, total);
        if (e != hipSuccess) return fail_hip(c, e, "sgx_rolloff_batch: stft launch");
        e = sgx::rolloff::launch_rolloff(c, c->d_ws_mags.get(), m * c->pairs, power, shares, n_p, d_out + done * (size_t)c->pairs * 2 * n_p * 4);
        return e == hipSuccess ? (int)SGX_OK : fail_hip(c, e, "sgx_rolloff_batch: cumulative launch");
    });
    if (rc != SGX_OK) return rc;
    if (n_out) *n_out = n;
    return SGX_OK;
}

// ---- per-bin order statistics over groups of frames (sgx_quantile.hpp): the rows of whole columns through the workspace, the selection ----

size_t sgx_quantile_max_group(const sgx_ctx *c) { return c ? quantile_cap(c) : 0; }

int sgx_quantile_mags(sgx_ctx *c, const float *d_mags, size_t n_frames, size_t group, const double *q, uint32_t n_q, float *d_out, size_t *n_out)
{
    if (n_out) *n_out = 0;
    if (!c) return SGX_ERR_INVALID_ARG;
    const int rc = check_quantile(c, "sgx_quantile_mags", group, q, n_q);
    if (rc != SGX_OK) return rc;
    if (n_frames == 0) return SGX_OK;
    if (!d_mags || !d_out) return fail(c, SGX_ERR_INVALID_ARG, "sgx_quantile_mags: null buffer");
    SGX_HIP(c, hipSetDevice(c->device));
    const size_t g = group < n_frames ? group : n_frames;
    const hipError_t e = sgx::quantile::launch_quantile(c, d_mags, n_frames, g, q, n_q, d_out);
    if (e != hipSuccess) return fail_hip(c, e, "sgx_quantile_mags: kernel launch");
    if (n_out) *n_out = (n_frames - 1) / g + 1;
    return SGX_OK;
}

int sgx_quantile_batch(sgx_ctx *c, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames, size_t group, const double *q,
                       uint32_t n_q, float *d_out, size_t *n_out)
{
    if (n_out) *n_out = 0;
    if (c) {
        const int bad = check_quantile(c, "sgx_quantile_batch", group, q, n_q);
        if (bad != SGX_OK) return bad;
    }
    size_t total, n;
    int rc = begin_batch(c, "sgx_quantile_batch", n_samples, first_frame, max_frames, d_pcm, d_out, n_out, total, n);
    if (rc != SGX_OK || n == 0) return rc;
    // a quantile does not decompose: a column is selected from rows that lie in the workspace together, or not at all
    const size_t cap = quantile_cap(c), g = group < n ? group : n;
    if (g > cap)
        return fail(c, SGX_ERR_UNSUPPORTED, "sgx_quantile_batch: a column of " + std::to_string(g) + " frames exceeds the cap of " + std::to_string(cap) +
                                                " frames (sgx_quantile_max_group); sgx_quantile_mags takes any group over rows the caller holds");
    // ranges of whole columns: their rows by the rows' own route into the workspace, then the selection kernel over them into d_out
    const size_t range = cap / g * g, row_floats = mags_bytes_per_frame(c) / sizeof(float);
    rc = ensure_workspace(c, range < n ? range : n);
    for (size_t f = 0; rc == SGX_OK && f < n; f += range) {
        const size_t m = n - f < range ? n - f : range;
        hipError_t e = rows_to_workspace(c, d_pcm, first_frame + f, m, total);
        if (e != hipSuccess) return fail_hip(c, e, "sgx_quantile_batch: stft launch");
        // (m < g: the call's short last column alone in the last range)
        e = sgx::quantile::launch_quantile(c, c->d_ws_mags.get(), m, g < m ? g : m, q, n_q, d_out + f / g * n_q * row_floats);
        if (e != hipSuccess) return fail_hip(c, e, "sgx_quantile_batch: selection launch");
    }
    if (rc != SGX_OK) return rc;
    if (n_out) *n_out = (n - 1) / g + 1;
    return SGX_OK;
}

int sgx_render_bands(sgx_ctx *c, const float *d_bands, size_t n_columns, uint8_t *d_rgba)
{
    if (!c) return SGX_ERR_INVALID_ARG;
    if (n_columns == 0) return SGX_OK;
    if (!d_bands || !d_rgba) return fail(c, SGX_ERR_INVALID_ARG, "sgx_render_bands: null buffer");
    SGX_HIP(c, hipSetDevice(c->device));
    hipError_t e = sgx::launch_render_bands(c, d_bands, n_columns, d_rgba);
    if (e != hipSuccess) return fail_hip(c, e, "sgx_render_bands: kernel launch");
    return SGX_OK;
}

int sgx_bands_fused(const sgx_ctx *c)
{
    if (!c) return SGX_ERR_INVALID_ARG;
    return stft_route(c, c->C, Out::kBands).fused ? 1 : 0;
}

int sgx_magnitude_in(sgx_ctx *c, const float *d_mags, size_t n_columns, const float *h_ranges, uint32_t n_ranges, float *d_out)
{
    if (!c) return SGX_ERR_INVALID_ARG;
    if (n_columns == 0 || n_ranges == 0) return SGX_OK;
    if (!d_mags || !h_ranges || !d_out) return fail(c, SGX_ERR_INVALID_ARG, "sgx_magnitude_in: null buffer");
    SGX_HIP(c, hipSetDevice(c->device));
    const std::vector<float> key(h_ranges, h_ranges + (size_t)n_ranges * 2);
    if (key != c->bands_key || !c->d_band_rows.get()) {
        std::vector<float> f0(n_ranges), f1(n_ranges);
        for (uint32_t i = 0; i < n_ranges; ++i) { f0[i] = h_ranges[2 * i]; f1[i] = h_ranges[2 * i + 1]; }
        std::vector<sgx::RowEntry> rows;
        std::vector<sgx::SampleEntry> samples;
        sgx::build_range_tables(c->W, c->sr_u32, c->cfg.interp, f0.data(), f1.data(), n_ranges, rows, samples);
        SGX_HIP(c, hipStreamSynchronize(c->stream));  // the previous range set may still be in use
        SGX_HIP(c, c->d_band_rows.upload(rows));
        SGX_HIP(c, c->d_band_samples.upload(samples));
        c->bands_key = key;
    }
    hipError_t e = sgx::launch_magnitude_in(c, d_mags, n_columns, c->d_band_rows.get(), c->d_band_samples.get(), n_ranges, d_out);
    if (e != hipSuccess) return fail_hip(c, e, "sgx_magnitude_in: kernel launch");
    return SGX_OK;
}

int sgx_set_gradient(sgx_ctx *c, const uint8_t *h_rgb, uint32_t n, int stereo)
{
    if (!c) return SGX_ERR_INVALID_ARG;
    if (!h_rgb || n < 2 || n > 65536) return fail(c, SGX_ERR_INVALID_ARG, "sgx_set_gradient: need 2..65536 entries");
    c->pal.rgb.assign(h_rgb, h_rgb + (size_t)n * 3);
    c->pal.n = n;
    c->pal.stereo = stereo ? 1 : 0;
    c->pal.segments = false;
    c->pal.fn = nullptr;
    c->pal.t_thr.clear();
    return upload_palette(c);
}

int sgx_set_gradient_fn(sgx_ctx *c, sgx_gradient_fn eval, void *user, int stereo)
{
    if (!c) return SGX_ERR_INVALID_ARG;
    if (!eval) return fail(c, SGX_ERR_INVALID_ARG, "sgx_set_gradient_fn: null callback");
    c->pal.fn = eval;
    c->pal.fn_user = user;
    c->pal.stereo = stereo ? 1 : 0;
    c->pal.segments = true;
    int rc = upload_palette(c);
    // the callback is only valid during this call (and sgx_lookup_table needs it again): keep the pointer,
    // the caller owns its lifetime as documented
    if (rc == SGX_OK && c->pal.n > 65536) return fail(c, SGX_ERR_INVALID_ARG, "sgx_set_gradient_fn: gradient has more than 65536 colour steps");
    return rc;
}

int sgx_builtin_gradient(const char *name, uint8_t *h_rgb_out)
{
    const unsigned char *g = builtin_gradient(name);
    if (!g || !h_rgb_out) return SGX_ERR_INVALID_ARG;
    std::memcpy(h_rgb_out, g, 256 * 3);
    return SGX_OK;
}

int sgx_set_builtin_scheme(sgx_ctx *c, const char *name, int stereo)
{
    if (!c) return SGX_ERR_INVALID_ARG;
    if (const unsigned char *g = builtin_gradient(name)) return sgx_set_gradient(c, g, 256, stereo);
    sgx_gradient_fn fn = nullptr;
    void *user = nullptr;
    if (continuous_gradient(name, &fn, &user)) return sgx_set_gradient_fn(c, fn, user, stereo);
    return fail(c, SGX_ERR_INVALID_ARG, std::string("sgx_set_builtin_scheme: unknown gradient '") + (name ? name : "(null)") + "'");
}

int sgx_set_builtin_gradient(sgx_ctx *c, const char *name) { return sgx_set_builtin_scheme(c, name, 0); }

int sgx_builtin_gradient_eval(const char *name, double t, uint8_t rgb_out[3])
{
    if (!rgb_out) return SGX_ERR_INVALID_ARG;
    sgx_gradient_fn fn = nullptr;
    void *user = nullptr;
    if (continuous_gradient(name, &fn, &user)) { fn(t, rgb_out, user); return SGX_OK; }
    if (const unsigned char *g = builtin_gradient(name)) {
        const int idx = sgx::lut_index_host(t, 256, SGX_LUT_FLOOR_N);
        std::memcpy(rgb_out, g + 3 * idx, 3);
        return SGX_OK;
    }
    return SGX_ERR_INVALID_ARG;
}

int sgx_lookup_table(sgx_ctx *c, uint32_t res, float *h_out)
{
    if (!c) return SGX_ERR_INVALID_ARG;
    if (!h_out || res < 2) return fail(c, SGX_ERR_INVALID_ARG, "sgx_lookup_table: resolution must be at least 2");
    // colorscheme.rs:73-92
    for (uint32_t i = 0; i < res; ++i)
        for (uint32_t j = 0; j < res; ++j) {
            const float magnitude = (float)i / (float)(res - 1);
            const float pan = 1.0f - ((float)j / (float)(res - 1));
            const double tt = c->pal.stereo ? (double)pan : (double)magnitude;
            uint8_t rgb[3];
            if (c->pal.segments) {
                c->pal.fn(tt, rgb, c->pal.fn_user);
            } else {
                const int idx = sgx::lut_index_host(tt, c->pal.n, c->cfg.lut_index_mode);
                rgb[0] = c->pal.rgb[3 * idx]; rgb[1] = c->pal.rgb[3 * idx + 1]; rgb[2] = c->pal.rgb[3 * idx + 2];
            }
            float *o = h_out + 4 * ((size_t)i * res + j);
            o[0] = (float)rgb[0] / 256.0f;
            o[1] = (float)rgb[1] / 256.0f;
            o[2] = (float)rgb[2] / 256.0f;
            o[3] = c->pal.stereo ? magnitude : 1.0f;
        }
    return SGX_OK;
}

int sgx_bin_edges(const sgx_ctx *c, float *h_out)
{
    if (!c || !h_out) return SGX_ERR_INVALID_ARG;
    std::memcpy(h_out, c->tab.edges.data(), c->tab.edges.size() * sizeof(float));
    return SGX_OK;
}

int sgx_row_sample_counts(const sgx_ctx *c, uint32_t *h_out)
{
    if (!c || !h_out) return SGX_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < c->R; ++i) h_out[i] = c->tab.rows[i].count;
    return SGX_OK;
}

int sgx_window(const sgx_ctx *c, float *h_out)
{
    if (!c || !h_out) return SGX_ERR_INVALID_ARG;
    std::memcpy(h_out, c->tab.window.data(), c->tab.window.size() * sizeof(float));
    return SGX_OK;
}

int sgx_synth_white_noise(sgx_ctx *c, float *d_out, uint64_t first, size_t n_samples, uint32_t channels, uint32_t seed)
{
    if (!c) return SGX_ERR_INVALID_ARG;
    if (n_samples == 0) return SGX_OK;
    if (!d_out || channels < 1) return fail(c, SGX_ERR_INVALID_ARG, "sgx_synth_white_noise: bad argument");
    SGX_HIP(c, hipSetDevice(c->device));
    hipError_t e = sgx::launch_white_noise(c, d_out, first, n_samples, channels, seed);
    if (e != hipSuccess) return fail_hip(c, e, "sgx_synth_white_noise: kernel launch");
    return SGX_OK;
}

int sgx_checksum(sgx_ctx *c, const void *d_buf, size_t n_bytes, uint64_t base_word, uint64_t *h_out)
{
    if (!c || !h_out) return SGX_ERR_INVALID_ARG;
    if (n_bytes % 4) return fail(c, SGX_ERR_INVALID_ARG, "sgx_checksum: size must be a multiple of 4");
    SGX_HIP(c, hipSetDevice(c->device));
    SGX_HIP(c, hipMemsetAsync(c->d_cksum.get(), 0, sizeof(unsigned long long), c->stream));
    if (n_bytes) {
        if (!d_buf) return fail(c, SGX_ERR_INVALID_ARG, "sgx_checksum: null buffer");
        hipError_t e = sgx::launch_checksum(c, static_cast<const uint32_t *>(d_buf), n_bytes / 4, base_word, c->d_cksum.get());
        if (e != hipSuccess) return fail_hip(c, e, "sgx_checksum: kernel launch");
    }
    unsigned long long v = 0;
    SGX_HIP(c, hipMemcpyAsync(&v, c->d_cksum.get(), sizeof(v), hipMemcpyDeviceToHost, c->stream));
    SGX_HIP(c, hipStreamSynchronize(c->stream));
    *h_out = v;
    return SGX_OK;
}

int sgx_checksum_add(sgx_ctx *c, const void *d_buf, size_t n_bytes, uint64_t base_word, uint64_t *d_acc)
{
    if (!c || !d_acc) return SGX_ERR_INVALID_ARG;
    if (n_bytes % 4) return fail(c, SGX_ERR_INVALID_ARG, "sgx_checksum_add: size must be a multiple of 4");
    if (n_bytes == 0) return SGX_OK;
    if (!d_buf) return fail(c, SGX_ERR_INVALID_ARG, "sgx_checksum_add: null buffer");
    SGX_HIP(c, hipSetDevice(c->device));
    hipError_t e = sgx::launch_checksum(c, static_cast<const uint32_t *>(d_buf), n_bytes / 4, base_word,
                                        reinterpret_cast<unsigned long long *>(d_acc));
    if (e != hipSuccess) return fail_hip(c, e, "sgx_checksum_add: kernel launch");
    return SGX_OK;
}

}  // extern "C"
