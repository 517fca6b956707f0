/*
 * sgx.h -- C ABI of the MI355X (gfx950) streaming-STFT spectrogram engine.
 *
 * This is the drop-in boundary for ONE path of JacksonCampolattaro/spectrogram-rs: PCM ->
 * Hann + 2x zero-pad -> c2c FFT -> stereo magnitudes -> log-frequency resample -> dB -> colour
 * -> RGBA pixel columns.  Every entry point names the reference interface it replaces
 * (file:line relative to the reference repository).  Plain pointers and sizes only; no C++ or
 * framework types cross this boundary.  INTEGRATION.md shows the Rust `extern "C"` binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - All `d_*` pointers are DEVICE pointers (hipMalloc'ed, or a torch tensor's data_ptr()).
 *     All `h_*` pointers are host pointers.  The caller owns every I/O buffer.
 *   - Work is enqueued on the context's stream (sgx_set_stream; default: the NULL stream) and is
 *     asynchronous; sgx_sync() waits for it.  The batch calls (sgx_stft_batch*, sgx_render_*, sgx_bands_*batch, sgx_magnitude_in,
 *     sgx_fbank_batch, sgx_fbank_mags, sgx_fbank_cross_batch, sgx_fbank_cross_spec, sgx_flux_batch, sgx_flux_mags, sgx_psd_batch, sgx_csd_batch, sgx_psd_mags, sgx_csd_spec, sgx_maxima_batch, sgx_maxima_mags, sgx_rolloff_batch, sgx_rolloff_mags, sgx_quantile_batch, sgx_quantile_mags, sgx_image_write_columns / _read, sgx_view_write_rows / _draw, sgx_synth_white_noise,
 *     sgx_checksum_add) only enqueue;
 *     the calls that hand host data back or free host slots (sgx_process_one, sgx_live_tick*, sgx_spectrum_levels,
 *     sgx_checksum) and the calls that replace tables (sgx_set_gradient*, sgx_set_builtin_*) wait for the context's OWN
 *     stream; no call waits for another context's stream (tests/test_gpu_streams.py).
 *     sgx_istft_batch builds its tables on a context's first call (sgx_create does not); that first call may wait for the
 *     context's own stream, as a grown workspace does.  Later calls only enqueue.  Every kernel, copy and memset of a call goes
 *     onto the context's stream, helper passes included (tests/test_gpu_stream_routes.py holds every route and entry point to it).
 *   - sgx_set_stream may be called at any time, also while the context's earlier work is pending.  With the stream the context
 *     is already on it returns at once (a wrapper may bind before every call).  With another stream it orders, on the device,
 *     everything enqueued on the new stream from now on behind everything the context has enqueued on the old one -- the context's
 *     own buffers (workspace, planes, scratch, partial columns, tables) are shared by both -- through an event the context holds;
 *     the host does not wait.  The stream the context leaves must still exist.  The caller's own buffers are the caller's to order.
 *   - Every function returns SGX_OK (0) or a negative sgx_status; the text of the last error is
 *     available from sgx_last_error().  The library never aborts the host process (the
 *     reference unwrap()s: fft.rs:24,77).
 *   - A context is not thread-safe: one context per thread / stream / GPU (the reference holds
 *     its transform in a RefCell on the GTK main thread: gpu_spectrogram.rs:58).
 *   - Device buffers are at least 8-byte aligned ((l, r) pairs are moved as 8-byte words); hipMalloc and torch
 *     allocations are 256-byte aligned, which is also what the store pattern of the kernels is tuned for.
 *   - There is NO CPU fallback: without a HIP device sgx_create() fails with SGX_ERR_NO_DEVICE.
 */
#ifndef SGX_H
#define SGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define SGX_API __attribute__((visibility("default")))
#else
#define SGX_API
#endif

typedef enum sgx_status {
    SGX_OK = 0,
    SGX_ERR_INVALID_ARG = -1,
    SGX_ERR_UNSUPPORTED = -2, /* e.g. a transform length this build has no kernel for */
    SGX_ERR_HIP = -3,         /* a HIP runtime call failed; see sgx_last_error */
    SGX_ERR_NOMEM = -4,
    SGX_ERR_NO_DEVICE = -5
} sgx_status;

/* interpolated_frequency_sample.rs:46-48 calls cubic_interpolate (:88-105); cosine_interpolate
 * (:78-86) is dead code there but is what README.md:19-20 and BASELINE config 3 name. */
#define SGX_INTERP_CUBIC 0u
#define SGX_INTERP_COSINE 1u

/* colorous Gradient::eval_continuous index rule for 256-entry ramps (un-vendored crate; the
 * rule is an input so it can be corrected without touching kernels) */
#define SGX_LUT_FLOOR_N 0u   /* idx = clamp(floor(t * n), 0, n-1) */
#define SGX_LUT_ROUND_NM1 1u /* idx = clamp(round(t * (n-1)), 0, n-1) */

typedef struct sgx_ctx sgx_ctx;

/* One plain struct replaces the reference's compile-time constants:
 *   FastFourierTransform::new(sample_rate, period)                      fft.rs:18
 *   AudioStreamTransform::new(stream, transform, stride)                audio_transform.rs:22-32
 *   TEXTURE_HEIGHT = 1024, y range 32..22030 Hz                         simple_spectrogram.rs:34-35,107
 *   MIN_DB = -70, MAX_DB = -10                                          colorscheme.rs:16-17        */
typedef struct sgx_config {
    uint32_t struct_size;    /* = sizeof(sgx_config); set by sgx_config_init */
    float sample_rate;       /* Hz */
    float period;            /* s; W = (period * sample_rate) as usize            (fft.rs:19)  */
    float stride;            /* s; H = (stride * sample_rate) as usize  (audio_transform.rs:35) */
    uint32_t window_samples; /* if non-zero, W directly (period ignored)                        */
    uint32_t hop_samples;    /* if non-zero, H directly (stride ignored)                        */
    uint32_t channels;       /* interleaved channels in the PCM stream: 1 = mono, expanded to
                                (s, s) as audio_input_list_model.rs:67-69 does; 2 = (l, r);
                                2k = k independent (l, r) pairs (extension, BASELINE config 4),
                                at most 32768; odd counts above 1 are refused.  Every family
                                and entry point is held to the truth at 6, 12, 64 and 32768
                                channels by tests/test_gpu_channel_counts.py                  */
    uint32_t rows;           /* R, pixel rows per column (default 1024)                         */
    double f_min, f_max;     /* log axis range in Hz (default 32, 22030)                        */
    float min_db, max_db;    /* default -70, -10                                                */
    uint32_t interp;         /* SGX_INTERP_*                                                    */
    uint32_t lut_index_mode; /* SGX_LUT_*                                                       */
    int32_t device;          /* HIP device ordinal, or -1 for the current device                */
    uint32_t flags;          /* SGX_FLAG_*                                                      */
} sgx_config;

#define SGX_FLAG_FORCE_GENERIC 1u /* use the generic power-of-two kernel even where a tuned one exists, the chirp-z kernel even where the mixed-radix one applies (testing) */
#define SGX_FLAG_NO_FUSED_RENDER 4u /* sgx_render_batch: run STFT and pixel stage as two kernels even where the fused one applies (A/B);
                                       sgx_bands_batch likewise: STFT, then magnitude_in over the context's rows */
/* Mono streams.  The reference duplicates a mono sample into (s, s) and transforms every frame on its own
 * (audio_input_list_model.rs:67-69, fft.rs:47-99).  DEFAULT here, at every window and hop: exactly that dataflow, one transform per
 * frame -- every frame within north_star's tolerance of its OWN peak on any input.  At W 2048 (any hop, any alignment of the stream)
 * it is computed as the 4096-point spectrum of a REAL frame, a 2048-point complex transform + one butterfly per bin
 * (stft4096_real.hip; at H 256, the BASELINE shape, with the window sliding in registers): the cost of half a transform.  The
 * mixed-radix kernel does the same at every window it serves (stft_mixed.hip, real-input mode: the application's 2400 and 2205, every
 * 2-3-5-7-smooth length, W 512 / 1024 / 4096; any hop and alignment), the chirp-z kernel too from W 86 on (1102 at 22.05 kHz).
 * Elsewhere (W 8192, the small windows of the generic kernels) it is the (s, s) transform itself.
 * SGX_FLAG_PAIRED_FRAMES (opt-in): two frames (2j, 2j+1) per transform in its real and imaginary part -- half the work of the (s, s)
 * transform, but the quieter frame of a pair carries the louder one's float32 rounding floor: the tolerance then holds against the
 * PAIR's peak only (measured: up to 4.7 x the own-peak tolerance across a 60 dB step inside one hop, unbounded next to digital
 * silence; invisible on stationary signals.  DESIGN.md section 4).  At W 2400 and W 8192 a context whose hop and window together
 * exceed 2^31 - 1 bytes of mono samples (H + W >= 2^29) runs every frame as its own transform, as without the flag -- at W 8192 on a
 * duplicated (s, s) plane of the call's sample range, which the library allocates: 2 (n - 1) H + 2 W floats for n frames, 17 GB for three
 * frames at H = 2^30. */
#define SGX_FLAG_PAIRED_FRAMES 1024u /* mono: two frames per transform (the default of rounds 1-3) */
#define SGX_FLAG_COMPLEX_MONO 512u /* mono: the literal (s, s) 2W-point complex transform per frame -- fft.rs:47-57 -- wherever a
                                      real-input kernel would run (A/B; implies no pairing) */
#define SGX_FLAG_LUT_WALK 64u      /* fused pixel kernel: walk the dB thresholds from the log2 seed even where the host has shown that one compare pair settles the LUT index (A/B, and the test of the fallback) */
#define SGX_FLAG_MIXED_GENERIC 256u /* W = 2400: the composite-radix kernel (any 2-3-5-7-smooth length) instead of the tuned 4800-point one (A/B) */
#define SGX_FLAG_LARGE_TRANSFORM 4096u /* let sgx_create accept lengths that no in-LDS kernel serves: any W from 4 to 2^20 (2W up to 2^21
                                        points).  Such lengths run a multi-pass transform staged through device memory (stft_kernel 11), and
                                        the context holds a scratch buffer for it (64 MiB at most).  Lengths an in-LDS kernel serves run that
                                        kernel whether the flag is set or not. */

typedef struct sgx_info {
    uint32_t struct_size;
    uint32_t window_samples;  /* W  = num_input_samples()            fft.rs:41 */
    uint32_t fft_length;      /* P  = 2 W                            fft.rs:44 */
    uint32_t num_frequencies; /* M  = num_output_frequencies() = W-1 fft.rs:33 */
    uint32_t hop_samples;     /* H                                              */
    uint32_t channels;
    uint32_t pairs;           /* (l, r) pairs per hop position: 1 for mono/stereo, channels/2 otherwise */
    uint32_t rows;            /* R */
    uint32_t sample_rate_u32; /* SampleRate(sample_rate as u32)      simple_spectrogram.rs:138 */
    uint32_t total_samples_per_column; /* sum over rows of magnitude_in's sample count */
    uint32_t stft_kernel;     /* 0 = generic power-of-two, 2 = 4096-point workgroup-per-transform (default at W 2048), 4 = Bluestein chirp-z (any 2W), 6 = mixed radix (2W = 2^a 3^b 5^c 7^d <= 20480, e.g. the application's 4800, 4410 and 19200), 9 = 4800-point workgroup-per-transform, 16 x 20 x 15 (default for W = 2400, the application's window at 48 kHz; streams of more than two channels run 6), 10 = 16384-point as 32 x 32 x 16 in one 512-thread workgroup, 32 points per thread (W = 8192; the designs 5, 7 and 8 of rounds 1-5 are gone: profiles/r06_k16.txt), 11 = multi-pass four-step transform through a device-memory scratch (SGX_FLAG_LARGE_TRANSFORM only: lengths no other kernel serves; chirp-z over it where 2W has a prime factor above 7; render_path 0) */
                              /* (magnitudes: the tuned kernels -- 2, 6, 9, 10 and the chirp-z plans of 4 -- take |re + i im| through the hardware
                                 square root of fma(re, re, im * im): 1 ulp; the generic kernel (0) and the radix-4 Bluestein ladder use the
                                 correctly rounded sqrtf.  Rows of different kernels for the same input agree within the tolerance, not bit for bit) */
    uint32_t render_path;     /* sgx_render_batch as configured NOW (palette included): bit 0 = one fused PCM-to-pixel kernel (the
                                 4096-point kernel, or a compile-time plan of the mixed-radix kernel whose LDS image holds the column),
                                 bit 1 = its LUT index is seed + one compare pair (else seed + walk); neither = two kernels;
                                 bit 2 = the transform runs a compile-time plan of the composite-radix stages: stft_kernel 6 at the
                                 0.05 s windows of the usual sample rates (8 kHz to 192 kHz) and the powers of two from 512 on;
                                 stft_kernel 4 (chirp-z) for W = 86 .. 5461, e.g. 1102 at 22.05 kHz;
                                 bit 3 = a mono stream runs a real-input kernel, the W-point transform of sample pairs (unless
                                 SGX_FLAG_PAIRED_FRAMES / SGX_FLAG_COMPLEX_MONO): at W 2048, and at every window the mixed-radix kernel or the chirp-z
                                 stages serve (stft_kernel 6, 9 and 4 with bit 2; any hop and alignment) */
    uint64_t mags_bytes_per_frame; /* pairs * M * 2 * 4 */
    uint64_t rgba_bytes_per_frame; /* pairs * R * 4     */
} sgx_info;

/* ---- lifetime ---------------------------------------------------------------------------- */

SGX_API const char *sgx_version(void);

/* Fill `cfg` with the reference's defaults for BASELINE config A:
 * 48 kHz, W 2048 / H 256 (given as window_samples / hop_samples), 1 channel, 1024 rows,
 * 32..22030 Hz, -70..-10 dB, cubic interpolation, SGX_LUT_FLOOR_N, current device. */
SGX_API int sgx_config_init(sgx_config *cfg);

/* Replaces FastFourierTransform::new (fft.rs:18-31: FFTW planning) + AudioStreamTransform::new
 * (audio_transform.rs:22-32) + SimpleSpectrogram's axis/palette construction
 * (simple_spectrogram.rs:88-113).  Builds the Hann table, twiddles, per-row resampling tables,
 * dB thresholds and the default gradient (Magma, simple_spectrogram.rs:95) on the device.
 * Lengths: 2W a power of two up to 16384, 2W 2-3-5-7-smooth up to 20480, or any 2W with 3W - 1 <= 16384 (chirp-z); with
 * SGX_FLAG_LARGE_TRANSFORM also every other W from 4 to 2^20 (stft_kernel 11).  Any other length: SGX_ERR_UNSUPPORTED. */
SGX_API int sgx_create(const sgx_config *cfg, sgx_ctx **out_ctx);
SGX_API void sgx_destroy(sgx_ctx *ctx);

/* Text of the most recent error on this context (ctx == NULL: most recent sgx_create failure on
 * the calling thread).  Never NULL. */
SGX_API const char *sgx_last_error(const sgx_ctx *ctx);

SGX_API int sgx_query(const sgx_ctx *ctx, sgx_info *out);

/* Number of frames the hop loop of AudioStreamTransform::process (audio_transform.rs:34-42)
 * yields from n_samples samples per channel: max(0, (n - W) / H + 1).  Frame t covers samples
 * [t*H, t*H + W).  (The reference also skips H samples on its terminating short read -- a
 * live-capture artefact that a batch engine must not reproduce.) */
SGX_API size_t sgx_num_frames(const sgx_ctx *ctx, size_t n_samples);

/* `stream` is a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = default.  Unchanged stream: returns at once.
 * Another stream: its later work is ordered behind the context's earlier work on the old stream; asynchronous (the conventions above). */
SGX_API int sgx_set_stream(sgx_ctx *ctx, void *stream);
SGX_API int sgx_sync(sgx_ctx *ctx);

/* The number of compute units the context sizes its persistent launches for. Default: the device's own count.
 * n = 0 restores it; 1 .. the device's count is accepted; a larger n: SGX_ERR_INVALID_ARG.
 * Takes effect for calls made afterwards; does not wait; results do not depend on it (tests/test_gpu_cu_counts.py). */
SGX_API int sgx_set_cu_limit(sgx_ctx *ctx, uint32_t n);
SGX_API uint32_t sgx_cu_limit(const sgx_ctx *ctx);   /* the count in force; 0 for a null context */

/* Diagnostic: how the rows calls (sgx_stft_batch, _f16, _complex) of a mono W 2048 context deal their frame pairs ("jobs") to the
 * persistent workgroups. By default a long float or half rows call deals most of them as one static run per workgroup and lets the
 * workgroups claim the rest in chunks, so that all finish together: 15/16 in weighted runs (sgx_set_run_weights) and chunks of 4 at a
 * hop of 256 on the whole device, 12/16 in equal runs and chunks of 8 elsewhere. A call that would leave static runs of fewer than
 * 64 jobs at 12/16, and every complex rows call, is dealt statically.
 * (16, 0): always static. (0, 0): the default rule. Any other share 0 .. 16 with a chunk of 1 .. 2^20 jobs: that split at any size.
 * Anything else: SGX_ERR_INVALID_ARG. Results do not depend on it, bit for bit (tests/test_gpu_claimed_runs.py).
 * The rows launches of the workspace routes take the same deal -- sgx_psd_batch always, and sgx_render_batch, sgx_bands_batch,
 * sgx_bands_peak_batch and sgx_fbank_batch under SGX_FLAG_NO_FUSED_RENDER -- and the same file holds those consumers to it. */
SGX_API int sgx_set_run_claim(sgx_ctx *ctx, uint32_t static_sixteenths, uint32_t chunk_jobs);
/* the split a float or half rows call of n_frames frames would run under now: (16, 0) where that is the static one */
SGX_API int sgx_run_claim(const sgx_ctx *ctx, size_t n_frames, uint32_t *static_sixteenths, uint32_t *chunk_jobs);
/* Diagnostic: the weights of those calls' static runs. Four workgroups share a compute unit, the n-th one placed there runs at its own
 * rate, and its static run is w[n] / 64 of the equal one. Four weights of at least 1 each that sum to 256; (64, 64, 64, 64): equal runs.
 * NULL or all zero: the default, the measured weights where a call fills every compute unit of the device four times and equal runs
 * elsewhere. Weights that are set apply at any size and any sgx_set_cu_limit. Anything else: SGX_ERR_INVALID_ARG.
 * Results do not depend on the weights, bit for bit (tests/test_gpu_weighted_runs.py); the rows launches of the workspace routes take
 * the same deal, the automatic one included, and that file holds their consumers to it as well. */
SGX_API int sgx_set_run_weights(sgx_ctx *ctx, const uint32_t w[4]);
/* the four weights a float rows call of n_frames frames would run under now */
SGX_API int sgx_run_weights(const sgx_ctx *ctx, size_t n_frames, uint32_t w[4]);

/* ---- the transform: replaces AudioTransform::process / AudioStreamTransform::process ----- */

/* Batched FastFourierTransform::process (fft.rs:43-99) driven by the hop loop
 * (audio_transform.rs:34-42).
 *   d_pcm   [n_samples][channels] float, interleaved
 *   d_mags  [n_out][pairs][M][2] float: (left, right) magnitudes of bins k = 1..W-1, scaled 2/W
 * Frames [first_frame, first_frame + max_frames) that exist are produced; *n_out (may be NULL)
 * receives how many.  Too few samples is not an error: *n_out = 0 (the reference returns None,
 * fft.rs:72). */
SGX_API int sgx_stft_batch(sgx_ctx *ctx, const float *d_pcm, size_t n_samples, size_t first_frame,
                           size_t max_frames, float *d_mags, size_t *n_out);

/* The transform of sgx_stft_batch without the magnitude: the complex spectra of the (l, r) split (fft.rs:81-98 before `hypot`).
 *   d_spec [n_out][pairs][M][2][2] float: per bin k = 1..W-1 (L.re, L.im, R.re, R.im) with
 *     L[k] = (F[k] + conj F[P-k]) / 2 * (2/W),   R[k] = (F[k] - conj F[P-k]) / (2i) * (2/W),
 *   F = the 2W-point forward DFT (e^{-2 pi i k n / P}) of (l + i r) * Hann, zero-padded; time origin = the frame's first sample.
 *   So L = DFT(Hann * l) * 2/W and R = DFT(Hann * r) * 2/W, and |L|, |R| are sgx_stft_batch's rows.
 *   Mono: (X, X) per bin, X = DFT(Hann * s) * 2/W, the same as the (s, s) dataflow gives; with SGX_FLAG_PAIRED_FRAMES
 *   the frame's own X in both halves.
 * first_frame / max_frames / *n_out as sgx_stft_batch.  Stream-ordered and asynchronous. */
SGX_API int sgx_stft_batch_complex(sgx_ctx *ctx, const float *d_pcm, size_t n_samples, size_t first_frame,
                                   size_t max_frames, float *d_spec, size_t *n_out);

/* The inverse of sgx_stft_batch_complex: PCM from complex (L, R) spectra by weighted overlap-add.
 *   d_spec [n_frames][pairs][M][2][2] float, exactly what sgx_stft_batch_complex writes; frame t has its time origin at sample t*H.
 *   d_pcm  [n_out][channels] float, interleaved (the layout of the forward's input): samples [first_sample, first_sample + max_samples)
 *          that exist, n < (n_frames - 1) * H + W.  Sample n is stream sample f0 * H + n when the spectra came from a forward call at
 *          first_frame = f0.  (l, r): 2 channels; 2k channels: pair j writes channels 2j and 2j+1; mono: 1 channel from the L half.
 * Definition, per frame and channel, with L[k] given for k = 1 .. W-1 and P = 2W:
 *   1. g[n] = 1/2 Re sum_{k=1}^{W-1} L[k] e^{+i pi k n / W}, n in [0, 2W)  (numpy: A = zeros(P); A[1:W] = L; g = W * ifft(A).real).
 *   2. The forward drops DC and Nyquist; the zero padding pins them down: c_e = minus the mean of g over the even n in [W, 2W), c_o the
 *      same over the odd n, and the frame is f[m] = g[m] + c_{m mod 2}, m in [0, W).  For spectra the forward produced this is Hann * x;
 *      for edited spectra it is the least-squares choice of the two missing real bins.
 *   3. x[n] = sum_t w[m] f_t[m] / sum_t w[m]^2, m = n - t*H, over the frames t of d_spec that cover n, w = sgx_window (w[0] = 0);
 *      exactly 0.0f where the envelope sum_t w[m]^2 is 0 (sample 0, and the gaps when H > W).
 * Each sample's sum runs over its frames in ascending order: the output is bit-identical however the range is split across calls.
 * n_frames == 0 or first_sample past the end: *n_out = 0, not an error.  n_out may be NULL.  Stream-ordered and asynchronous; the first
 * call builds the context's inverse tables (see the conventions above).  SGX_ERR_UNSUPPORTED where sgx_istft_supported is 0. */
SGX_API int sgx_istft_batch(sgx_ctx *ctx, const float *d_spec, size_t n_frames, size_t first_sample,
                            size_t max_samples, float *d_pcm, size_t *n_out);
/* 1: this context's W is served by sgx_istft_batch; 0: it is not (SGX_ERR_UNSUPPORTED: the lengths only SGX_FLAG_LARGE_TRANSFORM
 * serves); < 0: error */
SGX_API int sgx_istft_supported(const sgx_ctx *ctx);

/* The same transform with the magnitudes stored as IEEE half (l, r) pairs, 4 bytes per bin
 * (round to nearest even): d_mags_f16 [n_out][pairs][M][2] half.  This is the texel format of the
 * F16F16 ring texture the default widget uploads its frames into (gpu_spectrogram.rs:218-226,
 * 268-274: rows of M texels), so a GL-interop consumer can take the rows as they are; it also
 * halves the bytes the transform writes. */
SGX_API int sgx_stft_batch_f16(sgx_ctx *ctx, const float *d_pcm, size_t n_samples, size_t first_frame,
                               size_t max_frames, void *d_mags_f16, size_t *n_out);

/* One call of AudioTransform::process (audio_transform.rs:10, fft.rs:43) on HOST buffers, for a
 * per-frame shim: h_lr [n_avail][2] (l, r) pairs, h_out [M][2].  Returns 1 (Some), 0 (None:
 * n_avail < W) or a negative sgx_status.  Synchronous. */
SGX_API int sgx_process_one(sgx_ctx *ctx, const float *h_lr, size_t n_avail, float *h_out);

/* ---- the pixel path: replaces the loop of SimpleSpectrogram::snapshot --------------------- */

/* PCM -> RGBA pixel columns in one call (simple_spectrogram.rs:136-165 for every frame):
 * InterpolatedFrequencySample::magnitude_in over the log-spaced row edges of
 * LogCoordf64::unmap (log_scaling.rs:114-119), ColorScheme::color_for (colorscheme.rs:55-71),
 * Pixbuf::put_pixel (simple_spectrogram.rs:153-160).
 *   d_rgba [n_out][pairs][R][4] uint8; index [y] is the IMAGE row y = R-1-py, i.e. row 0 is the
 *   highest frequency, exactly the column that put_pixel writes (simple_spectrogram.rs:150). */
SGX_API int sgx_render_batch(sgx_ctx *ctx, const float *d_pcm, size_t n_samples, size_t first_frame,
                             size_t max_frames, uint8_t *d_rgba, size_t *n_out);

/* The pixel stage alone, from magnitudes already on the device (stage-wise parity):
 *   d_mags [n_columns][M][2] -> d_rgba [n_columns][R][4]. */
SGX_API int sgx_render_mags(sgx_ctx *ctx, const float *d_mags, size_t n_columns, uint8_t *d_rgba);

/* FrequencySample::magnitude_in(f0..f1) (src/fourier/mod.rs:17-21; interpolated_frequency_sample.rs:60-75)
 * for n_ranges arbitrary frequency ranges and every column: the mean of the interpolated (l, r) samples,
 * no colour.  h_ranges [n_ranges][2] = (f0, f1) in Hz on the host; d_out [n_columns][n_ranges][2] float.
 * This is what SpectrumAnalyzer::push_frequencies consumes (spectrum_analyzer.rs:48-61: 128 log-spaced
 * bands).  The per-range tables are built on the host and cached until the range set changes. */
SGX_API int sgx_magnitude_in(sgx_ctx *ctx, const float *d_mags, size_t n_columns, const float *h_ranges,
                             uint32_t n_ranges, float *d_out);

/* FrequencySample::magnitude_in (src/fourier/mod.rs:17-21, interpolated_frequency_sample.rs:60-75) over the context's R
 * log-frequency rows (the ranges [edge[py], edge[py+1]) of sgx_bin_edges), for every frame of the hop loop: the column
 * sgx_render_batch colours, as floats.
 *   d_bands [n_out][pairs][R][2] float: (l, r) mean of the interpolated samples; index py = 0 is the LOWEST row (the
 *   order of sgx_bin_edges and sgx_magnitude_in, NOT the image order of sgx_render_batch).
 * Bit-identical to sgx_stft_batch followed by sgx_magnitude_in with ranges (edge[py], edge[py+1]).  A mono stream's rows hold
 * (b, b); with SGX_FLAG_PAIRED_FRAMES as well (frame a of a transform (l, l), frame b (r, r)).
 * first_frame / max_frames / *n_out as sgx_stft_batch.  Stream-ordered and asynchronous; nothing waits on the host. */
SGX_API int sgx_bands_batch(sgx_ctx *ctx, const float *d_pcm, size_t n_samples, size_t first_frame,
                            size_t max_frames, float *d_bands, size_t *n_out);
/* 1: sgx_bands_batch runs one fused kernel from PCM to bands in this context (the palette plays no part); 0: two kernels
 * (the STFT into a bounded workspace, then magnitude_in over the context's own tables); < 0: error */
SGX_API int sgx_bands_fused(const sgx_ctx *ctx);

/* Peak-hold of sgx_bands_batch over groups of `group` consecutive frames: the overview of a long stream, no transient lost.
 *   Frames [first_frame, first_frame + max_frames) that exist: F of them. Column j = 0 .. ceil(F / group) - 1 covers frames
 *   first_frame + [j * group, min((j + 1) * group, F)); the last column may cover fewer.
 *   d_peak [n_out][pairs][R][2] float: per pair, row py (0 = LOWEST, as sgx_bands_batch) and side, the maximum over the column's
 *   frames of the value sgx_bands_batch stores for that frame.  *n_out = number of COLUMNS.
 * group = 1 is sgx_bands_batch.  group = 0: SGX_ERR_INVALID_ARG.  Any group up to SIZE_MAX (one column).
 * The comparison is on float values: which of +0 and -0 is stored is unspecified, as is the output for non-finite PCM.
 * Stream-ordered and asynchronous; device memory beyond the caller's buffers is bounded (the 192 MiB workspace of the
 * two-kernel routes, or 16 KiB * R / 1024 per persistent workgroup) whatever the number of frames. */
SGX_API int sgx_bands_peak_batch(sgx_ctx *ctx, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames,
                                 size_t group, float *d_peak, size_t *n_out);
/* 1: one kernel from PCM to peak columns (plus at most one combine pass over partial columns); 0: the workspace route; < 0: error */
SGX_API int sgx_bands_peak_fused(const sgx_ctx *ctx);

/* ---- Welch-averaged spectra per bin: the mean over groups of frames ------------------------------------------------------------------
 * The standard spectrum estimate (Welch's method: scipy.signal.welch, csd, coherence) at full bin resolution: a noise floor, a long-term
 * average spectrum, and -- from the cross terms -- a transfer function or a coherence.  (The coherence quotient stated at
 * sgx_fbank_cross_batch is identically 1 for one frame and a one-bin band; it means something only after the four terms have been
 * averaged over frames, which is what sgx_csd_batch does.)
 *
 * Frames and columns as sgx_bands_peak_batch: frames [first_frame, first_frame + max_frames) that exist are the F frames of the call;
 * column j = 0 .. ceil(F / group) - 1 covers frames first_frame + [j * group, min((j + 1) * group, F)), n_j of them; the last column may
 * cover fewer.  group = 0: SGX_ERR_INVALID_ARG.  Any group up to SIZE_MAX (one column).  *n_out = number of COLUMNS.
 * Per frame, pair and stored bin the summand x is
 *   psd: x = rn(m * m) per side, m exactly the float32 that sgx_stft_batch stores (the x of a power-2 filterbank);
 *   csd: x0 .. x3 exactly as sgx_fbank_cross_batch defines them from the words sgx_stft_batch_complex stores (every product rounded, one
 *        add or subtract, no contraction).
 * The mean of a column, per bin and component; the order is part of the definition:
 *   1. the column's frames form blocks of 32 consecutive frames counted from the column's first frame (the last block may be shorter); a
 *      block's partial is one chain of float32 adds from +0 in ascending frame order, s = rn(s + x), the add never contracted with the
 *      product;
 *   2. the column's sum S is one chain of float64 adds from +0 over its block partials in ascending order;
 *   3. the output is (float)(S / (double)n_j): one float64 division, rounded once to float32.
 * The block length 32 is fixed here: it does not depend on the device, the compute-unit limit, the route or the chunking.  The output is
 * therefore a pure function of the rows: bit-identical across routes, compute-unit limits, streams, chunk seams and any split of a call
 * at a column boundary (tests/test_gpu_psd.py; the harnesses of every entry point hold these calls too: tests/test_gpu_bounds.py,
 * test_gpu_stream_routes.py, test_gpu_far_offsets.py, test_gpu_channel_counts.py, test_gpu_cu_counts.py), and numpy reproduces it bit for bit without a fused multiply-add (a float32 cumsum along
 * the frames of a block, a float64 cumsum over the blocks: tests/psd_reference.py).  group = 1 gives exactly rn(m * m), or x0 .. x3.
 * Against the float64 mean of the float64 products of the same float32 rows the error is at most 35 * 2^-24 times the mean of the
 * absolute products of the term (1 rounding for the product, 31 for the chain, 1 for the cast, 2 for second-order terms).
 *
 * Scaling.  The rows are scaled 2 / W, so a stationary sinusoid of amplitude A at a bin centre gives psd = (A * S1 / W)^2 at that bin,
 * with S1 = sum of w and S2 = sum of w^2 over w = sgx_window.  With p a psd value (or a csd component):
 *   the one-sided power spectrum, mean square per bin (A^2 / 2 for that sinusoid):   p * W^2 / (2 * S1^2);
 *   the one-sided power spectral density per Hz at sample rate fs:                   p * W^2 / (2 * fs * S2)
 * (scipy's scaling = 'spectrum' and 'density' for a window of W samples zero-padded to nfft = 2W, whose bins k = 1 .. W - 1 the rows hold).
 * No logarithm, no dB, and no division of one output by another: the coherence (out2^2 + out3^2) / (out0 * out1), the transfer function
 * (out2 - i out3) / out0 and their guards against small denominators are the caller's, as for the filterbanks.
 *
 * sgx_psd_batch: d_psd [n_out][pairs][M][2] float, (l, r) per bin; a mono stream holds (v, v) (with SGX_FLAG_PAIRED_FRAMES what the rows hold).
 * sgx_csd_batch: d_csd [n_out][pairs][M][4] float, 16-byte aligned (else SGX_ERR_INVALID_ARG, nothing written); on a mono context
 *   SGX_ERR_UNSUPPORTED (there L = R and the answer is x0, x0, x0, 0).
 * sgx_psd_mags / sgx_csd_spec: the stage alone over rows already on the device, d_mags [n_frames][pairs][M][2] as sgx_stft_batch writes
 *   them, d_spec [n_frames][pairs][M][2][2] as sgx_stft_batch_complex does (16-byte aligned; any channel count: mono rows give
 *   x0 = x1 = x2 and x3 = +0).  Every W the library accepts.  n_frames == 0: *n_out = 0, not an error.
 * Too few samples is *n_out = 0, not an error; a null buffer is SGX_ERR_INVALID_ARG; n_out may be NULL.  Stream-ordered and asynchronous;
 * nothing waits on the host (a grown workspace may, as elsewhere); every kernel of a call goes onto the context's stream.  Device
 * memory beyond the caller's buffers is bounded whatever F and group are: the 192 MiB workspace (rows of a range of frames and one
 * float32 partial row per block of the range) plus one float64 row [pairs][M][4] for a column that spans ranges.
 * sgx_psd_fused / sgx_csd_fused: 1 one kernel from PCM to block partials, 0 the workspace route (the rows of a range of frames by their
 * own route, then a block kernel and a combine kernel over them), < 0 error.  This build answers 0 on every context: no fused mode has been
 * built and measured against the workspace route. */
SGX_API int sgx_psd_batch(sgx_ctx *ctx, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames,
                          size_t group, float *d_psd, size_t *n_out);
SGX_API int sgx_csd_batch(sgx_ctx *ctx, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames,
                          size_t group, float *d_csd, size_t *n_out);
SGX_API int sgx_psd_mags(sgx_ctx *ctx, const float *d_mags, size_t n_frames, size_t group, float *d_psd, size_t *n_out);
SGX_API int sgx_csd_spec(sgx_ctx *ctx, const float *d_spec, size_t n_frames, size_t group, float *d_csd, size_t *n_out);
SGX_API int sgx_psd_fused(const sgx_ctx *ctx);
SGX_API int sgx_csd_fused(const sgx_ctx *ctx);
/* ---- The K strongest spectral maxima per frame: where a row's peaks are and how strong ----------------------------------------------
 * What a tuner, a partial tracker, a sinusoidal model, a landmark fingerprint or a pitch tracker reads off a spectrum (the reference has
 * none: it draws every bin).  No row reaches the caller: 32 * K bytes per frame and side do.
 *
 * Take one frame, pair and side (0 = l, 1 = r).  The row is m[j], j = 0 .. M - 1, exactly the float32 values that sgx_stft_batch stores;
 * element j is bin k = j + 1.  The order below is part of the definition.
 *   Candidate.  An interior j (1 <= j <= M - 2) is a candidate when all three hold: m[j] > m[j-1], m[j] >= m[j+1] and m[j] >= floor.  A
 *     plateau yields its leftmost bin only.  Bins 1 and W - 1 are never candidates: each has a neighbour that is not stored.  Where
 *     M < 3 there are none.
 *   Order.  Candidates are ordered by descending m[j], ties by ascending j; the first K are the result.  The output is therefore a pure
 *     function of the row, bit for bit: independent of route, launch geometry, compute-unit limit, run claim, run weights, stream, chunk
 *     seams and any split of a call (tests/test_gpu_maxima.py; numpy restates it with two masks and a lexsort: tests/maxima_reference.py).
 *   Record.  Each of the K results is four floats, ((float)k, m[j-1], m[j], m[j+1]).  The library applies no interpolation, logarithm
 *     or division: parabolic, log-parabolic or Gaussian refinement of frequency and level is the caller's, from the three values.  Slots
 *     beyond the number of candidates hold (0, 0, 0, 0); k = 0 is never a stored bin.  All K slots are always written.
 *   Arguments.  K from 1 to 64: K = 0 or K > 64 is SGX_ERR_INVALID_ARG.  floor is finite and >= 0, else SGX_ERR_INVALID_ARG.  The output
 *     for non-finite or negative row values (the stage call only) is unspecified.
 * Scaling as the rows': a stationary sinusoid of amplitude A at a bin centre has the centre value A * S1 / W, S1 = sum of sgx_window.
 *
 * sgx_maxima_batch: d_max [n_out][pairs][2][K][4] float, 16-byte aligned (else SGX_ERR_INVALID_ARG, nothing written).  A mono stream
 *   holds the same records on both sides (with SGX_FLAG_PAIRED_FRAMES each side holds what its rows hold).  first_frame, max_frames and
 *   *n_out as sgx_stft_batch: too few samples is *n_out = 0, not an error; a null buffer is SGX_ERR_INVALID_ARG; n_out may be NULL.
 * sgx_maxima_mags: the stage alone over rows already on the device, d_mags [n_columns][pairs][M][2] as sgx_stft_batch writes them, into
 *   d_max [n_columns][pairs][2][K][4].  Every W the library accepts, SGX_FLAG_LARGE_TRANSFORM lengths included.  n_columns == 0: SGX_OK.
 * Stream-ordered and asynchronous; nothing waits on the host (a grown workspace may, as elsewhere); every kernel of a call goes onto the
 * context's stream.  Device memory beyond the caller's buffers is the 192 MiB workspace only: the rows of a chunk of frames by their own
 * route, then one selection kernel over them (a wave per row).  There is no fused mode and no flag. */
SGX_API int sgx_maxima_batch(sgx_ctx *ctx, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames,
                             uint32_t k, float floor, float *d_max, size_t *n_out);
SGX_API int sgx_maxima_mags(sgx_ctx *ctx, const float *d_mags, size_t n_columns, uint32_t k, float floor, float *d_max);
/* ---- The cumulative spectrum per frame: where the running sum of a row crosses a share of its total ------------------------------------
 * Spectral roll-off (the 85 % / 95 % point), the spectral median (50 %), occupied bandwidth (the 0.5 % and 99.5 % points of ITU-R
 * SM.328), the 5 % / 95 % energy edges an auto-ranging display sets its axis by (the reference has none: it draws every bin).  No row
 * reaches the caller: 16 * n_p bytes per frame and side do.
 *
 * Take one frame, pair and side (0 = l, 1 = r).  The row is m[j], j = 0 .. M - 1, exactly the float32 words that sgx_stft_batch stores;
 * element j is bin k = j + 1.  rn() is one round-to-nearest-even float32 operation.  The order below is part of the definition.
 *   Summand.  x[j] = m[j] (power 1) or rn(m[j] * m[j]) (power 2: the x of a power-2 filterbank, never contracted into the add that
 *     follows).  Any other power is SGX_ERR_INVALID_ARG.
 *   Segments.  The row is cut into segments of S = 32 consecutive elements counted from element 0; the last may be short.  Within segment
 *     b the partial is one chain of float32 adds from +0 in ascending order: s[b][i] = rn(s[b][i-1] + x[32 b + i]).
 *   Offsets.  o[0] = +0 and o[b+1] = rn(o[b] + s[b][last i of b]): one chain of float32 adds over the segment totals in ascending order.
 *   Cumulative value.  c[j] = rn(o[b] + s[b][i]) for j = 32 b + i.  The total is T = c[M-1], not a separately formed sum.  For x >= 0, c
 *     never decreases:
 *       rn is monotone, so within a segment s[b][i] = rn(s[b][i-1] + x) >= s[b][i-1] and hence c[32 b + i] >= c[32 b + i - 1];
 *       the last c of segment b is rn(o[b] + s[b][last]), the very operation that forms o[b+1], so it EQUALS o[b+1];
 *       the first c of segment b + 1 is rn(o[b+1] + s[b+1][0]) >= o[b+1].
 *   S = 32 is fixed here.  It does not depend on the device, the route, the launch geometry or M.  In numpy: pad the row to a multiple of
 *     32 with +0 and reshape to [.., 32]; np.cumsum(axis=-1, dtype=float32); np.cumsum of the last column, shifted by one; one add
 *     (tests/rolloff_reference.py).
 *   Threshold.  p[i], i = 0 .. n_p - 1, n_p from 1 to 8, each a float32 in (0, 1], in any order and possibly repeated.  thr = rn(p[i] *
 *     T): one float32 product.  n_p = 0, n_p > 8, or any p that is NaN or outside (0, 1] is SGX_ERR_INVALID_ARG: nothing is written or
 *     enqueued.  h_p is a host array, read before the call returns.
 *   Result.  j* is the smallest j with c[j] >= thr; it exists whenever T > 0, because rn(p * T) <= T = c[M-1].  The record is four
 *     floats, ((float)(j* + 1), c[j* - 1], c[j*], T), with +0 in place of c[-1].  If !(T > 0) -- an all-zero row, or a NaN anywhere in
 *     it -- the record is (0, 0, 0, T); k = 0 is never a stored bin, as in sgx_maxima_*.  Every record is always written.  Rows with
 *     negative values (the stage call only) are unspecified; infinities follow IEEE arithmetic.
 *   The output is therefore a pure function of the row, bit for bit: independent of route, launch geometry, compute-unit limit, run claim,
 *     run weights, stream, chunk seams and any split of a call (tests/test_gpu_rolloff.py).
 * There is no interpolation and no conversion to Hz: k * sample_rate / (2 W) is the caller's, as is the fraction
 * (thr - c[j* - 1]) / (c[j*] - c[j* - 1]).  Scaling as the rows'.
 *
 * sgx_rolloff_batch: d_out [n_out][pairs][2][n_p][4] float, 16-byte aligned (else SGX_ERR_INVALID_ARG, nothing written).  A mono stream
 *   holds the same records on both sides (with SGX_FLAG_PAIRED_FRAMES each side holds what its rows hold).  first_frame, max_frames and
 *   *n_out as sgx_maxima_batch: too few samples is *n_out = 0, not an error; a null buffer or a null h_p is SGX_ERR_INVALID_ARG; n_out
 *   may be NULL.
 * sgx_rolloff_mags: the stage alone over rows already on the device, d_mags [n_columns][pairs][M][2] as sgx_stft_batch writes them, into
 *   d_out [n_columns][pairs][2][n_p][4].  Every W the library accepts, SGX_FLAG_LARGE_TRANSFORM lengths included.  n_columns == 0: SGX_OK.
 * Stream-ordered and asynchronous; nothing waits on the host (a grown workspace may, as elsewhere); every kernel of a call goes onto the
 * context's stream.  Device memory beyond the caller's buffers is the 192 MiB workspace only: the rows of a chunk of frames by their own
 * route, then one kernel over them (a wave per row).  There is no fused mode, no flag and no query for one. */
SGX_API int sgx_rolloff_batch(sgx_ctx *ctx, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames,
                              uint32_t power, const float *h_p, uint32_t n_p, float *d_out, size_t *n_out);
SGX_API int sgx_rolloff_mags(sgx_ctx *ctx, const float *d_mags, size_t n_columns, uint32_t power,
                             const float *h_p, uint32_t n_p, float *d_out);
/* ---- Per-bin order statistics over groups of frames: percentile spectra, the median spectrum, the per-bin minimum ---------------------
 * The level exceeded 90 %, 50 % and 10 % of the time per bin (L90, L50, L10), the median a spectral gate or a noise estimator uses
 * because one click does not move it, the minimum of minimum-statistics noise tracking.  None of them follows from a mean or a maximum.
 * No row reaches the caller: n_q rows per column do.
 *
 * Frames, columns, group, first_frame, max_frames and *n_out exactly as sgx_psd_batch: F frames of the call exist; column j covers frames
 * first_frame + [j * group, min((j + 1) * group, F)) and holds n_j of them, the last column may be short; group = 0 is
 * SGX_ERR_INVALID_ARG; *n_out is the number of columns.
 * Take one column, pair, stored bin and side.  The sample is v[t], t = 0 .. n_j - 1: exactly the float32 words sgx_stft_batch stores for
 * those frames.
 *   Order.  Words are ordered by the key key(u) = u ^ (u >> 31 ? 0xffffffff : 0x80000000) of their bit pattern u, compared as unsigned
 *     integers.  The resulting total order is -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN.  On the engine's own rows (>= +0, or NaN
 *     for non-finite PCM) this is the numeric order with NaN last, i.e. np.sort.
 *   Rank.  q[i] in [0, 1] for i = 0 .. n_q - 1, n_q from 1 to 16; the values may be in any order and may repeat.  The rank is
 *     k_i = (size_t)floor(q[i] * (double)(n_j - 1) + 0.5): one double product, one add, one floor.  That is nearest rank with a half going
 *     up: n_j = 2 and q = 0.5 gives k = 1.  q = 0 is the column's minimum and q = 1 its maximum.  n_q = 0, n_q > 16, or any q that is NaN
 *     or outside [0, 1] is SGX_ERR_INVALID_ARG: nothing is written or enqueued.
 *   Result.  The word of rank k_i in that order, bits unchanged.  There is no interpolation between ranks: a caller who wants it asks for
 *     both neighbours.  The output is therefore a pure function of the rows, bit for bit: independent of route, launch geometry,
 *     compute-unit limit, run claim, run weights, stream, chunk seams and any split of a call at a column boundary
 *     (tests/test_gpu_quantile.py; numpy restates it with a sort along the frame axis: tests/quantile_reference.py).
 *
 * q is a host array, read before the call returns.  d_out is [n_out][n_q][pairs][M][2] float (no alignment beyond float's): every
 * (column, q) is one row in sgx_stft_batch's layout, so sgx_render_mags, sgx_maxima_mags, sgx_fbank_mags and sgx_magnitude_in take a
 * percentile row as they take any other row.  A mono stream holds what its rows hold: (v, v), or with SGX_FLAG_PAIRED_FRAMES each side
 * its own.  Too few samples is *n_out = 0, not an error; a null buffer or a null q is SGX_ERR_INVALID_ARG; n_out may be NULL.
 * sgx_quantile_batch: the rows of a range of whole columns go by their own route into the 192 MiB workspace, then the selection kernel
 *   runs over the range and writes straight into d_out.  A quantile does not decompose, so a column is not carried across ranges: a call
 *   with min(group, F) > sgx_quantile_max_group(ctx) is SGX_ERR_UNSUPPORTED, sgx_last_error names the cap, nothing is written or
 *   enqueued.  Device memory beyond the caller's buffers is the workspace alone, whatever F is.
 * sgx_quantile_max_group: that cap, 192 MiB / the bytes of one frame's rows ([pairs][M][2] floats), at least 1: 12 294 frames at W 2048
 *   with 1 or 2 channels.
 * sgx_quantile_mags: the stage alone over rows already on the device, d_mags [n_frames][pairs][M][2] as sgx_stft_batch writes them.  Any
 *   group up to SIZE_MAX (one column), every W the library accepts, no workspace: also the way out for a caller whose column exceeds the
 *   cap.  n_frames == 0: *n_out = 0 and SGX_OK.
 * Stream-ordered and asynchronous; nothing waits on the host (a grown workspace may, as elsewhere); every kernel of a call goes onto the
 * context's stream.  A column of at most 512 frames is selected in LDS, a longer one where its rows lie (32 passes over them).  There is
 * no fused mode and no flag. */
SGX_API int sgx_quantile_batch(sgx_ctx *ctx, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames,
                               size_t group, const double *q, uint32_t n_q, float *d_out, size_t *n_out);
SGX_API int sgx_quantile_mags(sgx_ctx *ctx, const float *d_mags, size_t n_frames, size_t group,
                              const double *q, uint32_t n_q, float *d_out, size_t *n_out);
SGX_API size_t sgx_quantile_max_group(const sgx_ctx *ctx);
/* ---- filterbanks: weighted sums of bin magnitudes or powers over overlapping filters ---------------------------------------------
 * What a mel, bark or ERB front end, a third-octave analyser, a chroma vector or an A-weighted level is (the reference has none: every
 * reduction there is magnitude_in, an unweighted mean).
 *
 * A filterbank is n_filters sparse rows over the M = W - 1 stored bins.  Element j of a row of sgx_stft_batch is bin k = j + 1 of the
 * 2W-point transform.  Filter f is (first[f], count[f]) plus count[f] float weights, stored consecutively in filter order (CSR);
 * first[f] + count[f] <= M.  Filters may overlap, repeat, come in any order and have count == 0; weights are any finite floats,
 * negative ones included.  power is 1 (magnitude) or 2 (power).  Per frame, pair and side
 *
 *     out[f] = sum_{i < count[f]} w[f][i] * x[first[f] + i],    x[j] = m[j] (power 1) or m[j] * m[j] rounded to float (power 2)
 *
 * with m[j] exactly the float32 that sgx_stft_batch stores for that frame, side and bin.  The order of the sum is part of the definition:
 *   1. 64 partial sums: a[l], l = 0 .. 63, takes the elements i = l, l + 64, l + 128, ... in ascending order as one chain of fused
 *      multiply-adds from +0: a = fma(w[f][i], x[first[f] + i], a), one rounding per element;
 *   2. a balanced binary tree over a[0 .. 63] by halving, float32 adds: for s = 32, 16, 8, 4, 2, 1 in turn a[l] = a[l] + a[l + s] for every
 *      l < s; the sum is a[0].
 * (A wave of 64 lanes per filter on the device: consecutive lanes read consecutive bins and weights, and the tree serves both sides at
 * once; DESIGN.md says what was measured and what was not.)  count == 0 gives exactly +0.0f.  Every kernel that computes a bank runs this order,
 * so the output is a pure function of the frame's row and the bank: bit-identical across routes, sub-ranges, chunk seams,
 * compute-unit limits and streams (tests/test_gpu_fbank.py).  No logarithm, no dB: the output is about 1 KB per frame, and a log
 * over it is the caller's.
 *
 * The handle is `sgx_fbank *`; the prototypes below spell it `void *` (C converts both ways without a cast; pass `(void **)&fb` to
 * sgx_fbank_create) because the checker of the Rust binding maps the header's types by a fixed table (tests/test_rust_binding.py).
 * A bank belongs to its context: destroy it before sgx_destroy(ctx) (a bank that outlives its context answers SGX_ERR_INVALID_ARG).
 * Several banks may live on one context at once. */
typedef struct sgx_fbank sgx_fbank;

/* Validates the bank and uploads its tables.  SGX_ERR_INVALID_ARG for a null array, n_filters == 0 (or above 2^30),
 * first + count > M, a power other than 1 or 2, a non-finite weight, or 2^31 weights and more.  Waits for nothing but its own uploads on
 * the context's stream.  h_weights holds sum(count) floats. */
SGX_API int sgx_fbank_create(sgx_ctx *ctx, uint32_t n_filters, const uint32_t *h_first, const uint32_t *h_count,
                             const float *h_weights, uint32_t power, void **out_fbank);
SGX_API void sgx_fbank_destroy(void *fbank);
/* n_filters, or 0 for null */
SGX_API uint32_t sgx_fbank_filters(const void *fbank);
/* PCM to the bank's sums for every frame of the hop loop.
 *   d_out [n_out][pairs][n_filters][2] float: (l, r) per filter.  A mono stream holds (v, v), as sgx_bands_batch does; with
 *   SGX_FLAG_PAIRED_FRAMES it holds what the rows hold.
 * first_frame / max_frames / *n_out as sgx_bands_batch: too few samples is *n_out = 0, not an error; a null buffer is
 * SGX_ERR_INVALID_ARG.  Stream-ordered and asynchronous; nothing waits on the host.  Device memory beyond the caller's buffers is
 * bounded whatever the number of frames (none on the fused route, the 192 MiB workspace of the two-kernel routes otherwise). */
SGX_API int sgx_fbank_batch(void *fbank, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames,
                            float *d_out, size_t *n_out);
/* The stage alone, from rows already on the device (as sgx_render_mags is to sgx_render_batch):
 *   d_mags [n_columns][M][2] -> d_out [n_columns][n_filters][2].  Every W the library accepts, every bank. */
SGX_API int sgx_fbank_mags(void *fbank, const float *d_mags, size_t n_columns, float *d_out);
/* 1: sgx_fbank_batch runs one kernel from PCM to sums for this bank on its context; 0: the workspace route (the rows of a chunk of
 * frames by their own route, then the stage kernel); < 0: error.
 * One kernel: W = 2048 with 1, 2 or 2k channels (the 4096-point kernels; any hop), without SGX_FLAG_NO_FUSED_RENDER,
 * SGX_FLAG_PAIRED_FRAMES, SGX_FLAG_COMPLEX_MONO or SGX_FLAG_FORCE_GENERIC, for banks of at most 1024 filters and 16384 weights (a 128-
 * or 256-filter mel bank has about 4000).  Every other window, flag and bank: the workspace route.  Same bits either way. */
SGX_API int sgx_fbank_fused(const void *fbank);

/* The cross sums of a bank: per band what a stereo analyser needs of an (l, r) pair, with the phase that magnitudes lose.
 * For a bank on a context with at least two channels, per frame, (l, r) pair and stored bin j take a = L.re, b = L.im, c = R.re,
 * d = R.im: exactly the float32 words that sgx_stft_batch_complex stores for that frame, pair and bin.  Then
 *
 *     x0 = rn(rn(a * a) + rn(b * b))      |L|^2
 *     x1 = rn(rn(c * c) + rn(d * d))      |R|^2
 *     x2 = rn(rn(a * c) + rn(b * d))      Re L conj R
 *     x3 = rn(rn(b * c) - rn(a * d))      Im L conj R
 *
 * every product rounded to float32, then the sum or difference rounded once: no contraction into a fused multiply-add.  Bitwise-equal L
 * and R therefore give x0 = x1 = x2 and x3 = +0 exactly, and float32 arithmetic on the host reproduces x bit for bit.  The output is
 *
 *     out[f][q] = sum_{i < count[f]} w[f][i] * x_q[first[f] + i],    q = 0 .. 3
 *
 * summed in the order defined above for sgx_fbank_batch (the 64 chains from +0, then the tree by halving).  The bank's power plays
 * no part.  An empty filter gives four +0.0f.  The output is a pure function of the frame's complex row and the bank: bit-identical across
 * routes, sub-ranges, chunk seams, compute-unit limits and streams (tests/test_gpu_fbank_cross.py).
 * What a caller derives from the four sums of a band (none of it is computed here; the division by small band energies is the caller's to guard):
 *   the inter-channel phase is atan2(out3, out2);
 *   the correlation is out2 / sqrt(out0 * out1);
 *   the coherence is (out2 * out2 + out3 * out3) / (out0 * out1);
 *   the mid and side energies are out0 + out1 + 2 * out2 and out0 + out1 - 2 * out2.
 *
 * sgx_fbank_cross_batch: PCM to the four sums for every frame of the hop loop.
 *   d_out [n_out][pairs][n_filters][4] float, 16-byte aligned.
 * first_frame / max_frames / *n_out as sgx_fbank_batch: too few samples is *n_out = 0, not an error; a null buffer is
 * SGX_ERR_INVALID_ARG; a bank whose context is gone answers SGX_ERR_INVALID_ARG.  On a mono context: SGX_ERR_UNSUPPORTED (there L = R
 * and the answer is x0, x0, x0, 0).  Stream-ordered and asynchronous; nothing waits on the host.  Device memory beyond the caller's
 * buffers is bounded as for sgx_fbank_batch (the complex rows take 16 B per bin: a chunk of the workspace route holds half as many frames). */
SGX_API int sgx_fbank_cross_batch(void *fbank, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames,
                                  float *d_out, size_t *n_out);
/* The stage alone: d_spec [n_columns][M][2][2], what sgx_stft_batch_complex writes -> d_out [n_columns][n_filters][4] (both 16-byte
 * aligned).  Every W the library accepts, every bank, any channel count: mono rows are served like any other. */
SGX_API int sgx_fbank_cross_spec(void *fbank, const float *d_spec, size_t n_columns, float *d_out);
/* 1: sgx_fbank_cross_batch runs one kernel from PCM to sums for this bank on its context; 0: the workspace route (the complex rows of a
 * chunk of frames by their own route, then the stage kernel), and every mono context; < 0: error.
 * One kernel: W = 2048 with 2 or 2k channels (any hop), without SGX_FLAG_NO_FUSED_RENDER or SGX_FLAG_FORCE_GENERIC, for banks within
 * the size sgx_fbank_fused states.  Same bits either way. */
SGX_API int sgx_fbank_cross_fused(const void *fbank);

/* The flux of a bank: per band how much of the spectrum rose and how much fell against an earlier frame -- what an onset detector, a beat
 * tracker, a transient / steady-state splitter or a scene-change trigger reads off a spectrogram.  It is the one reduction here that
 * compares a frame with another one, and a caller cannot get it from sgx_fbank_batch: the rectification happens per bin, before the
 * band sum, so a rising partial and a falling one in the same band do not cancel.
 * Take a bank and a lag from 1 to 64.  Frame t is the absolute frame index of the hop loop (sgx_flux_batch) or the row index in
 * d_mags (sgx_flux_mags).  Per frame, pair, side and stored bin j
 *
 *     x_t[j]  = m (power 1) or rn(m * m) (power 2)      m exactly the float32 that sgx_stft_batch stores: the x of sgx_fbank_batch
 *     d[j]    = rn(x_t[j] - x_{t - lag}[j])              one float32 subtract, never contracted with the square
 *     rise[j] = d < 0 ? +0 : d
 *     fall[j] = d > 0 ? +0 : rn(+0 - d)
 *
 * Equal words give (+0, +0), never -0; a NaN in either row gives NaN in both.  Per filter f the record is four sums,
 *
 *     out[f] = (rise_l, rise_r, fall_l, fall_r),    each sum_{i < count[f]} w[f][i] * e[first[f] + i]
 *
 * in the order defined above for sgx_fbank_batch (the 64 chains from +0, then the tree by halving); count == 0 gives four +0.0f.  A frame
 * with t < lag has no predecessor: its record is (+0, +0, +0, +0) for every filter, as the onset functions of librosa and madmom leave
 * their first frames.  The output is a pure function of the two rows and the bank, bit for bit: independent of route, launch geometry,
 * compute-unit limit, run claim, run weights, stream, range seams and any split of a call (tests/test_gpu_fbank_flux.py; numpy
 * restates it: tests/flux_reference.py).
 * On finite rows rise - fall telescopes (it is the difference of two sgx_fbank_batch columns up to rounding), rise + fall is the weighted
 * L1 distance of the two rows, and rise of a one-filter all-ones bank is the classic full-band spectral flux.
 * What is not here: no logarithm or compression before the difference (the device's logarithm is not reproducible on the host:
 * log-flux is a later call), no normalisation, no peak picking.  For infinite row values the arithmetic is IEEE's, but the payload of a
 * resulting NaN is unspecified.  There is no fused mode, no flag and no query for one.
 * The three calls take a bank (the first argument is an sgx_fbank handle) and are named sgx_flux_*, as sgx_maxima_* and
 * sgx_quantile_* carry their own prefix: the names sgx_fbank_* of the library's tables are the bank's own sums and its handle.
 *
 * sgx_flux_batch: PCM to the records of every frame of the hop loop.
 *   d_out [n_out][pairs][n_filters][4] float, 16-byte aligned (else SGX_ERR_INVALID_ARG, nothing written).  A mono stream holds (v, v),
 *   so rise_l = rise_r; with SGX_FLAG_PAIRED_FRAMES each side is differenced against its own side.
 * first_frame / max_frames / *n_out as sgx_fbank_batch: too few samples is *n_out = 0, not an error; a null buffer is
 * SGX_ERR_INVALID_ARG; n_out may be NULL.  The call reads frame first_frame - lag out of the PCM itself: a call with first_frame >= lag
 * has no zero records, and any split of a call concatenates to the whole call.  lag == 0 or lag > 64 is SGX_ERR_INVALID_ARG, nothing
 * written or enqueued.  Stream-ordered and asynchronous; nothing waits on the host; every kernel goes onto the context's stream.
 * Device memory beyond the caller's buffers is the 192 MiB workspace alone: every range of the call puts the rows of its frames and of
 * the min(lag, first frame of the range) frames before them into it by the rows' own route, then one stage kernel writes the range's
 * records.  The head rows of a range are recomputed, not carried.
 * sgx_flux_max_lag: min(64, floor(192 MiB / bytes of one frame's rows) - 1), 0 where fewer than two frames' rows fit, 0 for a
 * null bank.  It is 64 on every in-LDS length and 23 at W = 2^20 with two channels.  sgx_flux_batch with lag above it is
 * SGX_ERR_UNSUPPORTED: sgx_last_error names the cap and points to sgx_flux_mags; nothing is written or enqueued.
 * sgx_flux_mags: the stage alone over rows already on the device, d_mags [n_frames][pairs][M][2] as sgx_stft_batch writes them
 * (frames, not flattened columns: the predecessor of (t, pair p) is (t - lag, pair p)) -> d_out [n_frames][pairs][n_filters][4].  Any
 * lag from 1 to 64 at every W the library accepts; n_frames == 0 is SGX_OK. */
SGX_API int sgx_flux_batch(void *fbank, const float *d_pcm, size_t n_samples, size_t first_frame, size_t max_frames,
                                 uint32_t lag, float *d_out, size_t *n_out);
SGX_API int sgx_flux_mags(void *fbank, const float *d_mags, size_t n_frames, uint32_t lag, float *d_out);
SGX_API uint32_t sgx_flux_max_lag(const void *fbank);

/* The triangular mel bank as sgx_fbank_create takes it.  Host only: no context, no device.
 * Over the TRUE bin frequencies f_k = k * sample_rate / (2W), k = 1 .. W - 1 (stored element j = k - 1) -- deliberately not the axis of
 * the reference's index_of (quirk Q2), which a caller comparing with librosa / torchaudio / HTK would not expect.
 *   n_mels + 2 points equally spaced in mel between f_min and f_max; filter m spans (f_lo, f_c, f_hi) = points m, m + 1, m + 2:
 *   w = max(0, min((f - f_lo) / (f_c - f_lo), (f_hi - f) / (f_hi - f_c))), times 2 / (f_hi - f_lo) with SGX_MEL_NORM_SLANEY;
 *   computed in double, rounded once to float.  A filter's support is its bins with w > 0 (none: count = 0, first = 0).
 *   scale: SGX_MEL_HTK, mel = 2595 log10(1 + f / 700); SGX_MEL_SLANEY, linear below 1 kHz at 200 / 3 Hz per mel, logarithmic above with
 *   step ln(6.4) / 27.
 * h_first [n_mels], h_count [n_mels], h_weights [*n_weights]; with all three null only *n_weights is returned, for sizing.
 * SGX_ERR_INVALID_ARG: n_mels == 0, f_min < 0, f_max <= f_min, f_max > sample_rate / 2, window_samples < 2, an unknown scale or norm,
 * a null n_weights, or only some of the arrays null. */
#define SGX_MEL_HTK 0u
#define SGX_MEL_SLANEY 1u
#define SGX_MEL_NORM_NONE 0u
#define SGX_MEL_NORM_SLANEY 1u
SGX_API int sgx_mel_weights(double sample_rate, uint32_t window_samples, uint32_t n_mels, double f_min, double f_max, uint32_t scale,
                            uint32_t norm, uint32_t *h_first, uint32_t *h_count, float *h_weights, size_t *n_weights);

/* ColorScheme::color_for (colorscheme.rs:55-71) + put_pixel's row order over columns of bands: d_bands [n_columns][R][2] (py = 0 lowest)
 * -> d_rgba [n_columns][R][4], image order (row 0 = highest frequency), the context's current colour scheme (mono or diverging). */
SGX_API int sgx_render_bands(sgx_ctx *ctx, const float *d_bands, size_t n_columns, uint8_t *d_rgba);

/* SpectrumAnalyzer::push_frequencies (spectrum_analyzer.rs:46-68) for ONE column of magnitudes
 * d_column [M][2] on the device: the n_bars (the widget has 128) adjacent bands of
 * log_space(32, max(sample_rate / 2, 22050), n_bars + 1, 10) (:20-36,52-58; f32 logf / powf on the host),
 * magnitude_in of each band on the device, then on the host level = (10 log10f(hypotf(l, r) + 1e-7) + 70) / 60
 * as f64 and h_levels[i] = max(level, h_levels[i] * 0.99) (:61-66: the bars decay by 1 % per pushed
 * column; a fresh widget starts every bar at 0.3, :92).  h_levels [n_bars] double, in/out.  Synchronous. */
SGX_API int sgx_spectrum_levels(sgx_ctx *ctx, const float *d_column, uint32_t n_bars, double *h_levels);

/* ---- live capture: the ring between the audio callback and the GUI tick -------------------- */

/* The reference's producer is the cpal input callback pushing (l, r) pairs into a 4096-entry
 * ringbuf::HeapRb (audio_input_list_model.rs:30,63-72); its consumer is the GTK tick running the
 * hop loop over that ring (audio_transform.rs:34-42 from gpu_spectrogram.rs:255-262 /
 * simple_spectrogram.rs:136-139).  sgx_live keeps the CONSUMED side of that ring on the device:
 * a push lands in a pinned host ring; a tick sends only the samples that arrived since the last
 * tick (one async copy, two when the ring wraps), runs every complete frame through one launch
 * of the context's transform (context channels must be 2: the ring holds (l, r) pairs), returns
 * the results to the host and keeps the W - H overlap resident.  One producer thread and one
 * consumer thread may run concurrently (lock-free single-producer / single-consumer, as HeapRb). */
typedef struct sgx_live sgx_live;

#define SGX_LIVE_MAGS 0     /* float [frames][M][2]: what AudioStreamTransform::process yields        */
#define SGX_LIVE_MAGS_F16 1 /* half  [frames][M][2]: rows of the F16F16 ring (gpu_spectrogram.rs:268) */
#define SGX_LIVE_RGBA 2     /* uint8 [frames][R][4]: columns of SimpleSpectrogram::snapshot           */
#define SGX_LIVE_BANDS 3    /* float [frames][R][2]: the columns of magnitude_in over the context's rows */

#define SGX_LIVE_REFERENCE_SKIP 1u /* also skip H samples on the terminating short read, exactly as
                                      audio_transform.rs:37-41 does (it drops up to H samples per tick);
                                      default: frames are t*H exact */

/* capacity_pairs: ring size in (l, r) pairs (the reference: 4096); must hold at least one window.
 * A ring belongs to its context: destroy it before sgx_destroy(ctx). */
SGX_API int sgx_live_create(sgx_ctx *ctx, size_t capacity_pairs, uint32_t flags, sgx_live **out);
SGX_API void sgx_live_destroy(sgx_live *live);
/* The cpal callback (audio_input_list_model.rs:63-75): h_samples holds n_values floats, interleaved by
 * `channels`.  1 channel -> (s, s) pairs, 2 -> (l, r) pairs, anything else -> SGX_ERR_UNSUPPORTED (the
 * reference prints "N-channel input not supported!").  Pairs that do not fit are dropped (push_iter).
 * Returns the number of pairs accepted, or a negative sgx_status.  Producer thread. */
SGX_API long long sgx_live_push(sgx_live *live, const float *h_samples, size_t n_values, uint32_t channels);
/* HeapRb::occupied_len: pairs pushed and not yet skipped */
SGX_API size_t sgx_live_occupied(const sgx_live *live);
/* One GUI tick (audio_transform.rs:34-42): every complete frame of the ring, at most max_frames, in the
 * format `what`, into the HOST buffer h_out; the ring advances by H per frame.  *n_frames may be 0 (not
 * an error).  Synchronous: returns when h_out is filled.  Consumer thread. */
SGX_API int sgx_live_tick(sgx_live *live, int what, void *h_out, size_t max_frames, size_t *n_frames);

/* ---- ColorScheme ---------------------------------------------------------------------------- */

/* ColorScheme::new_mono(gradient, name) / new_stereo(gradient, background, name)
 * (colorscheme.rs:24-39).  h_rgb: [n][3] table standing in for colorous' Gradient; stereo != 0
 * selects the diverging branch of color_for (colorscheme.rs:63-66: colour from the left/right
 * balance, alpha from the bounded dB magnitude). */
SGX_API int sgx_set_gradient(sgx_ctx *ctx, const uint8_t *h_rgb, uint32_t n, int stereo);
/* The same two constructors for ANY continuous gradient: `eval` stands in for colorous'
 * Gradient::eval_continuous(t) (colorscheme.rs:43-69) -- the integrator passes a thunk around colorous
 * itself, so spline (ColorBrewer) and closed-form (Turbo, Cividis, Cubehelix ...) gradients are rendered
 * with exactly the bytes colorous returns and no table of this library is involved.  `eval` is called
 * on the host, only inside this function (and sgx_lookup_table), never during a launch: the colour
 * as a function of the bounded dB value (or of the left/right balance) is a step function of bytes; its
 * switch points are located by bisection over float (double) bit patterns and uploaded as thresholds. */
typedef void (*sgx_gradient_fn)(double t, uint8_t rgb_out[3], void *user);
SGX_API int sgx_set_gradient_fn(sgx_ctx *ctx, sgx_gradient_fn eval, void *user, int stereo);
/* "viridis" | "magma" | "inferno" | "plasma" (colorscheme.rs:131-139) */
SGX_API int sgx_set_builtin_gradient(sgx_ctx *ctx, const char *name);
/* ColorScheme::new_mono / new_stereo (colorscheme.rs:24-39) with one of the gradients this library can evaluate itself:
 * "viridis" "magma" "inferno" "plasma" (256-entry ramps) and colorous' ColorBrewer B-spline gradients "red_yellow_blue"
 * "red_blue" "spectral" "red_yellow_green" "pink_green" "purple_orange" "purple_green" "brown_green" "red_grey" "reds"
 * "blues" "greens" "greys" "oranges" "purples" (continuous: anchors from ColorBrewer, d3's interpolateRgbBasis),
 * "turbo" "cividis" (d3's quintics) and "cubehelix" "cool" "warm" (d3's interpolateCubehelixLong, bytes by truncation as
 * the reference's screenshots/colorscheme-cool.png shows colorous doing) -- every one of the 19 entries of
 * default_color_schemes (colorscheme.rs:125-151).  [third-party]: colorous is not vendored; what the reference's four
 * screenshots pin (the values of the Viridis / Magma / Plasma tables, Cool's curve and byte rule) is tests/test_host_logic.py.
 * stereo != 0: the diverging rule of colorscheme.rs:63-66 (colour from l / (|l| + |r|), alpha from the level). */
SGX_API int sgx_set_builtin_scheme(sgx_ctx *ctx, const char *name, int stereo);
/* eval_continuous(t) of a built-in gradient on the host (ColorScheme::background / foreground, colorscheme.rs:41-53) */
SGX_API int sgx_builtin_gradient_eval(const char *name, double t, uint8_t rgb_out[3]);
SGX_API int sgx_builtin_gradient(const char *name, uint8_t *h_rgb_out /* [256][3] */);

/* ColorScheme::lookup_table(resolution) (colorscheme.rs:73-92): h_out [res][res][4] float,
 * the palette texture of the GLSL path (gpu_spectrogram.rs:233-238). */
SGX_API int sgx_lookup_table(sgx_ctx *ctx, uint32_t resolution, float *h_out);

/* ---- introspection (tests, tooling) --------------------------------------------------------- */

/* R+1 row edges in Hz as f32: LogCoordf64::unmap(p, (0, R)) for p = 0..R
 * (log_scaling.rs:114-119; simple_spectrogram.rs:142-145). */
SGX_API int sgx_bin_edges(const sgx_ctx *ctx, float *h_out);
/* per-row sample counts of magnitude_in (interpolated_frequency_sample.rs:63-64): h_out [R] */
SGX_API int sgx_row_sample_counts(const sgx_ctx *ctx, uint32_t *h_out);
/* the Hann table (fft.rs:61): h_out [W] */
SGX_API int sgx_window(const sgx_ctx *ctx, float *h_out);

/* ---- the default widget's variant: F16F16 ring texture + fragment program ---------------------
 * GPUSpectrogram keeps its frames as rows of a VIEWPORT_FRAMES x (W - 1) F16F16 texture used as a ring
 * (gpu_spectrogram.rs:21,67,218-226) and draws it with a fragment program (:150-186: log-frequency lookup, dB, pan,
 * 32 x 32 palette texture).  sgx_view is that texture on the device and that program as a kernel.  Not a parity target:
 * OpenGL leaves the filtering arithmetic to the implementation; the program text and the sampler state are restated
 * (GL_LINEAR = two nearest texels per axis weighted by the fractional part, REPEAT for the ring, CLAMP for the
 * palette; float32; the shader's hard-coded 32 / 22030 Hz, quirk Q9).  Destroy views before sgx_destroy(ctx). */
typedef struct sgx_view sgx_view;
SGX_API int sgx_view_create(sgx_ctx *ctx, uint32_t viewport_frames /* 2048 */, sgx_view **out);
SGX_API void sgx_view_destroy(sgx_view *view);
/* The upload loop of render() (gpu_spectrogram.rs:255-275): append n_rows rows of [M][2] half -- a DEVICE pointer,
 * e.g. what sgx_stft_batch_f16 wrote -- at the ring's offset, wrapping at its height; the new offset is returned. */
SGX_API int sgx_view_write_rows(sgx_view *view, const void *d_rows_f16, size_t n_rows, uint32_t *offset_out);
SGX_API uint32_t sgx_view_offset(const sgx_view *view);
/* One GUI tick of the default widget (gpu_spectrogram.rs:255-275: `for frame in fft.process()` -> fft_texture.write): every
 * complete frame of the live ring, at most max_frames, is transformed and its half-pair row appended to the view's ring texture,
 * device to device -- the only host traffic of the tick is the new samples going up.  `view` must belong to the ring's context: a view of another
 * (or of a destroyed) context is refused with SGX_ERR_INVALID_ARG before anything is uploaded, transformed or skipped. */
SGX_API int sgx_live_tick_view(sgx_live *live, sgx_view *view, size_t max_frames, size_t *n_frames);
/* The fragment program over a width x height viewport: d_rgba_f32 [height][width][4] float = f_color per fragment, row 0
 * at the BOTTOM (GL).  The palette texture is ColorScheme::lookup_table(32) of the context's current colour scheme,
 * min_db / max_db the context's. */
SGX_API int sgx_view_draw(sgx_view *view, uint32_t width, uint32_t height, float *d_rgba_f32);

/* ---- the CPU pixel path's image ring --------------------------------------------------------------
 * SimpleSpectrogram keeps a row-major width x height RGBA Pixbuf (simple_spectrogram.rs:89-94; 1024 x 1024), writes every new
 * frame as one pixel column at x = offset, image row height - 1 - py (:140-161), advances offset = (px + 1) % width (:164) and
 * composes the scrolling picture from the sub-images [offset, width) and [0, offset) (:181-209).  sgx_image is that Pixbuf on
 * the device: [height][width][4] bytes, rowstride 4 * width, height = the context's rows.  Destroy images before sgx_destroy(ctx)
 * (an image that outlives its context answers SGX_ERR_INVALID_ARG). */
typedef struct sgx_image sgx_image;
SGX_API int sgx_image_create(sgx_ctx *ctx, uint32_t width /* 1024 */, sgx_image **out);
SGX_API void sgx_image_destroy(sgx_image *image);
/* The pixel loop's put_pixel + offset update for n columns at once (:140-164): d_rgba [n][rows][4] -- a DEVICE pointer, e.g. what
 * sgx_render_batch wrote -- column i lands at x = (offset + i) % width, offset advances by n (mod width); with n > width the ring
 * laps itself and the later columns win, as written one by one.  The new offset is returned. */
SGX_API int sgx_image_write_columns(sgx_image *image, const uint8_t *d_rgba, size_t n_columns, uint32_t *offset_out);
SGX_API uint32_t sgx_image_offset(const sgx_image *image);
/* the Pixbuf's get_width() / get_height() (:89-94): width as created, height = the context's rows -- what a caller sizes the
 * buffer of sgx_image_read with (0 for a null image) */
SGX_API uint32_t sgx_image_width(const sgx_image *image);
SGX_API uint32_t sgx_image_height(const sgx_image *image);
/* One GUI tick of SimpleSpectrogram::snapshot (:136-165: `for frequency_sample in fft.process()` -> put_pixel): every complete frame
 * of the live ring, at most max_frames, becomes a pixel column of the image, device to device. */
SGX_API int sgx_live_tick_image(sgx_live *live, sgx_image *image, size_t max_frames, size_t *n_frames);
/* d_out [height][width][4]: the buffer as it lies (scrolled = 0), or the composed picture -- columns [offset, width) followed by
 * [0, offset) (:181-209; scrolled != 0). */
SGX_API int sgx_image_read(sgx_image *image, int scrolled, uint8_t *d_out);
/* the device buffer itself ([height][width][4], valid until sgx_image_destroy; ordered on the context's stream) */
SGX_API const uint8_t *sgx_image_pixels(const sgx_image *image);

/* ---- synthetic input + verification helpers (bench / multi-GPU harness, not reference API) -- */

/* Counter-based white noise, identical on CPU and GPU:
 * x[n] = ((lowbias32((seed + hi32(n) * 0x9E3779B9) ^ lo32(n)) >> 8) * 2^-23) - 1.
 * Writes d_out[i * channels + c] for sample index first + i and channel c (seed + c). */
SGX_API int sgx_synth_white_noise(sgx_ctx *ctx, float *d_out, uint64_t first, size_t n_samples,
                                  uint32_t channels, uint32_t seed);
/* 64-bit order-independent checksum (sum of a 64-bit mix of each (index, 32-bit word)) of a device buffer of
 * n_bytes (multiple of 4), with word indices starting at base_word: equal for any sharding of
 * the same bytes.  Synchronous. */
SGX_API int sgx_checksum(sgx_ctx *ctx, const void *d_buf, size_t n_bytes, uint64_t base_word, uint64_t *h_out);
/* The same sum, ADDED (mod 2^64) into a caller-owned device accumulator *d_acc and asynchronous on the context's
 * stream: the root of a sharded run consumes every gathered piece of pixel columns this way without a host
 * round trip per piece (1e8 columns are 410 GB: the image is never materialised).  Zero *d_acc first. */
SGX_API int sgx_checksum_add(sgx_ctx *ctx, const void *d_buf, size_t n_bytes, uint64_t base_word, uint64_t *d_acc);

#ifdef __cplusplus
}
#endif
#endif /* SGX_H */
