// src/fourier/sgx_sys.rs -- FFI declarations, a mirror of include/sgx.h (the parts the reference's path needs)
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
pub struct SgxConfig {
    pub struct_size: u32,
    pub sample_rate: f32, pub period: f32, pub stride: f32,
    pub window_samples: u32, pub hop_samples: u32, pub channels: u32, pub rows: u32,
    pub f_min: f64, pub f_max: f64,
    pub min_db: f32, pub max_db: f32,
    pub interp: u32, pub lut_index_mode: u32,
    pub device: i32, pub flags: u32,
}
#[repr(C)] pub struct SgxCtx { _private: [u8; 0] }
#[repr(C)] pub struct SgxFbank { _private: [u8; 0] }   // a filterbank's tables on the device (the header spells the handle `void *`)

extern "C" {
    pub fn sgx_config_init(cfg: *mut SgxConfig) -> c_int;
    pub fn sgx_create(cfg: *const SgxConfig, out: *mut *mut SgxCtx) -> c_int;
    pub fn sgx_destroy(ctx: *mut SgxCtx);
    pub fn sgx_last_error(ctx: *const SgxCtx) -> *const c_char;
    pub fn sgx_num_frames(ctx: *const SgxCtx, n_samples: usize) -> usize;
    pub fn sgx_process_one(ctx: *mut SgxCtx, h_lr: *const f32, n_avail: usize, h_out: *mut f32) -> c_int;
    pub fn sgx_stft_batch(ctx: *mut SgxCtx, d_pcm: *const f32, n_samples: usize, first_frame: usize,
                          max_frames: usize, d_mags: *mut f32, n_out: *mut usize) -> c_int;
    pub fn sgx_stft_batch_f16(ctx: *mut SgxCtx, d_pcm: *const f32, n_samples: usize, first_frame: usize,
                              max_frames: usize, d_mags_f16: *mut c_void, n_out: *mut usize) -> c_int;   // F16F16 ring rows
    pub fn sgx_stft_batch_complex(ctx: *mut SgxCtx, d_pcm: *const f32, n_samples: usize, first_frame: usize,
                                  max_frames: usize, d_spec: *mut f32, n_out: *mut usize) -> c_int;   // (L, R) complex spectra
    pub fn sgx_istft_batch(ctx: *mut SgxCtx, d_spec: *const f32, n_frames: usize, first_sample: usize,
                           max_samples: usize, d_pcm: *mut f32, n_out: *mut usize) -> c_int;   // PCM from (L, R) spectra
    pub fn sgx_istft_supported(ctx: *const SgxCtx) -> c_int;
    pub fn sgx_render_batch(ctx: *mut SgxCtx, d_pcm: *const f32, n_samples: usize, first_frame: usize,
                            max_frames: usize, d_rgba: *mut u8, n_out: *mut usize) -> c_int;
    pub fn sgx_magnitude_in(ctx: *mut SgxCtx, d_mags: *const f32, n_columns: usize, h_ranges: *const f32,
                            n_ranges: u32, d_out: *mut f32) -> c_int;              // FrequencySample::magnitude_in
    pub fn sgx_bands_batch(ctx: *mut SgxCtx, d_pcm: *const f32, n_samples: usize, first_frame: usize,
                           max_frames: usize, d_bands: *mut f32, n_out: *mut usize) -> c_int;   // magnitude_in over the context's rows
    pub fn sgx_bands_fused(ctx: *const SgxCtx) -> c_int;
    pub fn sgx_bands_peak_batch(ctx: *mut SgxCtx, d_pcm: *const f32, n_samples: usize, first_frame: usize, max_frames: usize,
                                group: usize, d_peak: *mut f32, n_out: *mut usize) -> c_int;   // peak-hold of the bands over groups of frames
    pub fn sgx_bands_peak_fused(ctx: *const SgxCtx) -> c_int;
    // Welch-averaged spectra per bin: the mean over groups of frames of |X|^2 (psd) and of the four (L, R) products (csd)
    pub fn sgx_psd_batch(ctx: *mut SgxCtx, d_pcm: *const f32, n_samples: usize, first_frame: usize, max_frames: usize,
                         group: usize, d_psd: *mut f32, n_out: *mut usize) -> c_int;   // PCM -> [columns][pairs][M][2]
    pub fn sgx_csd_batch(ctx: *mut SgxCtx, d_pcm: *const f32, n_samples: usize, first_frame: usize, max_frames: usize,
                         group: usize, d_csd: *mut f32, n_out: *mut usize) -> c_int;   // PCM -> [columns][pairs][M][4]
    pub fn sgx_psd_mags(ctx: *mut SgxCtx, d_mags: *const f32, n_frames: usize, group: usize, d_psd: *mut f32,
                        n_out: *mut usize) -> c_int;   // the stage alone, from magnitude rows
    pub fn sgx_csd_spec(ctx: *mut SgxCtx, d_spec: *const f32, n_frames: usize, group: usize, d_csd: *mut f32,
                        n_out: *mut usize) -> c_int;   // the stage alone, from complex rows
    pub fn sgx_psd_fused(ctx: *const SgxCtx) -> c_int;
    pub fn sgx_csd_fused(ctx: *const SgxCtx) -> c_int;
    // the K strongest spectral maxima per frame, pair and side: (bin, m[bin - 1], m[bin], m[bin + 1]) each, strongest first
    pub fn sgx_maxima_batch(ctx: *mut SgxCtx, d_pcm: *const f32, n_samples: usize, first_frame: usize, max_frames: usize,
                            k: u32, floor: f32, d_max: *mut f32, n_out: *mut usize) -> c_int;   // PCM -> [frames][pairs][2][K][4]
    pub fn sgx_maxima_mags(ctx: *mut SgxCtx, d_mags: *const f32, n_columns: usize, k: u32, floor: f32,
                           d_max: *mut f32) -> c_int;   // the stage alone, from magnitude rows
    // the cumulative spectrum per frame, pair and side: per share p, (bin, c[bin - 1], c[bin], total) where the running sum reaches p * total
    pub fn sgx_rolloff_batch(ctx: *mut SgxCtx, d_pcm: *const f32, n_samples: usize, first_frame: usize, max_frames: usize,
                             power: u32, h_p: *const f32, n_p: u32, d_out: *mut f32,
                             n_out: *mut usize) -> c_int;   // PCM -> [frames][pairs][2][n_p][4]
    pub fn sgx_rolloff_mags(ctx: *mut SgxCtx, d_mags: *const f32, n_columns: usize, power: u32, h_p: *const f32, n_p: u32,
                            d_out: *mut f32) -> c_int;   // the stage alone, from magnitude rows
    // per-bin order statistics over groups of frames: the word of rank floor(q * (n - 1) + 0.5) of every column, bin and side, NaN last
    pub fn sgx_quantile_batch(ctx: *mut SgxCtx, d_pcm: *const f32, n_samples: usize, first_frame: usize, max_frames: usize,
                              group: usize, q: *const f64, n_q: u32, d_out: *mut f32,
                              n_out: *mut usize) -> c_int;   // PCM -> [columns][n_q][pairs][M][2]
    pub fn sgx_quantile_mags(ctx: *mut SgxCtx, d_mags: *const f32, n_frames: usize, group: usize, q: *const f64, n_q: u32,
                             d_out: *mut f32, n_out: *mut usize) -> c_int;   // the stage alone, from magnitude rows; any group
    pub fn sgx_quantile_max_group(ctx: *const SgxCtx) -> usize;   // the longest column sgx_quantile_batch takes
    pub fn sgx_render_bands(ctx: *mut SgxCtx, d_bands: *const f32, n_columns: usize, d_rgba: *mut u8) -> c_int;   // color_for over band columns
    // filterbanks: weighted sums of bin magnitudes or powers over sparse filters (mel, bark, third octaves ...)
    pub fn sgx_fbank_create(ctx: *mut SgxCtx, n_filters: u32, h_first: *const u32, h_count: *const u32, h_weights: *const f32,
                            power: u32, out_fbank: *mut *mut SgxFbank) -> c_int;
    pub fn sgx_fbank_destroy(fbank: *mut SgxFbank);
    pub fn sgx_fbank_filters(fbank: *const SgxFbank) -> u32;
    pub fn sgx_fbank_batch(fbank: *mut SgxFbank, d_pcm: *const f32, n_samples: usize, first_frame: usize, max_frames: usize,
                           d_out: *mut f32, n_out: *mut usize) -> c_int;   // PCM -> [frames][pairs][n_filters][2]
    pub fn sgx_fbank_mags(fbank: *mut SgxFbank, d_mags: *const f32, n_columns: usize, d_out: *mut f32) -> c_int;   // the stage alone
    pub fn sgx_fbank_fused(fbank: *const SgxFbank) -> c_int;
    // the cross sums of a bank: |L|^2, |R|^2, Re and Im of L conj R per band
    pub fn sgx_fbank_cross_batch(fbank: *mut SgxFbank, d_pcm: *const f32, n_samples: usize, first_frame: usize, max_frames: usize,
                                 d_out: *mut f32, n_out: *mut usize) -> c_int;   // PCM -> [frames][pairs][n_filters][4]
    pub fn sgx_fbank_cross_spec(fbank: *mut SgxFbank, d_spec: *const f32, n_columns: usize, d_out: *mut f32) -> c_int;   // the stage alone, from complex rows
    pub fn sgx_fbank_cross_fused(fbank: *const SgxFbank) -> c_int;
    // the flux of a bank: per band (rise_l, rise_r, fall_l, fall_r) of every bin against the same bin `lag` frames earlier
    pub fn sgx_flux_batch(fbank: *mut SgxFbank, d_pcm: *const f32, n_samples: usize, first_frame: usize, max_frames: usize,
                                lag: u32, d_out: *mut f32, n_out: *mut usize) -> c_int;   // PCM -> [frames][pairs][n_filters][4]
    pub fn sgx_flux_mags(fbank: *mut SgxFbank, d_mags: *const f32, n_frames: usize, lag: u32, d_out: *mut f32) -> c_int;   // the stage alone, from frames of rows
    pub fn sgx_flux_max_lag(fbank: *const SgxFbank) -> u32;   // the largest lag sgx_flux_batch takes
    pub fn sgx_mel_weights(sample_rate: f64, window_samples: u32, n_mels: u32, f_min: f64, f_max: f64, scale: u32, norm: u32,
                           h_first: *mut u32, h_count: *mut u32, h_weights: *mut f32, n_weights: *mut usize) -> c_int;   // host only
    pub fn sgx_set_gradient(ctx: *mut SgxCtx, h_rgb: *const u8, n: u32, stereo: c_int) -> c_int;
    pub fn sgx_set_gradient_fn(ctx: *mut SgxCtx, eval: extern "C" fn(f64, *mut u8, *mut c_void), user: *mut c_void,
                               stereo: c_int) -> c_int;
    pub fn sgx_set_builtin_scheme(ctx: *mut SgxCtx, name: *const c_char, stereo: c_int) -> c_int;
    pub fn sgx_lookup_table(ctx: *mut SgxCtx, resolution: u32, h_out: *mut f32) -> c_int;
    pub fn sgx_sync(ctx: *mut SgxCtx) -> c_int;
    pub fn sgx_set_cu_limit(ctx: *mut SgxCtx, n: u32) -> c_int;
    pub fn sgx_cu_limit(ctx: *const SgxCtx) -> u32;
    pub fn sgx_set_run_claim(ctx: *mut SgxCtx, static_sixteenths: u32, chunk_jobs: u32) -> c_int;
    pub fn sgx_run_claim(ctx: *const SgxCtx, n_frames: usize, static_sixteenths: *mut u32, chunk_jobs: *mut u32) -> c_int;
    pub fn sgx_set_run_weights(ctx: *mut SgxCtx, w: *const u32) -> c_int;
    pub fn sgx_run_weights(ctx: *const SgxCtx, n_frames: usize, w: *mut u32) -> c_int;
}
extern "C" {   // from libamdhip64, for staging buffers
    pub fn hipMalloc(p: *mut *mut c_void, bytes: usize) -> c_int;
    pub fn hipFree(p: *mut c_void) -> c_int;
    pub fn hipMemcpy(dst: *mut c_void, src: *const c_void, bytes: usize, kind: c_int) -> c_int;
}
pub const HIP_MEMCPY_HOST_TO_DEVICE: c_int = 1;
pub const HIP_MEMCPY_DEVICE_TO_HOST: c_int = 2;
// SgxConfig::flags (include/sgx.h).  A mono device (audio_input_list_model.rs:67-69): `channels = 1` and no flag -- every frame is its
// own transform, the reference's dataflow (as a real-input transform at W 2048, the application's 2400 / 2205 and every other window but W 8192 and the smallest).
pub const SGX_FLAG_PAIRED_FRAMES: u32 = 1024;   // opt-in: two frames per transform (half the work; tolerance against the pair's peak)
pub const SGX_FLAG_COMPLEX_MONO: u32 = 512;     // A/B: the literal (s, s) transform per frame where a real-input kernel would run
pub const SGX_FLAG_LARGE_TRANSFORM: u32 = 4096; // opt-in: lengths no in-LDS kernel serves, W up to 2^20, as a multi-pass transform through a device scratch
pub const SGX_MEL_HTK: u32 = 0;                 // sgx_mel_weights: mel = 2595 log10(1 + f / 700)
pub const SGX_MEL_SLANEY: u32 = 1;              // linear below 1 kHz, logarithmic above
pub const SGX_MEL_NORM_NONE: u32 = 0;
pub const SGX_MEL_NORM_SLANEY: u32 = 1;         // every triangle times 2 / (f_hi - f_lo)
pub const SGX_LIVE_BANDS: c_int = 3;            // sgx_live_tick: [frames][R][2] f32, the rows of sgx_bands_batch
