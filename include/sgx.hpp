// sgx.hpp -- header-only C++ mirror of the reference's interface for the STFT path, over the C ABI
// of sgx.h.  The reference is Rust; this is the host side a C++ (or, transliterated, a Rust) caller
// programs against: same names, same argument meaning, same "None on short input" rule.
//
//   fourier::AudioTransform            src/fourier/audio_transform.rs:4-11     (abstract interface)
//   fourier::FastFourierTransform      src/fourier/fft.rs:11-99
//   fourier::AudioStreamTransform<T>   src/fourier/audio_transform.rs:14-43    (hop loop over a ring)
//   RingBuffer                         ringbuf::HeapRb<(f32, f32)> as used at src/devices/audio_input_list_model.rs:30,63-72
//   LiveRing                           the same ring, consumed side on the device (sgx_live_*)
//
// Host buffers in, host buffers out (the per-frame `process` of the trait works on host pairs); the
// batched `process` of AudioStreamTransform moves every complete frame of the ring through ONE
// device launch.  Needs libsgx.so and the HIP runtime (hipMalloc / hipMemcpy for staging).
#pragma once

#include <hip/hip_runtime_api.h>

#include <array>
#include <complex>
#include <cstddef>
#include <deque>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "sgx.h"

namespace sgx_host {

using StereoMagnitude = std::pair<float, float>;  // src/fourier/mod.rs:13
using Frequency = float;                          // :15
using Period = float;                             // :14

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

// audio_transform.rs:4-11
class AudioTransform {
public:
    using Output = std::vector<StereoMagnitude>;
    virtual ~AudioTransform() = default;
    virtual Frequency sample_rate() const = 0;
    virtual std::size_t num_input_samples() const = 0;
    // `samples`: at least num_input_samples() (l, r) pairs for Some, fewer for None (fft.rs:72)
    virtual std::optional<Output> process(const StereoMagnitude *samples, std::size_t n_available) = 0;
};

// Rust `f32 as usize`
inline std::size_t f32_as_usize(float v) { return v > 0.0f ? (std::size_t)v : 0; }

// fft.rs:11-99
class FastFourierTransform : public AudioTransform {
public:
    // FastFourierTransform::new(sample_rate, period) (fft.rs:18); `stride` is the hop the stream wrapper
    // will use (audio_transform.rs:35) -- the context is created per (window, hop)
    FastFourierTransform(Frequency sample_rate, Period period, Period stride = 0.0f, int device = -1)
        : sample_rate_(sample_rate), period_(period)
    {
        sgx_config cfg;
        sgx_config_init(&cfg);
        cfg.sample_rate = sample_rate;
        cfg.period = period;
        cfg.window_samples = 0;
        cfg.stride = stride;
        cfg.hop_samples = stride > 0.0f ? 0u : 1u;
        cfg.channels = 2;  // process() receives (l, r) pairs
        cfg.device = device;
        int rc = sgx_create(&cfg, &ctx_);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(nullptr));
    }
    FastFourierTransform(const FastFourierTransform &) = delete;
    FastFourierTransform &operator=(const FastFourierTransform &) = delete;
    ~FastFourierTransform() override
    {
        if (d_in_) (void)hipFree(d_in_);
        if (d_out_) (void)hipFree(d_out_);
        sgx_destroy(ctx_);
    }

    Frequency sample_rate() const override { return sample_rate_; }
    std::size_t num_input_samples() const override { return f32_as_usize(period_ * sample_rate_); }  // fft.rs:41
    std::size_t num_output_frequencies() const { return num_input_samples() - 1; }                   // fft.rs:33

    std::optional<Output> process(const StereoMagnitude *samples, std::size_t n_available) override
    {
        const std::size_t w = num_input_samples();
        Output out(w - 1);
        const int rc = sgx_process_one(ctx_, reinterpret_cast<const float *>(samples), n_available < w ? n_available : w,
                                       reinterpret_cast<float *>(out.data()));
        if (rc < 0) throw Error(rc, sgx_last_error(ctx_));
        if (rc == 0) return std::nullopt;
        return out;
    }

    // every complete frame of `lr` (n pairs) at the context's hop, one launch: frames x (W-1) pairs
    std::vector<Output> process_stream(const StereoMagnitude *lr, std::size_t n)
    {
        const std::size_t frames = sgx_num_frames(ctx_, n), m = num_output_frequencies();
        std::vector<Output> out(frames, Output(m));
        if (!frames) return out;
        reserve(n * 2 * sizeof(float), frames * m * 2 * sizeof(float));
        check_hip(hipMemcpy(d_in_, lr, n * 2 * sizeof(float), hipMemcpyHostToDevice));
        std::size_t got = 0;
        int rc = sgx_stft_batch(ctx_, d_in_, n, 0, frames, d_out_, &got);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        if ((rc = sgx_sync(ctx_)) != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        std::vector<float> flat(frames * m * 2);
        check_hip(hipMemcpy(flat.data(), d_out_, flat.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (std::size_t f = 0; f < frames; ++f)
            for (std::size_t j = 0; j < m; ++j) out[f][j] = {flat[(f * m + j) * 2], flat[(f * m + j) * 2 + 1]};
        return out;
    }

    // magnitude_in over the context's log-frequency rows (sgx_bin_edges) for every complete frame of `lr`: frames x R (l, r) means,
    // row 0 the lowest (sgx_bands_batch)
    std::vector<Output> bands_stream(const StereoMagnitude *lr, std::size_t n)
    {
        sgx_info info;
        int rc = sgx_query(ctx_, &info);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        const std::size_t frames = sgx_num_frames(ctx_, n), r = info.rows;
        std::vector<Output> out(frames, Output(r));
        if (!frames) return out;
        reserve(n * 2 * sizeof(float), frames * r * 2 * sizeof(float));
        check_hip(hipMemcpy(d_in_, lr, n * 2 * sizeof(float), hipMemcpyHostToDevice));
        std::size_t got = 0;
        rc = sgx_bands_batch(ctx_, d_in_, n, 0, frames, d_out_, &got);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        if ((rc = sgx_sync(ctx_)) != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        std::vector<float> flat(frames * r * 2);
        check_hip(hipMemcpy(flat.data(), d_out_, flat.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (std::size_t f = 0; f < frames; ++f)
            for (std::size_t j = 0; j < r; ++j) out[f][j] = {flat[(f * r + j) * 2], flat[(f * r + j) * 2 + 1]};
        return out;
    }

    // the overview of a long stream: bands_stream's columns as maxima over groups of `group` consecutive frames, ceil(frames / group)
    // columns x R (sgx_bands_peak_batch)
    std::vector<Output> bands_peak_stream(const StereoMagnitude *lr, std::size_t n, std::size_t group)
    {
        sgx_info info;
        int rc = sgx_query(ctx_, &info);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        if (group == 0) throw Error(SGX_ERR_INVALID_ARG, "bands_peak_stream: group is 0");
        const std::size_t frames = sgx_num_frames(ctx_, n), r = info.rows, cols = frames ? (frames - 1) / group + 1 : 0;
        std::vector<Output> out(cols, Output(r));
        if (!cols) return out;
        reserve(n * 2 * sizeof(float), cols * r * 2 * sizeof(float));
        check_hip(hipMemcpy(d_in_, lr, n * 2 * sizeof(float), hipMemcpyHostToDevice));
        std::size_t got = 0;
        rc = sgx_bands_peak_batch(ctx_, d_in_, n, 0, frames, group, d_out_, &got);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        if ((rc = sgx_sync(ctx_)) != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        std::vector<float> flat(cols * r * 2);
        check_hip(hipMemcpy(flat.data(), d_out_, flat.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (std::size_t f = 0; f < cols; ++f)
            for (std::size_t j = 0; j < r; ++j) out[f][j] = {flat[(f * r + j) * 2], flat[(f * r + j) * 2 + 1]};
        return out;
    }

    // Welch's estimate at full bin resolution: the mean of the squared magnitudes over groups of `group` consecutive frames,
    // ceil(frames / group) columns x (W-1) bins of (l, r) (sgx_psd_batch; include/sgx.h states the order of the sum and the scaling)
    std::vector<Output> psd_stream(const StereoMagnitude *lr, std::size_t n, std::size_t group)
    {
        if (group == 0) throw Error(SGX_ERR_INVALID_ARG, "psd_stream: group is 0");
        const std::size_t frames = sgx_num_frames(ctx_, n), m = num_output_frequencies(), cols = frames ? (frames - 1) / group + 1 : 0;
        std::vector<Output> out(cols, Output(m));
        if (!cols) return out;
        reserve(n * 2 * sizeof(float), cols * m * 2 * sizeof(float));
        check_hip(hipMemcpy(d_in_, lr, n * 2 * sizeof(float), hipMemcpyHostToDevice));
        std::size_t got = 0;
        int rc = sgx_psd_batch(ctx_, d_in_, n, 0, frames, group, d_out_, &got);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        if ((rc = sgx_sync(ctx_)) != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        std::vector<float> flat(cols * m * 2);
        check_hip(hipMemcpy(flat.data(), d_out_, flat.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (std::size_t f = 0; f < cols; ++f)
            for (std::size_t j = 0; j < m; ++j) out[f][j] = {flat[(f * m + j) * 2], flat[(f * m + j) * 2 + 1]};
        return out;
    }
    // the same mean of the four (L, R) products of every bin: columns x (W-1) bins of {|L|^2, |R|^2, Re L conj R, Im L conj R}
    // (sgx_csd_batch; a context of at least two channels)
    std::vector<std::vector<std::array<float, 4>>> csd_stream(const StereoMagnitude *lr, std::size_t n, std::size_t group)
    {
        if (group == 0) throw Error(SGX_ERR_INVALID_ARG, "csd_stream: group is 0");
        const std::size_t frames = sgx_num_frames(ctx_, n), m = num_output_frequencies(), cols = frames ? (frames - 1) / group + 1 : 0;
        std::vector<std::vector<std::array<float, 4>>> out(cols, std::vector<std::array<float, 4>>(m));
        if (!cols) return out;
        reserve(n * 2 * sizeof(float), cols * m * 4 * sizeof(float));
        check_hip(hipMemcpy(d_in_, lr, n * 2 * sizeof(float), hipMemcpyHostToDevice));
        std::size_t got = 0;
        int rc = sgx_csd_batch(ctx_, d_in_, n, 0, frames, group, d_out_, &got);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        if ((rc = sgx_sync(ctx_)) != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        std::vector<float> flat(cols * m * 4);
        check_hip(hipMemcpy(flat.data(), d_out_, flat.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (std::size_t f = 0; f < cols; ++f)
            for (std::size_t j = 0; j < m; ++j) {
                const float *b = &flat[(f * m + j) * 4];
                out[f][j] = {b[0], b[1], b[2], b[3]};
            }
        return out;
    }
    // the stage alone over rows already on the device (DEVICE pointers; stream-ordered, not waited for): the number of columns written
    // (sgx_psd_mags: [n_frames][pairs][M][2] -> [columns][pairs][M][2]; sgx_csd_spec: [n_frames][pairs][M][2][2] -> [columns][pairs][M][4])
    std::size_t psd_mags(const float *d_mags, std::size_t n_frames, std::size_t group, float *d_psd)
    {
        std::size_t got = 0;
        const int rc = sgx_psd_mags(ctx_, d_mags, n_frames, group, d_psd, &got);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        return got;
    }
    std::size_t csd_spec(const float *d_spec, std::size_t n_frames, std::size_t group, float *d_csd)
    {
        std::size_t got = 0;
        const int rc = sgx_csd_spec(ctx_, d_spec, n_frames, group, d_csd, &got);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        return got;
    }
    // 1: one kernel from PCM to block partials, 0: the workspace route (sgx_psd_fused, sgx_csd_fused)
    int psd_fused() const { return sgx_psd_fused(ctx_); }
    int csd_fused() const { return sgx_csd_fused(ctx_); }

    // where the peaks of every frame are and how strong: per frame and side (0 = l, 1 = r) the k strongest local maxima of the row,
    // strongest first, each {bin, m[bin - 1], m[bin], m[bin + 1]}; slots beyond the candidates are {0, 0, 0, 0} (sgx_maxima_batch;
    // include/sgx.h states the candidates and their order; refinement of frequency and level from the three values is the caller's)
    using Maximum = std::array<float, 4>;
    std::vector<std::array<std::vector<Maximum>, 2>> maxima_stream(const StereoMagnitude *lr, std::size_t n, uint32_t k, float floor = 0.0f)
    {
        if (k < 1 || k > 64) throw Error(SGX_ERR_INVALID_ARG, "maxima_stream: k must be 1 .. 64");
        const std::size_t frames = sgx_num_frames(ctx_, n);
        std::vector<std::array<std::vector<Maximum>, 2>> out(frames);
        if (!frames) return out;
        reserve(n * 2 * sizeof(float), frames * 2 * k * 4 * sizeof(float));
        check_hip(hipMemcpy(d_in_, lr, n * 2 * sizeof(float), hipMemcpyHostToDevice));
        std::size_t got = 0;
        int rc = sgx_maxima_batch(ctx_, d_in_, n, 0, frames, k, floor, d_out_, &got);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        if ((rc = sgx_sync(ctx_)) != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        std::vector<float> flat(frames * 2 * k * 4);
        check_hip(hipMemcpy(flat.data(), d_out_, flat.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (std::size_t f = 0; f < frames; ++f)
            for (std::size_t s = 0; s < 2; ++s) {
                out[f][s].resize(k);
                for (std::size_t r = 0; r < k; ++r) {
                    const float *b = &flat[((f * 2 + s) * k + r) * 4];
                    out[f][s][r] = {b[0], b[1], b[2], b[3]};
                }
            }
        return out;
    }
    // the stage alone over rows already on the device (DEVICE pointers; stream-ordered, not waited for)
    // (sgx_maxima_mags: [n_columns][pairs][M][2] -> [n_columns][pairs][2][k][4], d_max 16-byte aligned)
    void maxima_mags(const float *d_mags, std::size_t n_columns, uint32_t k, float floor, float *d_max)
    {
        const int rc = sgx_maxima_mags(ctx_, d_mags, n_columns, k, floor, d_max);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
    }

    // where the running sum of every frame's row crosses shares of its total: per frame, side (0 = l, 1 = r) and share p[i] the record
    // {bin, c[bin - 1], c[bin], T}, c the cumulative value of include/sgx.h (segments of 32, power 1: magnitudes, 2: their squares), bin
    // the first with c >= rn(p * T); {0, 0, 0, T} where !(T > 0) (sgx_rolloff_batch; interpolation and Hz are the caller's)
    using Crossing = std::array<float, 4>;
    std::vector<std::array<std::vector<Crossing>, 2>> rolloff_stream(const StereoMagnitude *lr, std::size_t n, uint32_t power,
                                                                     const std::vector<float> &p)
    {
        if (p.empty() || p.size() > 8) throw Error(SGX_ERR_INVALID_ARG, "rolloff_stream: 1 .. 8 shares");
        const std::size_t frames = sgx_num_frames(ctx_, n), n_p = p.size();
        std::vector<std::array<std::vector<Crossing>, 2>> out(frames);
        if (!frames) return out;
        reserve(n * 2 * sizeof(float), frames * 2 * n_p * 4 * sizeof(float));
        check_hip(hipMemcpy(d_in_, lr, n * 2 * sizeof(float), hipMemcpyHostToDevice));
        std::size_t got = 0;
        int rc = sgx_rolloff_batch(ctx_, d_in_, n, 0, frames, power, p.data(), (uint32_t)n_p, d_out_, &got);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        if ((rc = sgx_sync(ctx_)) != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        std::vector<float> flat(frames * 2 * n_p * 4);
        check_hip(hipMemcpy(flat.data(), d_out_, flat.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (std::size_t f = 0; f < frames; ++f)
            for (std::size_t s = 0; s < 2; ++s) {
                out[f][s].resize(n_p);
                for (std::size_t r = 0; r < n_p; ++r) {
                    const float *b = &flat[((f * 2 + s) * n_p + r) * 4];
                    out[f][s][r] = {b[0], b[1], b[2], b[3]};
                }
            }
        return out;
    }
    // the stage alone over rows already on the device (DEVICE pointers; stream-ordered, not waited for)
    // (sgx_rolloff_mags: [n_columns][pairs][M][2] -> [n_columns][pairs][2][n_p][4], d_out 16-byte aligned; h_p a HOST array)
    void rolloff_mags(const float *d_mags, std::size_t n_columns, uint32_t power, const float *h_p, uint32_t n_p, float *d_out)
    {
        const int rc = sgx_rolloff_mags(ctx_, d_mags, n_columns, power, h_p, n_p, d_out);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
    }

    // per-bin order statistics over groups of `group` frames: columns x q.size() rows of (W-1) bins of {l, r}, each the word of rank
    // floor(q * (n - 1) + 0.5) among the column's n frames, NaN last (sgx_quantile_batch; include/sgx.h states order and rank; a column
    // longer than quantile_max_group() is refused)
    std::vector<std::vector<Output>> quantile_stream(const StereoMagnitude *lr, std::size_t n, std::size_t group, const std::vector<double> &q)
    {
        if (group == 0) throw Error(SGX_ERR_INVALID_ARG, "quantile_stream: group is 0");
        if (q.empty() || q.size() > 16) throw Error(SGX_ERR_INVALID_ARG, "quantile_stream: 1 .. 16 quantiles");
        const std::size_t frames = sgx_num_frames(ctx_, n), m = num_output_frequencies(), cols = frames ? (frames - 1) / group + 1 : 0;
        std::vector<std::vector<Output>> out(cols, std::vector<Output>(q.size(), Output(m)));
        if (!cols) return out;
        reserve(n * 2 * sizeof(float), cols * q.size() * m * 2 * sizeof(float));
        check_hip(hipMemcpy(d_in_, lr, n * 2 * sizeof(float), hipMemcpyHostToDevice));
        std::size_t got = 0;
        int rc = sgx_quantile_batch(ctx_, d_in_, n, 0, frames, group, q.data(), (uint32_t)q.size(), d_out_, &got);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        if ((rc = sgx_sync(ctx_)) != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        std::vector<float> flat(cols * q.size() * m * 2);
        check_hip(hipMemcpy(flat.data(), d_out_, flat.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (std::size_t f = 0; f < cols; ++f)
            for (std::size_t i = 0; i < q.size(); ++i)
                for (std::size_t j = 0; j < m; ++j) {
                    const float *b = &flat[((f * q.size() + i) * m + j) * 2];
                    out[f][i][j] = {b[0], b[1]};
                }
        return out;
    }
    // the stage alone over rows already on the device (DEVICE pointers; stream-ordered, not waited for); any group
    // (sgx_quantile_mags: [n_frames][pairs][M][2] -> [columns][n_q][pairs][M][2]); answers the number of columns
    std::size_t quantile_mags(const float *d_mags, std::size_t n_frames, std::size_t group, const std::vector<double> &q, float *d_out)
    {
        std::size_t got = 0;
        const int rc = sgx_quantile_mags(ctx_, d_mags, n_frames, group, q.data(), (uint32_t)q.size(), d_out, &got);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        return got;
    }
    std::size_t quantile_max_group() const { return sgx_quantile_max_group(ctx_); }

    // the complex (L, R) spectra behind process_stream's magnitudes for every complete frame of `lr`: frames x (W-1) bins of
    // {L, R} (sgx_stft_batch_complex)
    std::vector<std::vector<std::array<std::complex<float>, 2>>> process_stream_complex(const StereoMagnitude *lr, std::size_t n)
    {
        const std::size_t frames = sgx_num_frames(ctx_, n), m = num_output_frequencies();
        std::vector<std::vector<std::array<std::complex<float>, 2>>> out(frames, std::vector<std::array<std::complex<float>, 2>>(m));
        if (!frames) return out;
        reserve(n * 2 * sizeof(float), frames * m * 4 * sizeof(float));
        check_hip(hipMemcpy(d_in_, lr, n * 2 * sizeof(float), hipMemcpyHostToDevice));
        std::size_t got = 0;
        int rc = sgx_stft_batch_complex(ctx_, d_in_, n, 0, frames, d_out_, &got);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        if ((rc = sgx_sync(ctx_)) != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        std::vector<float> flat(frames * m * 4);
        check_hip(hipMemcpy(flat.data(), d_out_, flat.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (std::size_t f = 0; f < frames; ++f)
            for (std::size_t j = 0; j < m; ++j) {
                const float *b = &flat[(f * m + j) * 4];
                out[f][j] = {std::complex<float>(b[0], b[1]), std::complex<float>(b[2], b[3])};
            }
        return out;
    }

    // PCM back from complex (L, R) spectra laid out as process_stream_complex returns them: the samples [0, (frames - 1) H + W) of the
    // signal, `channels` interleaved per sample (sgx_istft_batch)
    std::vector<float> istft(const std::vector<std::vector<std::array<std::complex<float>, 2>>> &spec)
    {
        sgx_info inf{};
        int rc = sgx_query(ctx_, &inf);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        const std::size_t frames = spec.size(), m = num_output_frequencies(), ch = inf.channels;
        if (!frames) return {};
        const std::size_t n = (frames - 1) * inf.hop_samples + inf.window_samples;
        for (std::size_t f = 0; f < frames; ++f)
            if (spec[f].size() != m)
                throw Error(SGX_ERR_INVALID_ARG, "istft: frame " + std::to_string(f) + " holds " + std::to_string(spec[f].size()) +
                                                     " bins, the context has " + std::to_string(m));
        std::vector<float> flat(frames * m * 4);
        for (std::size_t f = 0; f < frames; ++f)
            for (std::size_t j = 0; j < m; ++j) {
                float *b = &flat[(f * m + j) * 4];
                b[0] = spec[f][j][0].real(); b[1] = spec[f][j][0].imag(); b[2] = spec[f][j][1].real(); b[3] = spec[f][j][1].imag();
            }
        reserve(flat.size() * sizeof(float), n * ch * sizeof(float));
        check_hip(hipMemcpy(d_in_, flat.data(), flat.size() * sizeof(float), hipMemcpyHostToDevice));
        std::size_t got = 0;
        rc = sgx_istft_batch(ctx_, d_in_, frames, 0, n, d_out_, &got);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        if ((rc = sgx_sync(ctx_)) != SGX_OK) throw Error(rc, sgx_last_error(ctx_));
        std::vector<float> out(got * ch);
        check_hip(hipMemcpy(out.data(), d_out_, out.size() * sizeof(float), hipMemcpyDeviceToHost));
        return out;
    }
    bool istft_supported() const { return sgx_istft_supported(ctx_) == 1; }

    sgx_ctx *ctx() { return ctx_; }

private:
    static void check_hip(hipError_t e)
    {
        if (e != hipSuccess) throw Error(SGX_ERR_HIP, hipGetErrorString(e));
    }
    void reserve(std::size_t in_bytes, std::size_t out_bytes)
    {
        if (in_bytes > in_cap_) {
            if (d_in_) (void)hipFree(d_in_);
            check_hip(hipMalloc(reinterpret_cast<void **>(&d_in_), in_bytes));
            in_cap_ = in_bytes;
        }
        if (out_bytes > out_cap_) {
            if (d_out_) (void)hipFree(d_out_);
            check_hip(hipMalloc(reinterpret_cast<void **>(&d_out_), out_bytes));
            out_cap_ = out_bytes;
        }
    }
    sgx_ctx *ctx_ = nullptr;
    Frequency sample_rate_;
    Period period_;
    float *d_in_ = nullptr, *d_out_ = nullptr;
    std::size_t in_cap_ = 0, out_cap_ = 0;
};

// the SPSC ring between the capture thread and the GUI thread (audio_input_list_model.rs:30,63-72)
class RingBuffer {
public:
    explicit RingBuffer(std::size_t capacity) : capacity_(capacity) {}
    std::size_t push_iter(const StereoMagnitude *s, std::size_t n)  // overflow is dropped (:70)
    {
        std::size_t pushed = 0;
        for (; pushed < n && data_.size() < capacity_; ++pushed) data_.push_back(s[pushed]);
        return pushed;
    }
    std::size_t skip(std::size_t n)
    {
        n = n < data_.size() ? n : data_.size();
        data_.erase(data_.begin(), data_.begin() + (std::ptrdiff_t)n);
        return n;
    }
    std::size_t occupied_len() const { return data_.size(); }
    std::vector<StereoMagnitude> peek(std::size_t n) const
    {
        n = n < data_.size() ? n : data_.size();
        return std::vector<StereoMagnitude>(data_.begin(), data_.begin() + (std::ptrdiff_t)n);
    }

private:
    std::size_t capacity_;
    std::deque<StereoMagnitude> data_;
};

// The same ring with its consumed side resident on the device (sgx_live_*): the capture callback pushes
// host samples (audio_input_list_model.rs:63-75), one tick() per GUI frame returns every complete frame
// (audio_transform.rs:34-42) and moves only the new samples to the GPU.
class LiveRing {
public:
    // reference_skip: also drop H samples on the terminating short read, exactly as audio_transform.rs:37-41
    LiveRing(FastFourierTransform &transform, std::size_t capacity = 4096, bool reference_skip = false)
        : transform_(transform)
    {
        const int rc = sgx_live_create(transform.ctx(), capacity, reference_skip ? SGX_LIVE_REFERENCE_SKIP : 0u, &live_);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(transform.ctx()));
    }
    LiveRing(const LiveRing &) = delete;
    LiveRing &operator=(const LiveRing &) = delete;
    ~LiveRing() { sgx_live_destroy(live_); }

    // interleaved samples of a 1- or 2-channel callback; returns the pairs accepted (overflow is dropped)
    std::size_t push(const float *data, std::size_t n_values, unsigned channels)
    {
        const long long rc = sgx_live_push(live_, data, n_values, channels);
        if (rc < 0) throw Error((int)rc, std::to_string(channels) + "-channel input not supported!");
        return (std::size_t)rc;
    }
    std::size_t occupied_len() const { return sgx_live_occupied(live_); }

    std::vector<AudioTransform::Output> tick(std::size_t max_frames = 64)
    {
        const std::size_t m = transform_.num_output_frequencies();
        std::vector<float> flat(max_frames * m * 2);
        std::size_t got = 0;
        const int rc = sgx_live_tick(live_, SGX_LIVE_MAGS, flat.data(), max_frames, &got);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(transform_.ctx()));
        std::vector<AudioTransform::Output> out(got, AudioTransform::Output(m));
        for (std::size_t f = 0; f < got; ++f)
            for (std::size_t j = 0; j < m; ++j) out[f][j] = {flat[(f * m + j) * 2], flat[(f * m + j) * 2 + 1]};
        return out;
    }

    sgx_live *raw() { return live_; }

private:
    FastFourierTransform &transform_;
    sgx_live *live_ = nullptr;
};

// SimpleSpectrogram's Pixbuf ring on the device (sgx_image_*): `buffer` + `offset` of simple_spectrogram.rs:60-66,89-94, the
// put_pixel loop with its offset update (:140-164) as tick(), the picture of the two sub-images (:181-209) as scrolled().
class ImageRing {
public:
    // (the height is never the caller's to choose: it is the context's row count, read back from the image)
    ImageRing(FastFourierTransform &transform, std::uint32_t width) : transform_(transform)
    {
        const int rc = sgx_image_create(transform.ctx(), width, &image_);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(transform.ctx()));
        width_ = sgx_image_width(image_);
        rows_ = sgx_image_height(image_);
    }
    ImageRing(const ImageRing &) = delete;
    ImageRing &operator=(const ImageRing &) = delete;
    ~ImageRing() { sgx_image_destroy(image_); }

    // one GUI tick: every complete frame of the capture ring becomes a pixel column at `offset`, device to device
    std::size_t tick(LiveRing &live)
    {
        std::size_t got = 0;
        const int rc = sgx_live_tick_image(live.raw(), image_, width_, &got);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(transform_.ctx()));
        return got;
    }
    std::size_t offset() const { return sgx_image_offset(image_); }
    std::uint32_t width() const { return width_; }
    std::uint32_t height() const { return rows_; }

    // [rows][width][4] bytes on the host: the buffer as it lies, or the scrolled picture
    std::vector<std::uint8_t> pixels(bool scrolled = false)
    {
        const std::size_t bytes = (std::size_t)rows_ * width_ * 4;
        void *d = nullptr;
        if (hipMalloc(&d, bytes) != hipSuccess) throw Error(SGX_ERR_HIP, "hipMalloc");
        std::vector<std::uint8_t> out(bytes);
        int rc = sgx_image_read(image_, scrolled ? 1 : 0, static_cast<std::uint8_t *>(d));
        if (rc == SGX_OK) rc = sgx_sync(transform_.ctx());
        const hipError_t e = rc == SGX_OK ? hipMemcpy(out.data(), d, bytes, hipMemcpyDeviceToHost) : hipSuccess;
        (void)hipFree(d);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(transform_.ctx()));
        if (e != hipSuccess) throw Error(SGX_ERR_HIP, hipGetErrorString(e));
        return out;
    }

private:
    FastFourierTransform &transform_;
    sgx_image *image_ = nullptr;
    std::uint32_t width_ = 0, rows_ = 0;
};

// A filterbank on the device (sgx_fbank_*): weighted sums of the bin magnitudes (power 1) or powers (power 2) over sparse filters --
// filter f weighs bins first[f] .. first[f] + count[f] - 1 with the next count[f] weights.  mel(): the triangular mel bank of
// sgx_mel_weights over the transform's own bins.  Destroyed before its transform.
class FilterBank {
public:
    FilterBank(FastFourierTransform &transform, const std::vector<std::uint32_t> &first, const std::vector<std::uint32_t> &count,
               const std::vector<float> &weights, std::uint32_t power = 2)
        : transform_(transform)
    {
        if (first.size() != count.size()) throw Error(SGX_ERR_INVALID_ARG, "FilterBank: first and count hold one entry per filter");
        const float none = 0.0f;
        void *h = nullptr;
        const int rc = sgx_fbank_create(transform.ctx(), (std::uint32_t)first.size(), first.data(), count.data(),
                                        weights.empty() ? &none : weights.data(), power, &h);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(transform.ctx()));
        bank_ = static_cast<sgx_fbank *>(h);
    }
    static FilterBank mel(FastFourierTransform &transform, double sample_rate, std::uint32_t window_samples, std::uint32_t n_mels = 128,
                          double f_min = 0.0, double f_max = -1.0, std::uint32_t scale = SGX_MEL_HTK, std::uint32_t norm = SGX_MEL_NORM_NONE,
                          std::uint32_t power = 2)
    {
        if (f_max < 0.0) f_max = sample_rate / 2.0;
        std::size_t n = 0;
        int rc = sgx_mel_weights(sample_rate, window_samples, n_mels, f_min, f_max, scale, norm, nullptr, nullptr, nullptr, &n);
        if (rc != SGX_OK) throw Error(rc, "sgx_mel_weights: invalid argument");
        std::vector<std::uint32_t> first(n_mels), count(n_mels);
        std::vector<float> weights(n ? n : 1);
        rc = sgx_mel_weights(sample_rate, window_samples, n_mels, f_min, f_max, scale, norm, first.data(), count.data(), weights.data(), &n);
        if (rc != SGX_OK) throw Error(rc, "sgx_mel_weights: invalid argument");
        weights.resize(n);
        return FilterBank(transform, first, count, weights, power);
    }
    FilterBank(const FilterBank &) = delete;
    FilterBank &operator=(const FilterBank &) = delete;
    FilterBank(FilterBank &&o) noexcept : transform_(o.transform_), bank_(o.bank_) { o.bank_ = nullptr; }
    ~FilterBank() { sgx_fbank_destroy(bank_); }

    std::uint32_t filters() const { return sgx_fbank_filters(bank_); }
    bool fused() const { return sgx_fbank_fused(bank_) == 1; }
    // device to device: PCM -> [frames][pairs][filters][2]; returns the frames written
    std::size_t batch(const float *d_pcm, std::size_t n_samples, float *d_out, std::size_t first_frame = 0, std::size_t max_frames = (std::size_t)-1)
    {
        std::size_t got = 0;
        const int rc = sgx_fbank_batch(bank_, d_pcm, n_samples, first_frame, max_frames, d_out, &got);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(transform_.ctx()));
        return got;
    }
    // the stage alone: [columns][M][2] rows -> [columns][filters][2]
    void apply(const float *d_mags, std::size_t n_columns, float *d_out)
    {
        const int rc = sgx_fbank_mags(bank_, d_mags, n_columns, d_out);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(transform_.ctx()));
    }
    // The cross sums (sgx_fbank_cross_*): per band the sums of |L|^2, |R|^2, Re and Im of L conj R over the complex rows of an (l, r) pair.
    bool cross_fused() const { return sgx_fbank_cross_fused(bank_) == 1; }
    // device to device: PCM -> [frames][pairs][filters][4]; returns the frames written
    std::size_t cross_batch(const float *d_pcm, std::size_t n_samples, float *d_out, std::size_t first_frame = 0,
                            std::size_t max_frames = (std::size_t)-1)
    {
        std::size_t got = 0;
        const int rc = sgx_fbank_cross_batch(bank_, d_pcm, n_samples, first_frame, max_frames, d_out, &got);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(transform_.ctx()));
        return got;
    }
    // the stage alone: [columns][M][2][2] complex rows -> [columns][filters][4]
    void cross_apply(const float *d_spec, std::size_t n_columns, float *d_out)
    {
        const int rc = sgx_fbank_cross_spec(bank_, d_spec, n_columns, d_out);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(transform_.ctx()));
    }
    // The flux (sgx_flux_*): per band (rise_l, rise_r, fall_l, fall_r) of every bin against the same bin `lag` frames earlier.
    std::uint32_t flux_max_lag() const { return sgx_flux_max_lag(bank_); }
    // device to device: PCM -> [frames][pairs][filters][4]; returns the frames written
    std::size_t flux_batch(const float *d_pcm, std::size_t n_samples, float *d_out, std::uint32_t lag = 1, std::size_t first_frame = 0,
                           std::size_t max_frames = (std::size_t)-1)
    {
        std::size_t got = 0;
        const int rc = sgx_flux_batch(bank_, d_pcm, n_samples, first_frame, max_frames, lag, d_out, &got);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(transform_.ctx()));
        return got;
    }
    // the stage alone: [frames][pairs][M][2] rows -> [frames][pairs][filters][4]
    void flux_apply(const float *d_mags, std::size_t n_frames, float *d_out, std::uint32_t lag = 1)
    {
        const int rc = sgx_flux_mags(bank_, d_mags, n_frames, lag, d_out);
        if (rc != SGX_OK) throw Error(rc, sgx_last_error(transform_.ctx()));
    }
    sgx_fbank *raw() const { return bank_; }

private:
    FastFourierTransform &transform_;
    sgx_fbank *bank_ = nullptr;
};

// audio_transform.rs:14-43; the three members are public and assignable, as in the reference
template <typename T>
struct AudioStreamTransform {
    RingBuffer &input_stream;
    T &transform;
    Period stride;

    AudioStreamTransform(RingBuffer &s, T &t, Period st) : input_stream(s), transform(t), stride(st) {}

    std::size_t stride_samples() const { return f32_as_usize(stride * transform.sample_rate()); }  // :35

    // every frame the reference's repeat_with / take_while loop would yield, from one batched launch;
    // the ring advances as the reference's does, including the skip of its terminating short read (:37-41)
    std::vector<typename T::Output> process()
    {
        const std::size_t h = stride_samples(), w = transform.num_input_samples(), n = input_stream.occupied_len();
        if (h == 0) throw Error(SGX_ERR_INVALID_ARG, "stride * sample_rate truncates to 0 samples");
        const std::size_t frames = n < w ? 0 : (n - w) / h + 1;
        std::vector<typename T::Output> out;
        if (frames) {
            const auto lr = input_stream.peek((frames - 1) * h + w);
            out = transform.process_stream(lr.data(), lr.size());
        }
        input_stream.skip((frames + 1) * h);
        return out;
    }
};

}  // namespace sgx_host
