// fbank_host.hpp -- the host-only part of the filterbank calls (include/sgx.h: sgx_fbank_*, sgx_mel_weights): bank validation and the
// triangular mel bank.  No HIP: a plain C++ compiler builds it (tests/cpp/fbank_host_check.cpp runs it under the sanitizers).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/sgx.h"

namespace sgx {
namespace fbank {

// the banks the fused 4096-point kernels serve (include/sgx.h states them); larger banks take the workspace route
constexpr uint32_t kFusedMaxFilters = 1024;
constexpr size_t kFusedMaxWeights = 16384;
// weight offsets are 32-bit words of the filter table
constexpr size_t kMaxWeights = (size_t)1 << 31;
constexpr uint32_t kMaxFilters = 1u << 30;

// One filter as the kernels read it: 16 bytes, one scalar load
struct Filter {
    uint32_t first, count, offset, pad;   // offset: index of the filter's first weight
};

// SGX_OK and the filter table (weight offsets in filter order: CSR), or SGX_ERR_INVALID_ARG and why
inline int validate(uint32_t M, uint32_t n_filters, const uint32_t *first, const uint32_t *count, const float *weights, uint32_t power,
                    std::vector<Filter> *table, size_t *n_weights, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    if (n_weights) *n_weights = 0;
    if (!first || !count || !weights) { *why = "null array"; return SGX_ERR_INVALID_ARG; }
    if (n_filters == 0 || n_filters > kMaxFilters) { *why = "n_filters is 0 or above 2^30"; return SGX_ERR_INVALID_ARG; }
    if (power != 1 && power != 2) { *why = "power must be 1 or 2"; return SGX_ERR_INVALID_ARG; }
    size_t nnz = 0;
    for (uint32_t f = 0; f < n_filters; ++f) {
        if ((uint64_t)first[f] + (uint64_t)count[f] > (uint64_t)M) { *why = "first + count exceeds the stored bins"; return SGX_ERR_INVALID_ARG; }
        nnz += count[f];
        if (nnz >= kMaxWeights) { *why = "more than 2^31 - 1 weights"; return SGX_ERR_INVALID_ARG; }
    }
    for (size_t i = 0; i < nnz; ++i)
        if (!std::isfinite(weights[i])) { *why = "non-finite weight"; return SGX_ERR_INVALID_ARG; }
    if (table) {
        table->resize(n_filters);
        size_t off = 0;
        for (uint32_t f = 0; f < n_filters; ++f) {
            (*table)[f] = Filter{first[f], count[f], (uint32_t)off, 0u};
            off += count[f];
        }
    }
    if (n_weights) *n_weights = nnz;
    return SGX_OK;
}

inline double hz_to_mel(double f, uint32_t scale)
{
    if (scale == SGX_MEL_HTK) return 2595.0 * std::log10(1.0 + f / 700.0);
    const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}

inline double mel_to_hz(double m, uint32_t scale)
{
    if (scale == SGX_MEL_HTK) return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0);
    const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}

// sgx_mel_weights (include/sgx.h states the definition)
inline int mel_weights(double sample_rate, uint32_t W, uint32_t n_mels, double f_min, double f_max, uint32_t scale, uint32_t norm,
                       uint32_t *h_first, uint32_t *h_count, float *h_weights, size_t *n_weights)
{
    if (n_weights) *n_weights = 0;
    if (!n_weights) return SGX_ERR_INVALID_ARG;
    const bool sizing = !h_first && !h_count && !h_weights;
    if (!sizing && (!h_first || !h_count || !h_weights)) return SGX_ERR_INVALID_ARG;
    if (!(sample_rate > 0.0) || !std::isfinite(sample_rate) || W < 2 || n_mels == 0) return SGX_ERR_INVALID_ARG;
    if (!(f_min >= 0.0) || !(f_max > f_min) || !(f_max <= sample_rate / 2.0)) return SGX_ERR_INVALID_ARG;
    if (scale != SGX_MEL_HTK && scale != SGX_MEL_SLANEY) return SGX_ERR_INVALID_ARG;
    if (norm != SGX_MEL_NORM_NONE && norm != SGX_MEL_NORM_SLANEY) return SGX_ERR_INVALID_ARG;
    // n_mels + 2 points equally spaced in mel: lo + i * step, the last one the upper end itself
    const double m_lo = hz_to_mel(f_min, scale), m_hi = hz_to_mel(f_max, scale), step = (m_hi - m_lo) / (double)(n_mels + 1);
    std::vector<double> pts((size_t)n_mels + 2);
    for (uint32_t i = 0; i < n_mels + 2; ++i) pts[i] = mel_to_hz(i == n_mels + 1 ? m_hi : m_lo + (double)i * step, scale);
    const double df = sample_rate / (2.0 * (double)W);   // bin k of the 2W-point transform lies at k * df; stored element j is bin j + 1
    const uint32_t M = W - 1;
    size_t nnz = 0;
    for (uint32_t m = 0; m < n_mels; ++m) {
        const double f_lo = pts[m], f_c = pts[m + 1], f_hi = pts[m + 2];
        const double scale_w = norm == SGX_MEL_NORM_SLANEY ? 2.0 / (f_hi - f_lo) : 1.0;
        auto weight = [&](uint32_t k) {
            const double f = (double)k * df, up = (f - f_lo) / (f_c - f_lo), down = (f_hi - f) / (f_hi - f_c);
            const double w = up < down ? up : down;
            return w > 0.0 ? w : 0.0;
        };
        // candidates: the bins strictly inside (f_lo, f_hi), found from the edges and settled by the weights themselves
        double k_lo = std::floor(f_lo / df) - 1.0, k_hi = std::ceil(f_hi / df) + 1.0;
        if (k_lo < 1.0) k_lo = 1.0;
        if (k_hi > (double)M) k_hi = (double)M;
        uint32_t first = 0, count = 0;
        for (uint32_t k = (uint32_t)k_lo; (double)k <= k_hi; ++k) {
            if (!(weight(k) > 0.0)) continue;
            if (count == 0) first = k - 1;
            count = k - first;   // (k - 1) - first + 1: a triangle's support is one run of bins
        }
        if (!sizing) {
            h_first[m] = first;
            h_count[m] = count;
            for (uint32_t i = 0; i < count; ++i) h_weights[nnz + i] = (float)(weight(first + 1 + i) * scale_w);
        }
        nnz += count;
    }
    *n_weights = nnz;
    return SGX_OK;
}

}  // namespace fbank
}  // namespace sgx
