// fbank_host_check.cpp -- the host-only half of the filterbank calls (csrc/fbank_host.hpp: bank validation and sgx_mel_weights) as a
// stand-alone program for the CPU sanitizers (tests/test_fbank_host.py builds it with g++ -fsanitize=address,undefined and runs it).
// Every array is sized exactly, on the heap, so that one element too many read or written is reported.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>

#include "fbank_host.hpp"

using namespace sgx::fbank;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

struct MelCase { double sr; uint32_t W, n_mels; double f_min, f_max; };

static void mel_cases()
{
    const MelCase cases[] = {{48000, 2048, 128, 0, 24000}, {48000, 2048, 80, 32, 22030}, {16000, 400, 80, 0, 8000},
                             {48000, 2048, 256, 20, 20000}, {48000, 64, 40, 0, 24000}};
    for (const MelCase &c : cases)
        for (uint32_t scale : {SGX_MEL_HTK, SGX_MEL_SLANEY})
            for (uint32_t norm : {SGX_MEL_NORM_NONE, SGX_MEL_NORM_SLANEY}) {
                size_t n = 0;
                CHECK(mel_weights(c.sr, c.W, c.n_mels, c.f_min, c.f_max, scale, norm, nullptr, nullptr, nullptr, &n) == SGX_OK);
                std::unique_ptr<uint32_t[]> first(new uint32_t[c.n_mels]), count(new uint32_t[c.n_mels]);
                std::unique_ptr<float[]> w(new float[n]);   // exactly n: one weight too many is a heap overflow
                size_t n2 = 0;
                CHECK(mel_weights(c.sr, c.W, c.n_mels, c.f_min, c.f_max, scale, norm, first.get(), count.get(), w.get(), &n2) == SGX_OK);
                CHECK(n2 == n);
                size_t sum = 0, empty = 0;
                for (uint32_t m = 0; m < c.n_mels; ++m) {
                    CHECK((uint64_t)first[m] + count[m] <= c.W - 1);
                    sum += count[m];
                    empty += count[m] == 0;
                }
                CHECK(sum == n);
                for (size_t i = 0; i < n; ++i) CHECK(std::isfinite(w[i]) && w[i] > 0.0f);
                if (c.W == 64) CHECK(empty == (scale == SGX_MEL_HTK ? 6u : 7u));   // filters narrower than the bin spacing, no bin inside
                else CHECK(empty == 0);
                // what the library does with it: the bank validates, and its table is the CSR offsets
                std::vector<Filter> table;
                size_t nnz = 0;
                const char *why = nullptr;
                CHECK(validate(c.W - 1, c.n_mels, first.get(), count.get(), n ? w.get() : reinterpret_cast<const float *>(first.get()), 2, &table,
                               &nnz, &why) == SGX_OK);
                CHECK(nnz == n && table.size() == c.n_mels);
                size_t off = 0;
                for (uint32_t m = 0; m < c.n_mels; ++m) {
                    CHECK(table[m].first == first[m] && table[m].count == count[m] && table[m].offset == off);
                    off += count[m];
                }
                std::printf("mel ok: sr %.0f W %u mels %u scale %u norm %u: %zu weights, %zu empty\n", c.sr, c.W, c.n_mels, scale, norm, n, empty);
            }
}

static void mel_invalid()
{
    size_t n = 7;
    uint32_t f[4], c[4];
    float w[64];
    auto call = [&](double sr, uint32_t W, uint32_t mels, double lo, double hi, uint32_t scale = SGX_MEL_HTK, uint32_t norm = SGX_MEL_NORM_NONE) {
        return mel_weights(sr, W, mels, lo, hi, scale, norm, nullptr, nullptr, nullptr, &n);
    };
    CHECK(call(48000, 2048, 4, 0, 24000) == SGX_OK);
    CHECK(call(48000, 2048, 0, 0, 24000) == SGX_ERR_INVALID_ARG && n == 0);
    CHECK(call(48000, 2048, 4, -1, 24000) == SGX_ERR_INVALID_ARG);
    CHECK(call(48000, 2048, 4, 100, 100) == SGX_ERR_INVALID_ARG);
    CHECK(call(48000, 2048, 4, 200, 100) == SGX_ERR_INVALID_ARG);
    CHECK(call(48000, 2048, 4, 0, 24000.5) == SGX_ERR_INVALID_ARG);
    CHECK(call(48000, 1, 4, 0, 24000) == SGX_ERR_INVALID_ARG);
    CHECK(call(48000, 0, 4, 0, 24000) == SGX_ERR_INVALID_ARG);
    CHECK(call(48000, 2048, 4, 0, 24000, 2) == SGX_ERR_INVALID_ARG);
    CHECK(call(48000, 2048, 4, 0, 24000, SGX_MEL_HTK, 2) == SGX_ERR_INVALID_ARG);
    CHECK(call(0, 2048, 4, 0, 24000) == SGX_ERR_INVALID_ARG);
    CHECK(call(std::numeric_limits<double>::quiet_NaN(), 2048, 4, 0, 24000) == SGX_ERR_INVALID_ARG);
    CHECK(call(48000, 2048, 4, std::numeric_limits<double>::quiet_NaN(), 24000) == SGX_ERR_INVALID_ARG);
    CHECK(mel_weights(48000, 2048, 4, 0, 24000, 0, 0, nullptr, nullptr, nullptr, nullptr) == SGX_ERR_INVALID_ARG);
    CHECK(mel_weights(48000, 2048, 4, 0, 24000, 0, 0, f, nullptr, w, &n) == SGX_ERR_INVALID_ARG);   // only some of the arrays
    CHECK(mel_weights(48000, 2048, 4, 0, 24000, 0, 0, f, c, nullptr, &n) == SGX_ERR_INVALID_ARG);
    CHECK(mel_weights(48000, 2048, 4, 0, 24000, 0, 0, nullptr, c, w, &n) == SGX_ERR_INVALID_ARG);
    std::printf("mel invalid ok\n");
}

static void validation()
{
    const uint32_t M = 2047;
    std::unique_ptr<uint32_t[]> first(new uint32_t[3]{0, M - 4, M}), count(new uint32_t[3]{3, 4, 0});
    std::unique_ptr<float[]> w(new float[7]{1, -2, 3, 4, 5, 6, 7});
    std::vector<Filter> table;
    size_t nnz = 0;
    const char *why = nullptr;
    CHECK(validate(M, 3, first.get(), count.get(), w.get(), 1, &table, &nnz, &why) == SGX_OK && nnz == 7 && table[2].offset == 7);
    CHECK(validate(M, 3, first.get(), count.get(), w.get(), 2, nullptr, nullptr, nullptr) == SGX_OK);
    CHECK(validate(M, 3, nullptr, count.get(), w.get(), 1, &table, &nnz, &why) == SGX_ERR_INVALID_ARG);
    CHECK(validate(M, 3, first.get(), nullptr, w.get(), 1, &table, &nnz, &why) == SGX_ERR_INVALID_ARG);
    CHECK(validate(M, 3, first.get(), count.get(), nullptr, 1, &table, &nnz, &why) == SGX_ERR_INVALID_ARG);
    CHECK(validate(M, 0, first.get(), count.get(), w.get(), 1, &table, &nnz, &why) == SGX_ERR_INVALID_ARG);
    CHECK(validate(M, 3, first.get(), count.get(), w.get(), 0, &table, &nnz, &why) == SGX_ERR_INVALID_ARG);
    CHECK(validate(M, 3, first.get(), count.get(), w.get(), 3, &table, &nnz, &why) == SGX_ERR_INVALID_ARG);
    first[1] = M - 3;   // first + count = M + 1: refused before a weight of it is read
    CHECK(validate(M, 3, first.get(), count.get(), w.get(), 1, &table, &nnz, &why) == SGX_ERR_INVALID_ARG && nnz == 0);
    first[1] = 0xffffffffu;   // the sum wraps 32 bits
    CHECK(validate(M, 3, first.get(), count.get(), w.get(), 1, &table, &nnz, &why) == SGX_ERR_INVALID_ARG);
    first[1] = M - 4;
    for (float bad : {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()}) {
        w[6] = bad;
        CHECK(validate(M, 3, first.get(), count.get(), w.get(), 1, &table, &nnz, &why) == SGX_ERR_INVALID_ARG);
        w[6] = 7;
    }
    CHECK(validate(M, 3, first.get(), count.get(), w.get(), 1, &table, &nnz, &why) == SGX_OK);
    std::printf("validation ok\n");
}

int main()
{
    mel_cases();
    mel_invalid();
    validation();
    if (failures) return 1;
    std::printf("fbank host ok\n");
    return 0;
}
