// sgx_quantile.hip -- the selection kernels of sgx_quantile_batch / sgx_quantile_mags (include/sgx.h): per flat element of a row
// ([pairs][M][2] floats: sides and pairs need no special handling) the words of n_q ranks among the frames of a column.
//
// A range is one matrix, frames x row_floats, and every element is independent.  Both kernels call quantile::select_keys
// (sgx_quantile.hpp), the one place a result is formed; they differ in where "key t" is read.
//   Path A (a column of at most kLdsFrames frames): a workgroup of four waves owns one column and kTile = 64 consecutive elements.  Wave w
//     loads frames w, w + 4, ...: a wave's load is one coalesced run of 256 B of a row, turned into keys on the way into LDS, laid out
//     [frame][element], so that in every step of the selection the lanes of a wave read consecutive banks.  The waves split the column's
//     frames in four, count their share in every round and add the four counts through LDS (one barrier per round, two areas by parity).
//     (Rows are float-aligned only -- a row of M = 2047 bins is 16 376 B -- so the loads are 4 B per lane, not 16.)
//   Path B (any longer column): a thread per element, the keys read where the rows lie in every round, lanes on consecutive elements so
//     that every wave load is one coalesced run; 64-bit offsets and counts throughout.  32 passes over the column.
// Results leave as coalesced runs of a row of d_out[column][i].
#include "sgx_quantile.hpp"

namespace sgx {
namespace quantile {

namespace {

constexpr uint32_t kThreads = kTile * kWaves;

template <int NQ>
__global__ void __launch_bounds__(kThreads) quantile_lds_kernel(Piece p, unsigned long long col0, unsigned long long tiles)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint32_t *image = reinterpret_cast<uint32_t *>(smem_raw);         // [frame][element]: p.g frames at most
    uint32_t *exchange = image + p.g * kTile;                          // [parity][wave][rank][element]
    const uint32_t lane = threadIdx.x & (kTile - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kTile);
    const unsigned long long col = col0 + blockIdx.x / tiles, e = (blockIdx.x % tiles) * kTile + lane;
    const unsigned long long f0 = col * p.g;
    const bool full = p.n_frames - f0 >= p.g, live = e < p.row_floats;
    const uint32_t n = (uint32_t)(full ? p.g : p.n_frames - f0);
    // ---- the column's keys, once ---------------------------------------------------------------------------------------------------------
    // (a lane beyond the row reads element 0 and its result is dropped: no branch around a load, so a wave keeps many in flight)
    const uint32_t *src = reinterpret_cast<const uint32_t *>(p.rows) + f0 * p.row_floats + (live ? e : 0);
#pragma unroll 16
    for (uint32_t t = wave; t < n; t += kWaves) image[t * kTile + lane] = to_key(src[(unsigned long long)t * p.row_floats]);
    __syncthreads();
    // ---- the selection: this wave's quarter of the frames, the counts added across the waves ---------------------------------------------
    uint32_t rank[NQ], prefix[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) rank[i] = (uint32_t)(full ? p.rank_full[i] : p.rank_last[i]);
    const uint32_t *mine = image + lane;
    const auto keys = [&](uint32_t t) { return mine[t * kTile]; };
    const auto combine = [&](uint32_t (&cnt)[NQ], uint32_t round) {
        uint32_t *x = exchange + (round & 1u) * (kWaves * NQ * kTile) + lane;
#pragma unroll
        for (int i = 0; i < NQ; ++i) x[(wave * NQ + i) * kTile] = cnt[i];
        __syncthreads();   // (the area of the other parity was last read before this barrier of the round before)
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            uint32_t s = 0;
#pragma unroll
            for (uint32_t w = 0; w < kWaves; ++w) s += x[(w * NQ + i) * kTile];
            cnt[i] = s;
        }
    };
    select_keys<NQ, uint32_t>(keys, wave * n / kWaves, (wave + 1) * n / kWaves, rank, combine, prefix);
    // ---- the rows of d_out[column][i]: wave w writes ranks w, w + 4, ... ------------------------------------------------------------------
    uint32_t *out = reinterpret_cast<uint32_t *>(p.out) + col * p.n_q * p.row_floats + e;
#pragma unroll
    for (int i = 0; i < NQ; ++i)
        if ((uint32_t)i % kWaves == wave && (uint32_t)i < p.n_q && live) out[(unsigned long long)i * p.row_floats] = from_key(prefix[i]);
}

template <int NQ>
__global__ void __launch_bounds__(kThreads) quantile_rows_kernel(Piece p, unsigned long long col0, unsigned long long tiles)
{
    const unsigned long long col = col0 + blockIdx.x / tiles, e = (blockIdx.x % tiles) * kThreads + threadIdx.x;
    if (e >= p.row_floats) return;
    const unsigned long long f0 = col * p.g;
    const bool full = p.n_frames - f0 >= p.g;
    const unsigned long long n = full ? p.g : p.n_frames - f0;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(p.rows) + f0 * p.row_floats + e;
    unsigned long long rank[NQ];
    uint32_t prefix[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) rank[i] = full ? p.rank_full[i] : p.rank_last[i];
    const auto keys = [&](unsigned long long t) { return to_key(src[t * p.row_floats]); };
    const auto alone = [](unsigned long long (&)[NQ], uint32_t) {};
    select_keys<NQ, unsigned long long>(keys, 0ull, n, rank, alone, prefix);
    uint32_t *out = reinterpret_cast<uint32_t *>(p.out) + col * p.n_q * p.row_floats + e;
#pragma unroll
    for (int i = 0; i < NQ; ++i)
        if ((uint32_t)i < p.n_q) out[(unsigned long long)i * p.row_floats] = from_key(prefix[i]);
}

// the ranks a kernel carries: n_q rounded up to a build (the slots beyond n_q repeat rank 0 and are not written)
uint32_t built_ranks(uint32_t n_q) { return n_q <= 4 ? n_q : n_q <= 6 ? 6 : n_q <= 8 ? 8 : n_q <= 12 ? 12 : 16; }

template <int NQ>
hipError_t launch(const sgx_ctx *c, const Piece &p, bool lds_path)
{
    const auto kernel = lds_path ? quantile_lds_kernel<NQ> : quantile_rows_kernel<NQ>;
    const size_t lds = lds_path ? lds_bytes((size_t)p.g, NQ) : 0;
    if (lds > 64 * 1024) {   // per launch: the attribute is per device, and a process may hold contexts on several
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const unsigned long long per_block = lds_path ? kTile : kThreads, tiles = (p.row_floats + per_block - 1) / per_block;
    const unsigned long long columns = (p.n_frames + p.g - 1) / p.g, max_blocks = 0x7fffffffull;
    const unsigned long long step = max_blocks / tiles < 1 ? 1 : max_blocks / tiles;   // columns per launch
    for (unsigned long long col0 = 0; col0 < columns; col0 += step) {
        const unsigned long long m = columns - col0 < step ? columns - col0 : step;
        hipLaunchKernelGGL(kernel, dim3((unsigned)(m * tiles)), dim3(kThreads), lds, c->stream, p, col0, tiles);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// true when a column of g frames with n_q ranks is selected in LDS on this context's device (path A)
bool in_lds(const sgx_ctx *c, size_t g, uint32_t n_q)
{
    const size_t cap = c->lds_optin < kLdsCap ? c->lds_optin : kLdsCap;
    return g <= kLdsFrames && lds_bytes(g, built_ranks(n_q)) <= cap;
}

}  // namespace

hipError_t launch_quantile(const sgx_ctx *c, const float *d_rows, size_t n_frames, size_t g, const double *q, uint32_t n_q, float *d_out)
{
    if (n_frames == 0) return hipSuccess;
    const unsigned long long row_floats = (unsigned long long)c->pairs * c->M * 2;
    if (g < 1 || g > n_frames || n_q < 1 || n_q > kMaxQ || row_floats == 0 || row_floats > 0x7fffffffull * kTile) return hipErrorInvalidValue;
    Piece p;
    p.rows = d_rows;
    p.out = d_out;
    p.n_frames = n_frames;
    p.g = g;
    p.row_floats = row_floats;
    p.n_q = n_q;
    const size_t last = n_frames - (n_frames - 1) / g * g;   // frames of the last column: g, or fewer
    for (uint32_t i = 0; i < kMaxQ; ++i) {
        const double qi = q[i < n_q ? i : 0];
        p.rank_full[i] = rank_of(qi, g);
        p.rank_last[i] = rank_of(qi, last);
    }
    const bool lds_path = in_lds(c, g, n_q);
    switch (built_ranks(n_q)) {
    case 1: return launch<1>(c, p, lds_path);
    case 2: return launch<2>(c, p, lds_path);
    case 3: return launch<3>(c, p, lds_path);
    case 4: return launch<4>(c, p, lds_path);
    case 6: return launch<6>(c, p, lds_path);
    case 8: return launch<8>(c, p, lds_path);
    case 12: return launch<12>(c, p, lds_path);
    default: return launch<16>(c, p, lds_path);
    }
}

}  // namespace quantile
}  // namespace sgx
