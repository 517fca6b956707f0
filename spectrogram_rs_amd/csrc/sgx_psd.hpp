// sgx_psd.hpp -- Welch-averaged spectra per bin (include/sgx.h: sgx_psd_batch, sgx_csd_batch, sgx_psd_mags, sgx_csd_spec): the block /
// column arithmetic the host and the kernels share, and the one device function that forms a block partial.
//
// A call's n frames fall into columns of g = min(group, n) frames; a column's frames fall into blocks of kBlock = 32 consecutive frames
// counted from the column's first frame, so a column has bpc = ceil(g / 32) blocks, the last one short where 32 does not divide g (and
// the last column short where g does not divide n).  Blocks are numbered through the call: block b lies in column b / bpc.  A block's
// partial is one chain of float32 adds from +0 in ascending frame order; a column's sum is one chain of float64 adds over its partials
// in ascending order; the output is (float)(S / (double)n_j).  That order is the definition: nothing here may reassociate it.
#pragma once

#include "sgx_fbank.hpp"
#include "sgx_internal.hpp"

namespace sgx {
namespace psd {

constexpr unsigned long long kBlock = 32;   // include/sgx.h fixes it: not a tuning knob

struct Geometry {
    unsigned long long n, g, bpc;   // frames of the call, frames per column (at most n), blocks per column
    __host__ __device__ unsigned long long columns() const { return (n - 1) / g + 1; }
    __host__ __device__ unsigned long long blocks() const
    {
        const unsigned long long full = n / g, rem = n - full * g;
        return full * bpc + (rem + kBlock - 1) / kBlock;
    }
    __host__ __device__ unsigned long long column_first(unsigned long long j) const { return j * g; }
    __host__ __device__ unsigned long long column_end(unsigned long long j) const { return n - j * g < g ? n : (j + 1) * g; }
    __host__ __device__ unsigned long long block_first(unsigned long long b) const { return (b / bpc) * g + (b % bpc) * kBlock; }
    __host__ __device__ unsigned long long block_end(unsigned long long b) const
    {
        const unsigned long long f = block_first(b), ce = column_end(b / bpc);
        return ce - f < kBlock ? ce : f + kBlock;
    }
    // one past the last block of column j
    __host__ __device__ unsigned long long column_block_end(unsigned long long j) const
    {
        const unsigned long long all = blocks();
        return all - j * bpc < bpc ? all : (j + 1) * bpc;
    }
};
inline Geometry geometry(size_t n, size_t group)   // n >= 1, group >= 1
{
    Geometry geo;
    geo.n = n;
    geo.g = group < n ? group : n;
    geo.bpc = (geo.g + kBlock - 1) / kBlock;
    return geo;
}

// One piece of a call.  Blocks [b0, b0 + nb) of the call; the rows given are those of frames [f_lo, f_hi), `rows` pointing at frame
// f_lo; a block takes the frames of its own that lie in that range.  resume: the range continues blocks begun by an earlier piece, whose
// partials are loaded instead of +0 (a row so long that no whole block of rows fits the workspace).  elems = pairs * M.
struct BlockPiece {
    const float *rows;
    float *partial;                 // [nb][elems][NC]
    Geometry geo;
    unsigned long long elems, b0, nb, f_lo, f_hi;
    uint32_t resume;
};
// The float64 chain over the partials of blocks [b0, b0 + nb): every column the range touches continues from +0 (its first block is in
// the range) or from `carry`, and is finished into `out` (its last block is in the range) or left in `carry`.  The host never gives a range
// in which one column reads `carry` and another writes it.
struct CombinePiece {
    const float *partial;
    float *out;                     // [columns][elems][NC], the call's
    double *carry;                  // [elems][NC], or null where every range holds whole columns
    Geometry geo;
    unsigned long long elems, b0, nb;
};

// psd: rows [frames][elems] of (l, r) magnitudes; csd: rows [frames][elems] of (L.re, L.im, R.re, R.im)
hipError_t launch_psd_blocks(const sgx_ctx *c, bool cross, const BlockPiece &p);      // sgx_psd.hip
hipError_t launch_psd_combine(const sgx_ctx *c, bool cross, const CombinePiece &p);   // sgx_psd.hip

#ifdef __HIPCC__
// Where frame f's summand of element e comes from.  MagRows: x = rn(m * m) per side of the stored magnitudes, a power-2 filterbank's x.
// SpecRows: the four products of the stored (L, R) words, fbank::cross_terms.
struct MagRows {
    static constexpr int kComponents = 2;
    const float2 *rows;
    unsigned long long elems;
    __device__ __forceinline__ void operator()(unsigned long long f, unsigned long long e, float (&x)[2]) const
    {
        const float2 m = rows[f * elems + e];
        x[0] = __fmul_rn(m.x, m.x);
        x[1] = __fmul_rn(m.y, m.y);
    }
};
struct SpecRows {
    static constexpr int kComponents = 4;
    const float4 *rows;
    unsigned long long elems;
    __device__ __forceinline__ void operator()(unsigned long long f, unsigned long long e, float (&x)[4]) const
    {
        const float4 s = rows[f * elems + e];
        float2 x01, x23;
        fbank::cross_terms(s.x, s.y, s.z, s.w, x01, x23);
        x[0] = x01.x; x[1] = x01.y; x[2] = x23.x; x[3] = x23.y;
    }
};

// The only code that forms a block partial: s = rn(s + x) for frames f = f0 .. f1 - 1 of element e in ascending order, the add never
// contracted with the product that made x.
template <typename Src>
__device__ __forceinline__ void block_chain(const Src &src, unsigned long long f0, unsigned long long f1, unsigned long long e,
                                            float (&s)[Src::kComponents])
{
#pragma unroll 8
    for (unsigned long long f = f0; f < f1; ++f) {
        float x[Src::kComponents];
        src(f, e, x);
#pragma unroll
        for (int q = 0; q < Src::kComponents; ++q) s[q] = __fadd_rn(s[q], x[q]);
    }
}
#endif

}  // namespace psd
}  // namespace sgx
