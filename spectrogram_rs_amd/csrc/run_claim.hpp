// run_claim.hpp -- a persistent launch whose workgroups take a static run of jobs each and then CLAIM the rest, chunk by chunk, from a pool.
// Plain C++ (no HIP): the launcher, the kernel and the CPU tests (tests/cpp/run_claim_check.cpp, run_weights_check.cpp) all read the split from here.
//
// Why: the workgroups of a store-bound launch do not run at one speed (profiles/k1r_claimed_tail.txt: the mono rows launch's workgroups
// finish between 0.58 and 0.99 of its duration, 0.83 on average), and with equal static runs the launch waits for the slowest while the
// CUs of the others idle.  The static part keeps what a long contiguous run is worth (the sliding window: one 8-byte load per thread and
// iteration); the pool, dealt in chunks long enough to pay for a window refill, is what lets every workgroup finish within one chunk of
// the others.  The static runs are equal (run_claim) or sized by the workgroup's slot on its CU (slot_deal, below): the mono rows launch
// at hop 256 runs the latter with 1/16 of the jobs pooled, its complex rows with none.
//
//   jobs [0, blocks * per)            static: workgroup b runs [b * per, (b + 1) * per)
//   jobs [pool_begin, n_jobs)         the pool: chunk i is [pool_begin + i * chunk, + chunk) cut at n_jobs, i < n_chunks
//
// A claim is one returning atomic add of 1 on a counter that starts at 0 in every launch; an index >= n_chunks ends the workgroup (every
// workgroup draws exactly one such index, so the counter ends at n_chunks + blocks: far from wrapping).
#pragma once

namespace sgx {

struct RunClaim {
    unsigned long long per;          // jobs of a workgroup's static run (may be 0)
    unsigned long long pool_begin;   // = blocks * per
    unsigned long long n_chunks;     // chunks of the pool
    unsigned long long chunk;        // jobs per chunk (>= 1)
};
struct JobRun { unsigned long long begin, end; };   // [begin, end); empty where begin == end

// static_sixteenths 0 .. 16: the share of the jobs dealt statically, rounded down to whole jobs per workgroup; chunk_jobs >= 1; blocks >= 1
inline RunClaim run_claim(unsigned long long n_jobs, unsigned long long blocks, unsigned static_sixteenths, unsigned long long chunk_jobs)
{
    RunClaim r;
    r.per = (n_jobs / 16 * static_sixteenths + n_jobs % 16 * static_sixteenths / 16) / blocks;   // floor(floor(n_jobs s / 16) / blocks), without the product n_jobs * s
    r.pool_begin = blocks * r.per;
    r.chunk = chunk_jobs < 1 ? 1 : chunk_jobs;
    r.n_chunks = (n_jobs - r.pool_begin + r.chunk - 1) / r.chunk;
    return r;
}
inline JobRun static_run(const RunClaim &r, unsigned long long block) { return {block * r.per, (block + 1) * r.per}; }
// the jobs of claim index i: empty for an index past the pool
inline JobRun claimed_run(const RunClaim &r, unsigned long long n_jobs, unsigned long long i)
{
    if (i >= r.n_chunks) return {n_jobs, n_jobs};
    const unsigned long long b = r.pool_begin + i * r.chunk, left = n_jobs - b;
    return {b, b + (left < r.chunk ? left : r.chunk)};
}

// The automatic rule: the pool pays only where the static run it leaves is still long -- below kClaimMinStatic jobs per workgroup the
// launch is the static one (live ticks, short batches: no counter, no memset).
constexpr unsigned kClaimAutoSixteenths = 12, kClaimAutoChunk = 8;
constexpr unsigned long long kClaimMinStatic = 64;
inline bool run_claim_engages(unsigned long long n_jobs, unsigned long long blocks)
{
    return run_claim(n_jobs, blocks, kClaimAutoSixteenths, kClaimAutoChunk).per >= kClaimMinStatic;
}
// what sgx_set_run_claim accepts: (0, 0) automatic, (16, 0) the static split, else a share 0 .. 16 with a chunk of 1 .. 2^20 jobs
inline bool run_claim_valid(unsigned static_sixteenths, unsigned chunk_jobs)
{
    if (chunk_jobs == 0) return static_sixteenths == 0 || static_sixteenths == 16;
    return static_sixteenths <= 16 && chunk_jobs <= (1u << 20);
}

// ---- The weighted deal: static runs sized by the workgroup's slot on its CU -------------------------------------------------------------
// A workgroup's rate in the mono rows launch is a function of its slot on the CU and of nothing else (profiles/k1r_claimed_tail.txt: the
// block-index quarters finish at 0.695 / 0.74 / 0.93 / 0.975 of the launch with equal runs; blocks are dealt round-robin over the CUs, so
// a quarter is "the n-th workgroup placed on its CU").  Equal runs for workgroups whose rates are known to differ leave the balance to the
// pool, and a pooled job is dearer than a static one; runs WEIGHTED by slot give the balance with every job in a long contiguous run.
//
//   slot(b) = min(b / n_cu, 3); slot s holds cnt_s = the blocks of [s n_cu, (s + 1) n_cu) (the last slot: all from 3 n_cu on), so a short
//   launch fills the slots from the front and blocks = 4 n_cu - 1 leaves the last slot one short
//   w[0 .. 3], each >= 1, summing to 256: (64, 64, 64, 64) is the equal deal
//   T     = the jobs dealt statically: floor(n_jobs share / 16) as run_claim rounds it; all of them at share 16
//   per_s = floor(T w_s / sum_t cnt_t w_t)       [= floor(4 per w_s / 256) of the equal run `per` where every slot is full]
//   block b of slot s runs [n_cu (per_0 + .. + per_{s-1}) + (b - s n_cu) per_s, + per_s)      (the slots in front of a block's are full)
// The weights are normalised over the blocks that exist, not over 4 n_cu: sum_s cnt_s per_s <= T whatever the weights and however short
// the last slot is (normalised over 4 n_cu, a light last slot that is one block short would deal more than n_jobs).  Equal weights give
// per_s = floor(T / blocks): with a pool exactly static_run / claimed_run of run_claim.
//   share < 16   pool_begin = sum_s cnt_s per_s: the rounding leftovers fall to the pool, which is claimed as above
//   share 16     no pool: the r = n_jobs - sum_s cnt_s per_s leftover jobs (r < blocks) go one each to the first r blocks in block order,
//                i.e. block b starts min(b, r) jobs later and runs one job more where b < r: an exact partition
// An empty static run is legal either way.  constexpr: the launcher, the kernel (which rebuilds the deal from its argument words) and
// the CPU test (tests/cpp/run_weights_check.cpp) call the same functions.
struct SlotDeal {
    unsigned long long per[4];       // jobs of a static run, by slot
    unsigned long long n_cu;         // blocks per slot
    unsigned long long leftover;     // share 16: the first `leftover` blocks run one job more; else 0
    RunClaim claim;                  // the pool behind the static runs (share 16: empty, n_chunks 0); claim.per is the EQUAL run and not used
};
constexpr unsigned long long slot_of(unsigned long long block, unsigned long long n_cu) { return block / n_cu < 3 ? block / n_cu : 3; }
constexpr unsigned long long slot_blocks(unsigned long long blocks, unsigned long long n_cu, unsigned s)
{
    const unsigned long long lo = s * n_cu;
    return blocks <= lo ? 0 : (s == 3 || blocks - lo < n_cu ? blocks - lo : n_cu);
}
constexpr bool run_weights_valid(const unsigned w[4]) { return w[0] >= 1 && w[1] >= 1 && w[2] >= 1 && w[3] >= 1 && w[0] <= 256 && w[1] <= 256 && w[2] <= 256 && w[3] <= 256 && w[0] + w[1] + w[2] + w[3] == 256; }
// n_jobs < 2^63 / 1024 (T w_s < 2^61); blocks >= 1, n_cu >= 1; w valid
constexpr SlotDeal slot_deal(unsigned long long n_jobs, unsigned long long blocks, unsigned long long n_cu, unsigned static_sixteenths, unsigned long long chunk_jobs,
                             const unsigned w[4])
{
    SlotDeal d{};
    const unsigned long long T = static_sixteenths >= 16 ? n_jobs : n_jobs / 16 * static_sixteenths + n_jobs % 16 * static_sixteenths / 16;
    unsigned long long den = 0, dealt = 0;
    for (unsigned s = 0; s < 4; ++s) den += slot_blocks(blocks, n_cu, s) * w[s];
    for (unsigned s = 0; s < 4; ++s) {
        d.per[s] = T * w[s] / den;
        dealt += slot_blocks(blocks, n_cu, s) * d.per[s];
    }
    d.n_cu = n_cu;
    d.leftover = static_sixteenths >= 16 ? n_jobs - dealt : 0;
    d.claim.per = T / blocks;
    d.claim.chunk = chunk_jobs < 1 ? 1 : chunk_jobs;
    d.claim.pool_begin = static_sixteenths >= 16 ? n_jobs : dealt;
    d.claim.n_chunks = (n_jobs - d.claim.pool_begin + d.claim.chunk - 1) / d.claim.chunk;
    return d;
}
// the static run of a block: compares, selects and three multiplications -- no division (the kernel runs this in front of its run loop)
constexpr JobRun slot_run(const SlotDeal &d, unsigned long long block)
{
    const unsigned s = (block >= d.n_cu ? 1u : 0u) + (block >= 2 * d.n_cu ? 1u : 0u) + (block >= 3 * d.n_cu ? 1u : 0u);
    const unsigned long long before = (s > 0 ? d.per[0] : 0) + (s > 1 ? d.per[1] : 0) + (s > 2 ? d.per[2] : 0);
    const unsigned long long per = s == 0 ? d.per[0] : s == 1 ? d.per[1] : s == 2 ? d.per[2] : d.per[3];
    const unsigned long long begin = d.n_cu * before + (block - s * d.n_cu) * per + (block < d.leftover ? block : d.leftover);
    return {begin, begin + per + (block < d.leftover ? 1 : 0)};
}
// the one call: block b's static run under (share, chunk, w)
constexpr JobRun weighted_run(unsigned long long n_jobs, unsigned long long blocks, unsigned long long n_cu, unsigned static_sixteenths, unsigned long long chunk_jobs,
                              const unsigned w[4], unsigned long long block)
{
    return slot_run(slot_deal(n_jobs, blocks, n_cu, static_sixteenths, chunk_jobs, w), block);
}

// The automatic rule (profiles/k1r_slot_weights.txt holds every figure).  It engages where the claimed tail always did (run_claim_engages: a
// static run of at least kClaimMinStatic jobs at 12/16).  Where the slots are the ones that were measured -- hop 256, more workgroups
// than three per CU, the device's own CU count -- the static runs carry the measured weights:
//   float and half rows   kSlotWeightsAuto, and the pool shrinks from 4/16 to 1/16 in chunks of 4 (the rates under a deep pool are
//                         78.6 / 73.2 / 56.4 / 47.8 and 76.9 / 70.4 / 59.5 / 49.1 of 256; one vector serves both within the noise)
//   complex rows          kSlotWeightsAutoComplex and no pool (rates 91.4 / 71.8 / 49.7 / 43.1; taken nearer to equal, the pool still loses)
// Elsewhere the deal stays the equal one, with the 4/16 pool for the float and half rows: at another hop the slots' rates are closer
// (hop 100: 69.5 / 66.4 / 62.2 / 57.9) and the weighted deal measured 2 % SLOWER than the equal one with its pool, and under a CU limit
// or with fewer workgroups than slots nothing is co-resident the way it was measured.  Forced weights (sgx_set_run_weights) apply anywhere.
constexpr unsigned kSlotWeightsEqual[4] = {64, 64, 64, 64};
constexpr unsigned kSlotWeightsAuto[4] = {80, 73, 56, 47};
constexpr unsigned kSlotWeightsAutoComplex[4] = {86, 72, 53, 45};
constexpr const unsigned *slot_weights_auto(bool complex_rows) { return complex_rows ? kSlotWeightsAutoComplex : kSlotWeightsAuto; }
constexpr unsigned kSlotAutoSixteenths = 15, kSlotAutoChunk = 4;
constexpr bool slot_weights_measured(unsigned long long blocks, unsigned long long n_cu, bool cu_limited, unsigned hop = 256) { return hop == 256 && !cu_limited && blocks > 3 * n_cu; }
constexpr bool slot_weights_equal(const unsigned w[4]) { return w[0] == 64 && w[1] == 64 && w[2] == 64 && w[3] == 64; }

}  // namespace sgx
