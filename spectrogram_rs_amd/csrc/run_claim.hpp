// run_claim.hpp -- a persistent launch whose workgroups take a static run of jobs each and then CLAIM the rest, chunk by chunk, from a pool.
// Plain C++ (no HIP): the launcher, the kernel and the CPU test (tests/cpp/run_claim_check.cpp) all read the split from here.
//
// Why: the workgroups of a store-bound launch do not run at one speed (profiles/k1r_claimed_tail.txt: the mono rows launch's workgroups
// finish between 0.58 and 0.99 of its duration, 0.83 on average), and with equal static runs the launch waits for the slowest while the
// CUs of the others idle.  The static part keeps what a long contiguous run is worth (the sliding window: one 8-byte load per thread and
// iteration); the pool, dealt in chunks long enough to pay for a window refill, is what lets every workgroup finish within one chunk of
// the others.
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

}  // namespace sgx
