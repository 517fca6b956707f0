// run_claim_check.cpp -- csrc/run_claim.hpp as a stand-alone program (tests/test_run_claim.py builds it with g++ -fsanitize=address,undefined):
// for every n_jobs 0 .. 5000, workgroup count, static share and chunk length, the jobs that the workgroups run -- their static runs and
// every claim index a launch can draw -- are counted in an array of exactly n_jobs cells (a job out of range is a sanitizer report).
//   every job exactly once; static runs contiguous from job 0 to the pool; chunks contiguous from the pool to n_jobs; a claim index past
//   the pool (a launch draws one per workgroup: n_chunks .. n_chunks + blocks - 1) is an empty run
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "run_claim.hpp"

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++fails < 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

int main()
{
    using namespace sgx;
    const unsigned long long blocks_of[] = {1, 4, 1023, 1024};
    const unsigned shares[] = {0, 8, 12, 16};
    const unsigned long long chunks[] = {1, 8, 64};
    unsigned long long cases = 0;
    for (unsigned long long n_jobs = 0; n_jobs <= 5000; ++n_jobs)
        for (unsigned long long blocks : blocks_of)
            for (unsigned s : shares)
                for (unsigned long long chunk : chunks) {
                    const RunClaim r = run_claim(n_jobs, blocks, s, chunk);
                    std::vector<unsigned char> taken(n_jobs, 0);
                    unsigned long long next = 0;
                    for (unsigned long long b = 0; b < blocks; ++b) {
                        const JobRun run = static_run(r, b);
                        CHECK(run.begin == next && run.end >= run.begin && run.end <= n_jobs, "static run n %llu blocks %llu s %u chunk %llu b %llu", n_jobs, blocks, s, chunk, b);
                        CHECK(run.end - run.begin == r.per, "static length");
                        for (unsigned long long j = run.begin; j < run.end; ++j) ++taken[j];
                        next = run.end;
                    }
                    CHECK(next == r.pool_begin && r.pool_begin <= n_jobs, "pool begin n %llu blocks %llu s %u", n_jobs, blocks, s);
                    CHECK(r.per * 16 * blocks <= n_jobs * s && (s != 16 || n_jobs - r.pool_begin < blocks), "share n %llu blocks %llu s %u per %llu", n_jobs, blocks, s, r.per);
                    CHECK(r.chunk == chunk, "chunk");
                    for (unsigned long long i = 0; i < r.n_chunks + blocks; ++i) {   // every index the counter can return in one launch
                        const JobRun run = claimed_run(r, n_jobs, i);
                        if (i < r.n_chunks) {
                            CHECK(run.begin == next && run.end > run.begin && run.end <= n_jobs && run.end - run.begin <= chunk, "chunk %llu of n %llu blocks %llu s %u chunk %llu", i, n_jobs, blocks, s, chunk);
                            CHECK(run.end - run.begin == chunk || i + 1 == r.n_chunks, "only the last chunk is short");
                            for (unsigned long long j = run.begin; j < run.end; ++j) ++taken[j];
                            next = run.end;
                        } else {
                            CHECK(run.begin == run.end && run.end <= n_jobs, "a claim past the pool is empty: %llu of %llu", i, r.n_chunks);
                        }
                    }
                    CHECK(next == n_jobs, "the chunks end at n_jobs: n %llu blocks %llu s %u chunk %llu", n_jobs, blocks, s, chunk);
                    for (unsigned long long j = 0; j < n_jobs; ++j) CHECK(taken[j] == 1, "job %llu taken %d times", j, (int)taken[j]);
                    ++cases;
                }
    // far from the test's range: no overflow in the share, a claim index at the end of 64 bits
    {
        const unsigned long long n = 0xffffffffffffffffull / 2;
        const RunClaim r = run_claim(n, 1024, 12, 8);
        CHECK(r.per == (n / 16 * 12 + n % 16 * 12 / 16) / 1024 && r.pool_begin <= n, "large n");
        const JobRun last = claimed_run(r, n, r.n_chunks - 1), past = claimed_run(r, n, 0xffffffffffffffffull);
        CHECK(last.end == n && last.begin < n && past.begin == past.end, "large n: last chunk and a claim past it");
    }
    // the automatic rule and the setter's arguments
    CHECK(!run_claim_engages(0, 1024) && !run_claim_engages(102, 4) && !run_claim_engages(340, 4) && !run_claim_engages(64 * 1024, 1024), "short launches stay static");
    CHECK(run_claim_engages(500000, 1023), "the 1e6-frame launch engages");
    CHECK(run_claim(500000, 1023, kClaimAutoSixteenths, kClaimAutoChunk).per >= kClaimMinStatic, "and keeps a long static run");
    CHECK(run_claim_valid(0, 0) && run_claim_valid(16, 0) && run_claim_valid(0, 1) && run_claim_valid(16, 1) && run_claim_valid(8, 1u << 20), "valid pairs");
    CHECK(!run_claim_valid(8, 0) && !run_claim_valid(17, 1) && !run_claim_valid(17, 0) && !run_claim_valid(8, (1u << 20) + 1), "invalid pairs");
    std::printf("%llu splits checked\n", cases);
    std::printf(fails ? "run claim FAILED\n" : "run claim ok\n");
    return fails ? 1 : 0;
}
