// run_weights_check.cpp -- the weighted deal of csrc/run_claim.hpp as a stand-alone program (tests/test_run_weights.py builds it with
// g++ -fsanitize=address,undefined): for every n_jobs 0 .. 5000, (workgroups, CUs), static share, chunk length and weight vector, the jobs
// that the workgroups run -- their static runs by slot and every claim index a launch can draw -- are counted in an array of exactly
// n_jobs cells (a job out of range is a sanitizer report).
//   every job exactly once; static runs contiguous and in block order from job 0 to the pool; chunks contiguous from the pool to n_jobs;
//   share 16: an exact partition with an empty pool, the leftover one each to the first blocks; equal weights with a pool: exactly
//   static_run / claimed_run of run_claim; a run is the slot's length; the one-call form agrees with the two-step form
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "run_claim.hpp"

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++fails < 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

int main()
{
    using namespace sgx;
    const unsigned long long grids[][2] = {{1, 1}, {4, 1}, {7, 2}, {8, 2}, {1023, 256}, {1024, 256}};   // workgroups x CUs
    const unsigned shares[] = {0, 8, 15, 16};
    const unsigned long long chunks[] = {1, 8};
    const unsigned weights[][4] = {{64, 64, 64, 64}, {88, 80, 48, 40}, {253, 1, 1, 1}, {1, 1, 1, 253}};
    unsigned long long cases = 0;
    for (unsigned long long n_jobs = 0; n_jobs <= 5000; ++n_jobs)
        for (const auto &g : grids)
            for (unsigned s : shares)
                for (unsigned long long chunk : chunks)
                    for (const auto &w : weights) {
                        const unsigned long long blocks = g[0], n_cu = g[1];
                        const SlotDeal d = slot_deal(n_jobs, blocks, n_cu, s, chunk, w);
                        std::vector<unsigned char> taken(n_jobs, 0);
                        unsigned long long next = 0, in_slot[4] = {0, 0, 0, 0};
                        for (unsigned long long b = 0; b < blocks; ++b) {
                            const JobRun run = slot_run(d, b), one = weighted_run(n_jobs, blocks, n_cu, s, chunk, w, b);
                            const unsigned long long slot = slot_of(b, n_cu);
                            CHECK(run.begin == next && run.end >= run.begin && run.end <= n_jobs, "static run n %llu blocks %llu s %u chunk %llu w0 %u b %llu: [%llu, %llu) after %llu",
                                  n_jobs, blocks, s, chunk, w[0], b, run.begin, run.end, next);
                            CHECK(one.begin == run.begin && one.end == run.end, "the one call");
                            CHECK(slot < 4 && run.end - run.begin == d.per[slot] + (b < d.leftover ? 1 : 0), "a run is its slot's length");
                            for (unsigned long long j = run.begin; j < run.end && j < n_jobs; ++j) ++taken[j];
                            next = run.end;
                            ++in_slot[slot];
                        }
                        for (unsigned q = 0; q < 4; ++q) CHECK(in_slot[q] == slot_blocks(blocks, n_cu, q), "blocks of slot %u", q);
                        CHECK(next == d.claim.pool_begin && d.claim.pool_begin <= n_jobs, "pool begin n %llu blocks %llu s %u w0 %u", n_jobs, blocks, s, w[0]);
                        CHECK(next * 16 <= n_jobs * s, "the static share n %llu blocks %llu s %u w0 %u", n_jobs, blocks, s, w[0]);
                        if (s == 16) CHECK(next == n_jobs && d.claim.n_chunks == 0 && d.leftover < blocks, "share 16 partitions exactly: n %llu blocks %llu w0 %u", n_jobs, blocks, w[0]);
                        else CHECK(d.leftover == 0, "a pool takes the leftover");
                        if (slot_weights_equal(w) && s < 16) {   // exactly today's split
                            const RunClaim r = run_claim(n_jobs, blocks, s, chunk);
                            CHECK(r.pool_begin == d.claim.pool_begin && r.n_chunks == d.claim.n_chunks && r.chunk == d.claim.chunk && r.per == d.claim.per, "equal weights: run_claim's pool");
                            for (unsigned long long b = 0; b < blocks; ++b) {
                                const JobRun a = static_run(r, b), c = slot_run(d, b);
                                CHECK(a.begin == c.begin && a.end == c.end, "equal weights: run_claim's static run of block %llu", b);
                            }
                            for (unsigned long long i = 0; i < r.n_chunks + 2; ++i) {
                                const JobRun a = claimed_run(r, n_jobs, i), c = claimed_run(d.claim, n_jobs, i);
                                CHECK(a.begin == c.begin && a.end == c.end, "equal weights: run_claim's chunk %llu", i);
                            }
                        }
                        for (unsigned long long i = 0; i < d.claim.n_chunks + blocks; ++i) {   // every index the counter can return in one launch
                            const JobRun run = claimed_run(d.claim, n_jobs, i);
                            if (i < d.claim.n_chunks) {
                                CHECK(run.begin == next && run.end > run.begin && run.end <= n_jobs && run.end - run.begin <= chunk, "chunk %llu of n %llu blocks %llu s %u", i, n_jobs, blocks, s);
                                for (unsigned long long j = run.begin; j < run.end && j < n_jobs; ++j) ++taken[j];
                                next = run.end;
                            } else {
                                CHECK(run.begin == run.end && run.end <= n_jobs, "a claim past the pool is empty");
                            }
                        }
                        CHECK(next == n_jobs, "the chunks end at n_jobs: n %llu blocks %llu s %u chunk %llu", n_jobs, blocks, s, chunk);
                        for (unsigned long long j = 0; j < n_jobs; ++j) CHECK(taken[j] == 1, "job %llu taken %d times (n %llu blocks %llu s %u w0 %u)", j, (int)taken[j], n_jobs, blocks, s, w[0]);
                        ++cases;
                    }
    // far from the sweep's range: no product overflows below 2^63 / 1024
    {
        const unsigned long long n = (1ull << 53) - 1;
        const unsigned w[4] = {253, 1, 1, 1};
        for (unsigned s : {15u, 16u}) {
            const SlotDeal d = slot_deal(n, 1023, 256, s, 8, w);
            const JobRun first = slot_run(d, 0), last = slot_run(d, 1022);
            CHECK(first.begin == 0 && last.end == d.claim.pool_begin && d.claim.pool_begin <= n && d.per[0] > d.per[1] && d.per[1] == d.per[3], "large n, share %u", s);
            CHECK(s != 16 || (last.end == n && d.leftover < 1023), "large n partitions");
        }
    }
    // the weights the setter accepts, and the automatic ones
    {
        const unsigned ok[4] = {88, 80, 48, 40}, zero[4] = {128, 0, 64, 64}, low[4] = {64, 64, 64, 63}, high[4] = {64, 64, 64, 65}, wrap[4] = {0xffffff00u, 1, 255, 256};
        CHECK(run_weights_valid(ok) && run_weights_valid(kSlotWeightsEqual) && run_weights_valid(kSlotWeightsAuto) && run_weights_valid(kSlotWeightsAutoComplex), "valid weights");
        CHECK(!run_weights_valid(zero) && !run_weights_valid(low) && !run_weights_valid(high) && !run_weights_valid(wrap), "invalid weights");
        CHECK(slot_weights_measured(1023, 256, false) && slot_weights_measured(1024, 256, false) && !slot_weights_measured(768, 256, false) && !slot_weights_measured(4, 1, true), "where the measured weights apply");
        CHECK(kSlotAutoSixteenths >= 14 && kSlotAutoSixteenths < 16 && kSlotAutoChunk >= 1, "a pool of at most 2/16");
        CHECK(run_claim(500000, 1023, kSlotAutoSixteenths, kSlotAutoChunk).per >= kClaimMinStatic, "and a long static run");
    }
    std::printf("%llu deals checked\n", cases);
    std::printf(fails ? "run weights FAILED\n" : "run weights ok\n");
    return fails ? 1 : 0;
}
