// lane_sum.hpp -- how many terms a lane of a big-round kernel adds into its running sums, and what those sums hold.
// Plain constexpr code: kernels.h includes it for the launchers and the kernels, and it compiles unchanged for the host
// (tests/cpp/test_lane_sum.cpp enumerates it; tests/fe_model.py carries the accumulator itself).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SC_LANE_FN __host__ __device__ constexpr
#else
#define SC_LANE_FN constexpr
#endif

namespace scd {

constexpr int kBlock = 256;         // 4 wavefronts of 64
constexpr int kMaxGrid = 1024;      // 256 CUs x 4 resident 256-thread blocks; longer ranges are grid-strided
constexpr int kRoundTreeGrid = 768; // k_round_tree holds 3 blocks per CU (156 VGPRs, 46 KB LDS): one full wave of blocks on 256 CUs

// Lazy sums of carry-free elements (fe_carry_pass(fe_add(acc, x)), lane by lane and down a shuffle tree) never reduce limb 8: the int32
// top limb holds floor(sum / 2^232).  A term of magnitude p puts p >> 232 = 7597479 there (7597480 for a negative one), and
// 2^31 / 7597479 = 282.6: at most 282 terms of magnitude p may meet in one accumulator before it has to be reduced
// (fe_from_fr(fe_to_fr(acc)), exact for every int32 top limb).  The rule, wave-uniform: terms x (worst magnitude of a term in units of p).
constexpr uint32_t kLazySumMaxP = 282;
SC_LANE_FN bool lazy_sum_needs_reduce(uint64_t terms, uint32_t worst_p) { return terms * (uint64_t)worst_p > (uint64_t)kLazySumMaxP; }

// blocks of a grid-strided launch over n_pairs items, one item per lane and iteration; cap: kMaxGrid (the experiments build: SC_GRID)
SC_LANE_FN int grid_blocks_for_pairs(uint64_t n_pairs, int cap) {
    const uint64_t g = (n_pairs + kBlock - 1) / kBlock;
    return g < 1 ? 1 : g > (uint64_t)cap ? cap : (int)g;
}

// Blocks per product row of the merged big-round launch (k_round_tree_split / k_round1_tree_split), before grid_blocks_for_pairs caps
// them.  Measured per round size on config 3's FOUR rows (profiles/r2e_split_rounds.txt): many small blocks for the rounds that stream
// tables, fewer for the short ones.  What a short round needs is enough blocks in all to keep the per-lane chain at one iteration:
// fewer rows get proportionally more blocks per row in the rounds that no longer stream (< 2^21 pairs); the streaming rounds of a
// single row keep one full wave of resident blocks (a second, partial wave would run alone at the end).
// base: 0, or the experiments build's SC_SPLIT_GRID; by_rows = false: the per-row counts whatever the number of rows (an A/B build)
SC_LANE_FN int merged_row_blocks(uint64_t n_pairs, uint32_t n_rows, int base = 0, bool by_rows = true) {
    int g = base > 0 ? base : n_pairs >= (1ULL << 21) ? 1024 : n_pairs >= (1ULL << 20) ? 768 : n_pairs >= (1ULL << 18) ? 384 : n_pairs >= (1ULL << 17) ? 256 : 192;
    if (by_rows && n_rows < 4 && n_pairs < (1ULL << 21)) {
        g = g * 4 / (int)n_rows;
        return g < kMaxGrid ? g : kMaxGrid;
    }
    return n_rows == 1 && g > kRoundTreeGrid ? kRoundTreeGrid : g;
}

// tree_pass takes TWO pairs per iteration (b and b + stride; their products share one Montgomery reduction and make ONE term of a node's
// running sum) for two and three multiplicands, and for four where pairs4 says so (round 1; every round in the SC_M4_PAIRS A/B build)
SC_LANE_FN bool tree_two_pairs(int M, bool pairs4) { return M == 2 || M == 3 || (M == 4 && pairs4); }

// terms the busiest lane (thread 0 of block 0) adds into one running sum over a pass of `grid` blocks: the two-pair loop runs while a
// second pair exists, a last single pair makes a term of its own
SC_LANE_FN uint64_t tree_lane_terms(uint64_t n_pairs, int grid, bool two_pairs) {
    const uint64_t stride = (uint64_t)grid * kBlock, pairs = (n_pairs + stride - 1) / stride;
    return two_pairs ? (pairs + 1) / 2 : pairs;
}

// A lane's running sums are made canonical after every kBigSumReduceEvery terms, so at most that many terms and the reduced sum before
// them (below p) meet in the int32 top limb.  One term is a fe_mul / fe_mul2_sum result or -- a product of ONE table -- the raw entry
// as LoadFactor returns it: canonical, or settled by f29_settle into the packed format's [-2^255, 2^255) = +-1.104 p WHATEVER the number
// of binds behind it (f29_pack.hpp); a product of lines through such entries stays below 2 p (the widest is 1.77 p, two
// pairs of a product of four at nodes -1 and 2).  So the sums hold for every pass length: no launch has to choose an interval.
constexpr uint32_t kBigSumReduceEvery = 32;
constexpr uint32_t kBigTermWorstP = 2;
SC_LANE_FN uint64_t big_sum_terms(uint64_t lane_terms) { return (lane_terms < kBigSumReduceEvery ? lane_terms : kBigSumReduceEvery) + 1; }
static_assert((kBigSumReduceEvery & (kBigSumReduceEvery - 1)) == 0, "tree_pass masks the iteration count");
static_assert(!lazy_sum_needs_reduce(big_sum_terms(~0ULL), kBigTermWorstP), "a lane's running sum must fit its top limb between two reductions");

} // namespace scd
