// test_lane_sum.cpp -- sumcheck_amd/csrc/lane_sum.hpp on the host: the grid of every big round and the terms its busiest lane adds into
// one running sum, against tree_pass's two loops restated lane by lane, and -- `--table` -- the enumeration that
// tests/test_fe_model_host.py feeds into the exact model of the accumulator.  Stand-alone; built with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "lane_sum.hpp"

using namespace scd;

static int g_fail = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            if (g_fail++ < 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                                     \
    } while (0)

constexpr uint64_t kSmallRoundPairs = 1u << 14; // kernels.h: rounds at or below this many pairs are not big rounds
constexpr int kMaxNv = 40;                      // validate_desc

// tree_pass's loops for one lane: how often `iter` is incremented, i.e. how many terms every running sum of the lane takes
static uint64_t lane_terms_by_loop(uint64_t n_pairs, int grid, bool two_pairs, uint64_t first) {
    const uint64_t stride = (uint64_t)grid * kBlock;
    uint64_t b = first, iter = 0;
    if (two_pairs)
        for (; b + stride < n_pairs; b += 2 * stride, ++iter) {}
    for (; b < n_pairs; b += stride, ++iter) {}
    return iter;
}

// the grid of a big round of n_pairs pairs: rows = 0: one launch per product (grid_for_pairs); else the merged launch of `rows` products
static int round_grid(uint64_t n_pairs, uint32_t rows, int cap) {
    const int g = grid_blocks_for_pairs(n_pairs, cap);
    return rows == 0 ? g : std::min(g, merged_row_blocks(n_pairs, rows));
}

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "--table") == 0) {
        // nv round rows M grid terms two_pairs: every big round of every nv the library admits, under the production cap
        for (int nv = 15; nv <= kMaxNv; ++nv)
            for (int round = 1; round < nv && (1ULL << (nv - round)) > kSmallRoundPairs; ++round)
                for (uint32_t rows : {0u, 1u, 2u, 3u, 4u, 12u})
                    for (int M = 1; M <= 4; ++M) {
                        const uint64_t n_pairs = 1ULL << (nv - round);
                        const int grid = round_grid(n_pairs, rows, kMaxGrid);
                        const bool two = tree_two_pairs(M, round == 1);
                        std::printf("%d %d %u %d %d %llu %d\n", nv, round, rows, M, grid, (unsigned long long)tree_lane_terms(n_pairs, grid, two), two ? 1 : 0);
                    }
        return 0;
    }
    // grid_blocks_for_pairs: one lane per pair up to the cap, never zero blocks
    CHECK(grid_blocks_for_pairs(0, kMaxGrid) == 1 && grid_blocks_for_pairs(1, kMaxGrid) == 1 && grid_blocks_for_pairs(256, kMaxGrid) == 1);
    CHECK(grid_blocks_for_pairs(257, kMaxGrid) == 2 && grid_blocks_for_pairs(1ULL << 18, kMaxGrid) == 1024 && grid_blocks_for_pairs(1ULL << 39, kMaxGrid) == 1024);
    CHECK(grid_blocks_for_pairs(1ULL << 13, 1) == 1 && grid_blocks_for_pairs(1ULL << 13, 2) == 2 && grid_blocks_for_pairs(1ULL << 13, 256) == 32);
    // merged_row_blocks: the measured table for four rows and more, proportionally more for fewer, one wave of resident blocks for one streaming row
    CHECK(merged_row_blocks(1ULL << 23, 4) == 1024 && merged_row_blocks(1ULL << 20, 4) == 768 && merged_row_blocks(1ULL << 19, 4) == 384);
    CHECK(merged_row_blocks(1ULL << 17, 4) == 256 && merged_row_blocks(1ULL << 15, 12) == 192);
    CHECK(merged_row_blocks(1ULL << 23, 1) == 768 && merged_row_blocks(1ULL << 21, 1) == 768 && merged_row_blocks(1ULL << 21, 2) == 1024);
    CHECK(merged_row_blocks(1ULL << 20, 1) == 1024 && merged_row_blocks(1ULL << 15, 1) == 768 && merged_row_blocks(1ULL << 15, 2) == 384 && merged_row_blocks(1ULL << 15, 3) == 256);
    CHECK(merged_row_blocks(1ULL << 15, 1, 100) == 400 && merged_row_blocks(1ULL << 15, 1, 0, false) == 192 && merged_row_blocks(1ULL << 23, 1, 0, false) == 768);
    // the grid a staged round 1 cuts into sections (protocol.hip, staged_copy_and_round1: spelled out there as it is here) is merged_row_blocks
    // with by_rows = false, over every shape staged_init_applies admits (nv >= 18: 2^17 pairs and more; one to kMetaProds = 16 rows)
    for (int lg = 17; lg <= 33; ++lg)
        for (uint32_t rows = 1; rows <= 16; ++rows)
            for (int cap : {kMaxGrid, 256, 1}) { // (grid_for_pairs: the production cap, and the experiments build's SC_GRID)
                const uint64_t n_pairs = 1ULL << lg;
                int G = n_pairs >= (1ULL << 21) ? 1024 : n_pairs >= (1ULL << 20) ? 768 : n_pairs >= (1ULL << 18) ? 384 : n_pairs >= (1ULL << 17) ? 256 : 192;
                if (rows == 1) G = std::min(G, kRoundTreeGrid);
                G = std::min(G, grid_blocks_for_pairs(n_pairs, cap));
                CHECK(std::min(merged_row_blocks(n_pairs, rows, 0, /*by_rows=*/false), grid_blocks_for_pairs(n_pairs, cap)) == G);
                CHECK(cap != kMaxGrid || G == (lg >= 21 ? (rows == 1 ? 768 : 1024) : lg == 20 ? 768 : lg >= 18 ? 384 : 256));
            }
    CHECK(tree_two_pairs(2, false) && tree_two_pairs(3, false) && !tree_two_pairs(1, true) && !tree_two_pairs(4, false) && tree_two_pairs(4, true));
    // tree_lane_terms is the busiest lane's count under the kernel's own loops, for every grid and pair count (powers of two and not)
    for (int grid : {1, 2, 3, 7, 192, 768, 1024})
        for (uint64_t n_pairs : {1ULL, 255ULL, 256ULL, 257ULL, 1ULL << 13, (1ULL << 13) + 1, 3ULL << 12, 1ULL << 18, (1ULL << 18) + 5, 1ULL << 24, (1ULL << 24) - 1})
            for (bool two : {false, true}) {
                uint64_t most = 0;
                const uint64_t lanes = (uint64_t)grid * kBlock;
                for (uint64_t first : {(uint64_t)0, (uint64_t)1, lanes / 2, lanes - 1}) most = std::max(most, lane_terms_by_loop(n_pairs, grid, two, first));
                CHECK(lane_terms_by_loop(n_pairs, grid, two, 0) == most);
                CHECK(tree_lane_terms(n_pairs, grid, two) == most);
            }
    // the shapes of tests/test_gpu_big_sum_bounds.py: round 10 of 23 variables on one block is 32 terms a lane, on two blocks 16
    CHECK(tree_lane_terms(1ULL << 13, round_grid(1ULL << 13, 1, 1), false) == 32 && tree_lane_terms(1ULL << 13, round_grid(1ULL << 13, 1, 2), false) == 16);
    CHECK(tree_lane_terms(1ULL << 13, round_grid(1ULL << 13, 2, 1), true) == 16 && tree_lane_terms(1ULL << 13, round_grid(1ULL << 13, 0, 1), false) == 32);
    // production grids: a lane still makes kBigSumReduceEvery terms of round 10 from 33 variables on (768 blocks; 1024: from 34 on)
    CHECK(tree_lane_terms(1ULL << 23, round_grid(1ULL << 23, 1, kMaxGrid), false) == 43 && tree_lane_terms(1ULL << 22, round_grid(1ULL << 22, 1, kMaxGrid), false) == 22);
    CHECK(tree_lane_terms(1ULL << 23, round_grid(1ULL << 23, 0, kMaxGrid), false) == 32);
    // the rule: whatever the pass length, at most kBigSumReduceEvery terms and the reduced sum meet, and at kBigTermWorstP p each they fit
    CHECK(big_sum_terms(1) == 2 && big_sum_terms(31) == 32 && big_sum_terms(32) == 33 && big_sum_terms(1ULL << 40) == 33);
    CHECK(!lazy_sum_needs_reduce(big_sum_terms(1ULL << 40), kBigTermWorstP) && lazy_sum_needs_reduce(big_sum_terms(32), 9) && !lazy_sum_needs_reduce(big_sum_terms(32), 8));
    CHECK((uint64_t)kLazySumMaxP == (1ULL << 31) / 7597479ULL);
    if (g_fail) {
        std::printf("%d CHECKS FAILED\n", g_fail);
        return 1;
    }
    std::printf("ALL TESTS PASSED\n");
    return 0;
}
