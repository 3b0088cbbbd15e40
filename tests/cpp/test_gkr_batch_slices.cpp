// test_gkr_batch_slices.cpp -- the plan rule of a GKR batch handle (sumcheck_amd/csrc/batch_slices.hpp: gkr_bs_plan) on the host: dim 1 .. 22,
// nnz around the cap of 64 x 2^dim, n up to and beyond the 16 GiB rule, the four combinations of the policies "batch" and "batch_slices",
// against the rule restated from its parts; and for every handle of the sliced plan which rounds are sliced and that their lazy sums hold.
// Stand-alone; built with -fsanitize=address,undefined (tests/test_gkr_batch_round_slices_host.py).
#include <cstdint>
#include <cstdio>

#include "batch_slices.hpp"

using namespace scd;

static int g_fail = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            if (g_fail++ < 20) std::printf("FAIL %s:%d: %s  (dim %u n %llu nnz %llu batch %d slices %d round %u)\n", __FILE__, __LINE__, #c, dim, (unsigned long long)n, (unsigned long long)nnz, pb, ps, j); \
        }                                                                     \
    } while (0)

constexpr size_t kLdsMax = 144 * 1024, kSlot = 48;
constexpr int kCombos = 3;                                          // one product of two tables: nodes 0, 1, 2
static size_t fin_bytes() { return ((size_t)1 * 3 * 5 * 32 + 15) / 16 * 16 + 3 * 32; } // bt_fin_bytes(K = 1, D = 3)
static bool fits(uint32_t log2_entries) { return fin_bytes() + ((size_t)2 << log2_entries) * kSlot <= kLdsMax; }

int main() {
    uint32_t dim = 0, j = 0;
    uint64_t n = 0, nnz = 0, handles = 0, sliced = 0, sliced_rounds = 0;
    int pb = 0, ps = 0;
    static_assert(kGkrBatchMaxDim == 9 && kGkrBatchMaxNnzPerCell == 64 && kBsMaxNv == 16 && kBsMaxWorkBytes == (16ULL << 30), "the constants");
    CHECK(fits(10) && !fits(11)); // one block holds two tables of 2^10 entries: at dim 10 no round is sliced
    // gkr_batch_shape_fits (batch_shape.hpp): dim 1 .. 9 -- 224 B a cell and the finalize scratch within one block's LDS -- and nnz within the cap
    CHECK(fin_bytes() + ((size_t)224 << 9) <= kLdsMax && fin_bytes() + ((size_t)224 << 10) > kLdsMax && fin_bytes() + ((size_t)160 << 10) > kLdsMax);
    for (dim = 0; dim <= 22; ++dim) {
        const uint64_t cap = 64ULL << dim;
        CHECK(bg_lds_bytes(dim) == fin_bytes() + ((size_t)(2 * kSlot + 2 * 32 + 64) << dim));
        const uint64_t around[] = {cap - 1, cap, cap + 1};
        for (uint64_t nnz_ : around) {
            nnz = nnz_;
            CHECK(gkr_batch_shape_fits(dim, nnz) == (dim >= 1 && dim <= 9 && nnz <= cap));
        }
    }
    nnz = 0;
    for (dim = 1; dim <= 22; ++dim) {
        const uint64_t cap = 64ULL << dim;
        const uint64_t per_inst = 2 * (2 * 2 * kSlot << dim) + (64ULL << dim); // areas A and B, the cells
        const uint64_t n_fit = (16ULL << 30) / per_inst;                      // the largest n of the 16 GiB rule
        const uint64_t n_list[] = {1, 2, 6, 16, 256, n_fit - 1, n_fit, n_fit + 1, 2 * n_fit, 1ULL << 33};
        const uint64_t nnz_list[] = {0, 1, 1ULL << dim, cap - 1, cap, cap + 1, 2 * cap};
        for (uint64_t n_ : n_list)
            for (uint64_t nnz_ : nnz_list)
                for (pb = 0; pb <= 2; ++pb)
                    for (ps = 0; ps <= 1; ++ps) {
                        n = n_, nnz = nnz_, j = 0;
                        if (n == 0) continue;
                        ++handles;
                        const int plan = gkr_bs_plan(n, dim, nnz, kCombos, pb, ps);
                        const bool envelope = pb != 0 && nnz <= cap && dim <= 16;
                        if (dim <= 16) CHECK(gkr_bs_handle_bytes(n, dim) == n * per_inst);
                        int want = kGbrSerial;
                        if (envelope && dim <= 9) want = kGbrOneBlock;
                        else if (envelope && ps == 1 && dim >= 10 && n * per_inst <= (16ULL << 30)) want = kGbrSlices; // (every grid of such a handle is far below 2^31: checked below)
                        CHECK(plan == want);
                        CHECK((plan == kGbrOneBlock) == (pb != 0 && gkr_batch_shape_fits(dim, nnz))); // one block exactly when the shape fits and the policy allows (what sc_gkr_batch_prover_init relies on)
                        CHECK(gkr_bs_plan(n, dim, nnz, kCombos, pb, 0) == (envelope && dim <= 9 ? kGbrOneBlock : kGbrSerial)); // the default of the key: nothing changes
                        CHECK(gkr_bs_plan(n, dim, nnz, kCombos, 0, ps) == kGbrSerial);
                        if (plan != kGbrSlices) continue;
                        ++sliced;
                        // ---- the grids ----
                        const uint64_t B = gkr_bs_term_blocks(nnz);
                        CHECK(B >= 1 && B <= kBsGkrMaxTermBlocks && (B == kBsGkrMaxTermBlocks || B * kBsGkrTermsPerBlock >= nnz) && (B == 1 || (B - 1) * kBsGkrTermsPerBlock < nnz));
                        CHECK(B * kBsGkrTermsPerBlock >= nnz); // at the cap of dim 16 a lane still takes eight terms
                        CHECK(n * B < (1ULL << 31) && ((n << dim) / 256) < (1ULL << 31));
                        // ---- the rounds: sliced exactly while the tables as loaded do not fit one block, r = 0 .. dim - 10 for dim >= 11 ----
                        uint32_t count = 0;
                        for (j = 0; j < dim; ++j) {
                            const bool sl = bs_round_sliced(dim, j, 2, 1, 3, 2);
                            CHECK(sl == !fits(bs_loaded_log2(dim, j)));
                            CHECK(sl == (dim >= 11 && j <= dim - 10));
                            if (!sl) continue;
                            ++count, ++sliced_rounds;
                            const uint32_t loaded = bs_loaded_log2(dim, j), es = bs_slice_log2(loaded, 2, 1, 3), ss = bs_slices_log2(loaded, 2, 1, 3);
                            CHECK(bs_lane_sums_hold(es, j, kCombos));
                            CHECK(es == 9 && ss == loaded - 9);                 // two tables of 2^9 slots: 48 KB
                            CHECK((n << ss) < (1ULL << 31));
                            CHECK(ss <= bs_slices_log2(dim, 2, 1, 3));           // round 0's S is the handle's largest: the partials
                        }
                        j = 0;
                        CHECK(count == (dim >= 11 ? dim - 9 : 0));
                        CHECK(bs_partials_bytes(n, dim, 2, 1, 3, kCombos) == n * bs_max_slices(dim, 2, 1, 3) * kCombos * 32);
                        if (dim == 11) CHECK(bs_max_slices(dim, 2, 1, 3) == 4);
                        if (dim == 16) CHECK(bs_max_slices(dim, 2, 1, 3) == 128);
                    }
    }
    // the lanes of a cell at the cap: 2^32 x 64 x 2^16 = 2^54, far below wide_fold_cell's 2^63
    dim = 16, n = 1, nnz = 64ULL << 16, pb = 1, ps = 1;
    CHECK(((nnz << 32) >> 54) == 1);
    std::printf("%llu handles, %llu of the sliced plan, %llu sliced rounds\n", (unsigned long long)handles, (unsigned long long)sliced, (unsigned long long)sliced_rounds);
    if (g_fail) {
        std::printf("%d CHECKS FAILED\n", g_fail);
        return 1;
    }
    std::printf("ALL TESTS PASSED\n");
    return 0;
}
