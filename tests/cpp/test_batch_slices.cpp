// test_batch_slices.cpp -- sumcheck_amd/csrc/batch_slices.hpp on the host: every (U <= 32, K, D <= 9, nv <= 16, round) against the rule
// restated from its parts -- which rounds are sliced, the slice size and count, what a block's LDS holds, the partials buffer, the lazy sums
// and the plan choice with its 16 GiB rule; and batch_shape.hpp's one spelling of the shape rule (batch_shape_fits, bt_lanes, bt_fin_bytes,
// batch_rounds_off) against formulas of this file's own.  Stand-alone; built with -fsanitize=address,undefined (tests/test_batch_round_slices_host.py).
#include <cstdint>
#include <cstdio>

#include "batch_slices.hpp"

using namespace scd;

static int g_fail = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            if (g_fail++ < 20) std::printf("FAIL %s:%d: %s  (U %u K %d D %d nv %u round %u)\n", __FILE__, __LINE__, #c, U, K, D, nv, j); \
        }                                                                     \
    } while (0)

constexpr size_t kLdsMax = 144 * 1024, kSlot = 48;                 // batch_round.hpp: kBtLdsMax, kBtEnt words
static size_t fin_bytes(int K, int D) { return (((size_t)K * D * (D + 2) * 32 + 15) / 16) * 16 + (size_t)D * 32; } // bt_fin_bytes
static bool fits(uint32_t log2_entries, uint32_t U, int K, int D) { return fin_bytes(K, D) + ((size_t)U << log2_entries) * kSlot <= kLdsMax; } // batch_shape_fits' LDS rule

int main() {
    uint64_t shapes = 0, sliced_rounds = 0, sliced_plans = 0, max_S = 0;
    uint32_t U = 0, nv = 0, j = 0;
    int K = 0, D = 0;
    static_assert(kBtLdsMax == kLdsMax && kBatchRoundSlotBytes == kSlot && kBtEnt * 4 == kSlot && kBsSliceLds <= kBtLdsMax, "the constants");
    // ---- bt_lanes at EVERY number of combinations: the largest power of two <= 64 with L x nc lanes inside the block ----
    for (int nc = 1; nc <= 24; ++nc) {
        const uint32_t L = (uint32_t)bt_lanes(nc);
        CHECK(L >= 1 && L <= 64 && (L & (L - 1)) == 0 && L * (uint32_t)nc <= 256 && (L == 64 || 2 * L * (uint32_t)nc > 256));
    }
    // ---- batch_rounds_off: depth b's region holds its 2^(nv - b) entries and ends where depth b + 1 begins; from depth 1 on the
    //      2^nv >> (b - 1) slots up to the end of the table's 2 x 2^nv ----
    for (nv = 1; nv <= 16; ++nv) {
        CHECK(batch_rounds_off(nv, 0) == 0 && batch_rounds_off(nv, 1) == (1ULL << nv)); // round 0's tables are never overwritten
        for (j = 1; j <= nv; ++j) { // (j: the depth)
            const uint64_t off = batch_rounds_off(nv, j), room = (1ULL << nv) >> (j - 1), entries = 1ULL << (nv - j);
            CHECK(off + room == (2ULL << nv));
            CHECK(j == nv ? off + entries <= (2ULL << nv) : off + entries == batch_rounds_off(nv, j + 1));
        }
    }
    nv = 0, j = 0;
    for (U = 1; U <= 32; ++U)
        for (K = 1; K <= 16; ++K)
            for (D = 2; D <= 9; ++D) { // (max_multiplicands = D - 1 <= 8)
                const uint32_t mm = (uint32_t)D - 1;
                CHECK(bt_fin_bytes(K, D) == fin_bytes(K, D));
                for (nv = 1; nv <= 16; ++nv) {
                    ++shapes;
                    CHECK(batch_shape_fits(nv, U, K, D, mm) == fits(nv, U, K, D));
                    CHECK(bt_lds_bytes(nv, U, K, D) == fin_bytes(K, D) + ((size_t)U << nv) * kSlot);
                    const bool env = bs_envelope(nv, U, K, D, mm);
                    CHECK(env == fits(nv < 2 ? nv : 2, U, K, D));
                    bool any_sliced = false, sums_hold = true;
                    for (j = 0; j < nv; ++j) {
                        const uint32_t loaded = nv - (j ? j - 1 : 0);
                        CHECK(bs_loaded_log2(nv, j) == loaded);
                        const bool sliced = bs_round_sliced(nv, j, U, K, D, mm);
                        CHECK(sliced == !fits(loaded, U, K, D)); // a round is sliced iff its loaded size does not fit
                        CHECK(batch_shape_fits(loaded, U, K, D, mm) == !sliced);
                        CHECK(br_lds_bytes(nv, j, U, K, D) == fin_bytes(K, D) + ((size_t)U << loaded) * kSlot);
                        if (j > 0) CHECK(!sliced || bs_round_sliced(nv, j - 1, U, K, D, mm)); // the sliced rounds are the first ones
                        if (!sliced || !env) continue;
                        any_sliced = true;
                        ++sliced_rounds;
                        const uint32_t es = bs_slice_log2(loaded, U, K, D), ss = bs_slices_log2(loaded, U, K, D);
                        const uint64_t Es = 1ULL << es, S = 1ULL << ss;
                        if (S > max_S) max_S = S;
                        CHECK(S >= 2 && S * Es == (1ULL << loaded));
                        CHECK(es >= 2);                                                    // a pair at least behind the bind
                        CHECK(U * Es * kSlot <= kBsSliceLds);                              // the block's dynamic LDS
                        CHECK(U * Es * kSlot + fin_bytes(K, D) <= kLdsMax);                // ... and with the finalize scratch one block's LDS
                        CHECK(es + 1 == loaded || U * (2 * Es) * kSlot > kBsSliceLds || U * (2 * Es) * kSlot + fin_bytes(K, D) > kLdsMax); // the largest such slice
                        CHECK(bs_block_pairs(es, j) == (j ? Es / 4 : Es / 2) && bs_block_pairs(es, j) >= 1);
                        CHECK(ss <= bs_slices_log2(nv, U, K, D));                          // round 0's S is the handle's largest
                        for (int nc = K; nc <= 24; nc += (nc < 8 ? 1 : 8)) {
                            const uint32_t L = (uint32_t)bt_lanes(nc), terms = (bs_block_pairs(es, j) + L - 1) / L;
                            CHECK(L >= 8 && L <= 64 && L * (uint32_t)nc <= 256 && (L == 64 || 2 * L * (uint32_t)nc > 256));
                            const bool hold = (uint64_t)(terms > 32 ? 33 : terms) * (j + 1) <= kLazySumMaxP;
                            CHECK(bs_lane_sums_hold(es, j, nc) == hold);
                            if (nc == 24 && !hold) sums_hold = false;
                        }
                    }
                    // ---- the partials buffer and the plan ----
                    j = 0;
                    const uint64_t n_list[] = {1, 3, 300, 1u << 20};
                    for (uint64_t n : n_list) {
                        const uint64_t work = 96 * n * U << nv;
                        CHECK(bs_work_bytes(n, U, nv) == work);
                        const int nc = 24;
                        const int plan = bs_plan(n, nv, U, K, D, mm, nc, true, 1, 1);
                        CHECK(bs_plan(n, nv, U, K, D, mm, nc, true, 0, 1) == kBrSerial);  // policy batch = 0
                        CHECK(bs_plan(n, nv, U, K, D, mm, nc, false, 1, 1) == kBrSerial); // the structure does not travel as arguments
                        const int plan0 = bs_plan(n, nv, U, K, D, mm, nc, true, 1, 0);    // the default: nothing changes
                        CHECK(plan0 == (fits(nv, U, K, D) ? kBrOneBlock : kBrSerial));
                        // one block exactly when the shape fits and the policy allows (what sc_batch_prover_init relies on)
                        for (int pol = 0; pol < 12; ++pol) {
                            const int pb = pol % 3, ps = (pol / 3) % 2;
                            const bool args = pol < 6;
                            CHECK((bs_plan(n, nv, U, K, D, mm, nc, args, pb, ps) == kBrOneBlock) == (pb != 0 && args && batch_shape_fits(nv, U, K, D, mm)));
                        }
                        if (fits(nv, U, K, D)) {
                            CHECK(plan == kBrOneBlock && !any_sliced);
                            continue;
                        }
                        const uint64_t S0 = env ? bs_max_slices(nv, U, K, D) : 0;
                        const bool want = env && work <= (16ULL << 30) && n * S0 < (1ULL << 31) && sums_hold;
                        CHECK((plan == kBrSlices) == want);                                // the 16 GiB rule among them
                        CHECK(plan == kBrSlices || plan == kBrSerial);
                        if (plan != kBrSlices) continue;
                        ++sliced_plans;
                        CHECK(any_sliced && bs_round_sliced(nv, 0, U, K, D, mm) && !bs_round_sliced(nv, nv - 1, U, K, D, mm));
                        CHECK(bs_partials_bytes(n, nv, U, K, D, nc) == n * S0 * nc * 32);  // n x S x n_combos elements
                        CHECK(bs_partials_bytes(n, nv, U, K, D, nc) < work);
                    }
                }
            }
    // beyond the limits the rule reads, nothing fits
    U = 33, K = 1, D = 2, nv = 4, j = 0;
    CHECK(batch_shape_fits(4, 32, 1, 2, 1) && !batch_shape_fits(4, 33, 1, 2, 1) && !batch_shape_fits(4, 0, 1, 2, 1));   // tables
    CHECK(batch_shape_fits(4, 2, 16, 2, 1) && !batch_shape_fits(4, 2, 17, 2, 1) && !batch_shape_fits(4, 2, 0, 2, 1));   // products
    CHECK(batch_shape_fits(4, 2, 1, 9, 8) && !batch_shape_fits(4, 2, 1, 9, 9));                                         // multiplicands
    CHECK(batch_shape_fits(4, 2, 1, 32, 8) && !batch_shape_fits(4, 2, 1, 33, 8));                                       // one lane per word of the message
    CHECK(batch_shape_fits(1, 1, 1, 2, 1) && !batch_shape_fits(0, 1, 1, 2, 1));                                         // variables
    CHECK(!batch_shape_fits(17, 1, 1, 2, 1) && !fits(16, 1, 1, 2) && !batch_shape_fits(16, 1, 1, 2, 1));
    // the shapes the GPU tests name: the envelope's ends and the number of sliced rounds, nv - nv_max + 1
    struct { uint32_t U; int K, D; uint32_t nv_max; } named[] = {{3, 1, 4, 9}, {2, 1, 3, 10}, {4, 2, 4, 9}, {3, 2, 4, 9}, {10, 4, 5, 8}, {6, 1, 7, 8}, {1, 1, 2, 11}, {8, 1, 9, 8}};
    for (const auto &s : named) {
        U = s.U, K = s.K, D = s.D;
        for (nv = s.nv_max + 1; nv <= 16; ++nv) {
            uint32_t count = 0;
            for (j = 0; j < nv; ++j) count += bs_round_sliced(nv, j, U, K, D, (uint32_t)D - 1) ? 1 : 0;
            CHECK(count == nv - s.nv_max + 1);
            CHECK(bs_plan(2, nv, U, K, D, (uint32_t)D - 1, K * D, true, 1, 1) == kBrSlices);
        }
        nv = s.nv_max, j = 0;
        CHECK(bs_plan(2, nv, U, K, D, (uint32_t)D - 1, K * D, true, 1, 1) == kBrOneBlock);
    }
    std::printf("%llu shapes, %llu sliced rounds, %llu sliced plans, largest S %llu\n", (unsigned long long)shapes, (unsigned long long)sliced_rounds,
                (unsigned long long)sliced_plans, (unsigned long long)max_S);
    if (g_fail) {
        std::printf("%d CHECKS FAILED\n", g_fail);
        return 1;
    }
    std::printf("ALL TESTS PASSED\n");
    return 0;
}
