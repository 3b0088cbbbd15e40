// batch_slices.hpp -- the sliced rounds of the batched interactive provers (kernels_batch_round_slices.hip, batch_rounds.hip): which rounds
// of a handle give an instance to several blocks, how large a block's slice is, and what the handle allocates for it.  Plain constexpr
// integer code: it compiles for the device and, unchanged, for the host (tests/cpp/test_batch_slices.cpp walks every shape).
//
// Round j of an instance of nv variables loads E_in = 2^(nv - max(j - 1, 0)) entries of each of its U tables (the tables bound
// max(j - 1, 0) times), binds them once (j > 0) and sums over the pairs.  Binding is LSB-first: entries [s E_s, (s + 1) E_s) of every table
// bind to entries [s E_s / 2, (s + 1) E_s / 2), so S = E_in / E_s blocks share an instance without ever reading what another block writes.
// A round is sliced exactly when its tables as loaded do not fit one block (batch_shape.hpp: batch_shape_fits, the one spelling of the
// rule, its limits and the LDS sizes); from the first round that fits, k_batch_round runs on the same work area.
#pragma once
#include <cstddef>
#include <cstdint>

#include "batch_shape.hpp"
#include "lane_sum.hpp"

namespace scd {

constexpr uint32_t kBsMaxNv = 16;                 // the work-area kernels' limit (k_batch_rounds_load / _export)
// A sliced block's tables.  Three blocks of 48 KB (+ ~1 KB of static LDS each) share a CU's 160 KB: a block is load | barrier | bind |
// barrier | sums | store, so a lone 144 KB block leaves its CU's four SIMDs idle through every load and store, while three smaller ones
// overlap one block's memory phase with another's arithmetic -- and a small batch (n = 1) gets three times the blocks.  Measured against
// 24 / 32 / 72 / 144 KB: the fastest or tied in every cell (profiles/batch_round_slices_lds_ab.txt).
#ifndef SC_BS_SLICE_LDS // (A/B builds: -DSC_BS_SLICE_LDS=73728)
#define SC_BS_SLICE_LDS (48 * 1024)
#endif
constexpr size_t kBsSliceLds = SC_BS_SLICE_LDS;
static_assert(kBsSliceLds <= kBtLdsMax, "a slice is within one block's dynamic LDS");
constexpr uint64_t kBsMaxWorkBytes = 16ULL << 30; // the work area of a sliced handle: the library's caches' default bound

// log2 of the entries per table round `round` (0-based) loads
SC_BS_FN uint32_t bs_loaded_log2(uint32_t nv, uint32_t round) { return nv - (round ? round - 1u : 0u); }
SC_BS_FN bool bs_round_sliced(uint32_t nv, uint32_t round, uint32_t U, int K, int D, uint32_t max_mult) {
    return !batch_shape_fits(bs_loaded_log2(nv, round), U, K, D, max_mult);
}
// Shapes whose LAST rounds fit one block (they load four entries per table, two when nv = 1): every round that does not fit then loads
// at least eight, and a slice of at least four leaves S >= 2 blocks a pair each after the bind.
SC_BS_FN bool bs_envelope(uint32_t nv, uint32_t U, int K, int D, uint32_t max_mult) {
    return nv >= 1 && nv <= kBsMaxNv && batch_shape_fits(nv < 2 ? nv : 2, U, K, D, max_mult);
}
// log2 E_s of a sliced round: the largest power of two whose U x E_s slots fit kBsSliceLds -- and, with the finalize scratch, one block's
// LDS -- and that leaves two slices.  The same for every block of a launch.  (bs_envelope: >= 2.)
SC_BS_FN uint32_t bs_slice_log2(uint32_t loaded_log2, uint32_t U, int K, int D) {
    const size_t room = kBtLdsMax - bt_fin_bytes(K, D), budget = room < kBsSliceLds ? room : kBsSliceLds;
    uint32_t e = loaded_log2 - 1u;
    while (e > 0 && ((size_t)U << e) * kBatchRoundSlotBytes > budget) --e;
    return e;
}
SC_BS_FN uint32_t bs_slices_log2(uint32_t loaded_log2, uint32_t U, int K, int D) { return loaded_log2 - bs_slice_log2(loaded_log2, U, K, D); }
// pairs a block sums over: round 0 does not bind
SC_BS_FN uint32_t bs_block_pairs(uint32_t slice_log2, uint32_t round) { return (1u << slice_log2) >> (round ? 2 : 1); }
// The lazy sums of a sliced round stay inside lane_sum.hpp's rule: a lane adds ceil(pairs / L) products of up to (round + 1) p each and
// reduces its sum every 32 of them (bt_combo_sum), so at most 32 terms and a reduced sum meet in its top limb; the shuffle tree is
// covered by lazy_sum_needs_reduce(pairs, round + 1) in the kernel itself.
SC_BS_FN bool bs_lane_sums_hold(uint32_t slice_log2, uint32_t round, int n_combos) {
    const uint32_t L = (uint32_t)bt_lanes(n_combos), pairs = bs_block_pairs(slice_log2, round), terms = (pairs + L - 1) / L;
    return !lazy_sum_needs_reduce(terms > 32 ? 33 : terms, round + 1u);
}
// slices per instance of round 0 and 1, the largest of a handle: the partials buffer is [instance][slice][combination] elements of 32 bytes
SC_BS_FN uint32_t bs_max_slices(uint32_t nv, uint32_t U, int K, int D) { return 1u << bs_slices_log2(nv, U, K, D); }
SC_BS_FN uint64_t bs_partials_bytes(uint64_t n, uint32_t nv, uint32_t U, int K, int D, int n_combos) {
    return n * bs_max_slices(nv, U, K, D) * (uint64_t)n_combos * 32u;
}
// the work area: every instance's tables at every binding depth, 2 x 2^nv slots per table
SC_BS_FN uint64_t bs_work_bytes(uint64_t n, uint32_t U, uint32_t nv) { return ((n * U * 2u * kBatchRoundSlotBytes) << nv); }

// ---- the plan of a batch handle (sc_batch_prover_init) ----
enum BatchRoundsPlan { kBrSerial = 0, kBrOneBlock = 1, kBrSlices = 2 };
// fits_args: SharedMeta::fits_args (the structure travels as kernel arguments); pol_batch / pol_slices: policy "batch" / "batch_slices"
SC_BS_FN int bs_plan(uint64_t n, uint32_t nv, uint32_t U, int K, int D, uint32_t max_mult, int n_combos, bool fits_args, int64_t pol_batch, int64_t pol_slices) {
    if (pol_batch == 0 || K < 1 || !fits_args || n == 0) return kBrSerial;
    if (batch_shape_fits(nv, U, K, D, max_mult)) return kBrOneBlock;
    if (pol_slices == 0 || !bs_envelope(nv, U, K, D, max_mult)) return kBrSerial;
    if (n > (1ULL << 32) || bs_work_bytes(n, U, nv) > kBsMaxWorkBytes) return kBrSerial;
    if ((n << bs_slices_log2(nv, U, K, D)) >= (1ULL << 31)) return kBrSerial; // (the grid of a sliced launch)
    for (uint32_t j = 0; j < nv && bs_round_sliced(nv, j, U, K, D, max_mult); ++j)
        if (!bs_lane_sums_hold(bs_slice_log2(bs_loaded_log2(nv, j), U, K, D), j, n_combos)) return kBrSerial;
    return kBrSlices;
}

// ---- the plan of a GKR batch handle (sc_gkr_batch_prover_init) ----
// Both phases are one product of two tables (U = 2, K = 1, D = 3, max_mult = 2).  Within gkr_batch_shape_fits (batch_shape.hpp: dim up to
// kGkrBatchMaxDim) the two initialisations run in one block per instance (k_batch_gkr_phase); beyond that dim, with policy
// "batch_slices" = 1, k_batch_gkr_terms / k_batch_gkr_fold (kernels_batch_gkr_round_slices.hip) give an instance to many blocks through
// wide cells in device memory, and the rounds are the sliced ones above.
constexpr uint64_t kBsGkrCellBytes = 64;          // eight uint64 lanes per cell
constexpr uint64_t kBsGkrTermsPerBlock = 8 * (uint64_t)kTsBlock; // non-zeros a block of k_batch_gkr_terms takes: eight per lane behind its two eq half tables
constexpr uint64_t kBsGkrMaxTermBlocks = 2048;    // ... blocks per instance at the most: beyond that a block grid-strides (64 x 2^16 / 2048 = 2048 per block, the same eight per lane)
enum GkrBatchRoundsPlan { kGbrSerial = 0, kGbrOneBlock = 1, kGbrSlices = 2 };
// blocks per instance of k_batch_gkr_terms, from the batch's largest list; an empty batch still gets one (it builds its eq tables and adds nothing)
SC_BS_FN uint64_t gkr_bs_term_blocks(uint64_t nnz_max) {
    const uint64_t b = (nnz_max + kBsGkrTermsPerBlock - 1) / kBsGkrTermsPerBlock;
    return b < 1 ? 1 : (b > kBsGkrMaxTermBlocks ? kBsGkrMaxTermBlocks : b);
}
// the handle's device memory that grows with the shape: areas A and B and the cells both phases share
SC_BS_FN uint64_t gkr_bs_handle_bytes(uint64_t n, uint32_t dim) { return 2 * bs_work_bytes(n, 2, dim) + ((n * kBsGkrCellBytes) << dim); }
SC_BS_FN int gkr_bs_plan(uint64_t n, uint32_t dim, uint64_t nnz_max, int n_combos, int64_t pol_batch, int64_t pol_slices) {
    if (pol_batch == 0 || n == 0 || dim == 0 || dim > kBsMaxNv) return kGbrSerial;
    if (nnz_max > (kGkrBatchMaxNnzPerCell << dim)) return kGbrSerial;
    if (gkr_batch_shape_fits(dim, nnz_max)) return kGbrOneBlock;
    if (pol_slices != 1 || !bs_envelope(dim, 2, 1, 3, 2)) return kGbrSerial;
    if (n > (1ULL << 32) || gkr_bs_handle_bytes(n, dim) > kBsMaxWorkBytes) return kGbrSerial;
    // the grids: a sliced round's, the terms kernel's, the fold kernel's (one lane per cell)
    if (bs_round_sliced(dim, 0, 2, 1, 3, 2) && (n << bs_slices_log2(dim, 2, 1, 3)) >= (1ULL << 31)) return kGbrSerial;
    if (n * gkr_bs_term_blocks(nnz_max) >= (1ULL << 31) || ((n << dim) + kTsBlock - 1) / kTsBlock >= (1ULL << 31)) return kGbrSerial;
    for (uint32_t j = 0; j < dim && bs_round_sliced(dim, j, 2, 1, 3, 2); ++j)
        if (!bs_lane_sums_hold(bs_slice_log2(bs_loaded_log2(dim, j), 2, 1, 3), j, n_combos)) return kGbrSerial;
    return kGbrSlices;
}

} // namespace scd
