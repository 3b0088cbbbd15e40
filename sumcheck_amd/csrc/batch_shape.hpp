// batch_shape.hpp -- the shape rule of the batched kernels: which shapes one block holds in LDS, and how much LDS a launch asks for.  The
// launchers (kernels_batch*.hip), the plans of the batch handles (batch_slices.hpp: bs_plan, gkr_bs_plan) and the non-interactive entry
// points (batch.hip) all read THIS spelling.  Plain constexpr integer code: it compiles for the device and, unchanged, for the host
// (tests/cpp/test_batch_slices.cpp and test_gkr_batch_slices.cpp check it against formulas of their own over every shape).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SC_BS_FN __host__ __device__ constexpr
#else
#define SC_BS_FN constexpr
#endif

namespace scd {

// ---- the limits the rule reads (what they bound: kernels.h, batch_round.hpp) ----
constexpr int kMaxFusedM = 8;       // products up to this many multiplicands run register-resident and fused with the bind
constexpr int kMaxSmallTables = 32; // table-pointer block that fits a kernel argument
constexpr int kMetaProds = 16;      // products whose finalize records travel as a kernel argument (FinMeta)
constexpr int kTsBlock = 256;       // lanes of a block of the LDS-resident round body
// an element in LDS: nine limbs in a 48-byte, 16-byte aligned slot (three ds_read_b128 / ds_write_b128 instead of nine 32-bit accesses)
constexpr int kBtEnt = 12;               // dwords per entry
constexpr size_t kBtLdsMax = 144 * 1024; // a launch's dynamic LDS: of the CU's 160 KB (k_tail_slices: one block per CU; its static LDS is ~3 KB)
constexpr size_t kBatchRoundSlotBytes = 48; // a slot of a batch work area: the LDS slot verbatim
static_assert(kBatchRoundSlotBytes == kBtEnt * sizeof(int32_t), "a work-area slot is an LDS entry");

// lanes per (product, node) combination of the LDS-resident round body (batch_round.hpp): a power of two, all of a combination's lanes in one wavefront
SC_BS_FN int bt_lanes(int n_combos) {
    int L = 64;
    while (L * n_combos > kTsBlock) L >>= 1;
    return L;
}
// finalize scratch | message: the head of a batched kernel's dynamic LDS
SC_BS_FN size_t bt_fin_bytes(int K, int D) { return (((size_t)K * D * (D + 2) * 32 + 15) & ~(size_t)15) + (size_t)D * 32; }
// a block's dynamic LDS with 2^loaded_log2 entries of each of n_tables tables behind that head ...
SC_BS_FN size_t bt_lds_bytes(uint32_t loaded_log2, uint32_t n_tables, int K, int D) { return bt_fin_bytes(K, D) + ((size_t)n_tables << loaded_log2) * (kBtEnt * 4); }
// ... and of round `round` (0-based) of a batch work area: the tables as loaded, bound max(round - 1, 0) times
SC_BS_FN size_t br_lds_bytes(uint32_t nv, uint32_t round, uint32_t n_tables, int K, int D) { return bt_lds_bytes(nv - (round ? round - 1 : 0), n_tables, K, D); }
// where a batch work area keeps a table bound `bound` times, in slots from the table's region of 2 x 2^nv (kernels.h: BatchRoundArgs)
SC_BS_FN uint64_t batch_rounds_off(uint32_t nv, uint32_t bound) { return bound ? (2ULL << nv) - ((1ULL << nv) >> (bound - 1)) : 0; }

// The envelope of k_batch_proofs and k_batch_round: one block holds 2^nv entries of all the tables behind the finalize scratch, products of
// <= kMaxFusedM multiplicands, the metadata within the kernel arguments.
SC_BS_FN bool batch_shape_fits(uint32_t nv, uint32_t n_tables, int K, int D, uint32_t max_multiplicands) {
    if (nv == 0 || nv > 16 || n_tables == 0 || n_tables > (uint32_t)kMaxSmallTables || K < 1 || K > kMetaProds || max_multiplicands > (uint32_t)kMaxFusedM) return false;
    if ((uint32_t)D * 8u > (uint32_t)kTsBlock) return false; // (one lane per word of the message)
    return bt_lds_bytes(nv, n_tables, K, D) <= kBtLdsMax;
}

// Batched GKR round proofs (k_batch_gkr, k_batch_gkr_phase): one product of two tables (K = 1, D = 3).  Per cell the two tables 2 x 48 B,
// eq(g, .) and eq(u, .) 2 x 32 B, the accumulator 64 B: 224 B x 2^dim + finalize scratch <= 144 KB holds to dim 9 (dim = 10 does not fit
// even with the eq tables as halves), and nnz <= kGkrBatchMaxNnzPerCell x 2^dim per instance (one block of 256 lanes walks the list twice:
// beyond that sc_gkr_prove's grids win).
constexpr int kGkrBatchMaxDim = 9;
constexpr uint64_t kGkrBatchMaxNnzPerCell = 64;
SC_BS_FN size_t bg_lds_bytes(uint32_t dim) { return bt_fin_bytes(1, 3) + ((size_t)1 << dim) * (2 * kBtEnt * 4 + 2 * 32 + 64); }
SC_BS_FN bool gkr_batch_shape_fits(uint32_t dim, uint64_t nnz_max) {
    if (dim == 0 || dim > (uint32_t)kGkrBatchMaxDim) return false;
    if (nnz_max > ((uint64_t)kGkrBatchMaxNnzPerCell << dim)) return false; // (one block walks the whole list twice)
    return bg_lds_bytes(dim) <= kBtLdsMax;
}

} // namespace scd
