// kernels_batch_rounds.hip -- one interactive round of many small provers in one launch (k_batch_round): sc_batch_prove_round.
//
// The interactive half of the batched provers: the caller owns the transcript (the reference takes fs_rng: &mut impl FeedableRNG), so
// every challenge exists before the round it belongs to is launched.  One block per instance runs ONE round of k_batch_proofs' body
// (batch_round.hpp) between a load from and a store to a device work area:
//   load     the instance's E current entries of all U tables, 48-byte slots copied verbatim into LDS;
//   bind     (not in round 0) in place with the instance's challenge, read from a device array uploaded in front of the launch;
//   sums     every (product, node) combination over its pairs, the block reduction, finalize_message from the instance's matrices;
//   store    the message as plain vector stores into the batch's output slab, the E / 2 bound entries back to the work area -- into the
//            region of the NEXT binding depth (kernels.h: batch_rounds_off), never over what this or another block reads.
// NOTHING HERE WAITS: no poll, no mailbox, no ticket, no tagged word; a block depends on its own instance's data and on nothing a
// concurrent block or the host writes.  Entries are stored as they are held in LDS, so their magnitudes are exactly k_batch_proofs':
// round j of tables loaded canonical has entries in (-j p, p) and worst_p = j + 1 (batch_round.hpp).
// k_batch_rounds_load fills round 0's slots from canonical tables; k_batch_rounds_export makes entries canonical again on the way out
// (sc_batch_prover_state), optionally binding them once more (sc_batch_prover_bind_final).
#include "batch_round.hpp"

namespace scd {

static_assert(kBatchRoundSlotBytes == kBtEnt * sizeof(int32_t), "the work area holds LDS slots verbatim");
// (a slot of the work area: br_slot_load / br_slot_store, batch_round.hpp)

template <int kSlots>
__global__ __launch_bounds__(kTsBlock) void k_batch_round(const BatchRoundArgs A, const ComboMeta meta, const FinMeta fin) {
    extern __shared__ uint4 dyn_lds[];
    __shared__ uint64_t r_sh[4];
    __shared__ uint32_t stop_sh; // (BtBlock's; never raised here)
    __shared__ Combo combo_sh[kMetaCombos];
    __shared__ uint32_t slot_table_sh[kMetaSlots], slot_exp_sh[kMetaSlots];
    __shared__ int prod_index_sh[kMetaCombos];
    const int tid = threadIdx.x;
    const uint32_t inst = blockIdx.x; // (the grid is exactly n blocks)
    const int U = (int)A.n_tables;
    const uint32_t cap = 1u << A.nv;                                 // entries per table in round 0
    const uint32_t E_in = A.round ? cap >> (A.round - 1u) : cap;     // entries per table as loaded: the tables bound max(round - 1, 0) times
    const int shE = (int)A.nv - (A.round ? (int)A.round - 1 : 0);    // log2 E_in
    bt_load_meta(meta, fin, A.n_combos, A.K, combo_sh, slot_table_sh, slot_exp_sh, prod_index_sh);
    if (tid < 4) r_sh[tid] = A.round ? reinterpret_cast<const uint64_t *>(A.chal)[(A.chal_shared ? 0 : (size_t)inst * 4) + tid] : 0;
    if (tid == 0) stop_sh = 0;
    auto prod_of = [&](int k) -> FinProd { return fin.prod[k]; };
    BtBlock B;
    B.fin_lds = dyn_lds;
    B.msg_lds = reinterpret_cast<uint4 *>(reinterpret_cast<char *>(dyn_lds) + A.fin_bytes - (uint32_t)A.D * 32u);
    B.tabs = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(dyn_lds) + A.fin_bytes); // [table][E_in][kBtEnt]
    B.r_sh = r_sh;
    B.stop_sh = &stop_sh;
    B.combo_sh = combo_sh;
    B.prod_index_sh = prod_index_sh;
    B.cap = E_in;
    B.U = U;
    B.n_combos = A.n_combos;
    B.K = A.K;
    B.D = A.D;
    B.mail_local = 0;
    B.max_spins = 0;
    B.Wm = A.Wm + 2 * (size_t)inst * A.w_stride;
    B.mail = nullptr;
    B.h_msg = nullptr;
    B.h_giveup = nullptr;
    B.L = bt_lanes(A.n_combos);
    // ---- the instance's current entries -> LDS, slot by slot ------------------------------------------------------------------------------
    int32_t *const region = A.work + (size_t)inst * A.n_tables * 2 * cap * kBtEnt; // table u at + u * 2 * cap slots
    {
        const uint64_t off_in = batch_rounds_off(A.nv, A.round ? A.round - 1u : 0u);
        const uint32_t total = E_in * (uint32_t)U;
        for (uint32_t i = tid; i < total; i += kTsBlock) {
            const uint32_t u = i >> shE, e = i & (E_in - 1);
            const int4 *src = reinterpret_cast<const int4 *>(region + ((size_t)u * 2 * cap + off_in + e) * kBtEnt);
            int4 *dst = reinterpret_cast<int4 *>(B.tabs + (u * E_in + e) * (uint32_t)kBtEnt);
            const int4 a = src[0], b = src[1], c = src[2];
            dst[0] = a;
            dst[1] = b;
            dst[2] = c;
        }
    }
    __syncthreads(); // (the metadata, the challenge and the tables)
    const BtLane<kSlots> ln = bt_lane<kSlots>(B, slot_table_sh, slot_exp_sh);
    uint32_t E = E_in;
    if (A.round > 0) bt_bind(B, E);
    bt_sum_message<kSlots>(B, ln, prod_of, E, A.round + 1u);
    // ---- the message: D elements of 32 bytes, one 16-byte store per lane --------------------------------------------------------------------
    if ((uint32_t)tid < (uint32_t)A.D * 2u) A.out[(size_t)inst * A.D * 2 + tid] = B.msg_lds[tid];
    // ---- the bound entries -> the region of the next binding depth ----------------------------------------------------------------------------
    if (A.round > 0) {
        const uint64_t off_out = batch_rounds_off(A.nv, A.round);
        const uint32_t total = E * (uint32_t)U;
        for (uint32_t i = tid; i < total; i += kTsBlock) {
            const uint32_t u = i >> (shE - 1), e = i & (E - 1);
            br_slot_store(region + ((size_t)u * 2 * cap + off_out + e) * kBtEnt, bt_lds_load(B.tabs + (u * E_in + e) * (uint32_t)kBtEnt));
        }
    }
}

__global__ __launch_bounds__(kTsBlock) void k_batch_rounds_load(const uint4 *const *__restrict__ tables, const uint64_t total, const uint32_t nv, int32_t *__restrict__ work) {
    const uint64_t i = (uint64_t)blockIdx.x * kTsBlock + threadIdx.x; // (table, entry)
    if (i >= total) return;
    const uint64_t t = i >> nv, e = i & ((1ULL << nv) - 1);
    br_slot_store(work + ((t * 2) << nv) * kBtEnt + e * kBtEnt, fe_from_fr(fr_load(tables[t] + 2 * e)));
}

__global__ __launch_bounds__(kTsBlock) void k_batch_rounds_export(const int32_t *__restrict__ work, const uint32_t first, const uint64_t total, const uint32_t n_tables, const uint32_t nv,
                                                                  const uint32_t bound, const uint4 *__restrict__ chal, const uint32_t chal_shared, uint4 *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * kTsBlock + threadIdx.x; // (instance - first, table, entry out)
    if (i >= total) return;
    const uint32_t sh_out = nv - bound - (chal ? 1u : 0u);
    const uint64_t t = i >> sh_out, e = i & ((1ULL << sh_out) - 1);
    const uint64_t il = t / n_tables;
    const int32_t *src = work + ((((uint64_t)first * n_tables + t) * 2) << nv) * kBtEnt + batch_rounds_off(nv, bound) * kBtEnt;
    Fe v;
    if (chal) {
        const FeU r32 = feu_shl5(fr_load(chal + 2 * (chal_shared ? 0 : (uint64_t)first + il)).v);
        const Fe lo = br_slot_load(src + 2 * e * kBtEnt), hi = br_slot_load(src + (2 * e + 1) * kBtEnt);
        v = fe_carry_pass(fe_add(lo, fe_mul_u<true>(fe_sub(hi, lo), r32)));
    } else {
        v = br_slot_load(src + e * kBtEnt);
    }
    fr_store(out + 2 * i, fe_to_fr(v));
}

// (the launch's dynamic LDS, finalize scratch | message | the tables as loaded: br_lds_bytes, batch_shape.hpp)
hipError_t launch_batch_round(BatchRoundArgs args, const ComboMeta &meta, const FinMeta &fin, hipStream_t stream) {
    if (args.n == 0 || args.round >= args.nv || args.nv > 16 || !batch_shape_fits(args.nv - (args.round ? args.round - 1 : 0), args.n_tables, args.K, args.D, (uint32_t)kMaxFusedM)) return hipErrorInvalidValue;
    if (args.n_combos < 1 || args.n_combos > kMetaCombos || !args.work || !args.Wm || !args.out || (args.round && !args.chal)) return hipErrorInvalidValue;
    static bool done[64] = {}; // (more dynamic LDS than the default 64 KB limit of a launch)
    if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(k_batch_round<kMaxFusedM>), (int)kBtLdsMax, done); e != hipSuccess) return e;
    args.fin_bytes = (uint32_t)bt_fin_bytes(args.K, args.D);
    hipLaunchKernelGGL(k_batch_round<kMaxFusedM>, dim3(args.n), dim3(kTsBlock), br_lds_bytes(args.nv, args.round, args.n_tables, args.K, args.D), stream, args, meta, fin);
    return hipGetLastError();
}

hipError_t launch_batch_rounds_load(const uint4 *const *tables, uint32_t n, uint32_t n_tables, uint32_t nv, int32_t *work, hipStream_t stream) {
    if (n == 0 || n_tables == 0 || nv == 0 || nv > 16 || !tables || !work) return hipErrorInvalidValue;
    const uint64_t total = ((uint64_t)n * n_tables) << nv, blocks = (total + kTsBlock - 1) / kTsBlock;
    if (blocks >= (1ULL << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_batch_rounds_load, dim3((uint32_t)blocks), dim3(kTsBlock), 0, stream, tables, total, nv, work);
    return hipGetLastError();
}

hipError_t launch_batch_rounds_export(const int32_t *work, uint32_t first, uint32_t count, uint32_t n_tables, uint32_t nv, uint32_t bound, const uint4 *chal_or_null,
                                      uint32_t chal_shared, uint4 *out, hipStream_t stream) {
    if (count == 0 || n_tables == 0 || nv == 0 || nv > 16 || bound + (chal_or_null ? 1u : 0u) > nv || !work || !out) return hipErrorInvalidValue;
    const uint64_t total = ((uint64_t)count * n_tables) << (nv - bound - (chal_or_null ? 1u : 0u)), blocks = (total + kTsBlock - 1) / kTsBlock;
    if (blocks >= (1ULL << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_batch_rounds_export, dim3((uint32_t)blocks), dim3(kTsBlock), 0, stream, work, first, total, n_tables, nv, bound, chal_or_null, chal_shared, out);
    return hipGetLastError();
}

} // namespace scd
