// kernels_batch_round_slices.hip -- an interactive round of many provers whose tables do not fit one block (sc_batch_prove_round, plan
// batch.rounds_slices): k_batch_round's round (kernels_batch_rounds.hip) with every instance given to S blocks, as TWO plain launches.
//
//   k_batch_round_slices  n x S blocks.  Block (i, s) of round j loads entries [s E_s, (s + 1) E_s) of each of instance i's U tables from
//                         the work area's region of depth max(j - 1, 0), slots copied verbatim into LDS; binds them in place with the
//                         instance's challenge (j > 0); adds up every (product, node) combination over the pairs it holds; writes the
//                         sums, canonical, into partials[instance][slice][combination]; stores its E_s / 2 bound entries into the
//                         region of depth j at s E_s / 2 (j > 0).  It writes no message.
//   k_batch_round_fin     one block per instance, on the same stream directly behind: adds the S partials of every combination, runs
//                         finalize_message from the instance's matrices and stores the message where k_batch_round stores it.
// Binding is LSB-first, so a contiguous slice of every table binds to a contiguous slice (k_tail_slices rests on the same fact) and no
// block needs another's entries.  NOTHING HERE WAITS, as in kernels_batch_rounds.hip: no atomics, no counters, no "last block finishes",
// no fence -- a block reads only what an earlier launch wrote and writes only what a later launch reads; the order of the two kernels is
// the stream's.  The slot format, the offsets (batch_rounds_off) and the magnitudes are k_batch_round's: entries bound k times lie in
// (-k p, p), worst_p = round + 1, so the first round that fits one block is k_batch_round's on the same work area.
// The slice size, S and the buffer sizes: batch_slices.hpp.
#include "batch_round.hpp"
#include "batch_slices.hpp"

namespace scd {

template <int kSlots>
__global__ __launch_bounds__(kTsBlock) void k_batch_round_slices(const BatchRoundSlicesArgs A, const ComboMeta meta, const FinMeta fin) {
    extern __shared__ uint4 dyn_lds[];
    __shared__ uint64_t r_sh[4];
    __shared__ Combo combo_sh[kMetaCombos];
    __shared__ uint32_t slot_table_sh[kMetaSlots], slot_exp_sh[kMetaSlots];
    __shared__ int prod_index_sh[kMetaCombos];
    const int tid = threadIdx.x;
    const uint32_t inst = blockIdx.x >> A.slices_log2, sl = blockIdx.x & ((1u << A.slices_log2) - 1u); // (the grid is exactly n << slices_log2 blocks)
    const int U = (int)A.n_tables;
    const uint32_t cap = 1u << A.nv;    // entries per table in round 0
    const uint32_t Es = 1u << A.slice_log2; // entries per table this block loads
    bt_load_meta(meta, fin, A.n_combos, A.K, combo_sh, slot_table_sh, slot_exp_sh, prod_index_sh);
    if (tid < 4) r_sh[tid] = A.round ? reinterpret_cast<const uint64_t *>(A.chal)[(A.chal_shared ? 0 : (size_t)inst * 4) + tid] : 0;
    const struct { int32_t *tabs; uint32_t cap; int U; } T = {reinterpret_cast<int32_t *>(dyn_lds), Es, U}; // [table][Es][kBtEnt]
    const int L = bt_lanes(A.n_combos);
    // ---- the slice of the instance's current entries -> LDS, slot by slot -----------------------------------------------------------------
    int32_t *const region = A.work + (size_t)inst * A.n_tables * 2 * cap * kBtEnt; // table u at + u * 2 * cap slots
    {
        const uint64_t off_in = batch_rounds_off(A.nv, A.round ? A.round - 1u : 0u) + (uint64_t)sl * Es;
        const uint32_t total = Es * (uint32_t)U;
        for (uint32_t i = tid; i < total; i += kTsBlock) {
            const uint32_t u = i >> A.slice_log2, e = i & (Es - 1);
            const int4 *src = reinterpret_cast<const int4 *>(region + ((size_t)u * 2 * cap + off_in + e) * kBtEnt);
            int4 *dst = reinterpret_cast<int4 *>(T.tabs + (u * Es + e) * (uint32_t)kBtEnt);
            const int4 a = src[0], b = src[1], c = src[2];
            dst[0] = a;
            dst[1] = b;
            dst[2] = c;
        }
    }
    __syncthreads(); // (the metadata, the challenge and the slice)
    const BtLane<kSlots> ln = bt_lane<kSlots>(L, A.n_combos, Es, combo_sh, slot_table_sh, slot_exp_sh);
    uint32_t E = Es;
    if (A.round > 0) bt_bind_pass(T, E, bt_bind_multiplier(r_sh), false);
    // ---- sums: lane (combination, q) multiplies out the combination's pairs q, q + L, ... of this slice, as bt_sum_message does ----------
    const uint32_t pairs_here = E / 2;
    const Fe acc = bt_combo_sum(ln.combo_live, (uint32_t)ln.my_q, L, pairs_here, lazy_sum_needs_reduce(pairs_here, A.round + 1u), BtPairProduct<kSlots, decltype(T)>{T, ln, ln.my_nv});
    if (ln.combo_live && ln.my_q == 0) fr_store(A.partials + 2 * ((size_t)blockIdx.x * (uint32_t)A.n_combos + (uint32_t)ln.my_combo), fe_to_fr(acc));
    // ---- the bound entries -> this slice's half of the region of the next binding depth ------------------------------------------------------
    if (A.round > 0) {
        const uint64_t off_out = batch_rounds_off(A.nv, A.round) + (uint64_t)sl * E;
        const uint32_t total = E * (uint32_t)U;
        for (uint32_t i = tid; i < total; i += kTsBlock) {
            const uint32_t u = i >> (A.slice_log2 - 1u), e = i & (E - 1);
            br_slot_store(region + ((size_t)u * 2 * cap + off_out + e) * kBtEnt, bt_lds_load(T.tabs + (u * Es + e) * (uint32_t)kBtEnt));
        }
    }
}

// The partials are canonical elements and fr_add keeps its sum below p, so the running sum of up to 2^11 of them is an ordinary field sum:
// nothing lazy meets in a top limb here (lane_sum.hpp's rule holds with one term), and any order gives the reference's bits.
__global__ __launch_bounds__(kTsBlock) void k_batch_round_fin(const BatchRoundFinArgs A, const ComboMeta meta, const FinMeta fin) {
    extern __shared__ uint4 dyn_lds[];
    __shared__ Combo combo_sh[kMetaCombos];
    __shared__ uint32_t slot_table_sh[kMetaSlots], slot_exp_sh[kMetaSlots];
    __shared__ int prod_index_sh[kMetaCombos];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t inst = blockIdx.x; // (the grid is exactly n blocks)
    bt_load_meta(meta, fin, A.n_combos, A.K, combo_sh, slot_table_sh, slot_exp_sh, prod_index_sh);
    auto prod_of = [&](int k) -> FinProd { return fin.prod[k]; };
    uint4 *const fin_lds = dyn_lds;
    uint4 *const msg_lds = reinterpret_cast<uint4 *>(reinterpret_cast<char *>(dyn_lds) + A.fin_bytes - (uint32_t)A.D * 32u);
    __syncthreads(); // (the metadata)
    // ---- combination c0 + wave: lane l adds slices l, l + 64, ...; a shuffle tree adds the lanes -------------------------------------------
    const uint32_t S = 1u << A.slices_log2;
    const uint4 *const mine = A.partials + 2 * (((size_t)inst << A.slices_log2) * (uint32_t)A.n_combos);
    for (int c0 = 0; c0 < A.n_combos; c0 += kTsBlock / 64) { // (uniform trip count: every lane takes part in the shuffles)
        const int c = c0 + wave;
        const bool live = c < A.n_combos;
        Fr acc = fr_zero();
        if (live)
            for (uint32_t s = (uint32_t)lane; s < S; s += 64u) acc = fr_add(acc, fr_load(mine + 2 * ((size_t)s * (uint32_t)A.n_combos + (uint32_t)c)));
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc = fr_add(acc, fr_shfl_down(acc, off));
        if (live && lane == 0) fr_store(fin_lds + 2 * (prod_index_sh[c] * A.D + (int)combo_sh[c].t), acc); // (where bt_sum_message puts it)
    }
    __syncthreads();
    // ---- the message, from the instance's own matrices, into LDS and out ---------------------------------------------------------------------
    finalize_message<kTsBlock>(prod_of, A.Wm + 2 * (size_t)inst * A.w_stride, A.K, A.D, fin_lds, msg_lds, (uint64_t *)nullptr, (uint4 *)nullptr, (uint32_t *)nullptr, 0u, 1, (const Fr *)nullptr);
    __syncthreads();
    if ((uint32_t)tid < (uint32_t)A.D * 2u) A.out[(size_t)inst * A.D * 2 + tid] = msg_lds[tid];
}

hipError_t launch_batch_round_slices(BatchRoundArgs args, uint4 *partials, const ComboMeta &meta, const FinMeta &fin, hipStream_t stream) {
    if (args.n == 0 || args.round >= args.nv || args.nv > kBsMaxNv || !bs_envelope(args.nv, args.n_tables, args.K, args.D, (uint32_t)kMaxFusedM)) return hipErrorInvalidValue;
    if (args.n_combos < 1 || args.n_combos > kMetaCombos || !args.work || !args.Wm || !args.out || !partials || (args.round && !args.chal)) return hipErrorInvalidValue;
    const uint32_t loaded = bs_loaded_log2(args.nv, args.round);
    if (!bs_round_sliced(args.nv, args.round, args.n_tables, args.K, args.D, (uint32_t)kMaxFusedM)) return hipErrorInvalidValue; // (sliced rounds only: the others are launch_batch_round's)
    const uint32_t es = bs_slice_log2(loaded, args.n_tables, args.K, args.D), ss = loaded - es;
    const size_t lds = ((size_t)args.n_tables << es) * (kBtEnt * 4);
    if (es < 2 || ss < 1 || lds > kBsSliceLds || ((uint64_t)args.n << ss) >= (1ULL << 31) || !bs_lane_sums_hold(es, args.round, args.n_combos)) return hipErrorInvalidValue;
    static bool done[64] = {}; // (the finalize scratch of a long list may pass the default 64 KB limit of a launch)
    if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(k_batch_round_fin), (int)kBtLdsMax, done); e != hipSuccess) return e;
    if constexpr (kBsSliceLds > 64 * 1024) { // (an A/B build with larger slices: beyond the default limit of a launch)
        static bool done_slices[64] = {};
        if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(k_batch_round_slices<kMaxFusedM>), (int)kBsSliceLds, done_slices); e != hipSuccess) return e;
    }
    BatchRoundSlicesArgs S;
    S.work = args.work;
    S.chal = args.chal;
    S.chal_shared = args.chal_shared;
    S.partials = partials;
    S.n_tables = args.n_tables;
    S.nv = args.nv;
    S.round = args.round;
    S.n_combos = args.n_combos;
    S.K = args.K;
    S.slice_log2 = es;
    S.slices_log2 = ss;
    hipLaunchKernelGGL(k_batch_round_slices<kMaxFusedM>, dim3(args.n << ss), dim3(kTsBlock), lds, stream, S, meta, fin);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    BatchRoundFinArgs F;
    F.partials = partials;
    F.Wm = args.Wm;
    F.w_stride = args.w_stride;
    F.out = args.out;
    F.slices_log2 = ss;
    F.n_combos = args.n_combos;
    F.K = args.K;
    F.D = args.D;
    F.fin_bytes = (uint32_t)bt_fin_bytes(args.K, args.D);
    hipLaunchKernelGGL(k_batch_round_fin, dim3(args.n), dim3(kTsBlock), F.fin_bytes, stream, F, meta, fin);
    return hipGetLastError();
}

} // namespace scd
