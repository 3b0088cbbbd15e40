// kernels_batch.hip -- many small independent proofs in one launch (k_batch_proofs): sc_ml_prove_batch.
//
// A whole proof over 2^6 .. 2^10 entries is 6 .. 10 latency-bound rounds of 12-15 us each, with a few microseconds of arithmetic in
// them.  A caller with many such instances (a GKR prover's side claims, a lookup argument per column) gains nothing from
// proving them one after the other: the GPU idles through every round trip.  Binding is LSB-first, so a block that holds ALL of an
// instance's tables never needs another block -- "one block finishes the proof alone, out of LDS" is the last phase of k_tail_slices
// (kernels_tail.hip); here it is the whole proof, once per instance, with every instance in flight at once:
//   a block      takes an instance number from the ticket; loads the instance's U tables into LDS as nine 29-bit limbs; then per round
//                multiplies out every (product, node) combination over its pairs (k_tail_slices' lane mapping), reduces within the
//                block, forms the message from the INSTANCE's own weight matrices (its coefficients are folded in), publishes it into
//                the instance's slot of a host-mapped page as self-validating words (limb | tag << 32), polls the instance's own
//                mailbox slot for the challenge, binds in place; after the last message it takes the next ticket.
//   the host     serves whichever instance's message has appeared (batch.hip): copy, hash, sample, post.
// NO BLOCK EVER WAITS FOR ANOTHER BLOCK: a grid larger than what is resident is safe, the host may answer in any order.  Every wait
// for the host is bounded (policy "wait_spins"); a block whose wait expires raises its instance's give-up marker and moves on -- the
// host proves that instance again by the serial plan, and nothing computed on a stale challenge is ever published.
#include "batch_round.hpp"

namespace scd {

template <int kSlots>
__global__ __launch_bounds__(kTsBlock) void k_batch_proofs(const BatchArgs A, const ComboMeta meta, const FinMeta fin) {
    extern __shared__ uint4 dyn_lds[];
    __shared__ uint64_t r_sh[4];
    __shared__ uint32_t stop_sh, inst_sh;
    __shared__ Combo combo_sh[kMetaCombos];
    __shared__ uint32_t slot_table_sh[kMetaSlots], slot_exp_sh[kMetaSlots];
    __shared__ int prod_index_sh[kMetaCombos];
    const int tid = threadIdx.x;
    const int U = (int)A.n_tables;
    const uint32_t cap = 1u << A.nv; // entries per table
    bt_load_meta(meta, fin, A.n_combos, A.K, combo_sh, slot_table_sh, slot_exp_sh, prod_index_sh);
    auto prod_of = [&](int k) -> FinProd { return fin.prod[k]; };
    BtBlock B;
    B.fin_lds = dyn_lds;                                                                                                      // finalize_message's scratch
    B.msg_lds = reinterpret_cast<uint4 *>(reinterpret_cast<char *>(dyn_lds) + A.fin_bytes - (uint32_t)A.D * 32u);             // the round's message
    B.tabs = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(dyn_lds) + A.fin_bytes);                                    // [table][entry][kBtEnt]
    B.r_sh = r_sh;
    B.stop_sh = &stop_sh;
    B.combo_sh = combo_sh;
    B.prod_index_sh = prod_index_sh;
    B.cap = cap;
    B.U = U;
    B.n_combos = A.n_combos;
    B.K = A.K;
    B.D = A.D;
    B.mail_local = A.mail_local;
    B.max_spins = A.max_spins;
    B.L = bt_lanes(A.n_combos);
    __syncthreads(); // (the metadata above)
    const BtLane<kSlots> ln = bt_lane<kSlots>(B, slot_table_sh, slot_exp_sh);
    const uint32_t msg_words = (uint32_t)A.D * 8u;

    for (;;) {
        // ---- the next instance (a vector atomic by one lane; the barrier also ends the previous instance's use of LDS) ------------------
        if (tid == 0) {
            inst_sh = __hip_atomic_fetch_add(A.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            stop_sh = 0;
        }
        __syncthreads();
        const uint32_t inst = inst_sh;
        if (inst >= A.n) return;
        const uint4 *const *my_tabs = A.tables + (size_t)inst * A.n_tables;
        B.Wm = A.Wm + 2 * (size_t)inst * A.w_stride;
        B.mail = A.mail + (size_t)inst * 16;
        B.h_msg = A.h_msg + (size_t)inst * msg_words;
        B.h_giveup = A.h_giveup + inst;
        // ---- the instance's tables -> LDS --------------------------------------------------------------------------------------------
        {
            const uint32_t total = cap * (uint32_t)U;
            for (uint32_t i = tid; i < total; i += kTsBlock) {
                const uint32_t u = i >> A.nv, e = i & (cap - 1);
                bt_lds_store(B.tabs + (u * cap + e) * (uint32_t)kBtEnt, fe_from_fr(fr_load(my_tabs[u] + 2 * (size_t)e)));
            }
        }
        __syncthreads();
        uint32_t E = cap; // entries per table still held
        for (uint32_t j = 0; j < A.nv; ++j) {
            const uint32_t tag = A.tag0 + j;
            if (j > 0) { // the challenge behind message j - 1, then the bind
                if (!bt_fetch_challenge(B, tag - 1u, (j - 1u) & 1u)) break;
                bt_bind(B, E);
            }
            bt_sum_publish<kSlots>(B, ln, prod_of, E, tag, j + 1u);
        }
    }
}

// (the envelope and the launch's dynamic LDS: batch_shape_fits, bt_lds_bytes -- batch_shape.hpp)
static hipError_t batch_attr() { // (more dynamic LDS than the default 64 KB limit of a launch)
    static bool done[64] = {};
    return ensure_dynamic_lds(reinterpret_cast<const void *>(k_batch_proofs<kMaxFusedM>), (int)kBtLdsMax, done);
}
int batch_blocks_per_cu(int device, uint32_t nv, uint32_t n_tables, int K, int D) {
    (void)device;
    int per_cu = 0;
    if (batch_attr() != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_batch_proofs<kMaxFusedM>, kTsBlock, bt_lds_bytes(nv, n_tables, K, D)) != hipSuccess || per_cu < 1) {
        (void)hipGetLastError();
        return 0;
    }
    return per_cu;
}
hipError_t launch_batch_proofs(BatchArgs args, const ComboMeta &meta, const FinMeta &fin, int grid, hipStream_t stream) {
    if (grid < 1 || args.n == 0 || !batch_shape_fits(args.nv, args.n_tables, args.K, args.D, (uint32_t)kMaxFusedM)) return hipErrorInvalidValue;
    if (args.n_combos < 1 || args.n_combos > kMetaCombos) return hipErrorInvalidValue;
    hipError_t e = batch_attr();
    if (e != hipSuccess) return e;
    args.fin_bytes = (uint32_t)bt_fin_bytes(args.K, args.D);
    hipLaunchKernelGGL(k_batch_proofs<kMaxFusedM>, dim3(grid), dim3(kTsBlock), bt_lds_bytes(args.nv, args.n_tables, args.K, args.D), stream, args, meta, fin);
    return hipGetLastError();
}

} // namespace scd
