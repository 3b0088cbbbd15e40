// kernels_batch_gkr.hip -- many small GKR round proofs in one launch (k_batch_gkr): sc_gkr_prove_batch.
//
// GKRRoundSumcheck::prove (reference src/gkr_round_sumcheck/mod.rs:93-139) of a small instance is two initialisations and 2 x dim
// latency-bound rounds; a caller with many small layers (or many copies of a sub-circuit) gains nothing from proving them one after the
// other.  Here ONE block proves a whole instance out of LDS, every instance of the call in flight at once, the host only hashes and
// answers (batch.hip) -- k_batch_proofs' scheme (kernels_batch.hip, the round body is shared: batch_round.hpp), with the two tables of
// each phase BUILT in LDS by the block itself:
//   load        f2 -> table 1 as nine 29-bit limbs; eq(g, .) over the 2^dim cells (two half tables by doubling, then their outer product);
//   phase one   h_g[x] = sum over non-zeros (z, x, y) of eq(g,z) * v * f3[y]   (mod.rs:30-38): lanes stride over the non-zeros, each term
//               is added into cell x of an LDS accumulator of eight uint64 lanes of 32-bit limbs with LDS atomic adds (k_bucket_accumulate's
//               form, gkr.hip: exact in any order), the cells are folded mod p into table 0; then dim rounds over (h_g, f2);
//   between     the LAST challenge of phase one is fetched as well and bound: the two remaining entries of f2 give f2(u) (what
//               gkr.coeff_from_bound_table does on the host path); f3 is read again, scaled by f2(u) (mod.rs:71-75, literally), into table 1;
//               eq(u, .) is built;
//   phase two   f1_gu[y] = sum of eq(g,z) * eq(u,x) * v   (mod.rs:62) through the same accumulator into table 0; dim rounds over
//               (f1_gu, f2(u) f3) under the tags tag0 + dim ..
// Every index is masked to dim bits per component before it addresses LDS or f3: whatever the list holds, no access leaves the
// instance's tables.  (An index with a bit at or above 3 dim is an argument error: k_batch_gkr_idx_range reports it in front of the launch.)
#include <algorithm>

#include "batch_round.hpp"

namespace scd {

// (bg_accumulate, the cells both phases are added up in: batch_round.hpp -- shared with k_batch_gkr_phase, kernels_batch_gkr_rounds.hip)
__global__ __launch_bounds__(kTsBlock) void k_batch_gkr(const BatchGkrArgs A, const ComboMeta meta, const FinMeta fin) {
    constexpr int kSlots = 2; // one product of two tables
    extern __shared__ uint4 dyn_lds[];
    __shared__ uint64_t r_sh[4];
    __shared__ uint32_t stop_sh, inst_sh;
    __shared__ Combo combo_sh[kMetaCombos];
    __shared__ uint32_t slot_table_sh[kMetaSlots], slot_exp_sh[kMetaSlots];
    __shared__ int prod_index_sh[kMetaCombos];
    __shared__ uint4 g_sh[2 * kGkrBatchMaxDim], u_sh[2 * kGkrBatchMaxDim]; // the points g and u
    const int tid = threadIdx.x;
    const uint32_t dim = A.dim, cap = 1u << dim;
    auto prod_of = [&](int k) -> FinProd { return fin.prod[k]; };
    // dynamic LDS: finalize scratch | message | tables 0, 1 (48 B per entry) | eq(g, .) | eq(u, .) (32 B per cell) | the accumulator (64 B per cell)
    char *const lds = reinterpret_cast<char *>(dyn_lds);
    BtBlock B;
    B.fin_lds = dyn_lds;
    B.msg_lds = reinterpret_cast<uint4 *>(lds + A.fin_bytes - 3u * 32u);
    B.tabs = reinterpret_cast<int32_t *>(lds + A.fin_bytes);
    uint4 *const eq_g = reinterpret_cast<uint4 *>(lds + A.fin_bytes + 2u * cap * (uint32_t)(kBtEnt * 4));
    uint4 *const eq_u = eq_g + 2 * (size_t)cap;
    uint64_t *const cell = reinterpret_cast<uint64_t *>(eq_u + 2 * (size_t)cap);
    B.r_sh = r_sh;
    B.stop_sh = &stop_sh;
    B.combo_sh = combo_sh;
    B.prod_index_sh = prod_index_sh;
    B.cap = cap;
    B.U = 2;
    B.n_combos = 3;
    B.K = 1;
    B.D = 3;
    B.L = bt_lanes(B.n_combos); // (three combinations of 64 lanes)
    B.mail_local = A.mail_local;
    B.max_spins = A.max_spins;
    B.Wm = A.Wm; // a coefficient of one: the same matrices for every instance
    bt_load_meta(meta, fin, B.n_combos, B.K, combo_sh, slot_table_sh, slot_exp_sh, prod_index_sh); // (K = 1: every prod_index is 0)
    __syncthreads(); // (the metadata above)
    const BtLane<kSlots> ln = bt_lane<kSlots>(B, slot_table_sh, slot_exp_sh);
    int32_t *const tab0 = B.tabs, *const tab1 = B.tabs + cap * (uint32_t)kBtEnt;

    for (;;) {
        // ---- the next instance (the barrier also ends the previous instance's use of LDS) ----------------------------------------------
        if (tid == 0) {
            inst_sh = __hip_atomic_fetch_add(A.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            stop_sh = 0;
        }
        __syncthreads();
        const uint32_t inst = inst_sh;
        if (inst >= A.n) return;
        const GkrBatchInst I = A.inst[inst];
        B.mail = A.mail + (size_t)inst * 16;
        B.h_msg = A.h_msg + (size_t)inst * 24;
        B.h_giveup = A.h_giveup + inst;
        // ---- f2 -> table 1, g, eq(g, .), phase one's table (mod.rs:30-38) ----------------------------------------------------------------
        for (uint32_t e = tid; e < cap; e += kTsBlock) bt_lds_store(tab1 + e * (uint32_t)kBtEnt, fe_from_fr(fr_load(I.f2 + 2 * (size_t)e)));
        if ((uint32_t)tid < 2 * dim) g_sh[tid] = I.g[tid];
        __syncthreads();
        bg_build_eq(eq_g, reinterpret_cast<uint4 *>(cell), g_sh, dim);
        bg_accumulate<1>(cell, I, dim, eq_g, eq_u, [&](const uint32_t c, const Fe &v) { bt_lds_store(tab0 + c * (uint32_t)kBtEnt, v); });
        // ---- phase one: dim rounds over (h_g, f2); EVERY challenge is fetched, the last one too ------------------------------------------
        uint32_t E = cap;
        bool dropped = false;
        for (uint32_t j = 0; j <= dim && !dropped; ++j) {
            if (j > 0) {
                if (!bt_fetch_challenge(B, A.tag0 + j - 1u, (j - 1u) & 1u)) {
                    dropped = true;
                    break;
                }
                if (tid < 4) reinterpret_cast<uint64_t *>(u_sh)[4 * (j - 1u) + tid] = r_sh[tid];
                bt_bind(B, E); // (the barriers inside also publish u_sh)
            }
            if (j < dim) bt_sum_publish<kSlots>(B, ln, prod_of, E, A.tag0 + j, j + 1u);
        }
        if (dropped) continue;
        // ---- between the phases: f2(u) is what is left of table 1; f3 * f2(u) -> table 1 (mod.rs:71-75); eq(u, .); f1(g, u, .) -> table 0 --
        const Fr f2u = fe_to_fr(bt_lds_load(tab1));
        __syncthreads(); // (every lane has read it)
        for (uint32_t e = tid; e < cap; e += kTsBlock) bt_lds_store(tab1 + e * (uint32_t)kBtEnt, fe_from_fr(fr_mul(fr_load(I.f3 + 2 * (size_t)e), f2u)));
        bg_build_eq(eq_u, reinterpret_cast<uint4 *>(cell), u_sh, dim);
        bg_accumulate<2>(cell, I, dim, eq_g, eq_u, [&](const uint32_t c, const Fe &v) { bt_lds_store(tab0 + c * (uint32_t)kBtEnt, v); });
        // ---- phase two: dim rounds over (f1_gu, f2(u) f3), messages dim .. 2 dim - 1 -----------------------------------------------------
        E = cap;
        for (uint32_t r = 0; r < dim; ++r) {
            const uint32_t j = dim + r;
            if (r > 0) {
                if (!bt_fetch_challenge(B, A.tag0 + j - 1u, (j - 1u) & 1u)) break;
                bt_bind(B, E);
            }
            bt_sum_publish<kSlots>(B, ln, prod_of, E, A.tag0 + j, r + 1u);
        }
    }
}

// flags[i] |= 1 if instance i's list holds an index with a bit at or above 3 dim (device-resident lists: the check in front of the launch)
__global__ __launch_bounds__(kBlock) void k_batch_gkr_idx_range(const GkrBatchInst *__restrict__ inst, const uint32_t n, const uint32_t bits, uint32_t *__restrict__ flags) {
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint64_t *idx = inst[i].idx;
        const uint64_t nnz = inst[i].nnz;
        bool bad = false;
        for (uint64_t k = threadIdx.x; k < nnz; k += kBlock) bad |= (idx[k] >> bits) != 0;
        if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flags + i, 1u);
    }
}

// (the envelope and the launch's dynamic LDS: gkr_batch_shape_fits, bg_lds_bytes -- batch_shape.hpp)
static hipError_t batch_gkr_attr() { // (more dynamic LDS than the default 64 KB limit of a launch)
    static bool done[64] = {};
    return ensure_dynamic_lds(reinterpret_cast<const void *>(k_batch_gkr), (int)kBtLdsMax, done);
}
int gkr_batch_blocks_per_cu(int device, uint32_t dim) {
    (void)device;
    int per_cu = 0;
    if (batch_gkr_attr() != hipSuccess || hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_batch_gkr, kTsBlock, bg_lds_bytes(dim)) != hipSuccess || per_cu < 1) {
        (void)hipGetLastError();
        return 0;
    }
    return per_cu;
}
hipError_t launch_batch_gkr_idx_range(const GkrBatchInst *inst, uint32_t n, uint32_t dim, uint32_t *flags, hipStream_t stream) {
    if (n == 0 || dim == 0 || 3 * dim >= 64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_batch_gkr_idx_range, dim3(std::min<uint32_t>(n, 1024u)), dim3(kBlock), 0, stream, inst, n, 3 * dim, flags);
    return hipGetLastError();
}
hipError_t launch_batch_gkr(BatchGkrArgs args, const ComboMeta &meta, const FinMeta &fin, int grid, hipStream_t stream) {
    if (grid < 1 || args.n == 0 || !gkr_batch_shape_fits(args.dim, 0)) return hipErrorInvalidValue;
    hipError_t e = batch_gkr_attr();
    if (e != hipSuccess) return e;
    args.fin_bytes = (uint32_t)bt_fin_bytes(1, 3);
    hipLaunchKernelGGL(k_batch_gkr, dim3(grid), dim3(kTsBlock), bg_lds_bytes(args.dim), stream, args, meta, fin);
    return hipGetLastError();
}

} // namespace scd
