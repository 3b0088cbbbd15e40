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
#include "finalize_device.hpp"
#include "kernel_common.hpp"

namespace scd {

// (an element in LDS: k_tail_slices' 48-byte slot)
constexpr int kBtEnt = 12;
constexpr size_t kBtLdsMax = 144 * 1024; // k_tail_slices' budget (kTsLdsMax): of the CU's 160 KB
__device__ __forceinline__ Fe bt_lds_load(const int32_t *t) {
    const int4 a = *reinterpret_cast<const int4 *>(t), b = *reinterpret_cast<const int4 *>(t + 4), c = *reinterpret_cast<const int4 *>(t + 8);
    Fe r;
    r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
    r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
    r.l[8] = c.x;
    return r;
}
__device__ __forceinline__ void bt_lds_store(int32_t *t, const Fe &v) {
    *reinterpret_cast<int4 *>(t) = make_int4(v.l[0], v.l[1], v.l[2], v.l[3]);
    *reinterpret_cast<int4 *>(t + 4) = make_int4(v.l[4], v.l[5], v.l[6], v.l[7]);
    t[8] = v.l[8];
}
__device__ __forceinline__ Fe bt_shfl_down(const Fe &a, const int off) {
    Fe r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = __shfl_down(a.l[i], off, 64);
    return r;
}

template <int kSlots>
__global__ __launch_bounds__(kTsBlock) void k_batch_proofs(const BatchArgs A, const ComboMeta meta, const FinMeta fin) {
    extern __shared__ uint4 dyn_lds[];
    uint4 *fin_lds = dyn_lds;                                                                      // finalize_message's scratch
    uint4 *msg_lds = reinterpret_cast<uint4 *>(reinterpret_cast<char *>(dyn_lds) + A.fin_bytes - (uint32_t)A.D * 32u); // the round's message
    int32_t *tabs = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(dyn_lds) + A.fin_bytes);  // [table][entry][kBtEnt]
    __shared__ uint64_t r_sh[4];
    __shared__ uint32_t stop_sh, inst_sh;
    __shared__ Combo combo_sh[kMetaCombos];
    __shared__ uint32_t slot_table_sh[kMetaSlots], slot_exp_sh[kMetaSlots];
    __shared__ int prod_index_sh[kMetaCombos];
    const int tid = threadIdx.x;
    const int U = (int)A.n_tables;
    const uint32_t cap = 1u << A.nv; // entries per table
    for (int i = tid; i < kMetaCombos; i += kTsBlock) {
        combo_sh[i] = meta.combo[i];
        int k = 0;
        if (i < A.n_combos)
            while (k < A.K - 1 && fin.prod[k].partial_off != meta.combo[i].partial_off) ++k;
        prod_index_sh[i] = k;
    }
    for (int i = tid; i < kMetaSlots; i += kTsBlock) {
        slot_table_sh[i] = meta.slot_table[i];
        slot_exp_sh[i] = meta.slot_exp[i];
    }
    auto prod_of = [&](int k) -> FinProd { return fin.prod[k]; };
    auto tab_at = [&](int u, uint32_t e) -> int32_t * { return tabs + ((uint32_t)u * cap + e) * (uint32_t)kBtEnt; }; // (32-bit index arithmetic: LDS)
    // lanes per (product, node) combination: a power of two, all of a combination's lanes in one wavefront
    int L = 64;
    while (L * A.n_combos > kTsBlock) L >>= 1;
    const int my_combo = tid / L, my_q = tid % L;
    const bool combo_live = my_combo < A.n_combos;
    __syncthreads(); // (the metadata above)
    const Combo my_c = combo_sh[combo_live ? my_combo : 0];
    const int32_t my_nv = node_value((int)my_c.t);
    uint32_t my_base[kSlots], my_exp[kSlots];
#pragma unroll
    for (int sl = 0; sl < kSlots; ++sl) {
        const bool in = (uint32_t)sl < my_c.n_slots;
        my_base[sl] = in ? slot_table_sh[my_c.slot_off + sl] * cap : 0u;
        my_exp[sl] = in ? slot_exp_sh[my_c.slot_off + sl] : 0u;
    }
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
        const uint4 *Wm = A.Wm + 2 * (size_t)inst * A.w_stride;
        const uint64_t *mail = A.mail + (size_t)inst * 16;
        uint64_t *h_msg = A.h_msg + (size_t)inst * msg_words;
        // ---- the instance's tables -> LDS --------------------------------------------------------------------------------------------
        {
            const uint32_t total = cap * (uint32_t)U;
            for (uint32_t i = tid; i < total; i += kTsBlock) {
                const uint32_t u = i >> A.nv, e = i & (cap - 1);
                bt_lds_store(tab_at((int)u, e), fe_from_fr(fr_load(my_tabs[u] + 2 * (size_t)e)));
            }
        }
        __syncthreads();
        uint32_t E = cap; // entries per table still held
        for (uint32_t j = 0; j < A.nv; ++j) {
            const uint32_t tag = A.tag0 + j;
            if (j > 0) {
                // ---- the challenge behind message j - 1: the poll is the fetch (eight tagged words) ---------------------------------------
                if (tid < 64) {
                    const uint32_t want = tag - 1u;
                    const uint64_t *slot = mail + 8 * ((j - 1u) & 1u);
                    const uint32_t spins_max = A.mail_local ? (A.max_spins > (0xffffffffu >> 3) ? 0xffffffffu : 8u * A.max_spins) : A.max_spins; // (a local poll is ~10x shorter than one over PCIe: same patience)
                    uint64_t w = 0;
                    bool seen = false;
                    for (uint32_t spin = 0; spin < spins_max; ++spin) {
                        if (tid < 8) w = __hip_atomic_load(slot + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        const bool mine = tid >= 8 || (uint32_t)w == want;
                        if (__all(mine)) { seen = true; break; }
                        if (__any(tid == 0 && (uint32_t)w == (want ^ 0x80000000u))) break; // the host asks the block to drop this instance
                        __builtin_amdgcn_s_sleep(1);
                    }
                    if (!seen && tid == 0) {
                        __hip_atomic_store(A.h_giveup + inst, want, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
                        stop_sh = 1;
                    }
                    const uint32_t lo32 = (uint32_t)(w >> 32);
                    const uint32_t hi32 = __shfl_down(lo32, 1, 64);
                    if (tid < 8 && (tid & 1) == 0) r_sh[tid >> 1] = (uint64_t)lo32 | ((uint64_t)hi32 << 32);
                }
                __syncthreads();
                if (stop_sh) { // (uniform: the whole block drops the instance and takes the next ticket)
                    __syncthreads(); // every lane has read the word before the ticket step clears it
                    break;
                }
                FrHost rh;
#pragma unroll
                for (int i = 0; i < 4; ++i) rh.l[i] = r_sh[i];
                const FeU r32 = feu_shl5(fru_from_host(rh).v); // the carry-free bind's multiplier: r * 2^5 as 29-bit limbs
                // ---- bind in place: entry e <- entries 2e, 2e + 1.  A pass reads everything it needs before it writes (one barrier);
                // later passes read higher entries than any earlier pass wrote (2 e'' > e for e'' > e).
                const uint32_t half = E / 2, total = half * (uint32_t)U;
                const int shH = 31 - __builtin_clz(half);
                for (uint32_t i0 = 0; i0 < total; i0 += kTsBlock) {
                    const uint32_t i = i0 + tid;
                    const bool live = i < total;
                    const uint32_t u = live ? i >> shH : 0, e = live ? i & (half - 1) : 0;
                    Fe v = fe_zero();
                    if (live) {
                        const Fe lo = bt_lds_load(tab_at((int)u, 2 * e)), hi = bt_lds_load(tab_at((int)u, 2 * e + 1));
                        v = fe_carry_pass(fe_add(lo, fe_mul_u<true>(fe_sub(hi, lo), r32)));
                    }
                    __syncthreads();
                    if (live) bt_lds_store(tab_at((int)u, e), v);
                }
                E = half;
                __syncthreads();
            }
            // ---- sums: lane (combination, q) multiplies out the combination's pairs q, q + L, ... ------------------------------------------
            const uint32_t pairs_here = E / 2;
            Fe acc = fe_zero();
            if (combo_live) {
                const int32_t nv = my_nv;
                uint32_t iter = 0;
                for (uint32_t pr = (uint32_t)my_q; pr < pairs_here; pr += (uint32_t)L, ++iter) {
                    Fe prod = fe_zero();
                    bool first = true;
#pragma unroll
                    for (int sl = 0; sl < kSlots; ++sl) {
                        if (my_exp[sl] == 0) break; // (slots are dense: the first empty one ends the list)
                        const int32_t *lo_p = tabs + (my_base[sl] + 2 * pr) * (uint32_t)kBtEnt;
                        Fe val;
                        if (nv == 0) val = bt_lds_load(lo_p);
                        else if (nv == 1) val = bt_lds_load(lo_p + kBtEnt);
                        else val = fe_line(bt_lds_load(lo_p), bt_lds_load(lo_p + kBtEnt), nv);
                        uint32_t k = 0;
                        if (first) { prod = val; k = 1; first = false; }
                        for (const uint32_t e = my_exp[sl]; k < e; ++k) prod = fe_mul<true>(val, prod);
                    }
                    acc = fe_carry_pass(fe_add(acc, prod));
                    if ((iter & 31u) == 31u) acc = fe_from_fr(fe_to_fr(acc)); // (keeps the top limb far from 2^31; never reached here)
                }
            }
            for (int off = L >> 1; off >= 1; off >>= 1) acc = fe_carry_pass(fe_add(acc, bt_shfl_down(acc, off)));
            if (combo_live && my_q == 0) fr_store(fin_lds + 2 * (prod_index_sh[my_combo] * A.D + (int)combo_sh[my_combo].t), fe_to_fr(acc));
            __syncthreads();
            // ---- the message, from the instance's own matrices, into LDS; then out as tagged words: every 8-byte word validates itself ----
            finalize_message<kTsBlock>(prod_of, Wm, A.K, A.D, fin_lds, msg_lds, (uint64_t *)nullptr, (uint4 *)nullptr, (uint32_t *)nullptr, 0u, 1, (const Fr *)nullptr);
            __syncthreads();
            if ((uint32_t)tid < msg_words) {
                const uint32_t limb = reinterpret_cast<const uint32_t *>(msg_lds)[tid];
                __hip_atomic_store(h_msg + tid, (uint64_t)limb | ((uint64_t)tag << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            __syncthreads(); // (fin_lds and msg_lds are written again by the next round)
        }
    }
}

static size_t bt_fin_bytes(int K, int D) { return (((size_t)K * D * (D + 2) * 32 + 15) & ~(size_t)15) + (size_t)D * 32; } // finalize scratch | message
static size_t bt_lds_bytes(uint32_t nv, uint32_t n_tables, int K, int D) { return bt_fin_bytes(K, D) + ((size_t)n_tables << nv) * (kBtEnt * 4); }

bool batch_shape_fits(uint32_t nv, uint32_t n_tables, int K, int D, uint32_t max_multiplicands) {
    if (nv == 0 || nv > 16 || n_tables == 0 || n_tables > (uint32_t)kMaxSmallTables || K < 1 || K > kMetaProds || max_multiplicands > (uint32_t)kMaxFusedM) return false;
    if ((uint32_t)D * 8u > (uint32_t)kTsBlock) return false; // (one lane per word of the message)
    return bt_lds_bytes(nv, n_tables, K, D) <= kBtLdsMax;
}
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
