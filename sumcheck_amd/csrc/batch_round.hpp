// batch_round.hpp -- the LDS-resident round body: a block holds tables in LDS as nine 29-bit limbs and runs a sumcheck round out of
// them -- the bind in place, the sums per (product, node) combination with their lane mapping, and the block's metadata prologue.
// Used by k_tail_slices (kernels_tail.hip: the hot path of every proof), whose blocks hold a SLICE of every table, fetch their challenge
// in three ways of their own and hand their sums to block 0; and by the batched kernels, whose blocks hold ALL tables of an instance and
// add (BtBlock) the poll of the instance's own mailbox slot (the poll is the fetch), finalize_message from the instance's matrices and the
// publication as self-validating words (limb | tag << 32): k_batch_proofs (kernels_batch.hip: sc_ml_prove_batch), k_batch_gkr
// (kernels_batch_gkr.hip: sc_gkr_prove_batch), which runs it twice per instance over tables it has built in LDS itself, and k_batch_round
// (kernels_batch_rounds.hip: sc_batch_prove_round), which runs ONE round per launch and uses neither the poll nor the tagged words.
// bg_build_eq and bg_accumulate, the two pieces of a GKR phase's initialisation, are here as well: k_batch_gkr uses them inside its persistent
// block, k_batch_gkr_phase (kernels_batch_gkr_rounds.hip: sc_gkr_batch_prover_*) as plain launches that write k_batch_round's work areas.
#pragma once
#include "finalize_device.hpp"
#include "kernel_common.hpp"
#include "wide_cell.hpp"

namespace scd {

// an element in LDS: nine limbs in a 48-byte, 16-byte aligned slot of kBtEnt dwords (batch_shape.hpp, with kBtLdsMax, a launch's dynamic LDS)
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
// a slot of a batch work area (global memory, batch_shape.hpp: batch_rounds_off): the LDS slot verbatim, three 16-byte words, the last one's upper lanes zero
__device__ __forceinline__ Fe br_slot_load(const int32_t *t) { return bt_lds_load(t); }
__device__ __forceinline__ void br_slot_store(int32_t *t, const Fe &v) {
    *reinterpret_cast<int4 *>(t) = make_int4(v.l[0], v.l[1], v.l[2], v.l[3]);
    *reinterpret_cast<int4 *>(t + 4) = make_int4(v.l[4], v.l[5], v.l[6], v.l[7]);
    *reinterpret_cast<int4 *>(t + 8) = make_int4(v.l[8], 0, 0, 0);
}
__device__ __forceinline__ Fe bt_shfl_down(const Fe &a, const int off) {
    Fe r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = __shfl_down(a.l[i], off, 64);
    return r;
}

// the launch's metadata -> the block's __shared__ copies, with the product every combination belongs to (visible behind the caller's next barrier)
__device__ __forceinline__ void bt_load_meta(const ComboMeta &meta, const FinMeta &fin, const int n_combos, const int K, Combo *combo_sh, uint32_t *slot_table_sh, uint32_t *slot_exp_sh,
                                             int *prod_index_sh) {
    const int tid = threadIdx.x;
    for (int i = tid; i < kMetaCombos; i += kTsBlock) {
        combo_sh[i] = meta.combo[i];
        int k = 0;
        if (i < n_combos)
            while (k < K - 1 && fin.prod[k].partial_off != meta.combo[i].partial_off) ++k;
        prod_index_sh[i] = k;
    }
    for (int i = tid; i < kMetaSlots; i += kTsBlock) {
        slot_table_sh[i] = meta.slot_table[i];
        slot_exp_sh[i] = meta.slot_exp[i];
    }
}

// what the round body needs of the block and of the instance it holds (every member wave-uniform)
struct BtBlock {
    uint4 *fin_lds;              // finalize_message's scratch
    uint4 *msg_lds;              // the round's message
    int32_t *tabs;               // [table][cap][kBtEnt]
    uint64_t *r_sh;              // __shared__, 4 words: the challenge just fetched
    uint32_t *stop_sh;           // __shared__: the block drops the instance
    const Combo *combo_sh;       // __shared__ copies of the launch's metadata
    const int *prod_index_sh;
    uint32_t cap;                // entries per table as loaded
    int U, L, n_combos, K, D;
    uint32_t mail_local, max_spins;
    // the instance
    const uint4 *Wm;
    const uint64_t *mail;
    uint64_t *h_msg;
    uint32_t *h_giveup;          // the instance's own marker
};
// ... and of the lane: its (product, node) combination
template <int kSlots>
struct BtLane {
    int my_combo, my_q;
    bool combo_live;
    int32_t my_nv;
    uint32_t my_base[kSlots], my_exp[kSlots];
};

// the eight tagged words (limb << 32 | tag) lanes 0 .. 7 of wavefront 0 hold -> the challenge's four 64-bit limbs in r_sh (all 64 lanes call)
__device__ __forceinline__ void bt_challenge_words(const uint64_t w, uint64_t *r_sh) {
    const int tid = threadIdx.x;
    const uint32_t lo32 = (uint32_t)(w >> 32);
    const uint32_t hi32 = __shfl_down(lo32, 1, 64);
    if (tid < 8 && (tid & 1) == 0) r_sh[tid >> 1] = (uint64_t)lo32 | ((uint64_t)hi32 << 32);
}
// the carry-free bind's multiplier from the challenge in r_sh: r * 2^5 as 29-bit limbs
__device__ __forceinline__ FeU bt_bind_multiplier(const uint64_t *r_sh) {
    FrHost rh;
#pragma unroll
    for (int i = 0; i < 4; ++i) rh.l[i] = r_sh[i];
    return feu_shl5(fru_from_host(rh).v);
}

// The challenge behind the message published under `want`: the poll is the fetch (eight tagged words).  false: the wait expired, or the
// host asked the block to drop the instance -- uniform; the give-up marker is raised (expired wait only) and every lane has passed
// the barrier behind the stop word.  true: the challenge is in B.r_sh.
__device__ __forceinline__ bool bt_fetch_challenge(const BtBlock &B, const uint32_t want, const uint32_t slot_ix) {
    const int tid = threadIdx.x;
    if (tid < 64) {
        const uint64_t *slot = B.mail + 8 * slot_ix;
        const uint32_t spins_max = B.mail_local ? (B.max_spins > (0xffffffffu >> 3) ? 0xffffffffu : 8u * B.max_spins) : B.max_spins; // (a local poll is ~10x shorter than one over PCIe: same patience)
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
            __hip_atomic_store(B.h_giveup, want, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            *B.stop_sh = 1;
        }
        bt_challenge_words(w, B.r_sh);
    }
    __syncthreads();
    if (*B.stop_sh) { // (uniform: the whole block drops the instance and takes the next ticket)
        __syncthreads(); // every lane has read the word before the ticket step clears it
        return false;
    }
    return true;
}

// bind in place: entry e <- entries 2e, 2e + 1 of each of the T.U tables (T.tabs: [table][T.cap][kBtEnt]), E entries held.  A pass reads
// everything it needs before it writes (one barrier); later passes read higher entries than any earlier pass wrote (2 e'' > e for e'' > e).
// canonical (wave-uniform): the results are stored reduced below p (k_tail_slices' wide lists: line_needs_canonical, kernels.h).
// Tabs: whatever has tabs, cap and U -- a BtBlock, or k_tail_slices' three words.  They are read through the reference, not passed by value:
// with values the batched kernels' instruction schedule moved and a lone instance's proof took 0.5 to 1.5 us longer; this form compiles
// to the code they had (profiles/lds_round_body_ab.txt).
template <typename Tabs>
__device__ __forceinline__ void bt_bind_pass(const Tabs &T, uint32_t &E, const FeU &r32, const bool canonical) {
    const int tid = threadIdx.x;
    const uint32_t half = E / 2, total = half * (uint32_t)T.U;
    const int shH = 31 - __builtin_clz(half); // (a power of two: no integer divisions on a latency-bound path)
    for (uint32_t i0 = 0; i0 < total; i0 += kTsBlock) {
        const uint32_t i = i0 + tid;
        const bool live = i < total;
        const uint32_t u = live ? i >> shH : 0, e = live ? i & (half - 1) : 0;
        int32_t *const tab = T.tabs + u * T.cap * (uint32_t)kBtEnt; // (32-bit index arithmetic: LDS)
        Fe v = fe_zero();
        if (live) {
            const Fe lo = bt_lds_load(tab + 2 * e * (uint32_t)kBtEnt), hi = bt_lds_load(tab + (2 * e + 1) * (uint32_t)kBtEnt);
            v = fe_carry_pass(fe_add(lo, fe_mul_u<true>(fe_sub(hi, lo), r32)));
            if (canonical) v = fe_from_fr(fe_to_fr(v));
        }
        __syncthreads();
        if (live) bt_lds_store(tab + e * (uint32_t)kBtEnt, v);
    }
    E = half;
    __syncthreads();
}
// ... with the challenge in B.r_sh
__device__ __forceinline__ void bt_bind(const BtBlock &B, uint32_t &E) { bt_bind_pass(B, E, bt_bind_multiplier(B.r_sh), false); }

// The product of a combination's lines at a pair, as bt_combo_sum's prod_at: T.tabs is the LDS table area, per slot of the lane's combination
// ln.my_base is the table's base (in entries) and ln.my_exp its multiplicity, nv the node's value.  A functor and not a __forceinline__
// function, with T read through the reference, for bt_bind_pass' reason: operator() is inlined as the lambda it replaces was, and the
// batched kernels keep the code they had.
template <int kSlots, typename Tabs>
struct BtPairProduct {
    const Tabs &T;
    const BtLane<kSlots> &ln;
    const int32_t &nv;
    __device__ Fe operator()(const uint32_t pr) const {
        Fe prod = fe_zero();
        bool first = true;
#pragma unroll
        for (int sl = 0; sl < kSlots; ++sl) {
            if (ln.my_exp[sl] == 0) break; // (slots are dense: the first empty one ends the list)
            const int32_t *lo_p = T.tabs + (ln.my_base[sl] + 2 * pr) * (uint32_t)kBtEnt;
            Fe val;
            if (nv == 0) val = bt_lds_load(lo_p);
            else if (nv == 1) val = bt_lds_load(lo_p + kBtEnt);
            else val = fe_line(bt_lds_load(lo_p), bt_lds_load(lo_p + kBtEnt), nv);
            uint32_t k = 0;
            if (first) { prod = val; k = 1; first = false; }
            for (const uint32_t e = ln.my_exp[sl]; k < e; ++k) prod = fe_mul<true>(val, prod);
        }
        return prod;
    }
};

// One combination's sum: lane q of the combination's L (a power of two, in one wavefront) adds the products of pairs q, q + L, ... lazily,
// then a shuffle tree adds the L lanes; lane q == 0 returns the total (the others partial sums).  prod_at(pair) is the product.
// reduce_lanes (wave-uniform, lazy_sum_needs_reduce(pairs, worst product in units of p)): the int32 top limb of ONE accumulator would not
// hold the combination's whole sum (kernels.h: kLazySumMaxP), so every lane's sum is made canonical before the tree -- L <= 64 values
// below p then.  Within a lane the sum is reduced every 32 terms: terms of up to 8 p each stay inside fe_to_fr's range.
template <typename ProdAt>
__device__ __forceinline__ Fe bt_combo_sum(const bool live, const uint32_t q, const int L, const uint32_t pairs_here, const bool reduce_lanes, const ProdAt &prod_at) {
    Fe acc = fe_zero();
    if (live) {
        uint32_t iter = 0;
        for (uint32_t pr = q; pr < pairs_here; pr += (uint32_t)L, ++iter) {
            acc = fe_carry_pass(fe_add(acc, prod_at(pr)));
            if ((iter & 31u) == 31u) acc = fe_from_fr(fe_to_fr(acc)); // (keeps the top limb far from 2^31; reached only beyond 32 L pairs: L <= 8 at k_tail_slices' 256 pairs a block)
        }
    }
    if (reduce_lanes) acc = fe_from_fr(fe_to_fr(acc));
    for (int off = L >> 1; off >= 1; off >>= 1) acc = fe_carry_pass(fe_add(acc, bt_shfl_down(acc, off)));
    return acc;
}

// the round's sums over the E entries still held and its message from the instance's matrices, left in B.msg_lds behind a barrier.
// worst_p: a bound on the magnitude of one product in units of p (round j of tables loaded canonical: entries in (-j p, p), products of
// two or more within (1 + j^2 / 70) p -- j + 1 covers both)
template <int kSlots, typename ProdFn>
__device__ __forceinline__ void bt_sum_message(const BtBlock &B, const BtLane<kSlots> &ln, const ProdFn &prod_of, const uint32_t E, const uint32_t worst_p) {
    // ---- sums: lane (combination, q) multiplies out the combination's pairs q, q + L, ... ----------------------------------------------
    const uint32_t pairs_here = E / 2;
    const int32_t nv = ln.my_nv;
    const Fe acc = bt_combo_sum(ln.combo_live, (uint32_t)ln.my_q, B.L, pairs_here, lazy_sum_needs_reduce(pairs_here, worst_p), BtPairProduct<kSlots, BtBlock>{B, ln, nv});
    if (ln.combo_live && ln.my_q == 0) fr_store(B.fin_lds + 2 * (B.prod_index_sh[ln.my_combo] * B.D + (int)B.combo_sh[ln.my_combo].t), fe_to_fr(acc));
    __syncthreads();
    // ---- the message, from the instance's own matrices, into LDS -----------------------------------------------------------------------
    finalize_message<kTsBlock>(prod_of, B.Wm, B.K, B.D, B.fin_lds, B.msg_lds, (uint64_t *)nullptr, (uint4 *)nullptr, (uint32_t *)nullptr, 0u, 1, (const Fr *)nullptr);
    __syncthreads();
}
// ... and the message out under `tag`, as tagged words: every 8-byte word validates itself (the kernels whose host polls for it)
template <int kSlots, typename ProdFn>
__device__ __forceinline__ void bt_sum_publish(const BtBlock &B, const BtLane<kSlots> &ln, const ProdFn &prod_of, const uint32_t E, const uint32_t tag, const uint32_t worst_p) {
    const int tid = threadIdx.x;
    bt_sum_message<kSlots>(B, ln, prod_of, E, worst_p);
    const uint32_t msg_words = (uint32_t)B.D * 8u;
    if ((uint32_t)tid < msg_words) {
        const uint32_t limb = reinterpret_cast<const uint32_t *>(B.msg_lds)[tid];
        __hip_atomic_store(B.h_msg + tid, (uint64_t)limb | ((uint64_t)tag << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __syncthreads(); // (fin_lds and msg_lds are written again by the next round)
}

// the lane's combination, from the block's copy of the metadata (call behind the barrier that follows the copy): its node and, per slot,
// the table's LDS base (in entries) and the multiplicity
template <int kSlots>
__device__ __forceinline__ BtLane<kSlots> bt_lane(const int L, const int n_combos, const uint32_t cap, const Combo *combo_sh, const uint32_t *slot_table_sh, const uint32_t *slot_exp_sh) {
    BtLane<kSlots> ln;
    const int tid = threadIdx.x;
    ln.my_combo = tid / L;
    ln.my_q = tid % L;
    ln.combo_live = ln.my_combo < n_combos;
    const Combo my_c = combo_sh[ln.combo_live ? ln.my_combo : 0];
    ln.my_nv = node_value((int)my_c.t);
#pragma unroll
    for (int sl = 0; sl < kSlots; ++sl) {
        const bool in = (uint32_t)sl < my_c.n_slots;
        ln.my_base[sl] = in ? slot_table_sh[my_c.slot_off + sl] * cap : 0u;
        ln.my_exp[sl] = in ? slot_exp_sh[my_c.slot_off + sl] : 0u;
    }
    return ln;
}
template <int kSlots>
__device__ __forceinline__ BtLane<kSlots> bt_lane(const BtBlock &B, const uint32_t *slot_table_sh, const uint32_t *slot_exp_sh) {
    return bt_lane<kSlots>(B.L, B.n_combos, B.cap, B.combo_sh, slot_table_sh, slot_exp_sh);
}

// eq(point, .) over dim variables into out[2^dim] (32-byte elements in LDS): precompute_eq's doubling (ark-poly: dp[b + 2^i] = dp[b] * g_i ;
// dp[b] -= dp[b + 2^i]) on the two halves of the variables at once -- wavefront 0 the low kl, wavefront 1 the high kh -- then the outer
// product.  Depth ceil(dim / 2) + 1 dependent products instead of dim.  tmp: 2 x 2^kl elements of scratch.  Ends behind a barrier.
__device__ __forceinline__ void bg_build_eq(uint4 *out, uint4 *tmp, const uint4 *point, const uint32_t dim) {
    const uint32_t tid = threadIdx.x, kl = (dim + 1) / 2, kh = dim - kl;
    uint4 *lo = tmp, *hi = tmp + 2 * ((size_t)1 << kl);
    if (tid == 0) fr_store(lo, fr_one());
    if (tid == 64) fr_store(hi, fr_one());
    __syncthreads();
    for (uint32_t i = 0; i < kl; ++i) {
        const uint32_t w = tid >> 6, t = tid & 63u;
        if (w < 2 && t < (1u << i) && (w == 0 || i < kh)) {
            uint4 *tab = w == 0 ? lo : hi;
            const Fr a = fr_load(tab + 2 * t), m = fr_mul(a, fr_load(point + 2 * (w == 0 ? i : kl + i)));
            fr_store(tab + 2 * (t + (1u << i)), m);
            fr_store(tab + 2 * t, fr_sub(a, m));
        }
        __syncthreads();
    }
    for (uint32_t b = tid; b < (1u << dim); b += kTsBlock) {
        const Fr l = fr_load(lo + 2 * (b & ((1u << kl) - 1u)));
        fr_store(out + 2 * b, kh ? fr_mul(l, fr_load(hi + 2 * (b >> kl))) : l);
    }
    __syncthreads();
}

// The first half of bg_build_eq alone, for blocks that keep eq(point, .) as its two factors (k_batch_gkr_terms, dim up to 16: the outer
// product would not fit LDS): lo[2^kl] over the low kl = ceil(dim / 2) variables, hi[2^kh] over the rest, so that
// eq(point, b) = lo[b & (2^kl - 1)] * hi[b >> kl] (hi[0] = 1 when kh = 0).  Lanes 0 .. 127 double lo, lanes 128 .. 255 hi: up to 2^7
// entries a step, kl <= 8.  Ends behind a barrier.
__device__ __forceinline__ void bg_build_eq_halves(uint4 *lo, uint4 *hi, const uint4 *point, const uint32_t dim) {
    const uint32_t tid = threadIdx.x, kl = (dim + 1) / 2, kh = dim - kl;
    static_assert(kTsBlock == 256, "two halves of 128 lanes");
    if (tid == 0) fr_store(lo, fr_one());
    if (tid == 128) fr_store(hi, fr_one());
    __syncthreads();
    for (uint32_t i = 0; i < kl; ++i) {
        const uint32_t w = tid >> 7, t = tid & 127u;
        if (t < (1u << i) && (w == 0 || i < kh)) {
            uint4 *tab = w == 0 ? lo : hi;
            const Fr a = fr_load(tab + 2 * t), m = fr_mul(a, fr_load(point + 2 * (w == 0 ? i : kl + i)));
            fr_store(tab + 2 * (t + (1u << i)), m);
            fr_store(tab + 2 * t, fr_sub(a, m));
        }
        __syncthreads();
    }
}

// A GKR phase's table from the instance's non-zeros (k_batch_gkr, k_batch_gkr_phase).  kPhase 1: cell x, term eq(g,z) * v * f3[y];
// kPhase 2: cell y, term eq(g,z) * eq(u,x) * v.  The cells (eight uint64 lanes of 32-bit limbs each, lane-major: cell[j << dim | c],
// neighbouring cells in neighbouring banks) are zeroed, filled with LDS atomic adds (exact in any order) and folded mod p; store(c, value)
// takes cell c's element: an LDS table, or a slot of a work area.  Every index is masked to dim bits per component before it addresses
// LDS or f3.  Ends behind a barrier.
template <int kPhase, typename Store>
__device__ __forceinline__ void bg_accumulate(uint64_t *cell, const GkrBatchInst &I, const uint32_t dim, const uint4 *eq_g, const uint4 *eq_u, const Store &store) {
    const uint32_t tid = threadIdx.x, cap = 1u << dim, mask = cap - 1u;
    for (uint32_t i = tid; i < 8u * cap; i += kTsBlock) cell[i] = 0;
    __syncthreads();
    for (uint64_t i = tid; i < I.nnz; i += kTsBlock) {
        const uint64_t id = I.idx[i];
        const uint32_t z = (uint32_t)id & mask, x = (uint32_t)(id >> dim) & mask, y = (uint32_t)(id >> (2 * dim)) & mask;
        const Fr a = fr_mul(fr_load(eq_g + 2 * z), fr_load(I.vals + 2 * i));
        const Fr t = kPhase == 1 ? fr_mul(a, fr_load(I.f3 + 2 * (size_t)y)) : fr_mul(a, fr_load(eq_u + 2 * x));
        const uint32_t c = kPhase == 1 ? x : y;
#pragma unroll
        for (int j = 0; j < 8; ++j) __hip_atomic_fetch_add(cell + (((uint32_t)j << dim) | c), (uint64_t)t.v[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    for (uint32_t c = tid; c < cap; c += kTsBlock) {
        uint64_t lane[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) lane[j] = cell[((uint32_t)j << dim) | c];
        store(c, fe_from_fr(wide_fold_cell(lane)));
    }
    __syncthreads();
}

// bg_accumulate's sibling for a caller that brings its own term (k_batch_gkr_eval_layers: a circuit layer's values): term(i, x, y) returns
// non-zero i's canonical term, which is added into cell z; store(c, value) takes cell c's canonical element.  The same cells, the same
// three steps, the same masking of every index component; bg_accumulate itself is left as it is -- k_batch_gkr and k_batch_gkr_phase keep
// their code (profiles/gkr_layers_eval_kernel_resources.txt).  Ends behind a barrier.
template <typename Term, typename Store>
__device__ __forceinline__ void bg_accumulate_terms(uint64_t *cell, const uint64_t *idx, const uint64_t nnz, const uint32_t dim, const Term &term, const Store &store) {
    const uint32_t tid = threadIdx.x, cap = 1u << dim, mask = cap - 1u;
    for (uint32_t i = tid; i < 8u * cap; i += kTsBlock) cell[i] = 0;
    __syncthreads();
    for (uint64_t i = tid; i < nnz; i += kTsBlock) {
        const uint64_t id = idx[i];
        const uint32_t z = (uint32_t)id & mask, x = (uint32_t)(id >> dim) & mask, y = (uint32_t)(id >> (2 * dim)) & mask;
        const Fr t = term(i, x, y);
#pragma unroll
        for (int j = 0; j < 8; ++j) __hip_atomic_fetch_add(cell + (((uint32_t)j << dim) | z), (uint64_t)t.v[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    for (uint32_t c = tid; c < cap; c += kTsBlock) {
        uint64_t lane[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) lane[j] = cell[((uint32_t)j << dim) | c];
        store(c, wide_fold_cell(lane));
    }
    __syncthreads();
}

// (bt_fin_bytes, the head of a batched kernel's dynamic LDS -- finalize scratch | message: batch_shape.hpp)

} // namespace scd
