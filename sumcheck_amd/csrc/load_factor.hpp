// load_factor.hpp -- one factor of a product at one pair, as the fused bind + sum kernels take it (kernels_big.hip: product tree for
// up to four multiplicands; kernels_wide.hip: five to eight).  A slot lists ONE factor (a table that occurs twice in a product is listed
// twice).  Slot modes: 0 read this round's table; 1 bind the previous table, store, use; 3 bind without storing (a repeated factor, or a
// table that an earlier product of the same launch stores).
#pragma once
#include "kernel_common.hpp"

namespace scd {

// factor F of the product at pair b: its line's two end points (lo, hi), binding / storing as the slot's mode says
// kR1: round 1 of a proof -- every factor is read from the caller's canonical table, nothing is bound (k_round1_tree)
template <int F, bool kR1 = false, bool kChain = kChainDefault>
struct LoadFactor {
    static __device__ __forceinline__ void run(const Slot *S, const uint64_t b, const int32_t (&r)[kBindLds], Fe &lo_out, Fe &hi_out) {
        const Slot &sl = S[F];
        if constexpr (kR1) {
            const uint4 *p = sl.src + 4 * b;
            lo_out = fe_from_fr(fr_load(p));
            hi_out = fe_from_fr(fr_load(p + 2));
            return;
        }
        const uint32_t mode = sl.mode;
        const bool sf29 = sl.src_f29 != 0; // the source table is in the internal F29 format
        if (mode == 0) {
            const uint4 *p = sl.src + 4 * b;
            if (sf29) {
                lo_out = fe_load_f29(sl.src, 2 * b);
                hi_out = fe_load_f29(sl.src, 2 * b + 1);
            } else {
                lo_out = fe_from_fr(fr_load(p));
                hi_out = fe_from_fr(fr_load(p + 2));
            }
        } else {
            const uint4 *p = sl.src + 8 * b; // entries 4b..4b+3 of the previous table: 128 contiguous bytes
            Fe e0, e1, e2, e3;
            if (sf29) {
                const uint4 *m = sl.src;
                e0 = fe_load_f29(m, 4 * b); e1 = fe_load_f29(m, 4 * b + 1);
                e2 = fe_load_f29(m, 4 * b + 2); e3 = fe_load_f29(m, 4 * b + 3);
            } else {
                e0 = fe_from_fr(fr_load(p)); e1 = fe_from_fr(fr_load(p + 2)); e2 = fe_from_fr(fr_load(p + 4)); e3 = fe_from_fr(fr_load(p + 6));
            }
            const Fe l0 = fe_add(e0, fe_mul_bind<kChain>(fe_sub(e1, e0), r));
            asm volatile("" : "+v"(e3.l[8]) : "v"(l0.l[8])); // one product at a time: interleaving the two doubles the live constants
            const Fe h0 = fe_add(e2, fe_mul_bind<kChain>(fe_sub(e3, e2), r));
            if (sl.dst_f29 || (mode == 3 && sf29)) {
                // internal F29 tables: no modular reduction.  fe_mul_bind's term lies in (-p - 2^230, 2^230); where the sum reads below
                // -p / 2, p is added back once, inside the carry chain that makes limbs 0..7 exact 29-bit digits (fe_settle_f29).  From
                // canonical tables, k binds leave an entry in (-p / 2 - (k - 1) 2^230, p + k 2^230): inside the packed form's
                // [-2^255, 2^255) for any nv <= 40, and inside the (-(k + 1) p, p) that every consumer's bound was written for.
                lo_out = fe_settle_f29(l0);
                hi_out = fe_settle_f29(h0);
                if (mode == 1) {
                    fe_store_f29(sl.dst, 2 * b, lo_out);
                    fe_store_f29(sl.dst, 2 * b + 1, hi_out);
                }
            } else { // tables stay canonical in the reference layout
                const Fr lc = fe_to_fr(l0), hc = fe_to_fr(h0);
                if (mode == 1) {
                    uint4 *q = sl.dst + 4 * b;
                    fr_store(q, lc);
                    fr_store(q + 2, hc);
                }
                lo_out = fe_from_fr(lc);
                hi_out = fe_from_fr(hc);
            }
        }
    }
};


} // namespace scd
