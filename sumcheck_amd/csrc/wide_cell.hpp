// wide_cell.hpp -- a cell of wide integer lanes -> the field element it stands for.  A sum of field elements taken as eight uint64 lanes
// of 32-bit limbs (LDS or global integer atomics, an integer all-reduce) is exact in any order; the fold mod p is made once per cell.
// Used by the GKR initialisations (gkr.hip: k_bucket_accumulate, k_wide_fold) and by k_batch_gkr (kernels_batch_gkr.hip).
#pragma once
#include "fr_device.hpp"

namespace scd {

__device__ __forceinline__ Fr wide_fold_cell(const uint64_t lane[8]) { // V = sum_j lane_j 2^(32 j) (lanes < 2^63) -> V mod p
    Fr lo;
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint64_t t = lane[j] + carry; // < 2^63 + 2^32: no wrap
        lo.v[j] = (uint32_t)t;
        carry = t >> 32;
    }
    lo = fr_reduce_once(fr_reduce_once(lo)); // lo < 2^256 < 3p
    // V = lo + carry * 2^256 and carry * 2^256 mod p = mont_mul(carry, R^2)
    Fr hi = fr_zero(), r2;
    hi.v[0] = (uint32_t)carry;
    hi.v[1] = (uint32_t)(carry >> 32);
    const uint64_t R2[4] = {0xc999e990f3f29c6dULL, 0x2b6cedcb87925c23ULL, 0x05d314967254398fULL, 0x0748d9d99f59ff11ULL};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        r2.v[2 * q] = (uint32_t)R2[q];
        r2.v[2 * q + 1] = (uint32_t)(R2[q] >> 32);
    }
    return fr_add(lo, fr_mul(hi, r2));
}

} // namespace scd
