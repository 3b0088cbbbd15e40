// kernels_lag.hip -- k_fix_deep: the catch-up pass of a lagging table (lag_index.hpp; the host side is materialize_lagging in
// protocol.hip).  A table that only single-table products name is not bound in the big rounds that follow round 1 -- its class sums
// stand in for it --, and this kernel applies every challenge it missed in ONE pass over the original table: the table moves
// E + E / 2^k bytes instead of the 3 E (1 - 2^-k) of k binding rounds.
#include "kernel_common.hpp"

#include <algorithm>

namespace scd {

// a freshly bound entry in the form a big round keeps it in after storing it (load_factor.hpp): F29 tables settle (no reduction),
// canonical tables reduce -- level after level the same values, so the table written here is the one the rounds would have left
template <bool kF29>
__device__ __forceinline__ Fe deep_bind(const Fe &lo, const Fe &hi, const int32_t (&rt)[kBindLds]) {
    const Fe v = fe_add(lo, fe_mul_bind<kChainDefault>(fe_sub(hi, lo), rt));
    if constexpr (kF29) return fe_settle_f29(v);
    else return fe_from_fr(fe_to_fr(v));
}
template <bool kF29>
__device__ __forceinline__ void deep_store(uint4 *dst, const uint64_t entry, const Fe &v) {
    if constexpr (kF29) {
        uint32_t w[8];
        f29_pack(v.l, w);
        f29_st(dst + lag_f29_chunk(entry, 0), w[0], w[1], w[2], w[3]);
        f29_st(dst + lag_f29_chunk(entry, 1), w[4], w[5], w[6], w[7]);
    } else {
        fr_store(dst + 2 * entry, fe_to_fr(v));
    }
}

// one level >= 3 over a lane's slots (lag_index.hpp): slots i and i + half meet their partners' in the lane lag_deep_xor(kLevel) away
template <bool kF29, int kN, int kLevel>
__device__ __forceinline__ void deep_level(Fe (&v)[kN], const int32_t (&rt)[kBindLds]) {
    constexpr int half = kN >> (kLevel - 2);
    const bool odd = lag_deep_bit(threadIdx.x, kLevel) != 0;
#pragma unroll
    for (int i = 0; i < half; ++i) {
        const Fe mine = v[i], other = v[i + half]; // (copies: a select between two array elements would index the array)
        Fe got, lo, hi;
#pragma unroll
        for (int l = 0; l < 9; ++l) {
            const int32_t send = odd ? mine.l[l] : other.l[l];
            got.l[l] = __shfl_xor(send, (int)lag_deep_xor(kLevel), 64);
            lo.l[l] = odd ? got.l[l] : mine.l[l];
            hi.l[l] = odd ? other.l[l] : got.l[l];
        }
        v[i] = deep_bind<kF29>(lo, hi, rt);
    }
}

// levels 1 and 2 of slot kI (iteration kI of the batch), then the next slot's: written as a recursion so that the slots are registers
template <bool kF29, int kLevels, int kN, int kI>
__device__ __forceinline__ void deep_first(Fe (&v)[kN], const DeepArgs &A, const uint64_t g0, const uint64_t stride, const int32_t (&rt)[kLevels][kBindLds]) {
    const uint64_t g = g0 + kI * stride;
    const uint4 *p = A.src + 8 * g;
    const Fe e0 = fe_from_fr(fr_load(p)), e1 = fe_from_fr(fr_load(p + 2)), e2 = fe_from_fr(fr_load(p + 4)), e3 = fe_from_fr(fr_load(p + 6));
    const Fe a0 = deep_bind<kF29>(e0, e1, rt[0]);
    const Fe a1 = deep_bind<kF29>(e2, e3, rt[0]);
    if constexpr (kLevels == 1) {
        deep_store<kF29>(A.dst, lag_deep_entry(g, 1), a0);
        deep_store<kF29>(A.dst, lag_deep_entry(g, 1) + 1, a1);
    } else {
        v[kI] = deep_bind<kF29>(a0, a1, rt[1]);
        // one iteration at a time: with every iteration's loads hoisted to the top the batch would not fit the registers
        asm volatile("" : "+v"(v[kI].l[0]), "+v"(v[kI].l[8])::"memory");
    }
    if constexpr (kI + 1 < kN) deep_first<kF29, kLevels, kN, kI + 1>(v, A, g0, stride, rt);
}

// A lane reads entries 4g .. 4g+3 of the canonical source -- 128 contiguous bytes, round 2's access pattern, which lives off the L1 hits
// of neighbouring lanes' lines --, binds levels 1 and 2 in registers and every further level with the lane lag_deep_xor(level) away,
// kN = lag_deep_batch(kLevels) grid-stride iterations at a time so that every lane of every level computes an entry that is kept
// (lag_index.hpp).  n_groups is a multiple of kN x the grid stride (the launcher's grid), so a wavefront is in or out of the loop as a whole.
template <bool kF29, int kLevels>
__global__ __launch_bounds__(kBlock) void k_fix_deep(const DeepArgs A) {
    __shared__ int32_t rt[kLevels][kBindLds];
    for (int i = threadIdx.x; i < kLevels * kBindLds; i += kBlock) {
        const int l = i / kBindLds, c = i % kBindLds, k = c / 12, row = c % 12;
        rt[l][c] = row < 9 ? A.r[l].R[row][k] : 0;
    }
    __syncthreads();
    constexpr int kN = lag_deep_batch(kLevels);
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t g0 = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g0 < A.n_groups; g0 += kN * stride) {
        Fe v[kN];
        deep_first<kF29, kLevels, kN, 0>(v, A, g0, stride, rt);
        if constexpr (kLevels >= 2) {
            if constexpr (kLevels >= 3) deep_level<kF29, kN, 3>(v, rt[2]);
            if constexpr (kLevels >= 4) deep_level<kF29, kN, 4>(v, rt[3]);
            if constexpr (kLevels >= 5) deep_level<kF29, kN, 5>(v, rt[4]);
            const uint64_t g = g0 + lag_deep_iter(threadIdx.x, kLevels) * stride;
            deep_store<kF29>(A.dst, lag_deep_entry(g, kLevels), v[0]);
        }
    }
}

template <bool kF29>
static void launch_fix_deep_t(const DeepArgs &args, int grid, hipStream_t stream) {
    switch (args.levels) {
    case 1: hipLaunchKernelGGL((k_fix_deep<kF29, 1>), dim3(grid), dim3(kBlock), 0, stream, args); break;
    case 2: hipLaunchKernelGGL((k_fix_deep<kF29, 2>), dim3(grid), dim3(kBlock), 0, stream, args); break;
    case 3: hipLaunchKernelGGL((k_fix_deep<kF29, 3>), dim3(grid), dim3(kBlock), 0, stream, args); break;
    case 4: hipLaunchKernelGGL((k_fix_deep<kF29, 4>), dim3(grid), dim3(kBlock), 0, stream, args); break;
    default: hipLaunchKernelGGL((k_fix_deep<kF29, 5>), dim3(grid), dim3(kBlock), 0, stream, args); break;
    }
}

hipError_t launch_fix_deep(const DeepArgs &args, bool dst_f29, hipStream_t stream) {
    if (args.levels < 1 || args.levels > (uint32_t)kLagMaxLevels || args.n_groups < (uint64_t)kBlock || (args.n_groups & (args.n_groups - 1)) != 0) return hipErrorInvalidValue;
    if (dst_f29 && ((args.n_groups * 4) >> args.levels) % 128 != 0) return hipErrorInvalidValue; // F29 tables hold whole blocks of 128 entries
    // a power of two of blocks, so that the lag_deep_batch(levels) iterations a lane walks at once divide its share of the groups
    const uint64_t per_batch = (uint64_t)kBlock * (uint64_t)lag_deep_batch((int)args.levels);
    if (args.n_groups < per_batch) return hipErrorInvalidValue;
    const int grid = (int)std::min<uint64_t>(args.n_groups / per_batch, (uint64_t)kMaxGrid);
    if (dst_f29) launch_fix_deep_t<true>(args, grid, stream);
    else launch_fix_deep_t<false>(args, grid, stream);
    return hipGetLastError();
}

} // namespace scd
