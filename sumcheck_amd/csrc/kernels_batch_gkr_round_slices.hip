// kernels_batch_gkr_round_slices.hip -- the two initialisations of many GKR round proofs whose cells do not fit one block's LDS
// (sc_gkr_batch_prover_*, plan batch.gkr_rounds_slices, dim 10 .. 16): what k_batch_gkr_phase<1|2> (kernels_batch_gkr_rounds.hip) does
// with one block per instance, given to MANY blocks per instance as two plain launches per phase.
//
//   k_batch_gkr_terms<kPhase>  n x B blocks (B from the batch's largest list: batch_slices.hpp, gkr_bs_term_blocks).  Block (i, b) builds
//                              eq(g_i, .) -- phase 2: and eq(u_i, .) -- as two half tables in LDS (bg_build_eq_halves: at most
//                              2 x 2^8 x 32 B each), grid-strides over non-zeros b 256 + tid, + B 256, ... of instance i and adds the
//                              eight 32-bit limbs of every term into the eight uint64 lanes of the term's cell in DEVICE memory with
//                              relaxed agent-scope atomic adds.  The term is bg_accumulate's: phase 1 eq(g,z) v f3[y] into cell x, phase 2
//                              eq(g,z) eq(u,x) v into cell y; eq(., .) costs one more fr_mul for its two halves.  Integer sums are exact
//                              in any order, so the bits do not depend on the schedule.  A lane stays below 2^32 x 64 x 2^16 = 2^54 at
//                              the cap of 64 non-zeros per cell (wide_fold_cell needs < 2^63).
//   k_batch_gkr_fold<kPhase>   one lane per cell, directly behind on the same stream: wide_fold_cell -> fe_from_fr -> table 0, depth 0 of
//                              area A (phase 1) or B (phase 2); the same entry of table 1 gets f2[e] (phase 1) or f3[e] * f2(u)
//                              (fr_mul: mod.rs:71-75, literally).  f2(u) is what is left of area A's table 1 -- two entries at depth
//                              dim - 1, in (-(dim - 1) p, p): their difference's top limb stays below 16 x 2^22.9 < 2^29, fe_mul_u<true>'s
//                              documented range, as in k_batch_rounds_export at nv = 16 -- bound with u_{dim-1};
//                              canonical, kept in f2u[i].
// The cells are zeroed by the host side on the same stream in front of each terms launch; both phases share them.  NOTHING HERE WAITS:
// no block reads what a concurrent block writes (the atomics return nothing that is used), the order terms -> fold is the stream's.
// Every index component is masked to dim bits before it addresses LDS, f3 or a cell; an index with a bit at or above 3 dim is an
// argument error that k_batch_gkr_idx_range reports in front of the first launch that follows the indices.
// The lanes of a cell: lane-major per instance, cells[(i 8 + j) << dim | c] -- the eight atomics of a term go to eight lines, the same
// lane of neighbouring cells shares one; -DSC_GKR_CELLS_CELL_MAJOR builds cells[((i << dim | c) 8 + j] for the A/B
// (profiles/gkr_batch_round_slices_bench.json).
#include "batch_round.hpp"
#include "batch_slices.hpp"

namespace scd {

static_assert(kBsGkrTermsPerBlock % kTsBlock == 0 && kBsGkrCellBytes == 8 * sizeof(uint64_t), "a block's share is whole strides; eight lanes a cell");

constexpr uint32_t kGsHalf = 1u << ((kBsMaxNv + 1) / 2); // entries of a half table at the most

__device__ __forceinline__ size_t gs_lane_index(const uint32_t inst, const uint32_t j, const uint32_t c, const uint32_t dim) {
#ifdef SC_GKR_CELLS_CELL_MAJOR
    return ((((size_t)inst << dim) | c) << 3) | j;
#else
    return ((((size_t)inst << 3) | j) << dim) | c;
#endif
}

// kPoints 2 (sc_gkr_two_point_*): alpha eq(g, .) + beta eq(g2, .) stands where eq(g, .) stands.  It is not a product of halves, so g2 gets a
// pair of half tables of its own; alpha is folded into g's low half and beta into g2's (at most 2^8 products each, once per block), and a
// term's weight is lo[z_lo] hi[z_hi] + lo2[z_lo] hi2[z_hi]: one fr_mul and one fr_add more, canonical.  Terms per cell, and with them the
// lanes' bound, are unchanged.  Static LDS of <2, 2>: three pairs of half tables, 48 KB.
template <int kPhase, int kPoints>
__global__ __launch_bounds__(kTsBlock) void k_batch_gkr_terms(const BatchGkrSlicesArgs A) {
    __shared__ uint4 g_sh[2 * kBsMaxNv], u_sh[kPhase == 2 ? 2 * kBsMaxNv : 2];           // the points g and u
    __shared__ uint4 eq_g[2 * 2 * kGsHalf], eq_u[kPhase == 2 ? 2 * 2 * kGsHalf : 2];     // lo | hi half tables, 32-byte elements
    __shared__ uint4 eq_g2[kPoints == 2 ? 2 * 2 * kGsHalf : 2];                          // two-point form: g2's half tables
    const uint32_t tid = threadIdx.x, inst = blockIdx.x / A.blocks_per_inst, blk = blockIdx.x % A.blocks_per_inst; // (the grid is exactly n x blocks_per_inst)
    const uint32_t dim = A.dim, mask = (1u << dim) - 1u, kl = (dim + 1) / 2, lmask = (1u << kl) - 1u;
    const GkrBatchInst I = A.inst[inst];
    if (tid < 2 * dim) {
        g_sh[tid] = I.g[tid];
        if (kPhase == 2) u_sh[tid] = A.u[2 * ((size_t)(tid >> 1) * A.n + inst) + (tid & 1u)];
    }
    __syncthreads();
    bg_build_eq_halves(eq_g, eq_g + 2 * kGsHalf, g_sh, dim);
    if (kPhase == 2) bg_build_eq_halves(eq_u, eq_u + 2 * kGsHalf, u_sh, dim);
    if (kPoints == 2) {
        bg_build_eq_halves(eq_g2, eq_g2 + 2 * kGsHalf, A.g2 + 2 * (size_t)inst * dim, dim);
        const Fr alpha = fr_load(A.coef + 4 * (size_t)inst), beta = fr_load(A.coef + 4 * (size_t)inst + 2);
        for (uint32_t t = tid; t <= lmask; t += kTsBlock) {
            fr_store(eq_g + 2 * t, fr_mul(alpha, fr_load(eq_g + 2 * t)));
            fr_store(eq_g2 + 2 * t, fr_mul(beta, fr_load(eq_g2 + 2 * t)));
        }
        __syncthreads();
    }
    const uint64_t stride = (uint64_t)A.blocks_per_inst * kTsBlock;
    for (uint64_t i = (uint64_t)blk * kTsBlock + tid; i < I.nnz; i += stride) {
        const uint64_t id = I.idx[i];
        const uint32_t z = (uint32_t)id & mask, x = (uint32_t)(id >> dim) & mask, y = (uint32_t)(id >> (2 * dim)) & mask;
        Fr eg = fr_mul(fr_load(eq_g + 2 * (z & lmask)), fr_load(eq_g + 2 * kGsHalf + 2 * (z >> kl)));
        if (kPoints == 2) eg = fr_add(eg, fr_mul(fr_load(eq_g2 + 2 * (z & lmask)), fr_load(eq_g2 + 2 * kGsHalf + 2 * (z >> kl))));
        const Fr a = fr_mul(eg, fr_load(I.vals + 2 * i));
        Fr t;
        if (kPhase == 1) t = fr_mul(a, fr_load(I.f3 + 2 * (size_t)y));
        else t = fr_mul(a, fr_mul(fr_load(eq_u + 2 * (x & lmask)), fr_load(eq_u + 2 * kGsHalf + 2 * (x >> kl))));
        const uint32_t c = kPhase == 1 ? x : y;
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) __hip_atomic_fetch_add(A.cells + gs_lane_index(inst, j, c, dim), (uint64_t)t.v[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <int kPhase>
__global__ __launch_bounds__(kTsBlock) void k_batch_gkr_fold(const BatchGkrSlicesArgs A) {
    const uint32_t dim = A.dim, cap = 1u << dim;
    const uint64_t i = (uint64_t)blockIdx.x * kTsBlock + threadIdx.x; // (instance, cell): 2^dim is a multiple of the block, so a block is inside one instance
    if (i >= ((uint64_t)A.n << dim)) return;
    const uint32_t inst = (uint32_t)(i >> dim), c = (uint32_t)i & (cap - 1u);
    const GkrBatchInst I = A.inst[inst];
    const size_t region = (size_t)inst * 2 * 2 * cap * kBtEnt; // the instance's two tables, table u at + u * 2 * cap slots
    int32_t *const dst = (kPhase == 1 ? A.work_a : A.work_b) + region;
    uint64_t lane[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) lane[j] = A.cells[gs_lane_index(inst, j, c, dim)];
    br_slot_store(dst + (size_t)c * kBtEnt, fe_from_fr(wide_fold_cell(lane)));
    if (kPhase == 1) {
        br_slot_store(dst + ((size_t)2 * cap + c) * kBtEnt, fe_from_fr(fr_load(I.f2 + 2 * (size_t)c)));
    } else {
        // f2(u): every lane of the instance binds the same two entries (uniform loads), the lane of cell 0 keeps the result
        const int32_t *src = A.work_a + region + ((size_t)2 * cap + batch_rounds_off(dim, dim - 1u)) * kBtEnt;
        const FeU r32 = feu_shl5(fr_load(A.u + 2 * ((size_t)(dim - 1u) * A.n + inst)).v);
        const Fe lo = br_slot_load(src), hi = br_slot_load(src + kBtEnt);
        const Fr f2u = fe_to_fr(fe_carry_pass(fe_add(lo, fe_mul_u<true>(fe_sub(hi, lo), r32))));
        if (c == 0) fr_store(A.f2u + 2 * (size_t)inst, f2u);
        br_slot_store(dst + ((size_t)2 * cap + c) * kBtEnt, fe_from_fr(fr_mul(fr_load(I.f3 + 2 * (size_t)c), f2u)));
    }
}

hipError_t launch_batch_gkr_slices_phase(int phase, BatchGkrSlicesArgs args, uint64_t nnz_max, hipStream_t stream, int points) {
    if ((points != 1 && points != 2) || (points == 2 && (!args.g2 || !args.coef))) return hipErrorInvalidValue;
    if ((phase != 1 && phase != 2) || args.n == 0 || args.dim <= (uint32_t)kGkrBatchMaxDim || args.dim > kBsMaxNv || !args.inst || !args.work_a || !args.cells) return hipErrorInvalidValue;
    if (phase == 2 && (!args.work_b || !args.u || !args.f2u)) return hipErrorInvalidValue;
    if (nnz_max > (kGkrBatchMaxNnzPerCell << args.dim)) return hipErrorInvalidValue; // (the lanes' bound)
    const uint64_t B = gkr_bs_term_blocks(nnz_max), grid_terms = (uint64_t)args.n * B, grid_fold = (((uint64_t)args.n << args.dim) + kTsBlock - 1) / kTsBlock;
    if (grid_terms >= (1ULL << 31) || grid_fold >= (1ULL << 31)) return hipErrorInvalidValue;
    args.blocks_per_inst = (uint32_t)B;
    if (points == 1) {
        if (phase == 1) hipLaunchKernelGGL((k_batch_gkr_terms<1, 1>), dim3((uint32_t)grid_terms), dim3(kTsBlock), 0, stream, args);
        else hipLaunchKernelGGL((k_batch_gkr_terms<2, 1>), dim3((uint32_t)grid_terms), dim3(kTsBlock), 0, stream, args);
    } else {
        if (phase == 1) hipLaunchKernelGGL((k_batch_gkr_terms<1, 2>), dim3((uint32_t)grid_terms), dim3(kTsBlock), 0, stream, args);
        else hipLaunchKernelGGL((k_batch_gkr_terms<2, 2>), dim3((uint32_t)grid_terms), dim3(kTsBlock), 0, stream, args);
    }
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (phase == 1) hipLaunchKernelGGL(k_batch_gkr_fold<1>, dim3((uint32_t)grid_fold), dim3(kTsBlock), 0, stream, args);
    else hipLaunchKernelGGL(k_batch_gkr_fold<2>, dim3((uint32_t)grid_fold), dim3(kTsBlock), 0, stream, args);
    return hipGetLastError();
}

} // namespace scd
