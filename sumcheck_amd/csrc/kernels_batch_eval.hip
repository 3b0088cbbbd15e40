// kernels_batch_eval.hip -- the oracle queries of a whole batch in one launch: sc_poly_evaluate_batch and sc_gkr_subclaim_batch.
//
// A caller of the batched provers (kernels_batch.hip, kernels_batch_gkr.hip) ends every proof with an evaluation at the point the proof
// ended on: ListOfProductsOfPolynomials::evaluate (reference src/ml_sumcheck/data_structures.rs:99-109) or the three factors of
// GKRRoundSumcheckSubClaim::verify_subclaim (src/gkr_round_sumcheck/data_structures.rs:33-56).  One instance at a time that is several
// launches and a synchronisation each; here the whole batch is one plain launch (two for GKR, back to back on one stream).  Nothing in
// this file waits for the host: no ticket, no mailbox, no persistent block.
//   k_batch_eval      DenseMultilinearExtension::evaluate of one table per block.  Pass one reads the table from global memory, eight
//                     entries in and one out per lane (k_fold_multi's pass: variables 0..2, LSB first), into LDS as nine 29-bit limbs;
//                     every further variable is one in-place bind in LDS (bt_bind's pass, one barrier between its reads and writes).
//   k_batch_gkr_eval  SparseMultilinearExtension::evaluate at g | u | v of one list per block: eq(g, .), eq(u, .), eq(v, .) in LDS
//                     (bg_build_eq), then v * eq_g[z] * eq_u[x] * eq_v[y] per non-zero -- three products instead of 3 dim -- summed as
//                     eight 64-bit lanes of 32-bit limbs per lane of the block (exact in any order: wide_cell.hpp), folded mod p once.
// Every index is masked to dim bits per component before it addresses LDS (an index with a bit at or above 3 dim is an argument error
// that the host, or k_batch_gkr_idx_range in front of the launch, reports).
#include <algorithm>

#include "batch_round.hpp"
#include "wide_cell.hpp"

namespace scd {

// element `i` of a point in device memory as the carry-free bind's multiplier (r * 2^5 as 29-bit limbs: fe_device.hpp)
__device__ __forceinline__ FeU be_multiplier(const uint4 *pt, const uint32_t i) {
    const Fr r = fr_load(pt + 2 * (size_t)i);
    return feu_shl5(r.v);
}

// entries [i << L, (i + 1) << L) of `src` folded over variables 0..L-1, LSB first (k_fold_multi's body)
template <int L>
__device__ __forceinline__ Fe be_fold_first(const uint4 *__restrict__ src, const uint32_t i, const FeU (&r)[3]) {
    Fe v[1 << L];
    const uint4 *p = src + 2 * ((size_t)i << L);
#pragma unroll
    for (int j = 0; j < (1 << L); ++j) v[j] = fe_from_fr(fr_load(p + 2 * j));
#pragma unroll
    for (int l = 0; l < L; ++l) {
#pragma unroll
        for (int j = 0; j < (1 << (L - 1 - l)); ++j) v[j] = fe_carry_pass(fe_add(v[2 * j], fe_mul_u(fe_sub(v[2 * j + 1], v[2 * j]), r[l])));
    }
    return v[0];
}

__global__ __launch_bounds__(kTsBlock) void k_batch_eval(const EvalBatchArgs A) {
    extern __shared__ uint4 dyn_lds[];
    int32_t *const tab = reinterpret_cast<int32_t *>(dyn_lds); // [entry][kBtEnt]
    const uint32_t tid = threadIdx.x, b = blockIdx.x, group = b / A.group_size, member = b - group * A.group_size;
    const uint4 *__restrict__ src = A.tables[b];
    const uint4 *pt = A.points + 2 * ((size_t)group * A.pt_stride + A.pt_base + (size_t)member * A.pt_step);
    uint4 *const dst = A.out + 2 * ((size_t)group * A.out_stride + A.out_base + member);
    const uint32_t nv = A.nv;
    if (nv == 0) { // a table of zero variables is its single entry
        if (tid == 0) fr_store(dst, fr_load(src));
        return;
    }
    // ---- pass one: variables 0 .. L0 - 1 on the fly, 2^(nv - L0) entries into LDS ---------------------------------------------------------
    const uint32_t L0 = nv < 3u ? nv : 3u, m = 1u << (nv - L0);
    FeU r[3];
#pragma unroll
    for (uint32_t l = 0; l < 3u; ++l) r[l] = be_multiplier(pt, l < L0 ? l : 0u);
    for (uint32_t i = tid; i < m; i += kTsBlock) {
        const Fe v = L0 == 3u ? be_fold_first<3>(src, i, r) : L0 == 2u ? be_fold_first<2>(src, i, r) : be_fold_first<1>(src, i, r);
        bt_lds_store(tab + i * (uint32_t)kBtEnt, v);
    }
    __syncthreads();
    // ---- the remaining variables in LDS: entry e <- entries 2e, 2e + 1 (a pass reads everything it needs before it writes; later passes
    // read higher entries than any earlier pass wrote) ---------------------------------------------------------------------------------
    uint32_t E = m;
    for (uint32_t var = L0; var < nv; ++var) {
        const FeU r32 = be_multiplier(pt, var);
        const uint32_t half = E / 2;
        for (uint32_t i0 = 0; i0 < half; i0 += kTsBlock) {
            const uint32_t e = i0 + tid;
            const bool live = e < half;
            Fe v = fe_zero();
            if (live) {
                const Fe lo = bt_lds_load(tab + 2 * e * (uint32_t)kBtEnt), hi = bt_lds_load(tab + (2 * e + 1) * (uint32_t)kBtEnt);
                v = fe_carry_pass(fe_add(lo, fe_mul_u<true>(fe_sub(hi, lo), r32)));
            }
            __syncthreads();
            if (live) bt_lds_store(tab + e * (uint32_t)kBtEnt, v);
        }
        E = half;
        __syncthreads();
    }
    if (tid == 0) fr_store(dst, fe_to_fr(bt_lds_load(tab)));
}

__global__ __launch_bounds__(kTsBlock) void k_batch_gkr_eval(const GkrBatchInst *__restrict__ inst, const uint32_t dim, uint4 *__restrict__ out, const uint32_t out_stride) {
    extern __shared__ uint4 dyn_lds[];
    __shared__ uint4 pt_sh[2 * 3 * kGkrBatchMaxDim]; // g | u | v
    __shared__ uint64_t wave_sh[kTsBlock / 64][8];
    const uint32_t tid = threadIdx.x, cap = 1u << dim, mask = cap - 1u;
    const GkrBatchInst I = inst[blockIdx.x];
    // dynamic LDS: eq(g, .) | eq(u, .) | eq(v, .) (32 B per cell) | bg_build_eq's scratch
    uint4 *const eq_g = dyn_lds, *const eq_u = eq_g + 2 * (size_t)cap, *const eq_v = eq_u + 2 * (size_t)cap, *const tmp = eq_v + 2 * (size_t)cap;
    if (tid < 2 * 3 * dim) pt_sh[tid] = I.g[tid];
    __syncthreads();
    bg_build_eq(eq_g, tmp, pt_sh, dim);
    bg_build_eq(eq_u, tmp, pt_sh + 2 * dim, dim);
    bg_build_eq(eq_v, tmp, pt_sh + 4 * dim, dim);
    uint64_t lane[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) lane[j] = 0;
    for (uint64_t i = tid; i < I.nnz; i += kTsBlock) {
        const uint64_t id = I.idx[i];
        const uint32_t z = (uint32_t)id & mask, x = (uint32_t)(id >> dim) & mask, y = (uint32_t)(id >> (2 * dim)) & mask; // (masked: see the head of the file)
        const Fr a = fr_mul(fr_load(eq_g + 2 * z), fr_load(I.vals + 2 * i));
        const Fr t = fr_mul(fr_mul(a, fr_load(eq_u + 2 * x)), fr_load(eq_v + 2 * y));
#pragma unroll
        for (int j = 0; j < 8; ++j) lane[j] += (uint64_t)t.v[j]; // nnz <= 2^15 terms below 2^32 each: far from 2^63
    }
    // the block's lanes -> one cell: within the wavefront by shuffles, across the four wavefronts through LDS
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        uint32_t lo = (uint32_t)lane[j], hi = (uint32_t)(lane[j] >> 32);
        for (int off = 32; off >= 1; off >>= 1) {
            const uint64_t o = (uint64_t)__shfl_down(lo, off, 64) | ((uint64_t)__shfl_down(hi, off, 64) << 32);
            const uint64_t s = ((uint64_t)lo | ((uint64_t)hi << 32)) + o;
            lo = (uint32_t)s;
            hi = (uint32_t)(s >> 32);
        }
        lane[j] = (uint64_t)lo | ((uint64_t)hi << 32);
    }
    if ((tid & 63u) == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) wave_sh[tid >> 6][j] = lane[j];
    }
    __syncthreads();
    if (tid == 0) {
        uint64_t cell[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            cell[j] = 0;
#pragma unroll
            for (int w = 0; w < kTsBlock / 64; ++w) cell[j] += wave_sh[w][j];
        }
        fr_store(out + 2 * (size_t)blockIdx.x * out_stride, wide_fold_cell(cell));
    }
}

static size_t be_lds_bytes(uint32_t nv) { return ((size_t)1 << (nv > 3 ? nv - 3 : 0)) * (kBtEnt * 4); }
static size_t bge_lds_bytes(uint32_t dim) { return ((size_t)3 << dim) * 32 + ((size_t)2 << ((dim + 1) / 2)) * 32; }

bool eval_batch_shape_fits(uint32_t nv) { return nv <= kEvalBatchMaxNv && be_lds_bytes(nv) <= kBtLdsMax; }
bool gkr_eval_batch_shape_fits(uint32_t dim, uint64_t nnz_max) {
    if (dim == 0 || dim > (uint32_t)kGkrBatchMaxDim) return false;
    if (nnz_max > ((uint64_t)kGkrBatchMaxNnzPerCell << dim)) return false; // (one block walks the whole list)
    return bge_lds_bytes(dim) <= kBtLdsMax;
}

hipError_t launch_batch_eval(const EvalBatchArgs &args, uint32_t blocks, hipStream_t stream) {
    if (blocks == 0 || args.group_size == 0 || !eval_batch_shape_fits(args.nv)) return hipErrorInvalidValue;
    static bool done[64] = {}; // (more dynamic LDS than the default 64 KB limit of a launch)
    if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(k_batch_eval), (int)kBtLdsMax, done); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_batch_eval, dim3(blocks), dim3(kTsBlock), be_lds_bytes(args.nv), stream, args);
    return hipGetLastError();
}
hipError_t launch_batch_gkr_eval(const GkrBatchInst *inst, uint32_t n, uint32_t dim, uint4 *out, uint32_t out_stride, hipStream_t stream) {
    if (n == 0 || !gkr_eval_batch_shape_fits(dim, 0)) return hipErrorInvalidValue;
    static bool done[64] = {};
    if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(k_batch_gkr_eval), (int)kBtLdsMax, done); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_batch_gkr_eval, dim3(n), dim3(kTsBlock), bge_lds_bytes(dim), stream, inst, dim, out, out_stride);
    return hipGetLastError();
}

} // namespace scd
