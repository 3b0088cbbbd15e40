// kernels_batch_gkr_gates.hip -- the two initialisations of the GATE form of the batched interactive GKR rounds (k_batch_gkr_gates_phase<1|2>):
// sc_gkr_gates_init_batch / sc_gkr_gates_next_batch.  A layer of multiplication and addition gates (XZZPS19),
//     W_out[z] = sum over MUL of v f2[x] f3[y]  +  sum over ADD of v (f2[x] + f3[y]),
// is proved at E(z) = eq(g, z) (or alpha eq(g, z) + beta eq(g2, z)) by two sumchecks of ONE shape, t0 t1 + t2 -- three tables, a product of
// two multiplicands and a product of one, coefficients one, messages of three evaluations --, so the rounds are k_batch_round's as they
// are (kernels_batch_rounds.hip, U = 3, K = 2, D = 3) and what is new is the filling of the work areas:
//   phase<1>  area A, depth 0:  t0 = f2;  t1 = H1[x] = sum_MUL E[z] v f3[y] + sum_ADD E[z] v;  t2 = H2[x] = sum_ADD E[z] v f3[y];
//   phase<2>  f2(u) out of what is left of area A's t0, as k_batch_gkr_phase<2> binds it (canonical, kept per instance); eq(u, .);
//             area B, depth 0:  t0 = f3;  t1 = T1[y] = f2(u) sum_MUL E[z] eq(u,x) v + sum_ADD E[z] eq(u,x) v;  t2 = T2[y] = f2(u) sum_ADD E[z] eq(u,x) v.
// One block per instance.  The cells are bg_accumulate's (eight uint64 lanes of 32-bit limbs per cell, LDS atomic adds: exact in any
// order, folded mod p once per cell), ONE array used in two passes so that the LDS stays 128 B x 2^dim: eq(g, .) | eq(u, .) | the cells.
// Pass one takes BOTH lists into the same cells (t1), pass two the ADD list alone (t2).  In phase two MUL's terms are scaled by f2(u) before
// they are added, and T2 is f2(u) times the folded cell.  A cell receives at most 2 x 64 x 2^9 = 2^16 terms: a lane stays below 2^48.
// bg_accumulate_terms (batch_round.hpp) is not used: it zeroes its cells itself and addresses cell z, here two lists go into one pass and
// the cell is x or y; gg_add_terms below is its loop with the cell left to the term.  Every index is masked to dim bits per component
// before it addresses LDS, f3 or a cell; an index with a bit at or above 3 dim is an argument error found in front of the launch.
#include <algorithm>

#include "batch_round.hpp"
#include "batch_slices.hpp"

namespace scd {

namespace {

__device__ __forceinline__ void gg_zero_cells(uint64_t *cell, const uint32_t cap) {
    for (uint32_t i = threadIdx.x; i < 8u * cap; i += kTsBlock) cell[i] = 0;
    __syncthreads();
}

// term(i, z, x, y, c): non-zero i's canonical term, c <- its cell.  No barrier: the caller zeroes in front and folds behind one.
template <typename Term>
__device__ __forceinline__ void gg_add_terms(uint64_t *cell, const uint64_t *idx, const uint64_t nnz, const uint32_t dim, const Term &term) {
    const uint32_t mask = (1u << dim) - 1u;
    for (uint64_t i = threadIdx.x; i < nnz; i += kTsBlock) {
        const uint64_t id = idx[i];
        const uint32_t z = (uint32_t)id & mask, x = (uint32_t)(id >> dim) & mask, y = (uint32_t)(id >> (2 * dim)) & mask;
        uint32_t c = 0;
        const Fr t = term(i, z, x, y, c);
#pragma unroll
        for (int j = 0; j < 8; ++j) __hip_atomic_fetch_add(cell + (((uint32_t)j << dim) | (c & mask)), (uint64_t)t.v[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
}

// store(c, value) takes cell c's canonical element.  Ends behind a barrier: the cells may be zeroed again.
template <typename Store>
__device__ __forceinline__ void gg_fold_cells(const uint64_t *cell, const uint32_t dim, const Store &store) {
    for (uint32_t c = threadIdx.x; c < (1u << dim); c += kTsBlock) {
        uint64_t lane[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) lane[j] = cell[((uint32_t)j << dim) | c];
        store(c, wide_fold_cell(lane));
    }
    __syncthreads();
}

// kPoints 2: eq_g <- alpha eq(g, .) + beta eq(g2, .), canonical, eq(g2, .) built in eq(u, .)'s region (k_batch_gkr_phase's fold, restated:
// that kernel's translation unit keeps its code)
__device__ __forceinline__ void gg_fold_second_point(uint4 *eq_g, uint4 *eq_g2, uint4 *tmp, const uint4 *g2, const uint4 *coef, const uint32_t dim) {
    bg_build_eq(eq_g2, tmp, g2, dim);
    const Fr alpha = fr_load(coef), beta = fr_load(coef + 2);
    for (uint32_t b = threadIdx.x; b < (1u << dim); b += kTsBlock) fr_store(eq_g + 2 * b, fr_add(fr_mul(alpha, fr_load(eq_g + 2 * b)), fr_mul(beta, fr_load(eq_g2 + 2 * b))));
    __syncthreads();
}

} // namespace

template <int kPhase, int kPoints>
__global__ __launch_bounds__(kTsBlock) void k_batch_gkr_gates_phase(const BatchGkrGatesArgs A) {
    extern __shared__ uint4 dyn_lds[];
    __shared__ uint4 g_sh[2 * kGkrBatchMaxDim], u_sh[2 * kGkrBatchMaxDim]; // the points g and u
    const uint32_t tid = threadIdx.x, inst = blockIdx.x; // (the grid is exactly n blocks)
    const uint32_t dim = A.dim, cap = 1u << dim;
    uint4 *const eq_g = dyn_lds, *const eq_u = eq_g + 2 * (size_t)cap;
    uint64_t *const cell = reinterpret_cast<uint64_t *>(eq_u + 2 * (size_t)cap);
    const GkrGatesInst I = A.inst[inst];
    const size_t region = (size_t)inst * 3 * 2 * cap * kBtEnt; // the instance's three tables, table t at + t * 2 * cap slots
    int32_t *const dst = (kPhase == 1 ? A.work_a : A.work_b) + region;
    int32_t *const t0 = dst, *const t1 = dst + (size_t)2 * cap * kBtEnt, *const t2 = dst + (size_t)4 * cap * kBtEnt;
    if (tid < 2 * dim) {
        g_sh[tid] = I.g[tid];
        if (kPhase == 2) u_sh[tid] = A.u[2 * ((size_t)(tid >> 1) * A.n + inst) + (tid & 1u)];
    }
    __syncthreads();
    bg_build_eq(eq_g, reinterpret_cast<uint4 *>(cell), g_sh, dim);
    if (kPoints == 2) gg_fold_second_point(eq_g, eq_u, reinterpret_cast<uint4 *>(cell), A.g2 + 2 * (size_t)inst * dim, A.coef + 4 * (size_t)inst, dim);
    if (kPhase == 1) {
        // ---- H1: both lists into the same cells ----
        gg_zero_cells(cell, cap);
        gg_add_terms(cell, I.mul_idx, I.mul_nnz, dim, [&](const uint64_t i, const uint32_t z, const uint32_t x, const uint32_t y, uint32_t &c) {
            c = x;
            return fr_mul(fr_mul(fr_load(eq_g + 2 * z), fr_load(I.mul_vals + 2 * i)), fr_load(I.f3 + 2 * (size_t)y));
        });
        gg_add_terms(cell, I.add_idx, I.add_nnz, dim, [&](const uint64_t i, const uint32_t z, const uint32_t x, const uint32_t, uint32_t &c) {
            c = x;
            return fr_mul(fr_load(eq_g + 2 * z), fr_load(I.add_vals + 2 * i));
        });
        gg_fold_cells(cell, dim, [&](const uint32_t c, const Fr &v) { br_slot_store(t1 + (size_t)c * kBtEnt, fe_from_fr(v)); });
        // ---- H2: the ADD list alone ----
        gg_zero_cells(cell, cap);
        gg_add_terms(cell, I.add_idx, I.add_nnz, dim, [&](const uint64_t i, const uint32_t z, const uint32_t x, const uint32_t y, uint32_t &c) {
            c = x;
            return fr_mul(fr_mul(fr_load(eq_g + 2 * z), fr_load(I.add_vals + 2 * i)), fr_load(I.f3 + 2 * (size_t)y));
        });
        gg_fold_cells(cell, dim, [&](const uint32_t c, const Fr &v) { br_slot_store(t2 + (size_t)c * kBtEnt, fe_from_fr(v)); });
        for (uint32_t e = tid; e < cap; e += kTsBlock) br_slot_store(t0 + (size_t)e * kBtEnt, fe_from_fr(fr_load(I.f2 + 2 * (size_t)e)));
    } else {
        // f2(u): every lane binds the same two entries of area A's t0 (uniform loads), lane 0 keeps the result
        const int32_t *src = A.work_a + region + batch_rounds_off(dim, dim - 1u) * kBtEnt;
        const FeU r32 = feu_shl5(fr_load(u_sh + 2 * (dim - 1u)).v);
        const Fe lo = br_slot_load(src), hi = br_slot_load(src + kBtEnt);
        const Fr f2u = fe_to_fr(fe_carry_pass(fe_add(lo, fe_mul_u<true>(fe_sub(hi, lo), r32))));
        if (tid == 0) fr_store(A.f2u + 2 * (size_t)inst, f2u);
        bg_build_eq(eq_u, reinterpret_cast<uint4 *>(cell), u_sh, dim);
        // ---- T1: MUL's terms scaled by f2(u), ADD's as they are, into the same cells ----
        gg_zero_cells(cell, cap);
        gg_add_terms(cell, I.mul_idx, I.mul_nnz, dim, [&](const uint64_t i, const uint32_t z, const uint32_t x, const uint32_t y, uint32_t &c) {
            c = y;
            return fr_mul(fr_mul(fr_mul(fr_load(eq_g + 2 * z), fr_load(I.mul_vals + 2 * i)), fr_load(eq_u + 2 * x)), f2u);
        });
        gg_add_terms(cell, I.add_idx, I.add_nnz, dim, [&](const uint64_t i, const uint32_t z, const uint32_t x, const uint32_t y, uint32_t &c) {
            c = y;
            return fr_mul(fr_mul(fr_load(eq_g + 2 * z), fr_load(I.add_vals + 2 * i)), fr_load(eq_u + 2 * x));
        });
        gg_fold_cells(cell, dim, [&](const uint32_t c, const Fr &v) { br_slot_store(t1 + (size_t)c * kBtEnt, fe_from_fr(v)); });
        // ---- T2 = f2(u) x the ADD sum ----
        gg_zero_cells(cell, cap);
        gg_add_terms(cell, I.add_idx, I.add_nnz, dim, [&](const uint64_t i, const uint32_t z, const uint32_t x, const uint32_t y, uint32_t &c) {
            c = y;
            return fr_mul(fr_mul(fr_load(eq_g + 2 * z), fr_load(I.add_vals + 2 * i)), fr_load(eq_u + 2 * x));
        });
        gg_fold_cells(cell, dim, [&](const uint32_t c, const Fr &v) { br_slot_store(t2 + (size_t)c * kBtEnt, fe_from_fr(fr_mul(v, f2u))); });
        for (uint32_t e = tid; e < cap; e += kTsBlock) br_slot_store(t0 + (size_t)e * kBtEnt, fe_from_fr(fr_load(I.f3 + 2 * (size_t)e)));
    }
}

// ---- the values of gate layers (sc_gkr_gates_layers_eval_batch): k_batch_gkr_eval_layers / _terms / _fold (kernels_batch_gkr_eval_layers.hip)
// with the ADD list beside the MUL list.  W_out[z] = sum_MUL v A[x] B[y] + sum_ADD v (A[x] + B[y]); ADD's term is one fr_add and one fr_mul
// and goes into the same cells as MUL's.  A cell's lane stays below 2^63 while mul_nnz + add_nnz < 2^31 (the host side refuses more).
__global__ __launch_bounds__(kTsBlock) void k_batch_gkr_gates_eval_layers(const GkrGatesEvalArgs G) {
    extern __shared__ uint4 dyn_lds[];
    const GkrEvalLayersArgs &A = G.base;
    const uint32_t tid = threadIdx.x, inst = A.first + blockIdx.x; // (the grid is exactly the launch's instances)
    const uint32_t dim = A.dim, cap = 1u << dim;
    uint4 *const tab_a = dyn_lds, *const tab_b = tab_a + 2 * (size_t)cap;
    uint64_t *const cell = reinterpret_cast<uint64_t *>(tab_b + 2 * (size_t)cap);
    {
        const GkrBatchInst I = A.inst[inst];
        for (uint32_t e = tid; e < cap; e += kTsBlock) {
            fr_store(tab_a + 2 * e, fr_load(I.f2 + 2 * (size_t)e));
            fr_store(tab_b + 2 * e, fr_load(I.f3 + 2 * (size_t)e));
        }
    } // (visible behind gg_zero_cells' barrier)
    for (uint32_t k = 0; k < A.n_layers; ++k) {
        const size_t rec = (size_t)k * A.n + inst;
        const uint4 *const mv = A.inst[rec].vals, *const av = G.add[rec].vals;
        uint4 *const dst = A.out[rec];
        const uint4 *const tb = k == 0 ? tab_b : tab_a;
        gg_zero_cells(cell, cap);
        gg_add_terms(cell, A.inst[rec].idx, A.inst[rec].nnz, dim, [&](const uint64_t i, const uint32_t z, const uint32_t x, const uint32_t y, uint32_t &c) {
            c = z;
            return fr_mul(fr_mul(fr_load(mv + 2 * i), fr_load(tab_a + 2 * x)), fr_load(tb + 2 * y));
        });
        gg_add_terms(cell, G.add[rec].idx, G.add[rec].nnz, dim, [&](const uint64_t i, const uint32_t z, const uint32_t x, const uint32_t y, uint32_t &c) {
            c = z;
            return fr_mul(fr_load(av + 2 * i), fr_add(fr_load(tab_a + 2 * x), fr_load(tb + 2 * y)));
        });
        gg_fold_cells(cell, dim, [&](const uint32_t c, const Fr &v) {
            fr_store(dst + 2 * (size_t)c, v);
            fr_store(tab_a + 2 * c, v); // (every term of this layer is behind a barrier: nothing reads the old table any more)
        });
    }
}

hipError_t launch_batch_gkr_gates_eval_layers(GkrGatesEvalArgs args, hipStream_t stream) {
    if (args.base.n == 0 || args.base.n_layers == 0 || !gkr_batch_shape_fits(args.base.dim, 0) || !args.base.inst || !args.add || !args.base.out) return hipErrorInvalidValue;
    const size_t lds = (size_t)128 << args.base.dim; // (at most 64 KB: within a launch's default limit)
    constexpr uint32_t kMaxGrid = 1u << 30;
    for (uint32_t first = 0; first < args.base.n; first += kMaxGrid) {
        args.base.first = first;
        hipLaunchKernelGGL(k_batch_gkr_gates_eval_layers, dim3(std::min(args.base.n - first, kMaxGrid)), dim3(kTsBlock), lds, stream, args);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

namespace {
__device__ __forceinline__ size_t gg_lane_index(const uint32_t inst, const uint32_t j, const uint32_t c, const uint32_t dim) { return ((((size_t)inst << 3) | j) << dim) | c; }
} // namespace

// one list of every instance of ONE layer into the cells (k_batch_gkr_eval_terms' grid and layout); kAdd: the list is the ADD list
template <bool kAdd>
__global__ __launch_bounds__(kTsBlock) void k_batch_gkr_gates_eval_terms(const GkrGatesEvalArgs G) {
    const GkrEvalLayersArgs &A = G.base;
    const uint32_t tid = threadIdx.x, inst = A.first + blockIdx.x / A.blocks_per_inst, blk = blockIdx.x % A.blocks_per_inst; // (the grid is exactly instances x blocks_per_inst)
    const uint32_t dim = A.dim, mask = (1u << dim) - 1u;
    const GkrBatchInst T = A.inst[inst], I = kAdd ? G.add[inst] : T; // (the tables are the MUL record's)
    const uint64_t stride = (uint64_t)A.blocks_per_inst * kTsBlock;
    for (uint64_t i = (uint64_t)blk * kTsBlock + tid; i < I.nnz; i += stride) {
        const uint64_t id = I.idx[i];
        const uint32_t z = (uint32_t)id & mask, x = (uint32_t)(id >> dim) & mask, y = (uint32_t)(id >> (2 * dim)) & mask;
        const Fr a = fr_load(T.f2 + 2 * (size_t)x), b = fr_load(T.f3 + 2 * (size_t)y), v = fr_load(I.vals + 2 * i);
        const Fr t = kAdd ? fr_mul(v, fr_add(a, b)) : fr_mul(fr_mul(v, a), b);
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) __hip_atomic_fetch_add(A.cells + gg_lane_index(inst, j, z, dim), (uint64_t)t.v[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(kTsBlock) void k_batch_gkr_gates_eval_fold(const GkrEvalLayersArgs A) {
    const uint32_t dim = A.dim;
    const uint64_t i = ((uint64_t)A.first << dim) + (uint64_t)blockIdx.x * kTsBlock + threadIdx.x; // (instance, cell)
    if (i >= ((uint64_t)A.n << dim)) return;
    const uint32_t inst = (uint32_t)(i >> dim), c = (uint32_t)i & ((1u << dim) - 1u);
    uint64_t lane[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) lane[j] = A.cells[gg_lane_index(inst, j, c, dim)];
    fr_store(A.out[inst] + 2 * (size_t)c, wide_fold_cell(lane));
}

hipError_t launch_batch_gkr_gates_eval_cells(GkrGatesEvalArgs args, uint64_t nnz_max, hipStream_t stream) {
    GkrEvalLayersArgs &A = args.base;
    if (A.n == 0 || A.dim == 0 || A.dim > 21 || !A.inst || !args.add || !A.out || !A.cells || nnz_max >= (1ULL << 31)) return hipErrorInvalidValue;
    const uint64_t B = gkr_bs_term_blocks(nnz_max);
    A.blocks_per_inst = (uint32_t)B;
    // a launch takes as many whole instances as keep both grids below 2^30 blocks
    const uint64_t per_fold = ((1ULL << A.dim) + kTsBlock - 1) / kTsBlock, per_inst = std::max(B, per_fold);
    const uint32_t step = (uint32_t)std::max<uint64_t>(1, (1ULL << 30) / per_inst);
    for (uint64_t first = 0; first < A.n; first += step) {
        const uint64_t count = std::min<uint64_t>(step, A.n - first);
        A.first = (uint32_t)first;
        hipLaunchKernelGGL(k_batch_gkr_gates_eval_terms<false>, dim3((uint32_t)(count * B)), dim3(kTsBlock), 0, stream, args);
        hipLaunchKernelGGL(k_batch_gkr_gates_eval_terms<true>, dim3((uint32_t)(count * B)), dim3(kTsBlock), 0, stream, args);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    for (uint64_t first = 0; first < A.n; first += step) {
        const uint64_t count = std::min<uint64_t>(step, A.n - first);
        GkrEvalLayersArgs F = A;
        F.first = (uint32_t)first;
        F.n = (uint32_t)(first + count); // (the fold's bound: the launch ends with its last instance)
        hipLaunchKernelGGL(k_batch_gkr_gates_eval_fold, dim3((uint32_t)(((count << A.dim) + kTsBlock - 1) / kTsBlock)), dim3(kTsBlock), 0, stream, F);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_batch_gkr_gates_phase(int phase, const BatchGkrGatesArgs &args, hipStream_t stream, int points) {
    if ((phase != 1 && phase != 2) || args.n == 0 || !gkr_batch_shape_fits(args.dim, 0) || !args.inst || !args.work_a) return hipErrorInvalidValue;
    if (phase == 2 && (!args.work_b || !args.u || !args.f2u)) return hipErrorInvalidValue;
    if ((points != 1 && points != 2) || (points == 2 && (!args.g2 || !args.coef))) return hipErrorInvalidValue;
    const size_t lds = (size_t)128 << args.dim; // (at most 64 KB: within a launch's default limit)
    if (points == 1) {
        if (phase == 1) hipLaunchKernelGGL((k_batch_gkr_gates_phase<1, 1>), dim3(args.n), dim3(kTsBlock), lds, stream, args);
        else hipLaunchKernelGGL((k_batch_gkr_gates_phase<2, 1>), dim3(args.n), dim3(kTsBlock), lds, stream, args);
    } else {
        if (phase == 1) hipLaunchKernelGGL((k_batch_gkr_gates_phase<1, 2>), dim3(args.n), dim3(kTsBlock), lds, stream, args);
        else hipLaunchKernelGGL((k_batch_gkr_gates_phase<2, 2>), dim3(args.n), dim3(kTsBlock), lds, stream, args);
    }
    return hipGetLastError();
}

} // namespace scd
