// kernels_batch_gkr_eval_layers.hip -- the values of GKR circuit layers on the device (sc_gkr_layers_eval_batch): what every call of the
// sc_gkr_batch_prover_* family consumes as f2 and f3.  Per instance and layer
//     W_out[z] = sum over f1's non-zeros (z | x << dim | y << 2 dim, v) of  v * A[x] * B[y],
// (A, B) = the caller's (f2, f3) for layer 0, (W, W) of the layer before for every later one.  Two fr_mul per non-zero and a sum into
// 2^dim cells; the sum is the one the prover's initialisations make: a cell is eight uint64 lanes of 32-bit limbs, a term adds its eight
// limbs with integer atomics -- exact in any order, so both plans give the same canonical bits -- and wide_fold_cell folds a cell once.
//
//   k_batch_gkr_eval_layers  plan batch.gkr_eval_layers_one_block: ONE launch for all layers, one block of 256 lanes per instance.  LDS:
//                            table A | table B (canonical 32-byte elements) | the cells (lane-major, bg_accumulate's layout: the same lane
//                            of neighbouring cells in neighbouring banks), 128 B x 2^dim -- 64 KB at dim 9, two blocks per CU.  Layer 0
//                            loads f2 and f3 once; a layer's fold stores every element to the caller's table (plain 16-byte stores) AND
//                            into table A, which is both inputs of the next layer.  Nothing waits for the host or for another block.
//   k_batch_gkr_eval_terms   plan batch.gkr_eval_cells, per layer behind a zeroing of the cells: n x B blocks (B = gkr_bs_term_blocks of the
//                            layer's longest list), a grid stride over the instance's list, A[x] and B[y] gathered from device memory,
//                            eight relaxed agent-scope 64-bit atomic adds into cells[(i 8 + j) << dim | z] (k_batch_gkr_terms' layout);
//   k_batch_gkr_eval_fold    one lane per (instance, cell) directly behind on the same stream: wide_fold_cell -> the caller's table.
//                            Layer k + 1's terms read what layer k's fold wrote: the stream's order is the only dependence -- no counter,
//                            no fence, nothing polls.
// Lanes: a limb is below 2^32, so a lane stays below 2^63 -- wide_fold_cell's range -- while a list has fewer than 2^31 non-zeros (the host
// side refuses more); the one-block plan's lists end at 64 x 2^9 = 2^15.
// Every index component is masked to dim bits before it addresses a table or a cell; an index with a bit at or above 3 dim is an argument
// error that the host, or k_batch_gkr_idx_range in front of the first launch, reports.
#include "batch_round.hpp"
#include "batch_slices.hpp"

namespace scd {

__global__ __launch_bounds__(kTsBlock) void k_batch_gkr_eval_layers(const GkrEvalLayersArgs A) {
    extern __shared__ uint4 dyn_lds[];
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
    } // (visible behind bg_accumulate_terms' first barrier)
    for (uint32_t k = 0; k < A.n_layers; ++k) {
        const size_t rec = (size_t)k * A.n + inst;
        const uint64_t *const idx = A.inst[rec].idx;
        const uint4 *const vals = A.inst[rec].vals;
        uint4 *const dst = A.out[rec];
        const uint4 *const tb = k == 0 ? tab_b : tab_a;
        bg_accumulate_terms(
            cell, idx, A.inst[rec].nnz, dim,
            [&](const uint64_t i, const uint32_t x, const uint32_t y) { return fr_mul(fr_mul(fr_load(vals + 2 * i), fr_load(tab_a + 2 * x)), fr_load(tb + 2 * y)); },
            [&](const uint32_t c, const Fr &v) {
                fr_store(dst + 2 * (size_t)c, v);
                fr_store(tab_a + 2 * c, v); // (every term of this layer is behind a barrier: nothing reads the old table any more)
            });
    }
}

hipError_t launch_batch_gkr_eval_layers(GkrEvalLayersArgs args, hipStream_t stream) {
    if (args.n == 0 || args.n_layers == 0 || !gkr_batch_shape_fits(args.dim, 0) || !args.inst || !args.out) return hipErrorInvalidValue;
    const size_t lds = (size_t)128 << args.dim; // (at most 64 KB: within a launch's default limit)
    constexpr uint32_t kMaxGrid = 1u << 30;
    for (uint32_t first = 0; first < args.n; first += kMaxGrid) {
        args.first = first;
        hipLaunchKernelGGL(k_batch_gkr_eval_layers, dim3(std::min(args.n - first, kMaxGrid)), dim3(kTsBlock), lds, stream, args);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

__device__ __forceinline__ size_t ge_lane_index(const uint32_t inst, const uint32_t j, const uint32_t c, const uint32_t dim) { return ((((size_t)inst << 3) | j) << dim) | c; }

__global__ __launch_bounds__(kTsBlock) void k_batch_gkr_eval_terms(const GkrEvalLayersArgs A) {
    const uint32_t tid = threadIdx.x, inst = A.first + blockIdx.x / A.blocks_per_inst, blk = blockIdx.x % A.blocks_per_inst; // (the grid is exactly instances x blocks_per_inst)
    const uint32_t dim = A.dim, mask = (1u << dim) - 1u;
    const GkrBatchInst I = A.inst[inst];
    const uint64_t stride = (uint64_t)A.blocks_per_inst * kTsBlock;
    for (uint64_t i = (uint64_t)blk * kTsBlock + tid; i < I.nnz; i += stride) {
        const uint64_t id = I.idx[i];
        const uint32_t z = (uint32_t)id & mask, x = (uint32_t)(id >> dim) & mask, y = (uint32_t)(id >> (2 * dim)) & mask;
        const Fr t = fr_mul(fr_mul(fr_load(I.vals + 2 * i), fr_load(I.f2 + 2 * (size_t)x)), fr_load(I.f3 + 2 * (size_t)y));
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) __hip_atomic_fetch_add(A.cells + ge_lane_index(inst, j, z, dim), (uint64_t)t.v[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(kTsBlock) void k_batch_gkr_eval_fold(const GkrEvalLayersArgs A) {
    const uint32_t dim = A.dim;
    const uint64_t i = ((uint64_t)A.first << dim) + (uint64_t)blockIdx.x * kTsBlock + threadIdx.x; // (instance, cell)
    if (i >= ((uint64_t)A.n << dim)) return;
    const uint32_t inst = (uint32_t)(i >> dim), c = (uint32_t)i & ((1u << dim) - 1u);
    uint64_t lane[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) lane[j] = A.cells[ge_lane_index(inst, j, c, dim)];
    fr_store(A.out[inst] + 2 * (size_t)c, wide_fold_cell(lane));
}

hipError_t launch_batch_gkr_eval_cells(GkrEvalLayersArgs args, uint64_t nnz_max, hipStream_t stream) {
    if (args.n == 0 || args.dim == 0 || args.dim > 21 || !args.inst || !args.out || !args.cells || nnz_max >= (1ULL << 31)) return hipErrorInvalidValue;
    const uint64_t B = gkr_bs_term_blocks(nnz_max);
    args.blocks_per_inst = (uint32_t)B;
    // a launch takes as many whole instances as keep both grids below 2^30 blocks
    const uint64_t per_fold = ((1ULL << args.dim) + kTsBlock - 1) / kTsBlock, per_inst = std::max(B, per_fold);
    const uint32_t step = (uint32_t)std::max<uint64_t>(1, (1ULL << 30) / per_inst);
    for (uint64_t first = 0; first < args.n; first += step) {
        const uint64_t count = std::min<uint64_t>(step, args.n - first);
        args.first = (uint32_t)first;
        hipLaunchKernelGGL(k_batch_gkr_eval_terms, dim3((uint32_t)(count * B)), dim3(kTsBlock), 0, stream, args);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    for (uint64_t first = 0; first < args.n; first += step) {
        const uint64_t count = std::min<uint64_t>(step, args.n - first);
        GkrEvalLayersArgs F = args;
        F.first = (uint32_t)first;
        F.n = (uint32_t)(first + count); // (the fold's bound: the launch ends with its last instance)
        hipLaunchKernelGGL(k_batch_gkr_eval_fold, dim3((uint32_t)(((count << args.dim) + kTsBlock - 1) / kTsBlock)), dim3(kTsBlock), 0, stream, F);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace scd
