// kernels_batch_gkr_rounds.hip -- the two initialisations of many small GKR round proofs as plain launches (k_batch_gkr_phase<1|2>):
// sc_gkr_batch_prover_*, the interactive rounds of GKRRoundSumcheck::prove (reference src/gkr_round_sumcheck/mod.rs:93-139) under the
// caller's transcript.
//
// k_batch_gkr (kernels_batch_gkr.hip) builds both phases' tables inside ONE persistent block that then waits for the host's challenges.
// Here the caller hands in every challenge, so nothing waits: the rounds are k_batch_round's (kernels_batch_rounds.hip, one launch per
// round out of a device work area), and what is left of k_batch_gkr are its two initialisations, one block per instance each, that write
// their tables into a work area as 48-byte slots instead of keeping them in LDS:
//   phase<1>  (once, when the handle is built)  eq(g, .) by bg_build_eq; h_g[x] = sum eq(g,z) * v * f3[y] (mod.rs:30-38) through
//             bg_accumulate<1>'s cells -> area A, table 0, depth 0; f2 -> area A, table 1, depth 0.  Depth 0 is never written again.
//   phase<2>  (in front of round dim's launch)  what is left of area A's table 1 -- two entries at depth dim - 1 -- bound with u_{dim-1},
//             k_batch_rounds_export's arithmetic (entries in (-(dim - 1) p, p), dim <= 9): f2(u), canonical, stored per instance for the
//             caller's subclaim; eq(g, .) and eq(u, .); f1(g, u, .)[y] = sum eq(g,z) * eq(u,x) * v (mod.rs:62) through bg_accumulate<2>
//             -> area B, table 0, depth 0; f3 * f2(u) (fr_mul: mod.rs:71-75, literally) -> area B, table 1, depth 0.
// Every index is masked to dim bits per component before it addresses LDS or f3 (bg_accumulate); an index with a bit at or above 3 dim
// is an argument error that k_batch_gkr_idx_range reports in front of the first launch that follows the indices.
// LDS: eq(g, .) | eq(u, .) (32 B per cell) | the accumulator (64 B per cell, also bg_build_eq's scratch): 128 B x 2^dim; no tables.
// k_batch_gkr_phase<kPhase, 2> is the two-point form (sc_gkr_two_point_*): alpha eq(g, .) + beta eq(g2, .) stands where eq(g, .) stands,
// inside the same LDS; k_gkr_two_point_combine is the serial plan's share of it.
// Behind them k_batch_gkr_restage: the copy kernel that brings the next layer's device arrays into a handle (sc_gkr_layer_next_batch).
#include "batch_round.hpp"

namespace scd {

// kPoints 2 (sc_gkr_two_point_*): eq_g <- alpha eq(g, .) + beta eq(g2, .), canonical (fr_mul, fr_add), with eq(g2, .) built in eq(u, .)'s
// region -- unused in phase 1, rebuilt behind this in phase 2 -- and the cells as bg_build_eq's scratch.  g2 and the coefficients are read
// from the handle's device copies (uniform loads).  Ends behind a barrier.
__device__ __forceinline__ void bg_fold_second_point(uint4 *eq_g, uint4 *eq_g2, uint4 *tmp, const uint4 *g2, const uint4 *coef, const uint32_t dim) {
    bg_build_eq(eq_g2, tmp, g2, dim);
    const Fr alpha = fr_load(coef), beta = fr_load(coef + 2);
    for (uint32_t b = threadIdx.x; b < (1u << dim); b += kTsBlock) fr_store(eq_g + 2 * b, fr_add(fr_mul(alpha, fr_load(eq_g + 2 * b)), fr_mul(beta, fr_load(eq_g2 + 2 * b))));
    __syncthreads();
}

template <int kPhase, int kPoints>
__global__ __launch_bounds__(kTsBlock) void k_batch_gkr_phase(const BatchGkrPhaseArgs A) {
    extern __shared__ uint4 dyn_lds[];
    __shared__ uint4 g_sh[2 * kGkrBatchMaxDim], u_sh[2 * kGkrBatchMaxDim]; // the points g and u
    const uint32_t tid = threadIdx.x, inst = blockIdx.x; // (the grid is exactly n blocks)
    const uint32_t dim = A.dim, cap = 1u << dim;
    uint4 *const eq_g = dyn_lds, *const eq_u = eq_g + 2 * (size_t)cap;
    uint64_t *const cell = reinterpret_cast<uint64_t *>(eq_u + 2 * (size_t)cap);
    const GkrBatchInst I = A.inst[inst];
    const size_t region = (size_t)inst * 2 * 2 * cap * kBtEnt; // the instance's two tables, table u at + u * 2 * cap slots
    int32_t *const dst = (kPhase == 1 ? A.work_a : A.work_b) + region;
    if (tid < 2 * dim) {
        g_sh[tid] = I.g[tid];
        if (kPhase == 2) u_sh[tid] = A.u[2 * ((size_t)(tid >> 1) * A.n + inst) + (tid & 1u)];
    }
    __syncthreads();
    bg_build_eq(eq_g, reinterpret_cast<uint4 *>(cell), g_sh, dim);
    if (kPoints == 2) bg_fold_second_point(eq_g, eq_u, reinterpret_cast<uint4 *>(cell), A.g2 + 2 * (size_t)inst * dim, A.coef + 4 * (size_t)inst, dim);
    if (kPhase == 1) {
        bg_accumulate<1>(cell, I, dim, eq_g, eq_g, [&](const uint32_t c, const Fe &v) { br_slot_store(dst + (size_t)c * kBtEnt, v); });
        for (uint32_t e = tid; e < cap; e += kTsBlock) br_slot_store(dst + ((size_t)2 * cap + e) * kBtEnt, fe_from_fr(fr_load(I.f2 + 2 * (size_t)e)));
    } else {
        // f2(u): every lane binds the same two entries (uniform loads), lane 0 keeps the result
        const int32_t *src = A.work_a + region + ((size_t)2 * cap + batch_rounds_off(dim, dim - 1u)) * kBtEnt;
        const FeU r32 = feu_shl5(fr_load(u_sh + 2 * (dim - 1u)).v);
        const Fe lo = br_slot_load(src), hi = br_slot_load(src + kBtEnt);
        const Fr f2u = fe_to_fr(fe_carry_pass(fe_add(lo, fe_mul_u<true>(fe_sub(hi, lo), r32))));
        if (tid == 0) fr_store(A.f2u + 2 * (size_t)inst, f2u);
        bg_build_eq(eq_u, reinterpret_cast<uint4 *>(cell), u_sh, dim);
        bg_accumulate<2>(cell, I, dim, eq_g, eq_u, [&](const uint32_t c, const Fe &v) { br_slot_store(dst + (size_t)c * kBtEnt, v); });
        for (uint32_t e = tid; e < cap; e += kTsBlock) br_slot_store(dst + ((size_t)2 * cap + e) * kBtEnt, fe_from_fr(fr_mul(fr_load(I.f3 + 2 * (size_t)e), f2u)));
    }
}

hipError_t launch_batch_gkr_phase(int phase, const BatchGkrPhaseArgs &args, hipStream_t stream, int points) {
    if ((phase != 1 && phase != 2) || args.n == 0 || !gkr_batch_shape_fits(args.dim, 0) || !args.inst || !args.work_a) return hipErrorInvalidValue;
    if (phase == 2 && (!args.work_b || !args.u || !args.f2u)) return hipErrorInvalidValue;
    if ((points != 1 && points != 2) || (points == 2 && (!args.g2 || !args.coef))) return hipErrorInvalidValue;
    const size_t lds = (size_t)128 << args.dim; // (at most 64 KB: within a launch's default limit)
    if (points == 1) {
        if (phase == 1) hipLaunchKernelGGL((k_batch_gkr_phase<1, 1>), dim3(args.n), dim3(kTsBlock), lds, stream, args);
        else hipLaunchKernelGGL((k_batch_gkr_phase<2, 1>), dim3(args.n), dim3(kTsBlock), lds, stream, args);
    } else {
        if (phase == 1) hipLaunchKernelGGL((k_batch_gkr_phase<1, 2>), dim3(args.n), dim3(kTsBlock), lds, stream, args);
        else hipLaunchKernelGGL((k_batch_gkr_phase<2, 2>), dim3(args.n), dim3(kTsBlock), lds, stream, args);
    }
    return hipGetLastError();
}

// The serial plan's two-point tables (sc_gkr_two_point_*): out[e] = alpha a[e] + beta b[e] on canonical elements, one lane per element
// with a grid stride; out may be a or b (an element is read before it is written, by the same lane).
__global__ __launch_bounds__(kTsBlock) void k_gkr_two_point_combine(const uint4 *a, const uint4 *b, const uint4 *__restrict__ coef, uint4 *out, const uint64_t count) {
    const Fr alpha = fr_load(coef), beta = fr_load(coef + 2);
    const uint64_t stride = (uint64_t)gridDim.x * kTsBlock;
    for (uint64_t e = (uint64_t)blockIdx.x * kTsBlock + threadIdx.x; e < count; e += stride)
        fr_store(out + 2 * e, fr_add(fr_mul(alpha, fr_load(a + 2 * e)), fr_mul(beta, fr_load(b + 2 * e))));
}

hipError_t launch_gkr_two_point_combine(const uint4 *a, const uint4 *b, const uint4 *coef, uint4 *out, uint64_t count, hipStream_t stream) {
    if (!a || !b || !coef || !out || count == 0) return hipErrorInvalidValue;
    const uint64_t blocks = (count + kTsBlock - 1) / kTsBlock;
    hipLaunchKernelGGL(k_gkr_two_point_combine, dim3((uint32_t)(blocks < 4096 ? blocks : 4096)), dim3(kTsBlock), 0, stream, a, b, coef, out, count);
    return hipGetLastError();
}

// k_batch_gkr_restage (sc_gkr_layer_next_batch): every array a handle has to take from the caller's DEVICE memory, in one launch.  Block b
// serves chunk b - first_block of the last item whose first_block is <= b (a uniform binary search over the table: the items' first blocks
// ascend from 0), kGkrRestageChunk bytes at the most, so a large table is many blocks' work.  Every size is a multiple of 8 and a caller's
// uint64_t * is only 8-byte aligned: an item whose source and destination are both 16-byte aligned moves 16 bytes per lane (a chunk starts
// at a multiple of 16) and its last 8 bytes, where its size is an odd multiple of 8, by one lane; every other item moves 8 bytes per lane.
// Plain loads and stores: no atomics, no waits, no LDS.  The host side lays the destinations out: they do not overlap each other or a source.
__global__ __launch_bounds__(kTsBlock) void k_batch_gkr_restage(const GkrRestageItem *__restrict__ items, const uint32_t n_items, char *__restrict__ dst_base) {
    const uint64_t b = blockIdx.x;
    uint32_t lo = 0, hi = n_items; // items[lo].first_block <= b < items[hi].first_block (hi == n_items: the grid's end)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (items[mid].first_block <= b) lo = mid;
        else hi = mid;
    }
    const GkrRestageItem it = items[lo];
    const uint64_t begin = (b - it.first_block) * kGkrRestageChunk;
    if (begin >= it.bytes) return;
    const uint64_t len = it.bytes - begin < kGkrRestageChunk ? it.bytes - begin : kGkrRestageChunk;
    const char *const src = static_cast<const char *>(it.src) + begin;
    char *const dst = dst_base + it.dst_off + begin;
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0) {
        const uint4 *const s = reinterpret_cast<const uint4 *>(src);
        uint4 *const d = reinterpret_cast<uint4 *>(dst);
        const uint32_t n16 = (uint32_t)(len >> 4);
        for (uint32_t k = threadIdx.x; k < n16; k += kTsBlock) d[k] = s[k];
        if ((len & 8u) && threadIdx.x == 0) *reinterpret_cast<uint64_t *>(dst + ((size_t)n16 << 4)) = *reinterpret_cast<const uint64_t *>(src + ((size_t)n16 << 4));
    } else {
        const uint64_t *const s = reinterpret_cast<const uint64_t *>(src);
        uint64_t *const d = reinterpret_cast<uint64_t *>(dst);
        const uint32_t n8 = (uint32_t)(len >> 3);
        for (uint32_t k = threadIdx.x; k < n8; k += kTsBlock) d[k] = s[k];
    }
}

hipError_t launch_batch_gkr_restage(const GkrRestageItem *items, uint32_t n_items, uint64_t blocks, char *dst_base, hipStream_t stream) {
    if (!items || !dst_base || n_items == 0 || blocks == 0 || blocks >= (1ULL << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_batch_gkr_restage, dim3((uint32_t)blocks), dim3(kTsBlock), 0, stream, items, n_items, dst_base);
    return hipGetLastError();
}

} // namespace scd
