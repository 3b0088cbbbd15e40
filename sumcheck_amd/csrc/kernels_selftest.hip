// kernels_selftest.hip -- sc_debug_fe_op: one lane per element through ONE primitive of the carry-free arithmetic (fe_device.hpp,
// kernel_common.hpp: fe_line, wide_tree.hpp, wide_cell.hpp, batch_round.hpp: bt_combo_sum), on raw limb vectors.  The production kernels
// hand these primitives canonical tables only; the unit tests (tests/test_gpu_fe_primitives.py against tests/fe_model.py) hand them the
// limb and value ranges their call sites can reach.  A debug entry like sc_debug_tail_clocks: exported, not part of the ABI.
//
// All pointers are device memory.  a, b, c, d: n x 9 int32 (an Fr operand: its 8 words in a row's first 8 ints).  aux[0..3]: the op's
// parameters, read by the host.  out: n x 9 int32 (an Fr result: 8 words, the ninth 0).
#include <hip/hip_runtime.h>
#include "batch_round.hpp"
#include "host_fr.hpp"
#include "wide_cell.hpp"
#include "wide_tree.hpp"

void make_bind_const(const sch::Fr &r, scd::BindConst &rc); // protocol.hip

namespace scd {

enum FeOp : int {
    kOpNormalize = 0,    // fe_normalize(a)
    kOpCarryPass = 1,    // fe_carry_pass(a)
    kOpToFr = 2,         // fe_to_fr(a)
    kOpRoundTrip = 3,    // fe_to_fr(fe_from_fr(a))                     a: 8 words
    kOpFromFr = 4,       // fe_from_fr(a)                               a: 8 words
    kOpMul = 5,          // fe_mul<false>(a, b)
    kOpMulChain = 6,     // fe_mul<true>(a, b)
    kOpMulU = 7,         // fe_mul_u<false>(a, u), u = b's row through readlane
    kOpMulUChain = 8,    // fe_mul_u<true>(a, u)
    kOpMul2 = 9,         // fe_mul2_sum<false>(a, b, c, d)
    kOpMul2Chain = 10,   // fe_mul2_sum<true>(a, b, c, d)
    kOpBind = 11,        // fe_mul_bind<false>(a, RT), RT from the challenge aux[0..3] (Montgomery form) by make_bind_const / bind_consts_to_lds
    kOpBindChain = 12,   // fe_mul_bind<true>(a, RT)
    kOpShl5MulU = 13,    // fe_mul_u<true>(a, feu_shl5(b)): the LDS-resident kernels' bind product      b: 8 words, through readlane
    kOpLine = 14,        // fe_line(a, b, nv), nv = (int32) aux[0]
    kOpAccum = 15,       // bt_combo_sum: n lanes in groups of L = aux[1]; a group sums its aux[0] * L products (a: n * aux[0] rows, a group's
                         // products side by side), reduced first by lazy_sum_needs_reduce(aux[0] * L, aux[2]); every lane's accumulator comes back
    kOpFoldCell = 16,    // wide_fold_cell(aux + 4 + 8 i)
    kOpWideValue = 17,   // wide_value<m, t>(v), m = aux[0] (1: the single factor's line as WideNodes takes it), t = aux[1]      a: n x 5 x 9
    kOpWideExt = 18,     // wide_ext<m, t>(v)                                                                                   a: n x 9 x 9
    kOpF29RoundTrip = 19, // fe_load_f29(fe_store_f29(a)): the packed table format (f29_pack.hpp), one launch stores entry i from lane i, a second
                          // loads it back; n a multiple of 128 (the layout's block), b: n x 8 ints of scratch for the table
    kOpF29Settle = 20,    // fe_settle_f29(a): the range rule and the exact digits of a freshly bound entry
};

__device__ __forceinline__ Fe st_load(const int32_t *p, const uint64_t i) {
    Fe r;
#pragma unroll
    for (int l = 0; l < 9; ++l) r.l[l] = p[9 * i + l];
    return r;
}
__device__ __forceinline__ Fr st_load_fr(const int32_t *p, const uint64_t i) {
    Fr r;
#pragma unroll
    for (int l = 0; l < 8; ++l) r.v[l] = (uint32_t)p[9 * i + l];
    return r;
}
__device__ __forceinline__ void st_store(int32_t *p, const uint64_t i, const Fe &v) {
#pragma unroll
    for (int l = 0; l < 9; ++l) p[9 * i + l] = v.l[l];
}
__device__ __forceinline__ void st_store_fr(int32_t *p, const uint64_t i, const Fr &v) {
#pragma unroll
    for (int l = 0; l < 8; ++l) p[9 * i + l] = (int32_t)v.v[l];
    p[9 * i + 8] = 0;
}
__device__ __forceinline__ FeU st_feu_lane(const Fe &b, const int lane) { // a lane's element as a wave-uniform one
    FeU u;
#pragma unroll
    for (int l = 0; l < 9; ++l) u.l[l] = __builtin_amdgcn_readlane(b.l[l], lane);
    return u;
}

template <int kOp>
__global__ __launch_bounds__(kTsBlock) void k_fe_op(const int32_t *__restrict__ a, const int32_t *__restrict__ b, const int32_t *__restrict__ c,
                                                    const int32_t *__restrict__ d, const uint64_t *__restrict__ aux, const BindConst C, const int64_t p0,
                                                    const int64_t p1, const int64_t p2, int32_t *__restrict__ out, const uint64_t n) {
    __shared__ int32_t rt[kBindLds];
    const uint64_t gid = (uint64_t)blockIdx.x * kTsBlock + threadIdx.x;
    const bool live = gid < n;
    const uint64_t i = live ? gid : n - 1; // (every lane runs the primitive: the uniform operand's loop below reads all 64)
    if constexpr (kOp == kOpBind || kOp == kOpBindChain) bind_consts_to_lds(C, rt);
    if constexpr (kOp == kOpNormalize) {
        const Fe r = fe_normalize(st_load(a, i));
        if (live) st_store(out, i, r);
    } else if constexpr (kOp == kOpCarryPass) {
        const Fe r = fe_carry_pass(st_load(a, i));
        if (live) st_store(out, i, r);
    } else if constexpr (kOp == kOpToFr) {
        const Fr r = fe_to_fr(st_load(a, i));
        if (live) st_store_fr(out, i, r);
    } else if constexpr (kOp == kOpRoundTrip) {
        const Fr r = fe_to_fr(fe_from_fr(st_load_fr(a, i)));
        if (live) st_store_fr(out, i, r);
    } else if constexpr (kOp == kOpFromFr) {
        const Fe r = fe_from_fr(st_load_fr(a, i));
        if (live) st_store(out, i, r);
    } else if constexpr (kOp == kOpMul || kOp == kOpMulChain) {
        const Fe r = fe_mul<kOp == kOpMulChain>(st_load(a, i), st_load(b, i));
        if (live) st_store(out, i, r);
    } else if constexpr (kOp == kOpMulU || kOp == kOpMulUChain || kOp == kOpShl5MulU) {
        const Fe x = st_load(a, i);
        Fe y = st_load(b, i), r = fe_zero();
        const int me = threadIdx.x & 63;
#pragma unroll 1
        for (int lane = 0; lane < 64; ++lane) {
            const FeU raw = st_feu_lane(y, lane);
            Fe t;
            if constexpr (kOp == kOpShl5MulU) {
                uint32_t w[8];
#pragma unroll
                for (int l = 0; l < 8; ++l) w[l] = (uint32_t)raw.l[l];
                t = fe_mul_u<true>(x, feu_shl5(w));
            } else {
                t = fe_mul_u<kOp == kOpMulUChain>(x, raw);
            }
            if (lane == me) r = t;
        }
        if (live) st_store(out, i, r);
    } else if constexpr (kOp == kOpMul2 || kOp == kOpMul2Chain) {
        const Fe r = fe_mul2_sum<kOp == kOpMul2Chain>(st_load(a, i), st_load(b, i), st_load(c, i), st_load(d, i));
        if (live) st_store(out, i, r);
    } else if constexpr (kOp == kOpBind || kOp == kOpBindChain) {
        const Fe r = fe_mul_bind<kOp == kOpBindChain>(st_load(a, i), rt);
        if (live) st_store(out, i, r);
    } else if constexpr (kOp == kOpLine) {
        const Fe r = fe_line(st_load(a, i), st_load(b, i), (int32_t)p0);
        if (live) st_store(out, i, r);
    } else if constexpr (kOp == kOpAccum) {
        // (n is a multiple of the block, the block of L: every lane is live)
        const uint32_t per_lane = (uint32_t)p0, L = (uint32_t)p1, pairs = per_lane * L;
        const uint64_t group = gid / L;
        const Fe r = bt_combo_sum(true, (uint32_t)(gid % L), (int)L, pairs, lazy_sum_needs_reduce(pairs, (uint32_t)p2),
                                  [&](const uint32_t pr) -> Fe { return st_load(a, group * pairs + pr); });
        st_store(out, gid, r);
    } else if constexpr (kOp == kOpF29Settle) {
        const Fe r = fe_settle_f29(st_load(a, i));
        if (live) st_store(out, i, r);
    } else if constexpr (kOp == kOpFoldCell) {
        uint64_t lane[8];
#pragma unroll
        for (int l = 0; l < 8; ++l) lane[l] = aux[4 + 8 * i + l];
        const Fr r = wide_fold_cell(lane);
        if (live) st_store_fr(out, i, r);
    }
}

__global__ __launch_bounds__(kTsBlock) void k_f29_store_op(const int32_t *__restrict__ a, uint4 *__restrict__ table, const uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kTsBlock + threadIdx.x;
    if (i < n) fe_store_f29(table, i, st_load(a, i));
}
__global__ __launch_bounds__(kTsBlock) void k_f29_load_op(const uint4 *__restrict__ table, int32_t *__restrict__ out, const uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kTsBlock + threadIdx.x;
    if (i < n) st_store(out, i, fe_load_f29(table, i));
}

template <int m, int t>
__global__ __launch_bounds__(kTsBlock) void k_wide_value_op(const int32_t *__restrict__ a, int32_t *__restrict__ out, const uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kTsBlock + threadIdx.x;
    if (i >= n) return;
    Fe v[5];
#pragma unroll
    for (int s = 0; s < 5; ++s) v[s] = st_load(a, 5 * i + s);
    if constexpr (m == 1) st_store(out, i, fe_comb5(v, 1 - node_value(t), node_value(t), 0, 0, 0)); // (WideNodes: a single factor's line)
    else st_store(out, i, wide_value<m, t>(v));
}
template <int m, int t>
__global__ __launch_bounds__(kTsBlock) void k_wide_ext_op(const int32_t *__restrict__ a, int32_t *__restrict__ out, const uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kTsBlock + threadIdx.x;
    if (i >= n) return;
    Fe v[9];
#pragma unroll
    for (int s = 0; s < 9; ++s) v[s] = st_load(a, 9 * i + s);
    st_store(out, i, wide_ext<m, t>(v));
}

} // namespace scd

// 0: done.  -1: no such op / instantiation.  -2: bad arguments.  > 0: a hipError_t.
extern "C" __attribute__((visibility("default"))) int sc_debug_fe_op(int op, const int32_t *a, const int32_t *b, const int32_t *c, const int32_t *d,
                                                                     const uint64_t *aux, int32_t *out, uint64_t n) {
    using namespace scd;
    if (n == 0 || a == nullptr || out == nullptr || aux == nullptr || n > (1ULL << 24)) return -2;
    uint64_t par[4];
    hipError_t e = hipMemcpy(par, aux, sizeof(par), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return (int)e;
    const dim3 grid((unsigned)((n + kTsBlock - 1) / kTsBlock)), block(kTsBlock);
    BindConst C;
    std::memset(&C, 0, sizeof(C));
    if (op == kOpBind || op == kOpBindChain) {
        const sch::Fr r = {{par[0], par[1], par[2], par[3]}};
        if (sch::geq_p(r)) return -2;
        make_bind_const(r, C);
    }
    if (op == kOpAccum) {
        const uint64_t L = par[1];
        if (par[0] == 0 || par[0] > 64 || L == 0 || L > 64 || (L & (L - 1)) != 0 || n % kTsBlock != 0) return -2;
    }
    if ((op >= kOpMul && op <= kOpMul2Chain) || op == kOpShl5MulU || op == kOpLine || op == kOpF29RoundTrip) {
        if (b == nullptr) return -2;
    }
    if (op == kOpF29RoundTrip && n % 128 != 0) return -2; // whole blocks of the layout: every chunk index stays below n * 2
    if ((op == kOpMul2 || op == kOpMul2Chain) && (c == nullptr || d == nullptr)) return -2;
    const int64_t p0 = (int64_t)par[0], p1 = (int64_t)par[1], p2 = (int64_t)par[2];
#define SC_FE_OP(OP)                                                                                                    \
    case OP:                                                                                                            \
        hipLaunchKernelGGL(k_fe_op<OP>, grid, block, 0, 0, a, b, c, d, aux, C, p0, p1, p2, out, n);                        \
        break;
#define SC_WIDE_OP(KERNEL, M, T)                                                                                        \
    if (p0 == M && p1 == T) {                                                                                           \
        hipLaunchKernelGGL((KERNEL<M, T>), grid, block, 0, 0, a, out, n);                                               \
        found = true;                                                                                                   \
    }
    bool found = false;
    switch (op) {
        SC_FE_OP(kOpNormalize)
        SC_FE_OP(kOpCarryPass)
        SC_FE_OP(kOpToFr)
        SC_FE_OP(kOpRoundTrip)
        SC_FE_OP(kOpFromFr)
        SC_FE_OP(kOpMul)
        SC_FE_OP(kOpMulChain)
        SC_FE_OP(kOpMulU)
        SC_FE_OP(kOpMulUChain)
        SC_FE_OP(kOpMul2)
        SC_FE_OP(kOpMul2Chain)
        SC_FE_OP(kOpBind)
        SC_FE_OP(kOpBindChain)
        SC_FE_OP(kOpShl5MulU)
        SC_FE_OP(kOpLine)
        SC_FE_OP(kOpAccum)
        SC_FE_OP(kOpFoldCell)
        SC_FE_OP(kOpF29Settle)
    case kOpF29RoundTrip: {
        uint4 *table = reinterpret_cast<uint4 *>(const_cast<int32_t *>(b));
        hipLaunchKernelGGL(k_f29_store_op, grid, block, 0, 0, a, table, n);
        hipLaunchKernelGGL(k_f29_load_op, grid, block, 0, 0, table, out, n);
        break;
    }
    case kOpWideValue:
        // every instantiation the product trees of five to eight make (wide_tree.hpp: WideNodes<M, t>): the first half at the nodes beyond
        // its own, the second half (one to four factors) likewise
        SC_WIDE_OP(k_wide_value_op, 4, 5) SC_WIDE_OP(k_wide_value_op, 4, 6) SC_WIDE_OP(k_wide_value_op, 4, 7) SC_WIDE_OP(k_wide_value_op, 4, 8)
        SC_WIDE_OP(k_wide_value_op, 3, 4) SC_WIDE_OP(k_wide_value_op, 3, 5) SC_WIDE_OP(k_wide_value_op, 3, 6) SC_WIDE_OP(k_wide_value_op, 3, 7)
        SC_WIDE_OP(k_wide_value_op, 2, 3) SC_WIDE_OP(k_wide_value_op, 2, 4) SC_WIDE_OP(k_wide_value_op, 2, 5) SC_WIDE_OP(k_wide_value_op, 2, 6)
        SC_WIDE_OP(k_wide_value_op, 1, 3) SC_WIDE_OP(k_wide_value_op, 1, 4) SC_WIDE_OP(k_wide_value_op, 1, 5)
        if (!found) return -1;
        break;
    case kOpWideExt:
        // ... and the trees of nine to twelve (kernels_wide16.hip: Wide16Nodes<M, t>): eight factors at nodes 9 .. 12, M - 8 at the rest
        SC_WIDE_OP(k_wide_ext_op, 8, 9) SC_WIDE_OP(k_wide_ext_op, 8, 10) SC_WIDE_OP(k_wide_ext_op, 8, 11) SC_WIDE_OP(k_wide_ext_op, 8, 12)
        SC_WIDE_OP(k_wide_ext_op, 1, 3) SC_WIDE_OP(k_wide_ext_op, 1, 4) SC_WIDE_OP(k_wide_ext_op, 1, 5) SC_WIDE_OP(k_wide_ext_op, 1, 6)
        SC_WIDE_OP(k_wide_ext_op, 1, 7) SC_WIDE_OP(k_wide_ext_op, 1, 8) SC_WIDE_OP(k_wide_ext_op, 1, 9)
        SC_WIDE_OP(k_wide_ext_op, 2, 3) SC_WIDE_OP(k_wide_ext_op, 2, 4) SC_WIDE_OP(k_wide_ext_op, 2, 5) SC_WIDE_OP(k_wide_ext_op, 2, 6)
        SC_WIDE_OP(k_wide_ext_op, 2, 7) SC_WIDE_OP(k_wide_ext_op, 2, 8) SC_WIDE_OP(k_wide_ext_op, 2, 9) SC_WIDE_OP(k_wide_ext_op, 2, 10)
        SC_WIDE_OP(k_wide_ext_op, 3, 4) SC_WIDE_OP(k_wide_ext_op, 3, 5) SC_WIDE_OP(k_wide_ext_op, 3, 6) SC_WIDE_OP(k_wide_ext_op, 3, 7)
        SC_WIDE_OP(k_wide_ext_op, 3, 8) SC_WIDE_OP(k_wide_ext_op, 3, 9) SC_WIDE_OP(k_wide_ext_op, 3, 10) SC_WIDE_OP(k_wide_ext_op, 3, 11)
        SC_WIDE_OP(k_wide_ext_op, 4, 5) SC_WIDE_OP(k_wide_ext_op, 4, 6) SC_WIDE_OP(k_wide_ext_op, 4, 7) SC_WIDE_OP(k_wide_ext_op, 4, 8)
        SC_WIDE_OP(k_wide_ext_op, 4, 9) SC_WIDE_OP(k_wide_ext_op, 4, 10) SC_WIDE_OP(k_wide_ext_op, 4, 11) SC_WIDE_OP(k_wide_ext_op, 4, 12)
        if (!found) return -1;
        break;
    default:
        return -1;
    }
#undef SC_FE_OP
#undef SC_WIDE_OP
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    return (int)hipDeviceSynchronize();
}

// blocks of a grid-strided launch over n_pairs items as THIS build launches them (the experiments build: capped by SC_GRID), for tests
// that set the iterations a lane makes (tests/test_gpu_big_sum_bounds.py); exported, not part of the ABI
extern "C" __attribute__((visibility("default"))) int sc_debug_grid_for_pairs(uint64_t n_pairs) { return scd::grid_for_pairs(n_pairs); }
