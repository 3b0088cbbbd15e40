// kernels.h -- host-callable launchers for the gfx950 kernels in kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "batch_shape.hpp"
#include "lag_index.hpp"
#include "lane_sum.hpp"

namespace scd {

// (kMaxFusedM, kMaxSmallTables, kMetaProds, kTsBlock and the batched kernels' shape rule: batch_shape.hpp)
constexpr uint64_t kSmallRoundPairs = 1u << 14; // rounds at or below this many pairs are latency-bound: split finer (bind launch + one lane per
                                                // (combination, pair)).  2^16 until round 4: at 2^16 and 2^15 pairs that pair of launches moves 2.2x
                                                // the bytes of the fused tree kernel (every node's combination re-reads its product's tables) and
                                                // is memory-bound, 95 and 58 us a round; swept again with this round's kernels: 2^14 is the minimum
                                                // (config 3 5.125 -> 5.07 ms same-box, profiles/r4l_small_boundary_sweep.txt)

struct FrHost {
    uint64_t l[4];
};

// Evaluation nodes of a product's round polynomial, in the order the kernels use them: 0, 1, inf, -1, 2, -2, 3, ...
// A product with M multiplicands is evaluated at the first M+1 of them.  "inf" is the leading coefficient
// (the product of the slopes), whose operand -- the slope hi-lo -- is needed anyway; -1 and 2 are one lazy
// add away from the table entries.  k_finalize maps the M+1 sums to the message's points 0..deg with a
// host-computed (deg+1) x (M+1) matrix (exact Lagrange weights), so any node set gives the same canonical bits.
constexpr int32_t kNodeInf = 0x7fffffff;
__host__ __device__ constexpr int32_t node_value(int s) {
    return s == 0 ? 0 : s == 1 ? 1 : s == 2 ? kNodeInf : ((s - 3) % 2 == 0 ? -((s - 3) / 2 + 1) : ((s - 3) / 2 + 2));
}

// The round's challenge, prepared by the host for the bind of the tree kernels (fe_device.hpp: fe_mul_bind): row i holds the nine
// 29-bit limbs of (r * 2^(29 i + 58)) mod p as a plain integer, r the challenge's standard (non-Montgomery) value.
struct BindConst {
    int32_t R[9][9];
};

// One distinct table of a product.  mode 0: `src` already holds this round's table (2*n_pairs entries).
// mode 1: `src` holds the previous round's table (4*n_pairs entries); the kernel binds the previous
// challenge on the fly, writes this round's table (2*n_pairs entries) to `dst`, and sums from registers.
struct Slot {
    const uint4 *src;
    uint4 *dst;
    uint32_t mode;
    uint32_t exp; // multiplicity of the table inside the product (e.g. [1,4,4] -> table 4 has exp 2)
    // Internal table format "F29" (big rounds after the first bind): an element is nine signed 29-bit limbs packed into the same 32
    // bytes as a canonical element (fe_device.hpp, f29_pack.hpp), in a chunk-planar layout, so a bound table is stored after a carry
    // chain instead of a full canonical reduction.  src_f29 == 0: `src` is in the reference layout (canonical 8 x 32-bit).
    // dst_f29 != 0: the bound table is kept (mode 1: stored, mode 3: used) in the internal format.
    uint32_t src_f29;
    uint32_t dst_f29;
};

struct ProdArgs {
    Slot slot[kMaxFusedM];
    int n_slots;
};
constexpr int kMaxWideM = 12; // products of kMaxFusedM + 1 .. kMaxWideM multiplicands: big rounds as a tree of trees (kernels_wide16.hip)
struct WideArgs16 {
    Slot slot[kMaxWideM]; // one slot per FACTOR, every one in mode 0 (the tables are bound before the launch)
    int n_slots;
};

// One launch for a whole round (every product has <= 4 multiplicands): each block walks all the round's products over its
// own share of the pairs, so a round is one kernel with no launch gaps and the multiplier-bound products (M = 3, 4) of
// some blocks overlap the HBM-bound ones (M = 1, 2) of others.  Partials keep the per-product layout k_finalize reads.
constexpr int kMaxRoundProds = 12;
struct TreeProd {
    Slot slot[4];
    uint32_t M;
    // Lagging single-table product (lag_index.hpp; lag_m = 0: an ordinary row).  slot[0].dst is the product's class work area.
    //   round 1: besides its two node partials the block leaves its 2^lag_m class partials there;
    //   rounds 2 .. lag_m (lag_done + 2 = the round): the row binds the class table, lag_done binds so far, and never touches the table itself --
    //   block 0 does the work, the row's other blocks store zero partials.  lag_grid: blocks per row of the round-1 launch.
    uint8_t lag_m, lag_done;
    uint16_t lag_grid;
    uint64_t partial_off; // in field elements, as in FinProd
};
// the round's finalize step inside k_round_tree (kernels.hip): what k_finalize would have been given
struct RoundFin {
    int enabled;
    int D;
    uint64_t w_off[kMaxRoundProds]; // FinProd::w_off of every product
    const uint4 *Wm;
    uint4 *partials2;               // second-level partials: the layout of the partial array with one "block" per group of 32
    uint32_t *counters;             // device, zero at launch: [0] groups completed, [1 + g] blocks of group g arrived
    uint4 *out;                     // the message: device copy, ...
    uint64_t *out_wide;             // ... widened lanes for an all-reduce (sharded proofs), ...
    uint4 *h_out;                   // ... host-mapped copy with its sequence flag
    uint32_t *h_flag;
    uint32_t seq;
};
struct RoundArgs {
    TreeProd prod[kMaxRoundProds];
    int n_prod;
    RoundFin fin;
    // k_round1_tree_split only: this launch fills blocks [part_block0, part_block0 + gridDim.x) of node rows that are part_stride blocks long
    // (a staged sc_prover_init runs round 1 chunk by chunk under the host-to-device copy, one finalize over all of it); 0 / 0: the whole rows
    uint32_t part_stride, part_block0;
    uint32_t binding; // 1: a binding round, whatever its slots' modes (a round whose every table was bound by k_fix_deep just before has mode 0 throughout)
};

// static per-product record for the finalize kernel (device memory)
struct FinProd {
    uint32_t M;           // multiplicands = degree of this product's round polynomial
    uint32_t pad;
    uint64_t partial_off; // offset (in field elements) of this product's partial sums
    uint64_t w_off;       // offset (in field elements) of this product's node->message matrices in d_W:
                          //   [w_off, +D*(M+1))            c_k * W          (partials in the tables' R = 2^256 form)
                          //   [w_off + D*(M+1), +D*(M+1))  c_k * 2^(5(M-1)) * W  (partials from the 2^261-radix kernels, fe_device.hpp)
};

// table pointers passed by value (kernel argument) for the latency-bound small-round kernels
struct TablePtrs {
    const uint4 *src[kMaxSmallTables];
    uint4 *dst[kMaxSmallTables];
    uint8_t src_f29[kMaxSmallTables]; // non-zero: that source table is in the internal F29 format
};
// one (product, evaluation point) combination of the small-round sum kernel (device memory, static per prover)
struct Combo {
    uint32_t t;        // evaluation point
    uint32_t M;        // multiplicands of the product
    uint32_t slot_off; // into slot_table / slot_exp
    uint32_t n_slots;
    uint64_t partial_off;
};

// Evaluation at a point (ListOfProductsOfPolynomials::evaluate): every challenge is known up front, so one pass folds up to
// three variables at once -- 8 entries in, 1 out -- and a table moves (1 + 1/8 + ...) x its size instead of 3 x.
constexpr int kFoldMaxLevels = 3;
struct FoldArgs {
    const uint4 *src[kMaxSmallTables];
    uint4 *dst[kMaxSmallTables];
    FrHost r32[kFoldMaxLevels]; // challenges of this pass's variables (LSB first), each times 2^5 (fe_device.hpp radix)
};
// dst[y][i] = fold over `levels` variables of src[y][i << levels ...], i < n_out, y < n_tables (grid.y)
hipError_t launch_fold_multi(const FoldArgs &args, int levels, int n_tables, uint64_t n_out, hipStream_t stream);

struct FinMeta {
    FinProd prod[kMetaProds];
};
// the small-round sum kernel's metadata as a kernel argument when it fits (no dependent global loads before the table loads)
constexpr int kMetaCombos = 24, kMetaSlots = 48;
struct ComboMeta {
    Combo combo[kMetaCombos];
    uint32_t slot_table[kMetaSlots];
    uint32_t slot_exp[kMetaSlots];
};

// The persistent tail kernel (kernels.hip: k_tail_rounds): every latency-bound round of a proof in one launch.
#ifndef SC_TAIL_MAX_PAIRS // (A/B builds: tools/build_variant.sh NAME -DSC_TAIL_MAX_PAIRS=8192)
#define SC_TAIL_MAX_PAIRS 2048
#endif
constexpr uint64_t kTailMaxPairs = SC_TAIL_MAX_PAIRS; // rounds above this many pairs are throughput- rather than latency-bound: separate (pipelined) launches
                                                      // with full-chip grids beat a resident grid that pays a barrier per phase (measured: 32 vs 54 us at 4096 pairs)
static_assert(kTailMaxPairs >= kBlock && (kTailMaxPairs & (kTailMaxPairs - 1)) == 0 && kTailMaxPairs <= kSmallRoundPairs, "a power of two within the small rounds");
// (at the default, a combination has at most kTailMaxPairs / kBlock = 8 partial blocks: block 0 adds them up with eight lanes each)
constexpr int kTailMaxGrid = 1024; // at most 4 resident blocks per CU (120 VGPRs), all co-resident on a 256-CU device
constexpr int kTailFlatPairs = 16; // rounds with at most this many pairs run in block 0 alone, one lane per (combination, pair)
// ... and with few combinations (one product of two or three multiplicands: the GKR phases, configs 1 and 2) up to 64 pairs do: as long as
// every (combination, pair) has its own lane of the block and a combination's pairs share a wavefront
__host__ __device__ constexpr uint64_t tail_flat_pairs(int n_combos) {
    uint64_t p = kTailFlatPairs;
    while (p < 64 && 2 * p * (uint64_t)n_combos <= (uint64_t)kBlock) p *= 2;
    return p;
}
struct TailTables {
    const uint4 *cur0[kMaxSmallTables];       // where each table's evaluations are when the tail starts ...
    uint8_t cur0_f29[kMaxSmallTables];        // ... non-zero: in the internal F29 format (straight from the big rounds)
    uint4 *b0[kMaxSmallTables];               // the 1st, 3rd, ... bind of the tail writes here
    uint4 *b1[kMaxSmallTables];               // the 2nd, 4th, ... here
};
struct TailArgs {
    TailTables t;
    int n_tables;
    int n_rounds;         // rounds this launch runs
    int first_has_bind;   // the first of them binds r0 first (0: it is round 1 of the proof)
    uint64_t first_pairs; // pairs of the first of them (<= kSmallRoundPairs)
    FrHost r0;
    int n_combos, K, D;
    const uint4 *Wm;      // node -> message matrices (FinProd::w_off)
    uint4 *partials;
    uint32_t *sync;       // device, zeroed before the launch: [0] barrier generation [2] challenges released [3] stop [16 + b] arrival flag of block b
    uint4 *sums;          // device, K * D elements: the per-combination sums of a round with many partial blocks
    uint64_t *chal;       // device, 2 x 4 limbs: the challenge of tail round j in slot j & 1
    uint4 *h_out;         // host-mapped: the round message ...
    uint32_t *h_flag;     // ... and its sequence flag (round j publishes seq0 + j)
    uint32_t seq0;
    uint32_t *sig;        // host-mapped: sig[1] = give-up marker of the device-side poll
    const uint64_t *mail_host; // host-mapped, 2 slots x 8 words: the challenge of tail round j, 32-bit limb i as (limb << 32 | sig0 + j) in
                               // word i of slot (sig0 + j) & 1 -- the tag makes every word self-validating, one poll fetches the challenge
    uint32_t sig0;
    uint32_t max_spins;
};
// The same rounds with the tables resident in LDS (kernels_tail.hip: k_tail_slices): block g of B owns a contiguous range of every
// table for the whole launch; one hand-over per round (its sums -> block 0) as self-validating words in `xw`.
constexpr int kTsMaxBlocks = 256;
// (bt_lanes, the lanes per (product, node) combination of the LDS-resident round body: batch_shape.hpp)
// (kLazySumMaxP and lazy_sum_needs_reduce, the rule of every lazy sum: lane_sum.hpp)
// A line through two lazy entries leaves the entries' range: entries in (-(w - 1) p, p) put node x > 0 (x - 1 slopes beyond hi) and node -x
// (x slopes beyond lo) within (n w - 1) p, n = ceil(D / 2) for a list of degree D.  A product is the chain prod = fe_mul(line, prod), and a
// factor of magnitude L p scales the running product by L / 70.66 (2^261 = 70.66 p) and adds up to p: while L <= 69 the product stays below
// 69 p -- inside fe_mul's second operand, |limb 8| <= 2^29 + 16 --, beyond 70.66 it GROWS with every factor (twelve factors at 89 p: 1100 p,
// outside int32).  n w <= 70 holds by itself for every tail of products of up to kMaxFusedM multiplicands (n <= 4, w <= 17: DESIGN 4.6);
// k_tail_slices<kMaxWideM> (n = 5, 6) stores a bind's results canonical where it would not: w starts again at tail_worst_p(0).
constexpr uint32_t kLineReachMaxP = 70;
__host__ __device__ constexpr uint32_t line_reach_n(int D) { return ((uint32_t)D + 1) / 2; }
__host__ __device__ constexpr bool line_needs_canonical(uint32_t n, uint32_t w) { return n * w > kLineReachMaxP; }
constexpr uint64_t kTsMaxPairs = 1u << 16; // it takes over from the first latency-bound round (kSmallRoundPairs) where the slices fit LDS, and up to two
                                           // rounds earlier for shapes with few multiplications per pair (tail_slices_blocks)
// hand-over area (64-bit words): a ring of four accumulator sets (8 groups x kMetaCombos x 8 words) | the last entries of merging blocks
// ([table][block][9 limbs + a filler]) | the challenge as block 0 passes it on
constexpr size_t kTsAccWords = 4 * 8 * (size_t)kMetaCombos * 8;
constexpr size_t kTsXwWords = kTsAccWords + (size_t)kTsMaxBlocks * kMaxSmallTables * 10 + 8;
struct TailSlicesArgs {
    TailArgs base;        // the rounds, tables, finalize data and host mailbox, as k_tail_rounds takes them (sync[3] = the stop word)
    int B;                // blocks: a power of two <= kTsMaxBlocks (tail_slices_blocks)
    uint64_t *xw;         // device, kTsXwWords words, owned by the handle; zero when allocated, its first kTsAccWords zeroed before every launch
    const uint64_t *mail_vram; // non-null: the challenge mailbox in device memory (the host stores into it over the BAR); EVERY block polls it
    uint32_t tag0;        // tag of this launch's first round; >= 1 and above every tag an earlier launch of the handle used
    uint32_t fin_bytes;   // (filled in by the launcher: LDS layout)
    uint32_t lds_entries;
    uint32_t stage_off;
    uint32_t worst_p;     // a bound on one product's magnitude in this launch's first round, in units of p (tail_worst_p); round j: + j
};
// blocks for a tail that starts with `first_pairs` pairs, or 0 when the slices do not fit LDS (the caller then takes k_tail_rounds)
// max_blocks: how many blocks of the kernel the DEVICE holds at once (tail_slices_max_blocks): the blocks wait for each other, so a grid that is
// not co-resident (a CPX / DPX partition, masked CUs) would stall until its waits expire -- fewer, larger slices then, or 0 if those do not fit
// worst_p: tail_worst_p of the tables the tail starts from -- a lane adds up to 32 products (33 terms with its reduced sum) between two
// reductions, which has to stay inside kLazySumMaxP too
int tail_slices_blocks(uint64_t first_pairs, int n_tables, int K, int D, int n_combos, int max_multiplicands, int max_blocks, uint32_t worst_p);
// The magnitude, in units of p, that the LDS-resident tail counts for one product of its first round.  Tables in the internal format have
// been bound `lazy_binds` times with fe_mul_bind, never reduced: fe_mul_bind's term lies in (-p - 2^230, 2^230), so an
// entry lies in (-(lazy_binds + 1) p, p) -- the packed format's range rule (f29_pack.hpp) keeps it in a subset of that, about
// (-p / 2, p), and this bound is left as it was; canonical tables bound on the way in: (-p, p).
constexpr uint32_t tail_worst_p(uint32_t lazy_binds) { return lazy_binds + 2; }
int tail_slices_max_blocks(int device, int max_multiplicands); // occupancy of k_tail_slices<.> at its LDS limit x the device's CUs (0: unknown)
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, DEVICE): thread ranks of one process drive several GPUs
hipError_t ensure_dynamic_lds(const void *kernel, int bytes, bool (&done)[64]);
hipError_t launch_tail_slices(TailSlicesArgs args, const ComboMeta &meta, const FinMeta &fin, int max_multiplicands, hipStream_t stream);
// Batched proving (kernels_batch.hip: k_batch_proofs): n independent small instances of one structure, ONE block per instance from round 1
// on -- k_tail_slices' last phase ("one block finishes the proof alone, out of LDS") for the whole proof.  Persistent blocks take instance
// numbers from a ticket; a block waits for the host only, never for another block, so the grid may exceed what is resident.
struct BatchArgs {
    const uint4 *const *tables; // device: [n][n_tables] pointers to the instances' tables (reference layout, 2^nv entries, only read)
    const uint4 *Wm;            // device: n x w_stride elements, instance i's node -> message matrices with its c_k folded in (FinProd::w_off inside)
    uint32_t w_stride;
    uint32_t n, n_tables, nv;
    int n_combos, K, D;
    uint32_t *ticket;           // device, zero at launch: the next instance number
    uint64_t *h_msg;            // host-mapped, [n][D * 8] words: 32-bit limb | tag << 32 -- round j of an instance publishes its message under tag0 + j
    const uint64_t *mail;       // [n][2][8] words: limb << 32 | tag -- the challenge behind message j under tag0 + j in slot j & 1 (tail_post_challenge's form)
    uint32_t mail_local;        // 1: `mail` is device memory the host stores into over the BAR (a poll is local); 0: host-mapped
    uint32_t *h_giveup;         // host-mapped, [n]: the tag an instance's block waited for in vain (it then takes the next ticket)
    uint32_t tag0;              // a multiple of 64 >= 64, above every tag an earlier launch over the same pages used
    uint32_t max_spins;
    uint32_t fin_bytes;         // (filled in by the launcher: LDS layout -- finalize scratch | message | tables)
};
// (the envelope, one block's LDS and products of <= kMaxFusedM: batch_shape_fits, batch_shape.hpp)
int batch_blocks_per_cu(int device, uint32_t nv, uint32_t n_tables, int K, int D);             // occupancy of k_batch_proofs at that LDS size (0: unknown)
hipError_t launch_batch_proofs(BatchArgs args, const ComboMeta &meta, const FinMeta &fin, int grid, hipStream_t stream);
// Batched GKR round proofs (kernels_batch_gkr.hip: k_batch_gkr): n independent instances of GKRRoundSumcheck::prove of one dim, ONE block per
// instance: both initialisations into LDS (wide integer cells, LDS atomics), then 2 x dim rounds of k_batch_proofs' round body
// (batch_round.hpp) over one product of two tables.  The envelope, dim <= kGkrBatchMaxDim and nnz <= kGkrBatchMaxNnzPerCell x 2^dim per
// instance: gkr_batch_shape_fits, batch_shape.hpp.
struct GkrBatchInst { // device memory, one per instance; every pointer is device memory that is only read
    const uint64_t *idx; // nnz indices (z, x, y): z in the low dim bits
    const uint4 *vals;   // nnz values
    const uint4 *f2, *f3; // 2^dim entries each
    const uint4 *g;      // dim elements
    uint64_t nnz;
};
struct BatchGkrArgs {
    const GkrBatchInst *inst;
    const uint4 *Wm;            // device: the node -> message matrices of one product of two tables with a coefficient of one (both copies)
    uint32_t n, dim;
    uint32_t *ticket;           // the rest as in BatchArgs; an instance publishes 2 x dim messages under tag0 .. tag0 + 2 dim - 1, and the
    uint64_t *h_msg;            // challenge behind EVERY message but the last is fetched (the block needs u_{dim-1} to build phase two)
    const uint64_t *mail;
    uint32_t mail_local;
    uint32_t *h_giveup;
    uint32_t tag0;
    uint32_t max_spins;
    uint32_t fin_bytes;         // (filled in by the launcher)
};
int gkr_batch_blocks_per_cu(int device, uint32_t dim); // occupancy of k_batch_gkr at that LDS size (0: unknown)
hipError_t launch_batch_gkr_idx_range(const GkrBatchInst *inst, uint32_t n, uint32_t dim, uint32_t *flags, hipStream_t stream); // flags[i] |= 1: an index of instance i has a bit at or above 3 dim
hipError_t launch_batch_gkr(BatchGkrArgs args, const ComboMeta &meta, const FinMeta &fin, int grid, hipStream_t stream);
// Batched oracle queries (kernels_batch_eval.hip): what a caller of the two batched provers asks for at the point a proof ended on.  Plain
// launches: nothing here waits for the host.
//   k_batch_eval      one block per table: the first three variables bound on the fly from global memory (k_fold_multi's pass), the rest
//                     in LDS (bt_bind's pass); block b = group x group_size + member reads tables[b] and the nv-element point at element
//                     group x pt_stride + pt_base + member x pt_step of `points`, and writes out[group x out_stride + out_base + member].
//                     sc_poly_evaluate_batch: a group is an instance's U tables at the instance's point (pt_stride = nv, pt_step = 0);
//                     sc_gkr_subclaim_batch: a group is (f2, f3) of an instance at (u, v) of its g | u | v record.
//   k_batch_gkr_eval  one block per instance: eq(g, .), eq(u, .), eq(v, .) in LDS, three products per non-zero, exact integer lanes;
//                     GkrBatchInst::g is the instance's g | u | v (3 x dim elements), f2 / f3 are not read; writes out[instance x out_stride].
constexpr uint32_t kEvalBatchMaxNv = 14; // 2^11 entries of 48 B in LDS behind the first pass
struct EvalBatchArgs {
    const uint4 *const *tables; // device: [blocks] pointers, 2^nv entries each, only read
    const uint4 *points;        // device: canonical Montgomery elements
    uint4 *out;                 // device
    uint32_t nv, group_size, pt_stride, pt_base, pt_step, out_stride, out_base;
};
bool eval_batch_shape_fits(uint32_t nv);
hipError_t launch_batch_eval(const EvalBatchArgs &args, uint32_t blocks, hipStream_t stream);
bool gkr_eval_batch_shape_fits(uint32_t dim, uint64_t nnz_max); // sc_gkr_prove_batch's envelope: dim <= kGkrBatchMaxDim, nnz <= kGkrBatchMaxNnzPerCell x 2^dim
hipError_t launch_batch_gkr_eval(const GkrBatchInst *inst, uint32_t n, uint32_t dim, uint4 *out, uint32_t out_stride, hipStream_t stream);
// Batched interactive rounds (kernels_batch_rounds.hip): sc_batch_prove_round.  ONE plain launch per round for the whole batch, one block
// per instance, k_batch_proofs' round body (batch_round.hpp) between a load from and a store to a device work area -- every challenge is
// known before the launch, so nothing here waits for the host or for another block.  The work area holds every instance's tables as
// 48-byte LDS slots (kBtEnt words, copied verbatim: every magnitude is k_batch_proofs'), table u of instance i at slot
// (i * n_tables + u) * 2 * 2^nv, and inside that region the table bound b times at batch_rounds_off(nv, b): the round-0 tables are never
// overwritten (a reset to the same tables rewinds a counter), and a round never writes what it reads.
// (kBatchRoundSlotBytes, batch_rounds_off: batch_shape.hpp)
struct BatchRoundArgs {
    int32_t *work;              // device: n x n_tables x 2 x 2^nv slots of kBtEnt words
    const uint4 *Wm;            // device: n x w_stride elements, as in BatchArgs
    uint32_t w_stride;
    const uint4 *chal;          // device: the challenges behind the previous messages, n elements (ONE when chal_shared); not read in round 0
    uint32_t chal_shared;
    uint4 *out;                 // device: n x D elements, the round's messages
    uint32_t n, n_tables, nv, round; // round: 0-based; round j > 0 binds the tables bound j - 1 times and stores them bound j times
    int n_combos, K, D;
    uint32_t fin_bytes;         // (filled in by the launcher: LDS layout -- finalize scratch | message | tables)
};
hipError_t launch_batch_round(BatchRoundArgs args, const ComboMeta &meta, const FinMeta &fin, hipStream_t stream); // rounds whose tables AS LOADED (nv - max(round - 1, 0) variables) are a shape of batch_shape_fits
// The rounds of the same work area whose tables as loaded do not fit one block (kernels_batch_round_slices.hip; the rule, the slice size and
// the partials' size: batch_slices.hpp): k_batch_round_slices, n << slices_log2 blocks, each a slice of 2^slice_log2 entries of every table
// of its instance -- load, bind, sums into partials[instance][slice][combination], store --, then k_batch_round_fin, one block per
// instance: the partials' sums, finalize_message, the message.  Two plain launches on one stream; nothing waits, no atomics.
struct BatchRoundSlicesArgs {
    int32_t *work;              // as in BatchRoundArgs
    const uint4 *chal;
    uint32_t chal_shared;
    uint4 *partials;            // device: (n << slices_log2) x n_combos elements, canonical
    uint32_t n_tables, nv, round;
    int n_combos, K;
    uint32_t slice_log2, slices_log2; // log2 E_s, log2 S: E_s << slices_log2 entries per table as loaded
};
struct BatchRoundFinArgs {
    const uint4 *partials;
    const uint4 *Wm;            // as in BatchRoundArgs
    uint32_t w_stride;
    uint4 *out;
    uint32_t slices_log2;
    int n_combos, K, D;
    uint32_t fin_bytes;         // LDS layout: finalize scratch | message
};
// args as for launch_batch_round (fin_bytes is not read); partials: bs_partials_bytes of the handle's shape
hipError_t launch_batch_round_slices(BatchRoundArgs args, uint4 *partials, const ComboMeta &meta, const FinMeta &fin, hipStream_t stream);
// canonical tables (tables[i * n_tables + u]: 2^nv entries, reference layout) -> the work area's round-0 slots
hipError_t launch_batch_rounds_load(const uint4 *const *tables, uint32_t n, uint32_t n_tables, uint32_t nv, int32_t *work, hipStream_t stream);
// instances [first, first + count): the tables bound `bound` times -> canonical elements, out[(i - first) * n_tables + u][entry]; with
// chal (first + count elements, or ONE when chal_shared) every pair of entries is bound once more on the way out (bind_final)
hipError_t launch_batch_rounds_export(const int32_t *work, uint32_t first, uint32_t count, uint32_t n_tables, uint32_t nv, uint32_t bound, const uint4 *chal_or_null,
                                      uint32_t chal_shared, uint4 *out, hipStream_t stream);
// Batched interactive GKR rounds (kernels_batch_gkr_rounds.hip): sc_gkr_batch_prover_*.  The two initialisations of GKRRoundSumcheck::prove
// as plain launches, one block per instance, that WRITE k_batch_round's work areas (U = 2) instead of staying inside a persistent block:
//   k_batch_gkr_phase<1>  eq(g, .), h_g through bg_accumulate<1>'s cells -> area A, table 0, depth 0; f2 -> area A, table 1, depth 0;
//   k_batch_gkr_phase<2>  the two entries left of area A's table 1 (depth dim - 1) bound with u_{dim-1}: f2(u), canonical, kept in f2u[i];
//                         eq(g, .), eq(u, .), f1(g, u, .) through bg_accumulate<2> -> area B, table 0; f3 * f2(u) -> area B, table 1.
// Dynamic LDS: eq(g, .) | eq(u, .) | the cells, 128 B x 2^dim (64 KB at dim 9); no tables.  The envelope is gkr_batch_shape_fits'.
struct BatchGkrPhaseArgs {
    const GkrBatchInst *inst;   // device, n records
    int32_t *work_a, *work_b;   // device: n x 2 x 2 x 2^dim slots each (phase 1 writes A; phase 2 reads A and writes B)
    const uint4 *u;             // device: the challenges the handle has received, [challenge j][instance] elements (phase 2 reads j < dim)
    uint4 *f2u;                 // device: n elements (phase 2 writes)
    uint32_t n, dim;
    const uint4 *g2, *coef;     // two-point form only (points = 2): device, n x dim elements g2 and n x 2 elements (alpha, beta), instance-major
};
// points 1: eq(g, .) as above.  points 2 (sc_gkr_two_point_*): E = alpha eq(g, .) + beta eq(g2, .) stands where eq(g, .) stands -- eq(g2, .)
// is built in eq(u, .)'s region (free in phase 1, rebuilt afterwards in phase 2) and folded into eq(g, .) in one pass: no LDS beyond 128 B x 2^dim.
hipError_t launch_batch_gkr_phase(int phase, const BatchGkrPhaseArgs &args, hipStream_t stream, int points = 1);
// out[e] = alpha a[e] + beta b[e], e < count, canonical elements; coef: device, (alpha, beta).  The serial plan's two-point tables: by
// linearity the dense table of E is this combination of the dense tables of g and of g2 (any dim).  out may be a or b.
hipError_t launch_gkr_two_point_combine(const uint4 *a, const uint4 *b, const uint4 *coef, uint4 *out, uint64_t count, hipStream_t stream);
// sc_gkr_layer_next_batch: the arrays a handle takes from the caller's device memory, all in ONE launch (k_batch_gkr_restage) out of a
// device table of items.  An item is spread over ceil(bytes / kGkrRestageChunk) blocks, the first of them first_block: the items' first
// blocks ascend from 0 and `blocks` is their total.  Sizes are multiples of 8; 16 bytes per lane where an item's source and destination are
// both 16-byte aligned, 8 otherwise.  The caller answers for the destinations: inside its allocation, disjoint, no source among them.
constexpr uint64_t kGkrRestageChunk = 16384; // bytes a block moves: four 16-byte accesses per lane
struct GkrRestageItem {
    const void *src;      // device memory, 8-byte aligned
    uint64_t dst_off;     // bytes from dst_base, a multiple of 8
    uint64_t bytes;       // a multiple of 8, not 0
    uint64_t first_block;
};
hipError_t launch_batch_gkr_restage(const GkrRestageItem *items, uint32_t n_items, uint64_t blocks, char *dst_base, hipStream_t stream);
// The same two initialisations beyond one block's LDS (kernels_batch_gkr_round_slices.hip; the envelope and the grids: batch_slices.hpp,
// gkr_bs_plan), dim 10 .. 16, as two plain launches each over wide cells in DEVICE memory (n x 8 uint64 lanes x 2^dim, zeroed by the caller
// on the same stream in front of every phase):
//   k_batch_gkr_terms<kPhase>  n x blocks_per_inst blocks; a block builds eq(g, .) (phase 2: and eq(u, .)) as two half tables in LDS, strides
//                              over its share of the instance's non-zeros and adds every term's eight limbs into the cell's lanes with
//                              relaxed agent-scope atomics: integer sums, exact in any order;
//   k_batch_gkr_fold<kPhase>   one lane per cell: wide_fold_cell -> table 0, depth 0 of area A (phase 1) or B (phase 2); table 1 gets f2,
//                              or f3 * f2(u) with f2(u) bound out of area A as k_batch_gkr_phase<2> binds it (kept in f2u[i]).
struct BatchGkrSlicesArgs {
    const GkrBatchInst *inst;   // device, n records
    int32_t *work_a, *work_b;   // as in BatchGkrPhaseArgs
    const uint4 *u;             // as in BatchGkrPhaseArgs
    uint4 *f2u;                 // device: n elements (phase 2 writes)
    uint64_t *cells;            // device: n x 8 x 2^dim lanes, zero on entry
    uint32_t n, dim;
    uint32_t blocks_per_inst;   // (filled in by the launcher from nnz_max: gkr_bs_term_blocks)
    const uint4 *g2, *coef;     // two-point form only (points = 2): as in BatchGkrPhaseArgs
};
// points 2: a second pair of half tables for g2, alpha folded into g's low half and beta into g2's; a term's weight is
// lo[z_lo] hi[z_hi] + lo2[z_lo] hi2[z_hi], canonical -- the number of terms per cell and with it the lanes' bound are those of points 1.
hipError_t launch_batch_gkr_slices_phase(int phase, BatchGkrSlicesArgs args, uint64_t nnz_max, hipStream_t stream, int points = 1);
// The gate form of the batched interactive GKR rounds (kernels_batch_gkr_gates.hip: sc_gkr_gates_*): a layer of multiplication AND addition
// gates, W_out[z] = sum_MUL v f2[x] f3[y] + sum_ADD v (f2[x] + f3[y]).  Both phases are a sumcheck over three tables and two products,
// t0 t1 + t2 (coefficients one, D = 3), in k_batch_round's work areas with U = 3:
//   k_batch_gkr_gates_phase<1>  E (eq(g, .), or alpha eq(g, .) + beta eq(g2, .)); area A: t0 = f2, t1 = H1, t2 = H2 with
//                               H1[x] = sum_MUL E[z] v f3[y] + sum_ADD E[z] v,  H2[x] = sum_ADD E[z] v f3[y];
//   k_batch_gkr_gates_phase<2>  f2(u) out of area A's t0 as k_batch_gkr_phase<2> binds it (kept in f2u[i]); area B: t0 = f3, t1 = T1, t2 = T2 with
//                               T1[y] = f2(u) sum_MUL E[z] eq(u,x) v + sum_ADD E[z] eq(u,x) v,  T2[y] = f2(u) sum_ADD E[z] eq(u,x) v.
// One block per instance, two passes over ONE array of cells (128 B x 2^dim of LDS, as k_batch_gkr_phase); dim <= kGkrBatchMaxDim and each
// list <= kGkrBatchMaxNnzPerCell x 2^dim, so a cell's 64-bit lane takes at most 2^16 terms of 32-bit limbs.
struct GkrGatesInst { // device memory, one per instance; every pointer is device memory that is only read
    const uint64_t *mul_idx, *add_idx; // indices (z, x, y) of the two lists: z in the low dim bits
    const uint4 *mul_vals, *add_vals;
    const uint4 *f2, *f3; // 2^dim entries each
    const uint4 *g;       // dim elements
    uint64_t mul_nnz, add_nnz;
};
struct BatchGkrGatesArgs {
    const GkrGatesInst *inst;   // device, n records
    int32_t *work_a, *work_b;   // device: n x 3 x 2 x 2^dim slots each (phase 1 writes A; phase 2 reads A and writes B)
    const uint4 *u;             // as in BatchGkrPhaseArgs
    uint4 *f2u;                 // device: n elements (phase 2 writes)
    uint32_t n, dim;
    const uint4 *g2, *coef;     // points = 2 only: as in BatchGkrPhaseArgs
};
hipError_t launch_batch_gkr_gates_phase(int phase, const BatchGkrGatesArgs &args, hipStream_t stream, int points);
// The values of GKR circuit layers (kernels_batch_gkr_eval_layers.hip: sc_gkr_layers_eval_batch): per instance i and layer k
//     W_k[z] = sum over the non-zeros (z | x << dim | y << 2 dim, v) of layer k's list of  v * A[x] * B[y],
// with (A, B) = (f2, f3) of the record for layer 0 and (W_{k-1}, W_{k-1}) for every later layer.  inst: n_layers x n records, layer-major
// (GkrBatchInst::g is not read); out: n_layers x n tables of 2^dim canonical elements, disjoint from each other and from every input.
// The cells are bg_accumulate's and k_batch_gkr_terms': eight uint64 lanes of 32-bit limbs, integer adds, one wide_fold_cell per cell.
//   k_batch_gkr_eval_layers  ONE launch for all layers, one block per instance: the current layer's two input tables (one from layer 1 on)
//                            as canonical 32-byte elements in LDS beside the cells, 128 B x 2^dim; within gkr_batch_shape_fits(dim, the
//                            largest nnz of any layer).  The records of layers k >= 1 need no f2 / f3;
//   k_batch_gkr_eval_terms   per layer n x blocks_per_inst blocks behind a zeroing of the cells (n x 8 x 2^dim lanes in device memory, zeroed
//   k_batch_gkr_eval_fold    by the caller on the same stream), relaxed agent-scope atomic adds; then one lane per (instance, cell).  Any
//                            dim up to 21, nnz < 2^31 per list (a lane stays below 2^63); layer k's records name layer k - 1's outputs
//                            as f2 and f3, the stream's order is the only dependence.
struct GkrEvalLayersArgs {
    const GkrBatchInst *inst;   // device: one-block form n_layers x n records; cells form the n records of ONE layer
    uint4 *const *out;          // device: the output tables, as the records are laid out
    uint64_t *cells;            // cells form: n x 8 x 2^dim lanes, zero on entry
    uint32_t n, dim, n_layers;
    uint32_t first;             // (filled in by the launchers: the first instance of a launch -- a grid holds fewer than 2^31 blocks)
    uint32_t blocks_per_inst;   // (filled in by the cells form's launcher from nnz_max: gkr_bs_term_blocks)
};
hipError_t launch_batch_gkr_eval_layers(GkrEvalLayersArgs args, hipStream_t stream);                 // (the dynamic LDS: 128 B x 2^dim, at most 64 KB)
hipError_t launch_batch_gkr_eval_cells(GkrEvalLayersArgs args, uint64_t nnz_max, hipStream_t stream); // terms + fold of one layer
// ... with an ADD list beside every MUL list (kernels_batch_gkr_gates.hip: sc_gkr_gates_layers_eval_batch): W_out[z] = sum_MUL v A[x] B[y] +
// sum_ADD v (A[x] + B[y]), both lists into the same cells.  base.inst: the MUL records (with the tables f2 / f3), add: the ADD records in
// the same order (idx, vals and nnz are read); mul_nnz + add_nnz < 2^31 per (layer, instance).  The one-block form is ONE launch for all
// layers; the cells form is two terms launches and a fold per layer behind the caller's zeroing.
struct GkrGatesEvalArgs {
    GkrEvalLayersArgs base;
    const GkrBatchInst *add;
};
hipError_t launch_batch_gkr_gates_eval_layers(GkrGatesEvalArgs args, hipStream_t stream);
hipError_t launch_batch_gkr_gates_eval_cells(GkrGatesEvalArgs args, uint64_t nnz_max, hipStream_t stream); // nnz_max: the layer's longest list of either kind
int tail_max_resident_blocks(int device); // co-resident blocks of the tail kernel (0: unknown -> the tail kernel is not used)
uint32_t wait_spins_default(); // bound of the device-side polls for a challenge (sc_set_policy("wait_spins", n) overrides it: tests)

// ---- library policy: sc_set_policy / sc_get_policy (abi.hip).  Process-wide integers, read where a path is chosen; the shipped library
// reads no environment variable for any of them (the -DSC_EXPERIMENTS build takes their initial values from SC_<KEY> in the environment).
enum PolicyKey {
    kPolPipeline = 0,     // "pipeline"           1: device-side waits allowed (persistent tail kernel, pipelined launches); 0: every round launched after its challenge
    kPolResident,         // "resident"           1: the interactive sc_prove_round may keep a kernel on the GPU between calls
    kPolTailSlices,       // "tail_slices"        1: latency-bound rounds out of LDS (k_tail_slices) where the shape fits; 0: k_tail_rounds / launches
    kPolVramMailbox,      // "vram_mailbox"       1: challenges into device memory over the BAR where the host can store there
    kPolWideTree,         // "wide_tree"          1: products of 5..12 multiplicands as trees (kernels_wide*.hip); 0: node by node
    kPolRcclDirect,       // "rccl_direct"        1: an RCCL round's lanes land in the host-mapped page (if the probe agrees on every rank); 0: publish kernel
    kPolShardGatherLog2,  // "shard_gather_log2"  log2 entries per table and rank region at which a sharded proof gathers (1..15, default 15)
    kPolGkrDirect,        // "gkr_direct"         1: sc_gkr_prove initialises through the bucketed kernels; 0: sort + merge (the list form)
    kPolWaitSpins,        // "wait_spins"         bound of a device-side wait for a challenge, in polls (default 2^22)
    kPolTail,             // "tail"               1: the persistent tail kernels; 0: latency-bound rounds as pipelined launches (what sharded RCCL rounds use)
    kPolStagedInit,       // "staged_init"        1: sc_prover_init over HOST tables copies them in chunks and computes round 1 under the copy (shapes of the merged big-round kernel, >= 2^18 entries)
    kPolBatch,            // "batch"              sc_ml_prove_batch, sc_gkr_prove_batch: 0 always the serial plan; 1 the batched kernel from the measured crossover on; 2 the batched kernel for every n (tests, A/B runs)
    kPolLagSingle,        // "lag_single"         tables that only single-table products name skip this many big rounds after the first (0: off .. 4): class sums stand in for them (lag_index.hpp)
    kPolBatchSlices,      // "batch_slices"       sc_batch_prover_init, sc_gkr_batch_prover_init (dim 10 .. 16): 1 shapes beyond one block's LDS (to 2^16 entries) run their first rounds sliced over several blocks per instance (batch_slices.hpp); 0 they take the serial plan
    kPolGkrGatesFused,    // "gkr_gates_fused"    sc_gkr_gates_init_batch: 1 shapes of one block per instance run k_batch_gkr_gates_phase (batch.gkr_gates_one_block); 0 every handle is composed of three multiplication-only instances per instance (batch.gkr_gates_composed)
    kPolCount
};
int64_t policy(int key);

// ---- launch-plan counters: sc_plan_stats / sc_plan_name (abi.hip).  One counter per path the host side can choose for a round (or an
// initialisation); bumped where the choice is made.  tests/conftest.py accumulates them over the GPU suite per test and
// tests/test_zz_plan_coverage.py asserts that every plan was reached by a test that also computed the oracle's answer.
enum Plan {
    kPlanBigMergedRound1 = 0, // k_round1_tree_split: all products, one launch, no bind
    kPlanBigMergedBindChain,  // k_round_tree_split<chain>: round 2 (sources canonical)
    kPlanBigMergedBind,       // k_round_tree_split: rounds >= 3 (sources F29 or canonical)
    kPlanBigClaimIdentity,    // ... with node 1 from the claim identity (kSkip1)
    kPlanBigF29Store,         // a big binding round stored its tables in the internal F29 format
    kPlanBigCanonicalStore,   // ... in the reference layout (lists that keep canonical tables)
    kPlanBigPerProductTree,   // k_prod_tree<M <= 4>: one launch per product (more products than a merged launch takes)
    kPlanBigWide,             // k_prod_tree_wide<5..8>
    kPlanBigWide16,           // k_prod_tree_wide16<9..12>
    kPlanBigGeneric,          // k_sum_generic (13 and more, or wide_tree = 0 beyond 8)
    kPlanBigNodeByNode,       // k_prod_round_fe (wide_tree = 0, 5..8)
    kPlanBigBindPass,         // k_fix_multi up front (lists with products beyond kMaxFusedM)
    kPlanBigStreamed,         // rounds 1-2 of a streamed handle, chunk by chunk
    kPlanBigStagedRound1,     // round 1 computed inside sc_prover_init / sc_prover_reset, chunk by chunk under the host-to-device copy
    kPlanBigLagClassRound,    // a merged big round in which a lagging product's row bound its class table instead of the table
    kPlanBigLagCatchUp,       // k_fix_deep in front of the merged round that reads a lagging table again
    kPlanBigLagMaterialize,   // k_fix_deep because something else needed the table (materialize_lagging)
    kPlanFinalizeMultiBlock,  // k_finalize_mb
    kPlanFinalizeOneBlock,    // k_finalize (more products than a launch's arguments describe: metadata from device memory)
    kPlanFinalizeNoLds,       // k_finalize without LDS staging (node sums beyond 48 KB)
    kPlanSmallLaunched,       // k_fix_multi + k_sum_combos_meta after the challenge
    kPlanSmallCombosTable,    // ... k_sum_combos (combination metadata from device memory)
    kPlanSmallPtrs,           // ... k_sum_combos_ptrs (more than 32 tables)
    kPlanSmallPipelined,      // a latency-bound round enqueued behind k_wait_challenge
    kPlanTailSlices8,         // k_tail_slices<8>
    kPlanTailSlices12,        // k_tail_slices<12>
    kPlanTailRounds,          // k_tail_rounds
    kPlanResidentSlices,      // the interactive protocol's resident kernel: k_tail_slices
    kPlanResidentRounds,      // ... k_tail_rounds
    kPlanBatchGkrEvalLayersOneBlock, // sc_gkr_layers_eval_batch: k_batch_gkr_eval_layers, one block per instance, ONE launch for all layers (dim <= 9, every nnz <= 64 x 2^dim, policy "batch" != 0); counted once per successful call
    kPlanBatchGkrEvalLayersCells,    // ... per layer a zeroing of the cells, k_batch_gkr_eval_terms and k_batch_gkr_eval_fold on one stream (every other shape)
    kPlanBatchGkrGatesOneBlock, // a round call on a handle of sc_gkr_gates_init_batch: k_batch_round (three tables, two products) over the work areas k_batch_gkr_gates_phase<1|2> fill (dim <= 9, each list <= 64 x 2^dim, policy "batch" != 0, policy "gkr_gates_fused" = 1); counted once per round call
    kPlanBatchGkrGatesComposed, // ... an inner sc_gkr_batch_prover of 3 n multiplication-only instances (MUL, f2, f3), (ADD, f2, 1), (ADD, 1, f3) on a plan of its own, their messages added on the host (every other shape, or "gkr_gates_fused" = 0); counted once per round call
    kPlanBatchGkrGatesEvalOneBlock, // sc_gkr_gates_layers_eval_batch: k_batch_gkr_gates_eval_layers, one block per instance, ONE launch for all layers (dim <= 9, every list of either kind <= 64 x 2^dim, policy "batch" != 0); counted once per successful call
    kPlanBatchGkrGatesEvalCells,    // ... per layer a zeroing of the cells, k_batch_gkr_gates_eval_terms over the MUL and over the ADD lists, k_batch_gkr_gates_eval_fold on one stream (every other shape)
    kPlanShardedRcclDirect,   // sharded rounds: ncclAllReduce into the host-mapped page
    kPlanShardedRcclPublish,  // ... all-reduce + publish kernel
    kPlanShardedHost,         // ... the caller's host transport
    kPlanShardedP2P,          // ... k_p2p_allreduce
    kPlanBatchGkrTwoPoint,    // sc_gkr_two_point_init_batch / sc_gkr_two_point_next_batch: a GKR batch handle in two-point form (alpha eq(g, .) + beta eq(g2, .) where eq(g, .) stands), on any plan; counted once per successful call
    kPlanShardedGatherTail,   // bind + all-gather + replicated tail
    kPlanBatchRoundsSlices,   // sc_batch_prove_round: k_batch_round_slices + k_batch_round_fin, several blocks per instance, two launches for a round of the whole batch (the rounds whose tables do not fit one block; policy "batch_slices" = 1)
    kPlanGkrBucketedGrouped,  // GKR initialisation: buckets of an index-ordered list (k_bucket_bounds)
    kPlanBatchGkrNextLayer,   // sc_gkr_layer_next_batch on a handle with work areas (batch.gkr_rounds_one_block / _slices): new inputs into the handle's own copy (k_batch_gkr_restage for device arrays) and phase one's tables rebuilt, nothing allocated; counted once per successful call
    kPlanGkrBucketedCounted,  // ... counting sort into buckets
    kPlanBatchGkrRoundsSlices, // sc_gkr_batch_prove_round on a handle of dim 10 .. 16 built with policy "batch_slices" = 1: areas filled by k_batch_gkr_terms / k_batch_gkr_fold, the rounds k_batch_round_slices + k_batch_round_fin while the tables do not fit one block, then k_batch_round; counted once per round call
    kPlanGkrListForm,         // ... sort + merge + scatter
    kPlanGkrEqDirect,         // ... the list form's fold with eq evaluated per entry (k_sparse_scale_direct: 2^k > 8 n + 1024, no eq table)
    kPlanGkrCoeffFromBound,   // phase two's coefficient f2(u) from phase one's bound table
    kPlanBatchGkrRoundsOneBlock, // sc_gkr_batch_prove_round: k_batch_round over the work areas k_batch_gkr_phase<1|2> fill, one launch per round for the whole batch
    kPlanBatchGkrRoundsSerial, // ... a loop of sc_prove_round over n ordinary provers per phase inside the handle (dim or nnz beyond the envelope, policy "batch" = 0)
    kPlanGkrSharded,          // sc_gkr_prove_sharded
    kPlanBatchRoundsOneBlock, // sc_batch_prove_round: k_batch_round, one block per instance, one launch per round for the whole batch
    kPlanBatchRoundsSerial,   // ... a loop of sc_prove_round over n handles inside the batch handle (shapes beyond the envelope, policy "batch" = 0)
    kPlanFoldMulti,           // sc_poly_evaluate / sc_fix_variables (k_fold_multi)
    kPlanBatchEvalOneBlock,   // sc_poly_evaluate_batch: k_batch_eval, one block per (instance, table), one launch for the whole batch
    kPlanBatchEvalSerial,     // ... instance after instance through sc_poly_evaluate (num_vars beyond the envelope, policy "batch" = 0, work areas taken)
    kPlanBatchGkrEvalOneBlock, // sc_gkr_subclaim_batch: k_batch_gkr_eval (one block per instance) and k_batch_eval over (f2, f3)
    kPlanBatchGkrEvalSerial,  // ... instance after instance through sc_sparse_evaluate and sc_poly_evaluate (dim or nnz beyond the envelope, policy "batch" = 0)
    kPlanBatchOneBlock,       // sc_ml_prove_batch: k_batch_proofs, one block per instance, every round out of LDS
    kPlanBatchSerial,         // ... instance after instance on the kept prover (shapes beyond the envelope, small n, slot busy, device-side waits off)
    kPlanBatchGkrOneBlock,    // sc_gkr_prove_batch: k_batch_gkr, one block per instance, both initialisations and 2 x dim rounds out of LDS
    kPlanBatchGkrSerial,      // ... instance after instance through sc_gkr_prove (dim or nnz beyond the envelope, small n, slot busy, device-side waits off)
    kPlanCount
};
void plan_hit(int plan);
hipError_t launch_scale_w_by_table_eval(FrHost *W, const FrHost *W0, uint32_t n, const void *table, const FrHost &r, hipStream_t stream); // W = W0 * table(r)
hipError_t launch_zero_words(uint32_t *p, uint32_t n, hipStream_t stream, uint32_t *p2 = nullptr, uint32_t n2 = 0); // (a plain kernel: hipMemsetAsync may take runtime paths that wait on other streams)
hipError_t launch_tail_rounds(const TailArgs &args, const ComboMeta &meta, const FinMeta &fin, int grid, hipStream_t stream);

int grid_for_pairs(uint64_t n_pairs);

// product k of one round: partials[t*grid+blk] = sum over this block's pairs of prod_j line_j(t), t = 0..M (node-major, so the
// finalize kernel reads each node's partials as one contiguous run)
#ifdef SC_EXPERIMENTS // saturated-arithmetic cross-check kernel
hipError_t launch_prod_round(int M, const ProdArgs &args, const FrHost &r, uint64_t n_pairs, FrHost *d_partials, int grid,
                             hipStream_t stream);
#endif
// the same in carry-free 29-bit-limb arithmetic; r32 = challenge * 2^5, partials carry 2^(-5(M-1))
hipError_t launch_prod_round_fe(int M, const ProdArgs &args, const FrHost &r32, uint64_t n_pairs, FrHost *d_partials, int grid,
                                hipStream_t stream);
// production big-round kernel: args list exactly M factors (repeated tables listed repeatedly; modes 0 / 1 / 3), static
// multiplication tree per M; same partial layout and 2^(-5(M-1)) scaling as launch_prod_round_fe
hipError_t launch_prod_tree(int M, const ProdArgs &args, const BindConst &rc, uint64_t n_pairs, FrHost *d_partials, int grid,
                            hipStream_t stream);
// five to eight factors: the halves' product trees, extended to the product's nodes by integer combinations, one product per node
// (kernels_wide.hip); launch_prod_tree forwards to it
hipError_t launch_prod_tree_wide(int M, const ProdArgs &args, const BindConst &rc, uint64_t n_pairs, FrHost *d_partials, int grid, hipStream_t stream);
// nine to kMaxWideM multiplicands over bound tables; comp = 2^(5(M-1)) in Montgomery form: the sums leave in k_sum_generic's form
hipError_t launch_prod_tree_wide16(int M, const WideArgs16 &args, const FrHost &comp, uint64_t n_pairs, FrHost *d_partials, int grid, hipStream_t stream);
// all products of a round in one launch (see RoundArgs); d_partials is the base of the partial-sum array
// one product per block row: grid x n_prod blocks, `grid` partial blocks per product.  (split = false, experiments build only: the
// previous kernels, every block walking all products)
// skip1: node 1 of every product is left out (binding rounds only); the round's finalize launch must then carry ClaimArgs
hipError_t launch_round_tree(const RoundArgs &args, const BindConst &rc, uint64_t n_pairs, FrHost *d_partials, int grid, hipStream_t stream, bool split = true,
                             bool skip1 = false);
#ifdef SC_EXPERIMENTS // tiled variant (LDS-staged, one wavefront per node): grid from grid_for_tiles, same partial layout and scaling as _fe
int grid_for_tiles(uint64_t n_pairs);
hipError_t launch_round_tile(int M, const ProdArgs &args, const FrHost &r32, uint64_t n_pairs, FrHost *d_partials, int grid,
                             hipStream_t stream);
#endif
// generic (any M): tables already bound; slot lists in device memory
hipError_t launch_sum_generic(const uint4 *const *d_cur_tables, const uint32_t *d_slot_table, const uint32_t *d_slot_exp,
                              int n_slots, int M, uint64_t n_pairs, FrHost *d_partials, int grid, hipStream_t stream);
// out[b] = in[2b] + r*(in[2b+1]-in[2b]), b < n_out
hipError_t launch_fix(const uint4 *src, uint4 *dst, const FrHost &r, uint64_t n_out, hipStream_t stream);
// small rounds: bind every table in one launch (grid.y = table) ...
// one-wave kernel that holds the stream until flag_dev[0] == want (host-mapped word; bounded spin -- on giving up it stores want
// to flag_dev[1]), then copies the challenge from the host-mapped mailbox to device memory
hipError_t launch_wait_challenge(uint32_t *flag_dev, uint32_t want, const FrHost *mail_host_dev, FrHost *mail_dev, hipStream_t stream,
                                 uint32_t spins_override = 0);
// r_mail (device-visible, may be host-mapped) overrides r when non-null: the challenge is fetched at run time
hipError_t launch_fix_multi(const TablePtrs &tp, int n_tables, const FrHost &r, const FrHost *r_mail, uint64_t n_out, hipStream_t stream);
// ... and one launch for every (product, evaluation point) combination (grid.y = combination), one lane per pair
hipError_t launch_sum_combos(const TablePtrs &tp, const Combo *d_combos, int n_combos, const uint32_t *d_slot_table,
                             const uint32_t *d_slot_exp, uint64_t n_pairs, FrHost *d_partials, int grid, hipStream_t stream);
// the same with the metadata passed by value (n_combos <= kMetaCombos, slot entries <= kMetaSlots)
// the same for more tables than TablePtrs holds: pointers from a device array (table index -> this round's evaluations)
hipError_t launch_sum_combos_ptrs(const uint4 *const *d_cur_tables, const Combo *d_combos, int n_combos, const uint32_t *d_slot_table,
                                  const uint32_t *d_slot_exp, uint64_t n_pairs, FrHost *d_partials, int grid, hipStream_t stream);
hipError_t launch_sum_combos_meta(const TablePtrs &tp, const ComboMeta &meta, int n_combos, uint64_t n_pairs, FrHost *d_partials, int grid,
                                  hipStream_t stream);
// combine per-block partials of all products into the round polynomial (D evaluations)
// Node 1 from the previous round.  For every product, S(0) + S(1) of a binding round equals the previous round's polynomial of that
// product at the challenge just bound (the verifier's check, product by product), so a big round that follows one whose complete node
// sums are still on the device computes the nodes {0, inf, -1, 2} only: one final Montgomery product less per product and pair.
// The finalize launch gets the previous sums and the weights lam_s(r) of the node basis at the challenge (host, once per round, while
// the round kernel runs) and restores S(1) = sum_s lam_s S_prev(s) - S(0) before the message is formed.  Sums of both rounds carry the
// same 2^(-5(M-1)), so the identity holds between them as stored.
struct ClaimArgs {
    uint32_t skip1;    // 1: the round kernel left node 1 out
    uint32_t pad;
    const uint4 *prev; // the previous round's K * D node sums (the multi-block finalize's `d_scratch` of that round)
    FrHost lam[14];    // lam[claim_off(M) + s], s = 0..M, for M = 1..4
};
__host__ __device__ constexpr int claim_off(int M) { return (M - 1) * (M + 2) / 2; }
// Widened lanes (8 x 64-bit per evaluation: 32-bit limbs zero-extended, summable across ranks) may carry a TAG in their top bits:
// every rank's finalize step ORs wide_tag_of(seq) << kWideTagShift into its lanes, the integer all-reduce adds the tags up, and a word
// whose top bits read nranks * tag is this round's total -- RCCL can then deliver straight into host-mapped memory and the host's
// poll is the fetch (no publish kernel, no flag).  The lanes themselves stay below 2^40 (sums of 32-bit limbs over <= 16 ranks).
constexpr int kWideTagShift = 44;
__host__ __device__ constexpr uint32_t wide_tag_of(uint32_t seq) { return (seq & 0x7fffu) + 1u; } // 1 .. 2^15: nranks * tag < 2^20 for <= 16 ranks
bool finalize_keeps_sums(int K, int D, int nblocks, bool have_host_prods, bool have_counter);
// h_prods_or_null: host copy of the records; with at most kMetaProds products they travel as a kernel argument
hipError_t launch_finalize(const FinProd *d_prods, const FinProd *h_prods_or_null, const FrHost *d_W, int K, int D, int nblocks, const FrHost *d_partials, FrHost *d_scratch,
                           FrHost *d_out, uint64_t *d_out_wide, FrHost *h_out_mapped, uint32_t *h_flag_mapped, uint32_t seq,
                           int scaled /* bit 0: scaled partials; bit 1: tagged lanes */, uint32_t *d_counter_or_null, hipStream_t stream, const ClaimArgs *claim_or_null = nullptr);
// (d_counter_or_null: one zeroed device word owned by the caller selects the multi-block form, which needs d_scratch for K * D sums
// and leaves the word at zero)
hipError_t launch_synth(uint64_t seed, uint64_t stream_id, uint64_t first, uint64_t n, uint4 *d_out, hipStream_t stream);
hipError_t launch_scale(const uint4 *src, uint4 *dst, const FrHost &s, uint64_t n, hipStream_t stream);
hipError_t launch_tag_words(uint64_t *d_words, int n, uint32_t gen, hipStream_t stream); // words |= wide_tag_of(gen) << kWideTagShift
hipError_t launch_publish_words(const uint64_t *d_src, uint64_t *h_dst_mapped, int n, uint32_t *h_flag_mapped, uint32_t seq, hipStream_t stream);
// recv[g][u][e] -> tabs[u][g * per + e] (elements of 32 bytes): the all-gathered remainders of G shards become U tables of G * per entries
// Peer-to-peer all-reduce of a round's lanes (sc_comm_init_p2p): rank r PUSHES its n_words lanes into every peer's inbox (posted
// writes over xGMI, or plain device memory when ranks share a GPU) as self-validating words (generation << 40 | value: the lanes are
// sums of 32-bit limbs, far below 2^40), then polls its OWN inbox -- local memory -- until every source's words carry the generation,
// adds them up, leaves the totals in `lanes` and publishes them to the host-mapped page like k_publish_words.  No collective library,
// no second launch, no flag/data ordering to get wrong: a word that shows the generation IS the data.
// inbox layout (uint64 words): [generation & 1][source rank][kP2PWords].
constexpr int kP2PMaxRanks = 16, kP2PWords = 64;
constexpr size_t kP2PInboxWords = 2 * (size_t)kP2PMaxRanks * kP2PWords;
constexpr uint32_t kP2PRetryBit = 0x80000000u; // h_flag = seq | kP2PRetryBit: a peer had not arrived within max_spins (the host launches the kernel again)
struct P2PArgs {
    uint64_t *inbox[kP2PMaxRanks]; // every rank's inbox, addressable from this device
    int nranks, rank, n_words;
    uint32_t gen;                  // generation of this exchange, 1, 2, ... (24 bits are compared)
    uint32_t max_spins;
};
struct PeerLanes {
    const uint64_t *p[kP2PMaxRanks];
    int n;
};
hipError_t launch_sum_peer_lanes(const PeerLanes &peers, uint64_t n_words, uint64_t *out, hipStream_t stream); // out[i] = sum_q peers.p[q][i]
hipError_t launch_p2p_allreduce(const P2PArgs &args, uint64_t *d_lanes, uint64_t *h_dst_mapped, uint32_t *h_flag_mapped, uint32_t seq, hipStream_t stream);
hipError_t launch_gather_to_tables(const uint4 *recv, uint4 *tabs, uint32_t G, uint32_t U, uint32_t per, hipStream_t stream);
// acc (+)= in (D elements; first: acc = in); last: the sum also goes to d_out / the host-mapped page with its sequence flag (D <= 64)
hipError_t launch_msg_accumulate(const FrHost *in, FrHost *acc, int D, bool first, bool last, FrHost *d_out, uint64_t *d_out_wide, FrHost *h_out_mapped,
                                 uint32_t *h_flag_mapped, uint32_t seq, hipStream_t stream);
// A lagging table's catch-up (kernels_lag.hip: k_fix_deep): the canonical table `src` of n_in entries bound `levels` (1 .. kLagMaxLevels)
// times in one pass, r[0] first, into `dst` (n_in >> levels entries; F29 when dst_f29); every level's result takes the form a big round
// would have stored it in, so `dst` is bit for bit the table `levels` big rounds would have left.  n_in >= 256 entries, a power of two.
struct DeepArgs {
    BindConst r[kLagMaxLevels];
    const uint4 *src;
    uint4 *dst;
    uint64_t n_groups; // n_in / 4
    uint32_t levels;
};
hipError_t launch_fix_deep(const DeepArgs &args, bool dst_f29, hipStream_t stream);
// F29 table -> canonical reference layout (state export)
hipError_t launch_f29_to_sat(const uint4 *src, uint4 *dst, uint64_t n, hipStream_t stream);
hipError_t launch_fr_elementwise(int op, const uint4 *a, const uint4 *b, const FrHost &u, uint4 *out, uint64_t n, hipStream_t stream);
hipError_t launch_bench_modmul(uint64_t n_threads, uint32_t reps, uint32_t variant, uint64_t *d_sink, hipStream_t stream);

} // namespace scd
