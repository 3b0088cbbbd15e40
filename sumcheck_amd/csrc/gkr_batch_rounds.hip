// gkr_batch_rounds.hip -- sc_gkr_batch_prover_*: n x the two ProverStates of GKRRoundSumcheck::prove (reference
// src/gkr_round_sumcheck/mod.rs:93-139) of one dim behind ONE handle, a round of all n instances per call, under the caller's transcript.
// What batch_rounds.hip is to sc_ml_prove_batch, this is to sc_gkr_prove_batch: the caller hands in every challenge (one per instance, or
// one shared by all), so a round is launched after its challenges are known and nothing on the GPU ever waits for the host.  A proof is
// 2 x dim round calls -- phase one's dim messages, then phase two's -- and sc_gkr_batch_prover_finish.  Three plans, chosen when the handle
// is built (batch_slices.hpp: gkr_bs_plan), same bits:
//   batch.gkr_rounds_one_block  two work areas of k_batch_round's layout (U = 2): A for phase one, B for phase two.  k_batch_gkr_phase<1>
//                               (kernels_batch_gkr_rounds.hip) fills A's depth 0 once, at init -- it is never written again, so a reset
//                               rewinds counters --; round call dim launches k_batch_gkr_phase<2> in front of its k_batch_round, which
//                               binds what is left of f2 with u_{dim-1} and fills B from the challenges the handle has kept on the
//                               device.  Per round call: one upload of the challenges, one launch (call dim: two, back to back), one copy
//                               back, one synchronisation;
//   batch.gkr_rounds_slices     policy "batch_slices" = 1, dim 10 .. 16, nnz <= 64 x 2^dim, at most 16 GiB: the same two work areas and
//                               per-round sequence, but the areas are filled by k_batch_gkr_terms + k_batch_gkr_fold
//                               (kernels_batch_gkr_round_slices.hip: many blocks per instance, wide cells in device memory, zeroed in
//                               front of each phase) and the rounds whose tables as loaded do not fit one block run as
//                               k_batch_round_slices + k_batch_round_fin (dim >= 11: rounds 0 .. dim - 10 of each phase);
//   batch.gkr_rounds_serial     per instance the two dense tables by the route sc_gkr_prove takes (sc_internal_gkr_dense_table) and an
//                               ordinary sc_prover per phase (device-side waits off, no resident kernel); a round is a loop of
//                               sc_prove_round, the phase change and finish go through sc_prover_bind_final: dim > 9 without the key,
//                               dim > 16, nnz beyond 64 x 2^dim, policy "batch" = 0.
// The handle copies every input once per distinct pointer (phase two needs f1 and f3 again): nothing of the caller's is read after init.
// sc_gkr_layer_next_batch (at the end) puts a handle onto the next layer's inputs inside what init allocated.
// The two-point form (sc_gkr_two_point_init_batch, sc_gkr_two_point_next_batch): a layer below the output layer is claimed at two points, and
// alpha eq(g, .) + beta eq(g2, .) stands wherever eq(g, .) stands above -- k_batch_gkr_phase<., 2> folds eq(g2, .) into eq(g, .) in LDS,
// k_batch_gkr_terms<., 2> keeps a second pair of half tables, the serial plan combines the dense tables of g and g2 (k_gkr_two_point_combine).
// Every handle reserves room for g2 and the coefficients and takes either form layer by layer; a reset keeps the form.
#include <set>

#include "batch_slices.hpp"
#include "prover_internal.hpp"

struct sc_gkr_batch_prover {
    int device = 0;
    uint32_t n = 0, dim = 0, round = 0; // round: round calls answered so far, 0 .. 2 dim
    bool exhausted = false;
    int plan = scd::kGbrSerial; // scd::GkrBatchRoundsPlan; kGbrOneBlock and kGbrSlices share the work areas and everything that reads them
    bool work_areas() const { return plan != scd::kGbrSerial; }
    uint64_t nnz_max = 0;
    std::vector<std::vector<sch::Fr>> randomness; // per challenge received (u, then v): n elements, or ONE for a shared challenge
    std::vector<uint64_t> nnz;
    std::vector<sch::Fr> g;                        // n x dim
    std::vector<scd::GkrBatchInst> rec;            // the instances' arrays in the handle's copy (d_in), g in d_up
    hipStream_t stream = nullptr;
    char *d_buf = nullptr; // device, ONE allocation: area A | area B (work areas) | matrices | records | index flags | g | g2 | coefficients | challenges | messages | f2(u) | export area | a layer's staging image | inputs | serial tables, or (slices) cells | partials
    char *d_in = nullptr;  // (inside d_buf) the inputs, every distinct array once
    char *d_cells = nullptr, *d_part = nullptr; // (inside d_buf, slices) the wide cells both phases share, n x 64 B x 2^dim; the sliced rounds' partials
    size_t cells_bytes = 0;
    char *h_pin = nullptr; // pinned: matrices | ... | export area | a layer's staging image
    size_t work_bytes = 0, w_off = 0, rec_off = 0, flag_off = 0, g_off = 0, u_off = 0, msg_off = 0, f2u_off = 0, exp_off = 0, pin_bytes = 0; // (offsets into h_pin; d_buf: + 2 work_bytes)
    SharedMeta s; // one product of two tables with a coefficient of one: both phases (start_phase{1,2}_sumcheck, mod.rs:45-54, 66-82)
    // ---- sc_gkr_layer_next_batch ----
    bool dev_in = false;                   // SC_TABLES_ON_DEVICE at init: every later layer's arrays are where init's were
    int64_t pol_batch = 0, pol_slices = 0; // the policies the plan was chosen under
    size_t in_cap = 0, in_used = 0;        // d_in: the bytes reserved at init (never more), the bytes of the layout in force
    std::vector<size_t> dense_slots;       // (offsets into d_in) the places of the distinct f2 / f3 arrays that no wiring array shares: where a layer that keeps the wiring puts its own
    size_t nl_flag_off = 0, nl_chk_off = 0, nl_rec_off = 0, nl_g_off = 0, nl_item_off = 0; // (offsets into h_pin) the staging image of a layer: index flags | records over the caller's arrays | records | g | restage items
    // ---- batch.gkr_rounds_serial ----
    std::vector<sc_prover *> p1, p2;
    char *d_tabs = nullptr; // (inside d_buf) per instance h_g | f1(g, u, .) | f2(u) f3, 2^dim elements each
    char *d_fin = nullptr;  // (inside d_buf) bind_final's n x 2 elements
    std::vector<sch::Fr> f2u; // n: f2(u), from the phase change
    // ---- the two-point form (sc_gkr_two_point_init_batch / _next_batch): alpha eq(g, .) + beta eq(g2, .) where eq(g, .) stands ----
    bool two_point = false;          // the form of the layer in force: every init and every next call sets it, a reset keeps it
    std::vector<sch::Fr> g2, coef;   // n x dim; n x 2 (alpha, beta) -- read only in two-point form
    size_t g2_off = 0, coef_off = 0; // (offsets into h_pin, behind g) the upload area's g2 and coefficients: reserved by both inits
    size_t nl_g2_off = 0, nl_coef_off = 0; // ... and their places in a layer's staging image, behind its g
    char *d_tab2 = nullptr;          // (inside d_buf, serial plan) ONE scratch table of 2^dim elements: the dense table of g2 before it is combined
    int points() const { return two_point ? 2 : 1; }
    // ---- the gate form (sc_gkr_gates_init_batch, gkr_gates.hip): a handle built there is nothing but this, and every call below forwards ----
    GkrGates *gates = nullptr;
};

sc_gkr_batch_prover *gkr_gates_wrap(GkrGates *g) {
    sc_gkr_batch_prover *bp = new (std::nothrow) sc_gkr_batch_prover();
    if (bp) bp->gates = g;
    return bp;
}
GkrGates *gkr_gates_of(sc_gkr_batch_prover *bp) { return bp->gates; }

namespace {

void destroy(sc_gkr_batch_prover *bp) {
    if (!bp) return;
    if (bp->gates) gkr_gates_destroy(bp->gates);
    for (sc_prover *p : bp->p1)
        if (p) sc_prover_free(p);
    for (sc_prover *p : bp->p2)
        if (p) sc_prover_free(p);
    if (bp->d_buf || bp->h_pin || bp->stream) {
        DeviceGate gate_(bp->device);
        (void)hipSetDevice(bp->device);
        if (bp->stream) (void)hipStreamSynchronize(bp->stream);
        if (bp->d_buf) (void)hipFree(bp->d_buf);
        if (bp->h_pin) (void)hipHostFree(bp->h_pin);
        if (bp->stream) (void)hipStreamDestroy(bp->stream);
        (void)hipGetLastError();
    }
    delete bp;
}

// challenge number j (0-based: u_0 .. u_{dim-1}, v_0 ..) of every instance -> the handle's device copy, [j][instance]; a shared one is expanded
int upload_challenge(sc_gkr_batch_prover *bp, uint32_t j, const std::vector<sch::Fr> &chal) {
    const size_t off = bp->u_off + (size_t)j * bp->n * 32;
    sch::Fr *h = reinterpret_cast<sch::Fr *>(bp->h_pin + off);
    for (uint32_t i = 0; i < bp->n; ++i) h[i] = challenge_of(chal, i);
    HIP_TRY(hipMemcpyAsync(bp->d_buf + 2 * bp->work_bytes + off, h, (size_t)bp->n * 32, hipMemcpyHostToDevice, bp->stream));
    return SC_OK;
}

// the descriptor of a phase: one product of the two tables, coefficient one
struct PhaseDesc {
    uint32_t offs[2] = {0, 2}, idx2[2] = {0, 1};
    const uint64_t *tabs[2] = {nullptr, nullptr};
    sc_poly_desc d;
    PhaseDesc(uint32_t dim, uint32_t flags) {
        std::memset(&d, 0, sizeof(d));
        d.num_vars = dim;
        d.max_multiplicands = 2;
        d.n_products = 1;
        d.coeffs = sch::kOne.l;
        d.prod_offsets = offs;
        d.prod_indices = idx2;
        d.n_tables = 2;
        d.tables = tabs;
        d.flags = flags;
    }
};

char *serial_table(const sc_gkr_batch_prover *bp, uint32_t i, uint32_t which) { return bp->d_tabs + ((size_t)i * 3 + which) * ((size_t)32 << bp->dim); }

// a prover of the serial plan over two tables of the handle's (borrowed; device-side waits off, no resident kernel), or the old one rewound over them
int serial_prover(sc_gkr_batch_prover *bp, sc_prover **p, const void *t0, const void *t1) {
    PhaseDesc pd(bp->dim, SC_TABLES_ON_DEVICE | SC_TABLES_BORROW | SC_NO_DEVICE_POLLING);
    pd.tabs[0] = static_cast<const uint64_t *>(t0);
    pd.tabs[1] = static_cast<const uint64_t *>(t1);
    if (*p) return sc_prover_reset(*p, pd.tabs, SC_TABLES_ON_DEVICE);
    int rc = sc_prover_init(&pd.d, p);
    if (rc == SC_OK) rc = sc_prover_set_resident(*p, 0);
    return rc;
}

// the serial plan's two-point tables, by linearity: table <- alpha table + beta d_tab2 (the dense tables of g and of g2), one launch on the
// handle's stream and a synchronisation -- the tables' producer has synchronised, their consumer is a prover with a stream of its own
int serial_combine(sc_gkr_batch_prover *bp, uint32_t i, char *table) {
    DeviceGate gate_(bp->device);
    HIP_TRY(hipSetDevice(bp->device));
    const uint4 *coef = reinterpret_cast<const uint4 *>(bp->d_buf + 2 * bp->work_bytes + bp->coef_off) + 4 * (size_t)i;
    HIP_TRY(scd::launch_gkr_two_point_combine(reinterpret_cast<const uint4 *>(table), reinterpret_cast<const uint4 *>(bp->d_tab2), coef, reinterpret_cast<uint4 *>(table), 1ULL << bp->dim, bp->stream));
    HIP_TRY(hipStreamSynchronize(bp->stream));
    return SC_OK;
}

// the serial plan's phase change for instance i: f2(u) from phase one's prover, f1(g, u, .), f2(u) f3, phase two's prover
int serial_phase_two(sc_gkr_batch_prover *bp, uint32_t i, const std::vector<sch::Fr> &u_last) {
    const uint32_t dim = bp->dim;
    if (int rc = serial_bind_final(bp->p1[i], bp->device, challenge_of(u_last, i).l, bp->d_fin + (size_t)i * 64, 1, 1, &bp->f2u[i])) return rc;
    std::vector<sch::Fr> u(dim);
    for (uint32_t j = 0; j + 1 < dim; ++j) u[j] = challenge_of(bp->randomness[j], i);
    u[dim - 1] = challenge_of(u_last, i);
    const scd::GkrBatchInst &I = bp->rec[i];
    if (int rc = sc_internal_gkr_dense_table(2, I.idx, I.vals, bp->nnz[i], dim, I.f3, bp->g[(size_t)i * dim].l, u[0].l, serial_table(bp, i, 1))) return rc;
    if (bp->two_point) {
        if (int rc = sc_internal_gkr_dense_table(2, I.idx, I.vals, bp->nnz[i], dim, I.f3, bp->g2[(size_t)i * dim].l, u[0].l, bp->d_tab2)) return rc;
        if (int rc = serial_combine(bp, i, serial_table(bp, i, 1))) return rc;
    }
    if (int rc = sc_dense_scale(reinterpret_cast<const uint64_t *>(I.f3), 1ULL << dim, bp->f2u[i].l, reinterpret_cast<uint64_t *>(serial_table(bp, i, 2)), SC_TABLES_ON_DEVICE)) return rc; // mod.rs:71-75
    return serial_prover(bp, &bp->p2[i], serial_table(bp, i, 1), serial_table(bp, i, 2));
}

// the sliced plan's initialisation of a phase: the cells zeroed, k_batch_gkr_terms, k_batch_gkr_fold -- all on the handle's stream
int slices_phase(sc_gkr_batch_prover *bp, int phase) {
    char *d_up = bp->d_buf + 2 * bp->work_bytes;
    HIP_TRY(hipMemsetAsync(bp->d_cells, 0, bp->cells_bytes, bp->stream));
    scd::BatchGkrSlicesArgs P;
    std::memset(&P, 0, sizeof(P));
    P.inst = reinterpret_cast<const scd::GkrBatchInst *>(d_up + bp->rec_off);
    P.work_a = reinterpret_cast<int32_t *>(bp->d_buf);
    P.work_b = reinterpret_cast<int32_t *>(bp->d_buf + bp->work_bytes);
    P.u = reinterpret_cast<const uint4 *>(d_up + bp->u_off);
    P.f2u = reinterpret_cast<uint4 *>(d_up + bp->f2u_off);
    P.cells = reinterpret_cast<uint64_t *>(bp->d_cells);
    P.n = bp->n;
    P.dim = bp->dim;
    P.g2 = reinterpret_cast<const uint4 *>(d_up + bp->g2_off);
    P.coef = reinterpret_cast<const uint4 *>(d_up + bp->coef_off);
    HIP_TRY(scd::launch_batch_gkr_slices_phase(phase, P, bp->nnz_max, bp->stream, bp->points()));
    return SC_OK;
}

// phase one's tables of a handle with work areas out of the records and arrays on the device, on the handle's stream (init, and every later layer)
int areas_phase_one(sc_gkr_batch_prover *bp) {
    if (bp->plan == scd::kGbrSlices) return slices_phase(bp, 1);
    if (bp->plan != scd::kGbrOneBlock) return SC_OK;
    scd::BatchGkrPhaseArgs A;
    std::memset(&A, 0, sizeof(A));
    A.inst = reinterpret_cast<const scd::GkrBatchInst *>(bp->d_buf + 2 * bp->work_bytes + bp->rec_off);
    A.work_a = reinterpret_cast<int32_t *>(bp->d_buf);
    A.n = bp->n;
    A.dim = bp->dim;
    A.g2 = reinterpret_cast<const uint4 *>(bp->d_buf + 2 * bp->work_bytes + bp->g2_off);
    A.coef = reinterpret_cast<const uint4 *>(bp->d_buf + 2 * bp->work_bytes + bp->coef_off);
    HIP_TRY(scd::launch_batch_gkr_phase(1, A, bp->stream, bp->points()));
    return SC_OK;
}

// the serial plan's phase one: per instance h_g by sc_gkr_prove's route and a prover over (h_g, f2), or the old prover rewound over them
int serial_phase_one(sc_gkr_batch_prover *bp) {
    for (uint32_t i = 0; i < bp->n; ++i) {
        const scd::GkrBatchInst &I = bp->rec[i];
        int rc = sc_internal_gkr_dense_table(1, I.idx, I.vals, bp->nnz[i], bp->dim, I.f3, bp->g[(size_t)i * bp->dim].l, nullptr, serial_table(bp, i, 0)); // mod.rs:30-38
        if (rc == SC_OK && bp->two_point) {
            rc = sc_internal_gkr_dense_table(1, I.idx, I.vals, bp->nnz[i], bp->dim, I.f3, bp->g2[(size_t)i * bp->dim].l, nullptr, bp->d_tab2);
            if (rc == SC_OK) rc = serial_combine(bp, i, serial_table(bp, i, 0));
        }
        if (rc == SC_OK) rc = serial_prover(bp, &bp->p1[i], serial_table(bp, i, 0), I.f2);
        if (rc) return prefix_instance(rc, i);
    }
    return SC_OK;
}

// the places of a layout's distinct f2 / f3 arrays that no wiring array shares (offs: per instance idx, vals, f2, f3), in the layout's order
std::vector<size_t> dense_slots_of(const std::vector<size_t> &offs, const std::vector<uint64_t> &nnz) {
    std::set<size_t> wiring, dense;
    for (size_t i = 0; i < nnz.size(); ++i)
        if (nnz[i]) {
            wiring.insert(offs[4 * i + 0]);
            wiring.insert(offs[4 * i + 1]);
        }
    for (size_t i = 0; i < nnz.size(); ++i)
        for (int k = 2; k < 4; ++k)
            if (!wiring.count(offs[4 * i + k])) dense.insert(offs[4 * i + k]);
    return std::vector<size_t>(dense.begin(), dense.end());
}

// the two-point form's own checks on instance i, behind gkr_check_instance's (no HIP call)
int check_second_point(const uint64_t *const *g2, const uint64_t *coef, uint32_t dim, uint32_t i) {
    if (!g2[i]) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: null argument", i);
    for (uint32_t k = 0; k < dim; ++k) {
        sch::Fr e;
        std::memcpy(&e, g2[i] + 4 * (size_t)k, 32);
        if (sch::geq_p(e)) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: g2 is not canonical", i);
    }
    for (uint32_t k = 0; k < 2; ++k) {
        sch::Fr e;
        std::memcpy(&e, coef + 4 * ((size_t)i * 2 + k), 32);
        if (sch::geq_p(e)) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: coefficient is not canonical", i);
    }
    return SC_OK;
}

// sc_gkr_batch_prover_init (g2 and coef null: the one-point form) and sc_gkr_two_point_init_batch
int init_handle(uint32_t n, uint32_t dim, const uint64_t *const *f1_idx, const uint64_t *const *f1_vals, const uint64_t *nnz, const uint64_t *const *f2, const uint64_t *const *f3,
                const uint64_t *const *g, const uint64_t *const *g2, const uint64_t *coef, uint32_t flags, sc_gkr_batch_prover **out);
// sc_gkr_layer_next_batch (g2 and coef null: the layer is in one-point form) and sc_gkr_two_point_next_batch
int next_layer(sc_gkr_batch_prover *bp, const uint64_t *const *f1_idx_or_null, const uint64_t *const *f1_vals_or_null, const uint64_t *nnz_or_null, const uint64_t *const *f2,
               const uint64_t *const *f3, const uint64_t *const *g, const uint64_t *const *g2, const uint64_t *coef, uint32_t flags);

} // namespace

extern "C" int sc_gkr_batch_prover_init(uint32_t n, uint32_t dim, const uint64_t *const *f1_idx, const uint64_t *const *f1_vals, const uint64_t *nnz, const uint64_t *const *f2,
                                        const uint64_t *const *f3, const uint64_t *const *g, uint32_t flags, sc_gkr_batch_prover **out) {
    return init_handle(n, dim, f1_idx, f1_vals, nnz, f2, f3, g, nullptr, nullptr, flags, out);
}

// The two-point form of the init: per instance a second point g2[i] and coefficients coef[i] = (alpha, beta); alpha eq(g, .) + beta eq(g2, .)
// stands wherever the handle uses eq(g, .) -- the claim alpha W(g) + beta W(g2) a GKR layer below the output layer starts from.
extern "C" int sc_gkr_two_point_init_batch(uint32_t n, uint32_t dim, const uint64_t *const *f1_idx, const uint64_t *const *f1_vals, const uint64_t *nnz, const uint64_t *const *f2,
                                           const uint64_t *const *f3, const uint64_t *const *g, const uint64_t *const *g2, const uint64_t *coef, uint32_t flags, sc_gkr_batch_prover **out) {
    if (!g2 || !coef) {
        if (out) *out = nullptr;
        return sc_internal_fail(SC_ERR_BAD_ARG, "null argument");
    }
    const int rc = init_handle(n, dim, f1_idx, f1_vals, nnz, f2, f3, g, g2, coef, flags, out);
    if (rc == SC_OK) scd::plan_hit(scd::kPlanBatchGkrTwoPoint);
    return rc;
}

namespace {
int init_handle(uint32_t n, uint32_t dim, const uint64_t *const *f1_idx, const uint64_t *const *f1_vals, const uint64_t *nnz, const uint64_t *const *f2, const uint64_t *const *f3,
                const uint64_t *const *g, const uint64_t *const *g2, const uint64_t *coef, uint32_t flags, sc_gkr_batch_prover **out) {
    // ---- everything the host can check, before any HIP call (sc_gkr_prove_batch's checks: the lowest failing instance decides) ----
    if (!f1_idx || !f1_vals || !nnz || !f2 || !f3 || !g || !out) return sc_internal_fail(SC_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    if (n == 0) return sc_internal_fail(SC_ERR_BAD_ARG, "n == 0: a batch handle holds at least one instance");
    if (dim == 0) return sc_internal_fail(SC_ERR_CONSTANT_POLY, "instance 0: Attempt to prove a constant.");
    if (dim > 21) return sc_internal_fail(SC_ERR_BAD_ARG, "instance 0: dim %u: 3*dim index bits do not fit 64-bit indices", dim);
    const bool dev_in = flags & SC_TABLES_ON_DEVICE;
    const GkrBatchIn in = {n, dim, f1_idx, f1_vals, nnz, f2, f3, g, dev_in};
    uint64_t nnz_max = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (int rc = gkr_check_instance(in, i, nullptr)) return rc;
        if (g2)
            if (int rc = check_second_point(g2, coef, dim, i)) return rc;
        nnz_max = std::max(nnz_max, nnz[i]);
    }
    if (sc_device_count() <= 0) return sc_internal_fail(SC_ERR_HIP, "no HIP device visible: libsumcheck_hip has no CPU fallback");
    sc_gkr_batch_prover *bp = new (std::nothrow) sc_gkr_batch_prover();
    if (!bp) return sc_internal_fail(SC_ERR_OOM, "out of host memory");
    bp->device = sc_internal_device_ref();
    bp->n = n;
    bp->dim = dim;
    bp->nnz.assign(nnz, nnz + n);
    bp->g.resize((size_t)n * dim);
    for (uint32_t i = 0; i < n; ++i) std::memcpy(&bp->g[(size_t)i * dim], g[i], (size_t)dim * 32);
    bp->two_point = g2 != nullptr;
    bp->g2.resize((size_t)n * dim); // (zero in one-point form: room for a later two-point layer)
    bp->coef.resize((size_t)n * 2);
    if (g2) {
        for (uint32_t i = 0; i < n; ++i) std::memcpy(&bp->g2[(size_t)i * dim], g2[i], (size_t)dim * 32);
        std::memcpy(bp->coef.data(), coef, (size_t)n * 64);
    }
    bp->nnz_max = nnz_max;
    const size_t N = (size_t)1 << dim;
    auto build = [&]() -> int {
        PhaseDesc pd(dim, 0);
        build_shared(&pd.d, bp->s);
        bp->s.unit.push_back(unit_matrix(2, 3));
        bp->pol_batch = scd::policy(scd::kPolBatch);
        bp->pol_slices = scd::policy(scd::kPolBatchSlices);
        bp->plan = scd::gkr_bs_plan(n, dim, nnz_max, bp->s.n_combos, bp->pol_batch, bp->pol_slices);
        const bool areas = bp->work_areas(), slices = bp->plan == scd::kGbrSlices;
        // ---- the handle's copy of the inputs: every distinct (pointer, size) once ----
        StageMap st; // (offsets into d_in)
        st.align = 256;
        std::vector<size_t> offs((size_t)n * 4, 0);
        for (uint32_t i = 0; i < n; ++i) {
            offs[4 * (size_t)i + 0] = nnz[i] ? st.add(f1_idx[i], (size_t)nnz[i] * 8) : 0;
            offs[4 * (size_t)i + 1] = nnz[i] ? st.add(f1_vals[i], (size_t)nnz[i] * 32) : 0;
            offs[4 * (size_t)i + 2] = st.add(f2[i], N * 32);
            offs[4 * (size_t)i + 3] = st.add(f3[i], N * 32);
        }
        const size_t in_bytes = st.bytes;
        bp->in_cap = bp->in_used = in_bytes;
        bp->dense_slots = dense_slots_of(offs, bp->nnz);
        bp->dev_in = dev_in;
        bp->work_bytes = areas ? round_up((size_t)n * 2 * 2 * (scd::kBatchRoundSlotBytes << dim), 256) : 0;
        bp->w_off = 0;
        bp->rec_off = bp->w_off + round_up((size_t)bp->s.w_elems * 32, 256);
        bp->flag_off = bp->rec_off + round_up((size_t)n * sizeof(scd::GkrBatchInst), 256);
        bp->g_off = bp->flag_off + round_up((size_t)n * 4, 256);
        bp->g2_off = bp->g_off + round_up((size_t)n * dim * 32, 256);
        bp->coef_off = bp->g2_off + round_up((size_t)n * dim * 32, 256);
        bp->u_off = bp->coef_off + round_up((size_t)n * 64, 256);
        bp->msg_off = bp->u_off + round_up((size_t)2 * dim * n * 32, 256);
        bp->f2u_off = bp->msg_off + round_up((size_t)n * 3 * 32, 256);
        bp->exp_off = bp->f2u_off + round_up((size_t)n * 32, 256);
        bp->nl_flag_off = bp->exp_off + round_up(std::max(2 * N * 32, (size_t)n * 2 * 32), 256); // one instance's tables (state), or every instance's final values
        bp->nl_chk_off = bp->nl_flag_off + round_up((size_t)n * 4, 256);
        bp->nl_rec_off = bp->nl_chk_off + round_up((size_t)n * sizeof(scd::GkrBatchInst), 256);
        bp->nl_g_off = bp->nl_rec_off + round_up((size_t)n * sizeof(scd::GkrBatchInst), 256);
        bp->nl_g2_off = bp->nl_g_off + round_up((size_t)n * dim * 32, 256);
        bp->nl_coef_off = bp->nl_g2_off + round_up((size_t)n * dim * 32, 256);
        bp->nl_item_off = bp->nl_coef_off + round_up((size_t)n * 64, 256);
        bp->pin_bytes = bp->nl_item_off + round_up(((size_t)n * 4 + 4) * sizeof(scd::GkrRestageItem), 256); // (every array of every instance, the records, g, g2, the coefficients)
        {
            DeviceGate gate_(bp->device);
            HIP_TRY(hipSetDevice(bp->device));
            HIP_TRY(hipStreamCreateWithFlags(&bp->stream, hipStreamNonBlocking));
            const size_t tabs_bytes = areas ? 0 : ((size_t)n * 3 + 1) * N * 32, fin_bytes = areas ? 0 : round_up((size_t)n * 64, 256);
            bp->cells_bytes = slices ? (size_t)n * scd::kBsGkrCellBytes * N : 0;
            const size_t part_bytes = slices ? round_up((size_t)scd::bs_partials_bytes(n, dim, 2, 1, 3, bp->s.n_combos), 256) : 0;
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&bp->d_buf), 2 * bp->work_bytes + bp->pin_bytes + in_bytes + tabs_bytes + fin_bytes + bp->cells_bytes + part_bytes)); // (one allocation: a handle's life is short)
            bp->d_in = bp->d_buf + 2 * bp->work_bytes + bp->pin_bytes;
            if (!areas) {
                bp->d_tabs = bp->d_in + in_bytes;
                bp->d_tab2 = bp->d_tabs + (size_t)n * 3 * N * 32;
                bp->d_fin = bp->d_tabs + tabs_bytes;
            }
            if (slices) {
                bp->d_cells = bp->d_in + in_bytes;
                bp->d_part = bp->d_cells + bp->cells_bytes;
            }
            HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&bp->h_pin), bp->pin_bytes, hipHostMallocDefault));
            if (dev_in) HIP_TRY(hipDeviceSynchronize()); // the inputs' producers are waited for, as a copy on their stream would
            for (const StageMap::Item &it : st.items) HIP_TRY(hipMemcpyAsync(bp->d_in + it.off, it.src, it.bytes, dev_in ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, bp->stream));
            char *d_up = bp->d_buf + 2 * bp->work_bytes;
            instance_weights(bp->s, sch::kOne.l, reinterpret_cast<sch::Fr *>(bp->h_pin + bp->w_off));
            std::memset(bp->h_pin + bp->flag_off, 0, round_up((size_t)n * 4, 256));
            std::memcpy(bp->h_pin + bp->g_off, bp->g.data(), (size_t)n * dim * 32);
            std::memcpy(bp->h_pin + bp->g2_off, bp->g2.data(), (size_t)n * dim * 32);
            std::memcpy(bp->h_pin + bp->coef_off, bp->coef.data(), (size_t)n * 64);
            bp->rec.resize(n);
            for (uint32_t i = 0; i < n; ++i) {
                scd::GkrBatchInst &r = bp->rec[i];
                r.nnz = nnz[i];
                r.idx = reinterpret_cast<const uint64_t *>(bp->d_in + offs[4 * (size_t)i + 0]);
                r.vals = reinterpret_cast<const uint4 *>(bp->d_in + offs[4 * (size_t)i + 1]);
                r.f2 = reinterpret_cast<const uint4 *>(bp->d_in + offs[4 * (size_t)i + 2]);
                r.f3 = reinterpret_cast<const uint4 *>(bp->d_in + offs[4 * (size_t)i + 3]);
                r.g = reinterpret_cast<const uint4 *>(d_up + bp->g_off + (size_t)i * dim * 32);
            }
            std::memcpy(bp->h_pin + bp->rec_off, bp->rec.data(), (size_t)n * sizeof(scd::GkrBatchInst));
            HIP_TRY(hipMemcpyAsync(d_up, bp->h_pin, bp->u_off, hipMemcpyHostToDevice, bp->stream));
            const scd::GkrBatchInst *d_rec = reinterpret_cast<const scd::GkrBatchInst *>(d_up + bp->rec_off);
            // device-resident lists: an index out of range is found here, in front of any kernel that follows the indices (host lists: checked above)
            if (dev_in)
                if (int rc = gkr_check_idx_on_device(d_rec, n, dim, bp->h_pin, d_up, bp->flag_off, bp->stream)) return rc;
            if (int rc = areas_phase_one(bp)) return rc;
            HIP_TRY(hipStreamSynchronize(bp->stream)); // nothing of the caller's is read after the call returns
        }
        if (areas) return SC_OK;
        bp->p1.assign(n, nullptr);
        bp->p2.assign(n, nullptr);
        bp->f2u.resize(n);
        return serial_phase_one(bp);
    };
    if (int rc = build()) {
        const std::string why = sc_last_error(); // (the frees below may run library calls of their own)
        destroy(bp);
        return sc_internal_fail(rc, "%s", why.c_str());
    }
    *out = bp;
    return SC_OK;
}
} // namespace

extern "C" void sc_gkr_batch_prover_free(sc_gkr_batch_prover *bp) { destroy(bp); }

extern "C" int sc_gkr_batch_prove_round(sc_gkr_batch_prover *bp, const uint64_t *r_or_null, uint32_t r_shared, uint64_t *out_evals) {
    if (!bp || !out_evals) return sc_internal_fail(SC_ERR_BAD_ARG, "null argument");
    if (bp->gates) return gkr_gates_prove_round(bp->gates, r_or_null, r_shared, out_evals);
    // validation, sc_batch_prove_round's precedence; every check comes before the first change to the handle
    if (bp->exhausted) return sc_internal_fail(SC_ERR_NOT_ACTIVE, "Prover is not active");
    if (r_or_null && bp->round == 0) return sc_internal_fail(SC_ERR_FIRST_ROUND_HAS_MSG, "first round should be prover first.");
    if (!r_or_null && bp->round > 0) return sc_internal_fail(SC_ERR_MISSING_MSG, "verifier message is empty");
    if (bp->round + 1 > 2 * bp->dim) return sc_internal_fail(SC_ERR_NOT_ACTIVE, "Prover is not active");
    std::vector<sch::Fr> chal;
    if (r_or_null)
        if (int rc = take_challenges(bp->n, r_or_null, r_shared, chal)) return rc;
    const uint32_t n = bp->n, dim = bp->dim, t = bp->round, phase = t / dim, r = t % dim;
    if (bp->work_areas()) {
        const SharedMeta &s = bp->s;
        const bool slices = bp->plan == scd::kGbrSlices;
        DeviceGate gate_(bp->device);
        HIP_TRY(hipSetDevice(bp->device));
        char *d_up = bp->d_buf + 2 * bp->work_bytes;
        if (r_or_null)
            if (int rc = upload_challenge(bp, t - 1, chal)) return rc;
        if (t == dim && slices) { // the phase change: f2(u), f1(g, u, .), f2(u) f3 -> area B
            if (int rc = slices_phase(bp, 2)) return rc;
        } else if (t == dim) {
            scd::BatchGkrPhaseArgs P;
            std::memset(&P, 0, sizeof(P));
            P.inst = reinterpret_cast<const scd::GkrBatchInst *>(d_up + bp->rec_off);
            P.work_a = reinterpret_cast<int32_t *>(bp->d_buf);
            P.work_b = reinterpret_cast<int32_t *>(bp->d_buf + bp->work_bytes);
            P.u = reinterpret_cast<const uint4 *>(d_up + bp->u_off);
            P.f2u = reinterpret_cast<uint4 *>(d_up + bp->f2u_off);
            P.n = n;
            P.dim = dim;
            P.g2 = reinterpret_cast<const uint4 *>(d_up + bp->g2_off);
            P.coef = reinterpret_cast<const uint4 *>(d_up + bp->coef_off);
            HIP_TRY(scd::launch_batch_gkr_phase(2, P, bp->stream, bp->points()));
        }
        scd::BatchRoundArgs A;
        std::memset(&A, 0, sizeof(A));
        A.work = reinterpret_cast<int32_t *>(bp->d_buf + (phase ? bp->work_bytes : 0));
        A.Wm = reinterpret_cast<const uint4 *>(d_up + bp->w_off);
        A.w_stride = 0; // a coefficient of one: the same matrices for every instance
        A.chal = r ? reinterpret_cast<const uint4 *>(d_up + bp->u_off + (size_t)(t - 1) * n * 32) : nullptr;
        A.chal_shared = 0;
        A.out = reinterpret_cast<uint4 *>(d_up + bp->msg_off);
        A.n = n;
        A.n_tables = 2;
        A.nv = dim;
        A.round = r;
        A.n_combos = s.n_combos;
        A.K = 1;
        A.D = 3;
        if (slices && scd::bs_round_sliced(dim, r, 2, 1, 3, 2)) HIP_TRY(scd::launch_batch_round_slices(A, reinterpret_cast<uint4 *>(bp->d_part), s.combo, s.fin, bp->stream));
        else HIP_TRY(scd::launch_batch_round(A, s.combo, s.fin, bp->stream));
        scd::plan_hit(slices ? scd::kPlanBatchGkrRoundsSlices : scd::kPlanBatchGkrRoundsOneBlock);
        HIP_TRY(hipMemcpyAsync(bp->h_pin + bp->msg_off, d_up + bp->msg_off, (size_t)n * 96, hipMemcpyDeviceToHost, bp->stream));
        HIP_TRY(hipStreamSynchronize(bp->stream));
        std::memcpy(out_evals, bp->h_pin + bp->msg_off, (size_t)n * 96);
    } else {
        scd::plan_hit(scd::kPlanBatchGkrRoundsSerial);
        for (uint32_t i = 0; i < n; ++i) {
            int rc = SC_OK;
            if (t == dim) rc = serial_phase_two(bp, i, chal);
            if (rc == SC_OK) rc = sc_prove_round(phase ? bp->p2[i] : bp->p1[i], r ? challenge_of(chal, i).l : nullptr, out_evals + (size_t)i * 12);
            if (rc) {
                bp->exhausted = true; // (a failure part of the way through the batch: the handle needs a reset)
                return prefix_instance(rc, i);
            }
        }
    }
    if (r_or_null) bp->randomness.push_back(std::move(chal));
    bp->round++;
    return SC_OK;
}

extern "C" int sc_gkr_batch_prover_finish(sc_gkr_batch_prover *bp, const uint64_t *r, uint32_t r_shared, uint64_t *out_uv_or_null, uint64_t *out_final_or_null) {
    if (!bp || !r) return sc_internal_fail(SC_ERR_BAD_ARG, "null argument");
    if (bp->gates) return gkr_gates_finish(bp->gates, r, r_shared, out_uv_or_null, out_final_or_null);
    if (bp->exhausted || bp->round != 2 * bp->dim) return sc_internal_fail(SC_ERR_NOT_ACTIVE, "finish needs a prover that has answered its last round");
    std::vector<sch::Fr> chal;
    if (int rc = take_challenges(bp->n, r, r_shared, chal)) return rc;
    const uint32_t n = bp->n, dim = bp->dim;
    std::vector<sch::Fr> fin((size_t)n * 3); // f1(g,u,v), f2(u), f2(u) f3(v)
    if (bp->work_areas()) {
        DeviceGate gate_(bp->device);
        HIP_TRY(hipSetDevice(bp->device));
        char *d_up = bp->d_buf + 2 * bp->work_bytes;
        if (int rc = upload_challenge(bp, 2 * dim - 1, chal)) return rc;
        HIP_TRY(scd::launch_batch_rounds_export(reinterpret_cast<const int32_t *>(bp->d_buf + bp->work_bytes), 0, n, 2, dim, dim - 1,
                                                reinterpret_cast<const uint4 *>(d_up + bp->u_off + (size_t)(2 * dim - 1) * n * 32), 0u, reinterpret_cast<uint4 *>(d_up + bp->exp_off),
                                                bp->stream));
        HIP_TRY(hipMemcpyAsync(bp->h_pin + bp->f2u_off, d_up + bp->f2u_off, bp->exp_off - bp->f2u_off + (size_t)n * 64, hipMemcpyDeviceToHost, bp->stream));
        HIP_TRY(hipStreamSynchronize(bp->stream));
        const sch::Fr *f2u = reinterpret_cast<const sch::Fr *>(bp->h_pin + bp->f2u_off), *ex = reinterpret_cast<const sch::Fr *>(bp->h_pin + bp->exp_off);
        for (uint32_t i = 0; i < n; ++i) {
            fin[3 * (size_t)i + 0] = ex[2 * (size_t)i];
            fin[3 * (size_t)i + 1] = f2u[i];
            fin[3 * (size_t)i + 2] = ex[2 * (size_t)i + 1];
        }
    } else {
        for (uint32_t i = 0; i < n; ++i) {
            sch::Fr two[2];
            if (int rc = serial_bind_final(bp->p2[i], bp->device, challenge_of(chal, i).l, bp->d_fin + (size_t)i * 64, 0, 2, two)) {
                bp->exhausted = true;
                return prefix_instance(rc, i);
            }
            fin[3 * (size_t)i + 0] = two[0];
            fin[3 * (size_t)i + 1] = bp->f2u[i];
            fin[3 * (size_t)i + 2] = two[1];
        }
    }
    bp->randomness.push_back(std::move(chal));
    bp->exhausted = true;
    if (out_uv_or_null)
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t j = 0; j < 2 * dim; ++j) std::memcpy(out_uv_or_null + ((size_t)i * 2 * dim + j) * 4, &challenge_of(bp->randomness[j], i), 32);
    if (out_final_or_null) std::memcpy(out_final_or_null, fin.data(), fin.size() * 32);
    return SC_OK;
}

extern "C" int sc_gkr_batch_prover_state(sc_gkr_batch_prover *bp, uint32_t instance, uint64_t *randomness, uint32_t *n_randomness, uint64_t *tables_out, uint32_t *round) {
    if (!bp) return sc_internal_fail(SC_ERR_BAD_ARG, "null prover");
    if (bp->gates) return gkr_gates_state(bp->gates, instance, randomness, n_randomness, tables_out, round);
    if (instance >= bp->n) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: the handle holds %u instances", instance, bp->n);
    batch_state_head(bp->randomness, instance, bp->round, randomness, n_randomness, round);
    if (!tables_out) return SC_OK;
    if (bp->exhausted) return sc_internal_fail(SC_ERR_NOT_ACTIVE, "tables were consumed by sc_gkr_batch_prover_finish");
    // the current phase's two tables: phase one's until round call dim has built phase two's; bound = the phase's max(round - 1, 0)
    const uint32_t dim = bp->dim, phase = bp->round > dim ? 1u : 0u, pr = bp->round - phase * dim, bound = pr > 0 ? pr - 1 : 0;
    if (!bp->work_areas()) return sc_prover_state(phase ? bp->p2[instance] : bp->p1[instance], nullptr, nullptr, tables_out, nullptr);
    DeviceGate gate_(bp->device);
    HIP_TRY(hipSetDevice(bp->device));
    return batch_export_out(reinterpret_cast<const int32_t *>(bp->d_buf + (phase ? bp->work_bytes : 0)), instance, 1, 2, dim, bound, nullptr, 0, bp->d_buf + 2 * bp->work_bytes + bp->exp_off,
                            bp->h_pin + bp->exp_off, tables_out, bp->stream);
}

extern "C" int sc_gkr_batch_prover_reset(sc_gkr_batch_prover *bp) {
    if (!bp) return sc_internal_fail(SC_ERR_BAD_ARG, "null prover");
    if (bp->gates) return gkr_gates_reset(bp->gates);
    if (!bp->work_areas())
        for (uint32_t i = 0; i < bp->n; ++i) // phase one's provers borrow the handle's own tables: rewound in place (phase two's are rewound over new tables at the phase change)
            if (int rc = sc_prover_reset(bp->p1[i], nullptr, SC_TABLES_ON_DEVICE)) return prefix_instance(rc, i);
    // (work areas: area A's depth 0 was never overwritten)
    bp->round = 0;
    bp->exhausted = false;
    bp->randomness.clear();
    return SC_OK;
}

// ---- sc_gkr_layer_next_batch: the handle onto the next layer's inputs, inside what init allocated ------------------------------------
// A GKR prover runs one round sumcheck per layer under one transcript, and every layer has new inputs: its g is the previous layer's point
// (the output layer's; below it the claim stands at two points: next_layer's g2 and coef),
// its f2 and f3 are the next layer's values, often it has wiring of its own.  The input area is laid out again by init's rule (a layer that
// keeps the wiring leaves the wiring's arrays where they are and gives its distinct f2 / f3 the places the former ones had), phase one's
// tables are rebuilt, and the handle is at round 0 as a fresh init over these inputs would leave it -- same plan, same bits.
//   host arrays    one copy per distinct array into the handle's copy (init's staging), one upload of records and g;
//   device arrays  ONE upload of a staging image -- index flags | records over the CALLER's arrays | records | g | restage items --, the
//                  index check over the caller's arrays where the wiring is new (the last thing that can refuse: up to here nothing of the
//                  handle's has been written), then ONE launch of k_batch_gkr_restage that brings in every array, the records and g;
// then what init runs (k_batch_gkr_phase<1>, or the sliced plan's memset + terms + fold; serial plan: the per-instance loop, the provers
// rewound over the new tables) and one synchronisation.  A HIP error past the index check leaves the handle exhausted with undefined inputs:
// the next successful call of this function, or free.
extern "C" int sc_gkr_layer_next_batch(sc_gkr_batch_prover *bp, const uint64_t *const *f1_idx_or_null, const uint64_t *const *f1_vals_or_null, const uint64_t *nnz_or_null,
                                       const uint64_t *const *f2, const uint64_t *const *f3, const uint64_t *const *g, uint32_t flags) {
    return next_layer(bp, f1_idx_or_null, f1_vals_or_null, nnz_or_null, f2, f3, g, nullptr, nullptr, flags); // (a handle in two-point form returns to the one-point form)
}

// The two-point form of the call, on a handle built by either init: g2 and coef are staged where g is staged, and checked with it.
extern "C" int sc_gkr_two_point_next_batch(sc_gkr_batch_prover *bp, const uint64_t *const *f1_idx_or_null, const uint64_t *const *f1_vals_or_null, const uint64_t *nnz_or_null,
                                           const uint64_t *const *f2, const uint64_t *const *f3, const uint64_t *const *g, const uint64_t *const *g2, const uint64_t *coef, uint32_t flags) {
    if (!bp) return sc_internal_fail(SC_ERR_BAD_ARG, "null prover");
    if (!g2 || !coef) return sc_internal_fail(SC_ERR_BAD_ARG, "null argument");
    const int rc = next_layer(bp, f1_idx_or_null, f1_vals_or_null, nnz_or_null, f2, f3, g, g2, coef, flags);
    if (rc == SC_OK) scd::plan_hit(scd::kPlanBatchGkrTwoPoint);
    return rc;
}

namespace {
int next_layer(sc_gkr_batch_prover *bp, const uint64_t *const *f1_idx_or_null, const uint64_t *const *f1_vals_or_null, const uint64_t *nnz_or_null, const uint64_t *const *f2,
               const uint64_t *const *f3, const uint64_t *const *g, const uint64_t *const *g2, const uint64_t *coef, uint32_t flags) {
    // ---- everything the host can check, before any HIP call and before the first change to the handle ----
    if (!bp) return sc_internal_fail(SC_ERR_BAD_ARG, "null prover");
    if (bp->gates) return sc_internal_fail(SC_ERR_BAD_ARG, "the handle was built by sc_gkr_gates_init_batch: its layers come through sc_gkr_gates_next_batch");
    if (!f2 || !f3 || !g) return sc_internal_fail(SC_ERR_BAD_ARG, "null argument");
    const bool new_f1 = f1_idx_or_null && f1_vals_or_null && nnz_or_null;
    if (!new_f1 && (f1_idx_or_null || f1_vals_or_null || nnz_or_null))
        return sc_internal_fail(SC_ERR_BAD_ARG, "f1_idx, f1_vals and nnz come together (new wiring) or are all NULL (the handle's wiring is kept)");
    const bool dev_in = flags & SC_TABLES_ON_DEVICE;
    if (dev_in != bp->dev_in) return sc_internal_fail(SC_ERR_BAD_ARG, "flags: the handle was built over %s arrays, a later layer's are where init's were", bp->dev_in ? "device" : "host");
    const uint32_t n = bp->n, dim = bp->dim;
    const size_t N = (size_t)1 << dim, slot = round_up(N * 32, 256);
    static const char *const kPlanOf[3] = {"batch.gkr_rounds_serial", "batch.gkr_rounds_one_block", "batch.gkr_rounds_slices"};
    std::vector<const uint64_t *> none;
    std::vector<uint64_t> nnz = bp->nnz;
    if (!new_f1) none.assign(n, nullptr);
    else nnz.assign(nnz_or_null, nnz_or_null + n);
    const std::vector<uint64_t> zero(new_f1 ? 0 : n, 0); // (kept wiring: nothing of f1 to check)
    const GkrBatchIn in = {n, dim, new_f1 ? f1_idx_or_null : none.data(), new_f1 ? f1_vals_or_null : none.data(), new_f1 ? nnz_or_null : zero.data(), f2, f3, g, dev_in};
    uint64_t nnz_max = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (int rc = gkr_check_instance(in, i, nullptr)) return rc;
        if (g2)
            if (int rc = check_second_point(g2, coef, dim, i)) return rc;
        // the plan stays the one chosen at init (the serial plan takes every shape)
        if (new_f1 && bp->work_areas()) {
            const int would = scd::gkr_bs_plan(n, dim, nnz[i], bp->s.n_combos, bp->pol_batch, bp->pol_slices);
            if (would != bp->plan)
                return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: nnz %llu (the plan's limit: 64 x 2^dim = %llu) would take plan %s, the handle was built for %s: build a new handle", i,
                                        (unsigned long long)nnz[i], (unsigned long long)(scd::kGkrBatchMaxNnzPerCell << dim), kPlanOf[would], kPlanOf[bp->plan]);
        }
        nnz_max = std::max(nnz_max, nnz[i]);
    }
    // ---- the input area again: every distinct (pointer, size) once, inside the bytes reserved at init ----
    std::vector<size_t> offs((size_t)n * 4, 0), slots;
    std::vector<StageMap::Item> copy; // what has to be brought in (offsets into d_in)
    size_t used = 0;
    if (new_f1) {
        StageMap st;
        st.align = 256;
        for (uint32_t i = 0; i < n; ++i) {
            offs[4 * (size_t)i + 0] = nnz[i] ? st.add(f1_idx_or_null[i], (size_t)nnz[i] * 8) : 0;
            offs[4 * (size_t)i + 1] = nnz[i] ? st.add(f1_vals_or_null[i], (size_t)nnz[i] * 32) : 0;
            offs[4 * (size_t)i + 2] = st.add(f2[i], N * 32);
            offs[4 * (size_t)i + 3] = st.add(f3[i], N * 32);
        }
        copy = st.items;
        used = st.bytes;
        slots = dense_slots_of(offs, nnz);
    } else {
        slots = bp->dense_slots;
        used = bp->in_used;
        std::map<const void *, size_t> where;
        size_t taken = 0;
        for (uint32_t i = 0; i < n; ++i) {
            offs[4 * (size_t)i + 0] = reinterpret_cast<const char *>(bp->rec[i].idx) - bp->d_in;
            offs[4 * (size_t)i + 1] = reinterpret_cast<const char *>(bp->rec[i].vals) - bp->d_in;
            for (int k = 2; k < 4; ++k) {
                const void *src = (k == 2 ? f2 : f3)[i];
                auto it = where.find(src);
                if (it == where.end()) {
                    if (taken == slots.size()) { // more distinct arrays than the layout in force has places for: behind it, while the reserve lasts
                        slots.push_back(used);
                        used += slot;
                    }
                    it = where.emplace(src, slots[taken++]).first;
                    copy.push_back({src, N * 32, it->second});
                }
                offs[4 * (size_t)i + k] = it->second;
            }
        }
    }
    if (used > bp->in_cap)
        return sc_internal_fail(SC_ERR_BAD_ARG, "the layer's distinct arrays take %zu bytes of the handle's copy, init reserved %zu: build a new handle", used, bp->in_cap);
    char *const d_up = bp->d_buf + 2 * bp->work_bytes;
    std::vector<scd::GkrBatchInst> rec(n), chk(n);
    for (uint32_t i = 0; i < n; ++i) {
        scd::GkrBatchInst &r = rec[i], &c = chk[i];
        r.nnz = c.nnz = nnz[i];
        r.idx = reinterpret_cast<const uint64_t *>(bp->d_in + offs[4 * (size_t)i + 0]);
        r.vals = reinterpret_cast<const uint4 *>(bp->d_in + offs[4 * (size_t)i + 1]);
        r.f2 = reinterpret_cast<const uint4 *>(bp->d_in + offs[4 * (size_t)i + 2]);
        r.f3 = reinterpret_cast<const uint4 *>(bp->d_in + offs[4 * (size_t)i + 3]);
        r.g = c.g = reinterpret_cast<const uint4 *>(d_up + bp->g_off + (size_t)i * dim * 32);
        c.idx = new_f1 ? f1_idx_or_null[i] : r.idx;
        c.vals = new_f1 ? reinterpret_cast<const uint4 *>(f1_vals_or_null[i]) : r.vals;
        c.f2 = reinterpret_cast<const uint4 *>(f2[i]);
        c.f3 = reinterpret_cast<const uint4 *>(f3[i]);
    }
    const size_t rec_bytes = (size_t)n * sizeof(scd::GkrBatchInst), g_bytes = (size_t)n * dim * 32;
    size_t n_items = 0;
    uint64_t blocks = 0;
    auto upload_and_check = [&]() -> int { // device arrays: the staging image, the index check
        DeviceGate gate_(bp->device);
        HIP_TRY(hipSetDevice(bp->device));
        HIP_TRY(hipDeviceSynchronize()); // the inputs' producers are waited for, as at init
        std::memset(bp->h_pin + bp->nl_flag_off, 0, bp->nl_chk_off - bp->nl_flag_off);
        std::memcpy(bp->h_pin + bp->nl_chk_off, chk.data(), rec_bytes);
        std::memcpy(bp->h_pin + bp->nl_rec_off, rec.data(), rec_bytes);
        for (uint32_t i = 0; i < n; ++i) std::memcpy(bp->h_pin + bp->nl_g_off + (size_t)i * dim * 32, g[i], (size_t)dim * 32);
        if (g2) {
            for (uint32_t i = 0; i < n; ++i) std::memcpy(bp->h_pin + bp->nl_g2_off + (size_t)i * dim * 32, g2[i], (size_t)dim * 32);
            std::memcpy(bp->h_pin + bp->nl_coef_off, coef, (size_t)n * 64);
        }
        scd::GkrRestageItem *items = reinterpret_cast<scd::GkrRestageItem *>(bp->h_pin + bp->nl_item_off);
        auto item = [&](const void *src, size_t dst_off, size_t bytes) {
            items[n_items++] = {src, dst_off, bytes, blocks};
            blocks += (bytes + scd::kGkrRestageChunk - 1) / scd::kGkrRestageChunk;
        };
        for (const StageMap::Item &it : copy) item(it.src, (size_t)(bp->d_in - bp->d_buf) + it.off, it.bytes);
        item(d_up + bp->nl_rec_off, 2 * bp->work_bytes + bp->rec_off, rec_bytes);
        item(d_up + bp->nl_g_off, 2 * bp->work_bytes + bp->g_off, g_bytes);
        if (g2) {
            item(d_up + bp->nl_g2_off, 2 * bp->work_bytes + bp->g2_off, g_bytes);
            item(d_up + bp->nl_coef_off, 2 * bp->work_bytes + bp->coef_off, (size_t)n * 64);
        }
        HIP_TRY(hipMemcpyAsync(d_up + bp->nl_flag_off, bp->h_pin + bp->nl_flag_off, bp->nl_item_off + n_items * sizeof(scd::GkrRestageItem) - bp->nl_flag_off, hipMemcpyHostToDevice, bp->stream));
        // new device-resident wiring: an index out of range is found here, over the caller's arrays -- nothing of the handle's has been written
        if (new_f1)
            if (int rc = gkr_check_idx_on_device(reinterpret_cast<const scd::GkrBatchInst *>(d_up + bp->nl_chk_off), n, dim, bp->h_pin, d_up, bp->nl_flag_off, bp->stream)) return rc;
        return SC_OK;
    };
    if (dev_in)
        if (int rc = upload_and_check()) return rc;
    // ---- from here on the handle is the new layer's ----
    bp->round = 0;
    bp->exhausted = false;
    bp->randomness.clear();
    bp->nnz = nnz;
    bp->nnz_max = nnz_max;
    bp->rec = rec;
    for (uint32_t i = 0; i < n; ++i) std::memcpy(&bp->g[(size_t)i * dim], g[i], (size_t)dim * 32);
    bp->two_point = g2 != nullptr;
    if (g2) {
        for (uint32_t i = 0; i < n; ++i) std::memcpy(&bp->g2[(size_t)i * dim], g2[i], (size_t)dim * 32);
        std::memcpy(bp->coef.data(), coef, (size_t)n * 64);
        std::memcpy(bp->h_pin + bp->g2_off, bp->g2.data(), g_bytes);
        std::memcpy(bp->h_pin + bp->coef_off, bp->coef.data(), (size_t)n * 64);
    }
    bp->dense_slots = slots;
    bp->in_used = used;
    std::memcpy(bp->h_pin + bp->rec_off, rec.data(), rec_bytes);
    std::memcpy(bp->h_pin + bp->g_off, bp->g.data(), g_bytes);
    auto stage_on_stream = [&]() -> int {
        if (dev_in) {
            HIP_TRY(scd::launch_batch_gkr_restage(reinterpret_cast<const scd::GkrRestageItem *>(d_up + bp->nl_item_off), (uint32_t)n_items, blocks, bp->d_buf, bp->stream));
        } else {
            for (const StageMap::Item &it : copy) HIP_TRY(hipMemcpyAsync(bp->d_in + it.off, it.src, it.bytes, hipMemcpyHostToDevice, bp->stream));
            HIP_TRY(hipMemcpyAsync(d_up + bp->rec_off, bp->h_pin + bp->rec_off, bp->u_off - bp->rec_off, hipMemcpyHostToDevice, bp->stream));
        }
        if (int rc = areas_phase_one(bp)) return rc;
        HIP_TRY(hipStreamSynchronize(bp->stream)); // nothing of the caller's is read after the call returns
        return SC_OK;
    };
    auto stage = [&]() -> int {
        {
            DeviceGate gate_(bp->device);
            HIP_TRY(hipSetDevice(bp->device));
            if (int rc = stage_on_stream()) return rc;
        }
        return bp->work_areas() ? SC_OK : serial_phase_one(bp);
    };
    if (int rc = stage()) {
        bp->exhausted = true;
        return rc;
    }
    if (bp->work_areas()) scd::plan_hit(scd::kPlanBatchGkrNextLayer);
    return SC_OK;
}
} // namespace
