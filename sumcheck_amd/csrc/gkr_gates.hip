// gkr_gates.hip -- the GATE form of the GKR batch handle: sc_gkr_gates_init_batch, sc_gkr_gates_next_batch, and what
// sc_gkr_batch_prove_round / _finish / _state / _reset / _free do on a handle built here (gkr_batch_rounds.hip forwards them).
// A layer of multiplication and addition gates (XZZPS19),
//     W_out[z] = sum over MUL of v f2[x] f3[y]  +  sum over ADD of v (f2[x] + f3[y]),
// claimed at one point g or as alpha W(g) + beta W(g2), E(z) = eq(g, z) or alpha eq(g, z) + beta eq(g2, z):
//   phase one  a sumcheck over x of f2(x) H1(x) + H2(x),  H1[x] = sum_MUL E[z] v f3[y] + sum_ADD E[z] v,  H2[x] = sum_ADD E[z] v f3[y];
//   phase two  a sumcheck over y of f3(y) T1(y) + T2(y),  T1[y] = f2(u) sum_MUL E[z] eq(u,x) v + sum_ADD E[z] eq(u,x) v,  T2[y] = f2(u) sum_ADD E[z] eq(u,x) v.
// Two plans, chosen when the handle is built, same bits (every output is a canonical element):
//   batch.gkr_gates_one_block  dim <= 9, each list <= 64 x 2^dim, policy "batch" != 0 and "gkr_gates_fused" = 1: two work areas of
//                              k_batch_round's layout with THREE tables (t0 t1 + t2: K = 2, D = 3, coefficients one) that
//                              k_batch_gkr_gates_phase<1|2> fill (kernels_batch_gkr_gates.hip); per round call one upload of the challenges,
//                              one launch of k_batch_round (call dim: the phase kernel in front of it), one copy back, one synchronisation;
//   batch.gkr_gates_composed   every other shape: an inner sc_gkr_batch_prover of 3 n multiplication-only instances -- (MUL, f2, f3),
//                              (ADD, f2, 1), (ADD, 1, f3) per instance, the table of ones made once -- on whatever plan it chooses for itself;
//                              challenges are replicated three times, the three messages added on the host, and finish forms f2(u), f3(v)
//                              and a0 a2 + b0 b2 + c0 c2 from the inner final values.
// The handle copies every input once per distinct (pointer, size); nothing of the caller's is read after init or next returns.
#include "batch_slices.hpp"
#include "prover_internal.hpp"

struct GkrGates {
    int device = 0;
    uint32_t n = 0, dim = 0, round = 0; // round: round calls answered so far, 0 .. 2 dim
    bool exhausted = false, fused = false, two_point = false, dev_in = false;
    std::vector<std::vector<sch::Fr>> randomness; // per challenge received (u, then v): n elements, or ONE for a shared challenge
    hipStream_t stream = nullptr;
    // the index check of device-resident lists: 2 n records (mul, add per instance) and 2 n flags, device and pinned
    char *d_chk = nullptr, *h_chk = nullptr;
    size_t chk_flag_off = 0;
    // ---- batch.gkr_gates_composed ----
    sc_gkr_batch_prover *inner = nullptr;
    std::vector<sch::Fr> ones;  // host inputs: 2^dim ones
    char *d_ones = nullptr;     // device inputs: the same table in device memory
    // ---- batch.gkr_gates_one_block ----
    char *d_buf = nullptr; // device, ONE allocation: area A | area B | upload image (matrices | records | g | g2 | coefficients | challenges | messages | f2(u) | finals | restage items) | inputs (lists | f2, f3)
    char *h_pin = nullptr; // pinned: the upload image
    size_t work_bytes = 0, w_off = 0, rec_off = 0, g_off = 0, g2_off = 0, coef_off = 0, u_off = 0, msg_off = 0, f2u_off = 0, exp_off = 0, item_off = 0, pin_bytes = 0;
    size_t in_cap = 0, lists_used = 0; // d_in: the bytes reserved at init (never more); the bytes of the four list arrays in the layout in force, at its front
    char *d_in = nullptr;               // (inside d_buf) the handle's copy of the inputs: the lists, behind them f2 / f3, every distinct array once
    std::vector<scd::GkrGatesInst> rec;
    SharedMeta s; // t0 t1 + t2: both phases
    int points() const { return two_point ? 2 : 1; }
};

namespace {

struct GatesIn { // the caller's arrays of an init or next call
    uint32_t n, dim;
    const uint64_t *const *mul_idx, *const *mul_vals;
    const uint64_t *mul_nnz;
    const uint64_t *const *add_idx, *const *add_vals;
    const uint64_t *add_nnz;
    const uint64_t *const *f2, *const *f3, *const *g, *const *g2;
    const uint64_t *coef;
    bool dev;
};

// instance i, in gkr_check_instance's order and texts with the list's own name where that says f1: the sizes, the null pointers, g, the
// host-resident indices of mul and then of add; behind them the second point (no HIP call)
int check_instance(const GatesIn &in, uint32_t i) {
    const struct {
        const char *name;
        const uint64_t *idx, *vals;
        uint64_t nnz;
    } lists[2] = {{"mul", in.mul_idx[i], in.mul_vals[i], in.mul_nnz[i]}, {"add", in.add_idx[i], in.add_vals[i], in.add_nnz[i]}};
    for (const auto &l : lists)
        if (l.nnz >= (1ULL << 32)) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: %s nnz too large", i, l.name);
    for (const auto &l : lists)
        if (l.nnz && (!l.idx || !l.vals)) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: null argument", i);
    if (!in.f2[i] || !in.f3[i] || !in.g[i]) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: null argument", i);
    for (uint32_t k = 0; k < in.dim; ++k) {
        sch::Fr e;
        std::memcpy(&e, in.g[i] + 4 * (size_t)k, 32);
        if (sch::geq_p(e)) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: g[%u] is not a canonical field element", i, k);
    }
    if (!in.dev)
        for (const auto &l : lists)
            for (uint64_t k = 0; k < l.nnz; ++k)
                if ((l.idx[k] >> (3 * in.dim)) != 0) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: %s index %llu out of range", i, l.name, (unsigned long long)k);
    if (!in.g2) return SC_OK;
    if (!in.g2[i]) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: null argument", i);
    for (uint32_t k = 0; k < in.dim; ++k) {
        sch::Fr e;
        std::memcpy(&e, in.g2[i] + 4 * (size_t)k, 32);
        if (sch::geq_p(e)) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: g2 is not canonical", i);
    }
    for (uint32_t k = 0; k < 2; ++k) {
        sch::Fr e;
        std::memcpy(&e, in.coef + 4 * ((size_t)i * 2 + k), 32);
        if (sch::geq_p(e)) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: coefficient is not canonical", i);
    }
    return SC_OK;
}

// device-resident lists: an index with a bit at or above 3 dim, over the CALLER's arrays, in front of anything that follows the indices
// or writes the handle (the caller holds the device gate)
int check_idx_on_device(GkrGates *G, const GatesIn &in) {
    const uint32_t n = G->n;
    scd::GkrBatchInst *h = reinterpret_cast<scd::GkrBatchInst *>(G->h_chk);
    std::memset(G->h_chk, 0, G->chk_flag_off + (size_t)2 * n * 4);
    for (uint32_t i = 0; i < n; ++i) {
        h[2 * (size_t)i].idx = in.mul_idx[i];
        h[2 * (size_t)i].nnz = in.mul_nnz[i];
        h[2 * (size_t)i + 1].idx = in.add_idx[i];
        h[2 * (size_t)i + 1].nnz = in.add_nnz[i];
    }
    HIP_TRY(hipMemcpyAsync(G->d_chk, G->h_chk, G->chk_flag_off + (size_t)2 * n * 4, hipMemcpyHostToDevice, G->stream));
    HIP_TRY(scd::launch_batch_gkr_idx_range(reinterpret_cast<const scd::GkrBatchInst *>(G->d_chk), 2 * n, G->dim, reinterpret_cast<uint32_t *>(G->d_chk + G->chk_flag_off), G->stream));
    HIP_TRY(hipMemcpyAsync(G->h_chk + G->chk_flag_off, G->d_chk + G->chk_flag_off, (size_t)2 * n * 4, hipMemcpyDeviceToHost, G->stream));
    HIP_TRY(hipStreamSynchronize(G->stream));
    const uint32_t *fl = reinterpret_cast<const uint32_t *>(G->h_chk + G->chk_flag_off);
    for (uint32_t k = 0; k < 2 * n; ++k)
        if (fl[k]) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: %s has an index out of range", k / 2, k & 1u ? "add" : "mul");
    return SC_OK;
}

// the three multiplication-only instances per instance, as the inner handle's argument arrays
struct Tripled {
    std::vector<const uint64_t *> idx, vals, f2, f3, g, g2;
    std::vector<uint64_t> nnz, coef;
    Tripled(const GatesIn &in, bool wiring, const uint64_t *ones) {
        const uint32_t n = in.n;
        for (uint32_t i = 0; i < n; ++i) {
            if (wiring) {
                idx.insert(idx.end(), {in.mul_idx[i], in.add_idx[i], in.add_idx[i]});
                vals.insert(vals.end(), {in.mul_vals[i], in.add_vals[i], in.add_vals[i]});
                nnz.insert(nnz.end(), {in.mul_nnz[i], in.add_nnz[i], in.add_nnz[i]});
            }
            f2.insert(f2.end(), {in.f2[i], in.f2[i], ones});
            f3.insert(f3.end(), {in.f3[i], ones, in.f3[i]});
            g.insert(g.end(), 3, in.g[i]);
            if (in.g2) {
                g2.insert(g2.end(), 3, in.g2[i]);
                for (int k = 0; k < 3; ++k) coef.insert(coef.end(), in.coef + 8 * (size_t)i, in.coef + 8 * (size_t)i + 8);
            }
        }
    }
};

// the fused plan's layout of the caller's arrays in the handle's copy: the four lists of every instance at the front, f2 / f3 behind them,
// every distinct (pointer, size) once.  Kept wiring: the lists stay where they are (lists_kept bytes) and only f2 / f3 are laid out again.
struct Layout {
    StageMap lists, dense;
    std::vector<size_t> offs; // per instance: mul_idx, mul_vals, add_idx, add_vals, f2, f3 (offsets into d_in)
    size_t lists_bytes = 0, used = 0;
    Layout(const GatesIn &in, bool wiring, size_t lists_kept) {
        const size_t N = (size_t)1 << in.dim;
        lists.align = dense.align = 256;
        offs.assign((size_t)in.n * 6, 0);
        if (wiring)
            for (uint32_t i = 0; i < in.n; ++i) {
                size_t *o = &offs[6 * (size_t)i];
                o[0] = in.mul_nnz[i] ? lists.add(in.mul_idx[i], (size_t)in.mul_nnz[i] * 8) : 0;
                o[1] = in.mul_nnz[i] ? lists.add(in.mul_vals[i], (size_t)in.mul_nnz[i] * 32) : 0;
                o[2] = in.add_nnz[i] ? lists.add(in.add_idx[i], (size_t)in.add_nnz[i] * 8) : 0;
                o[3] = in.add_nnz[i] ? lists.add(in.add_vals[i], (size_t)in.add_nnz[i] * 32) : 0;
            }
        lists_bytes = wiring ? lists.bytes : lists_kept;
        dense.base = lists_bytes;
        for (uint32_t i = 0; i < in.n; ++i) {
            offs[6 * (size_t)i + 4] = dense.add(in.f2[i], N * 32);
            offs[6 * (size_t)i + 5] = dense.add(in.f3[i], N * 32);
        }
        used = lists_bytes + dense.bytes;
    }
};

void set_points(GkrGates *G, const GatesIn &in) { // g, g2 and the coefficients into the upload image
    const uint32_t n = G->n, dim = G->dim;
    G->two_point = in.g2 != nullptr;
    for (uint32_t i = 0; i < n; ++i) {
        std::memcpy(G->h_pin + G->g_off + (size_t)i * dim * 32, in.g[i], (size_t)dim * 32);
        if (in.g2) std::memcpy(G->h_pin + G->g2_off + (size_t)i * dim * 32, in.g2[i], (size_t)dim * 32);
    }
    if (in.g2) std::memcpy(G->h_pin + G->coef_off, in.coef, (size_t)n * 64);
}

// the fused plan: the caller's arrays into the handle's copy, the records and points up, phase one's tables -- on the handle's stream,
// behind every check; one synchronisation (the caller holds the device gate)
int fused_stage(GkrGates *G, const GatesIn &in, const Layout &L, bool wiring) {
    const uint32_t n = G->n, dim = G->dim;
    char *const d_up = G->d_buf + 2 * G->work_bytes;
    if (in.dev) { // device arrays: ONE launch of k_batch_gkr_restage brings all of them in (sc_gkr_layer_next_batch's way)
        scd::GkrRestageItem *items = reinterpret_cast<scd::GkrRestageItem *>(G->h_pin + G->item_off);
        size_t n_items = 0;
        uint64_t blocks = 0;
        auto item = [&](const StageMap::Item &it) { // (it.off + it.bytes <= L.used <= in_cap: inside the handle's copy)
            items[n_items++] = {it.src, (uint64_t)(G->d_in - G->d_buf) + it.off, it.bytes, blocks};
            blocks += (it.bytes + scd::kGkrRestageChunk - 1) / scd::kGkrRestageChunk;
        };
        if (wiring)
            for (const StageMap::Item &it : L.lists.items) item(it);
        for (const StageMap::Item &it : L.dense.items) item(it);
        HIP_TRY(hipMemcpyAsync(d_up + G->item_off, items, n_items * sizeof(scd::GkrRestageItem), hipMemcpyHostToDevice, G->stream));
        HIP_TRY(scd::launch_batch_gkr_restage(reinterpret_cast<const scd::GkrRestageItem *>(d_up + G->item_off), (uint32_t)n_items, blocks, G->d_buf, G->stream));
    } else {
        if (wiring)
            for (const StageMap::Item &it : L.lists.items) HIP_TRY(hipMemcpyAsync(G->d_in + it.off, it.src, it.bytes, hipMemcpyHostToDevice, G->stream));
        for (const StageMap::Item &it : L.dense.items) HIP_TRY(hipMemcpyAsync(G->d_in + it.off, it.src, it.bytes, hipMemcpyHostToDevice, G->stream));
    }
    G->lists_used = L.lists_bytes;
    for (uint32_t i = 0; i < n; ++i) {
        scd::GkrGatesInst &r = G->rec[i];
        const size_t *o = &L.offs[6 * (size_t)i];
        if (wiring) {
            r.mul_nnz = in.mul_nnz[i];
            r.add_nnz = in.add_nnz[i];
            r.mul_idx = reinterpret_cast<const uint64_t *>(G->d_in + o[0]);
            r.mul_vals = reinterpret_cast<const uint4 *>(G->d_in + o[1]);
            r.add_idx = reinterpret_cast<const uint64_t *>(G->d_in + o[2]);
            r.add_vals = reinterpret_cast<const uint4 *>(G->d_in + o[3]);
        }
        r.f2 = reinterpret_cast<const uint4 *>(G->d_in + o[4]);
        r.f3 = reinterpret_cast<const uint4 *>(G->d_in + o[5]);
        r.g = reinterpret_cast<const uint4 *>(d_up + G->g_off + (size_t)i * dim * 32);
    }
    std::memcpy(G->h_pin + G->rec_off, G->rec.data(), (size_t)n * sizeof(scd::GkrGatesInst));
    set_points(G, in);
    HIP_TRY(hipMemcpyAsync(d_up, G->h_pin, G->u_off, hipMemcpyHostToDevice, G->stream));
    scd::BatchGkrGatesArgs A;
    std::memset(&A, 0, sizeof(A));
    A.inst = reinterpret_cast<const scd::GkrGatesInst *>(d_up + G->rec_off);
    A.work_a = reinterpret_cast<int32_t *>(G->d_buf);
    A.n = n;
    A.dim = dim;
    A.g2 = reinterpret_cast<const uint4 *>(d_up + G->g2_off);
    A.coef = reinterpret_cast<const uint4 *>(d_up + G->coef_off);
    HIP_TRY(scd::launch_batch_gkr_gates_phase(1, A, G->stream, G->points()));
    HIP_TRY(hipStreamSynchronize(G->stream)); // nothing of the caller's is read after the call returns
    return SC_OK;
}

void rewind(GkrGates *G) {
    G->round = 0;
    G->exhausted = false;
    G->randomness.clear();
}

} // namespace

void gkr_gates_destroy(GkrGates *G) {
    if (!G) return;
    if (G->inner) sc_gkr_batch_prover_free(G->inner);
    {
        DeviceGate gate_(G->device);
        (void)hipSetDevice(G->device);
        if (G->stream) (void)hipStreamSynchronize(G->stream);
        if (G->d_buf) (void)hipFree(G->d_buf);
        if (G->d_chk) (void)hipFree(G->d_chk);
        if (G->d_ones) (void)hipFree(G->d_ones);
        if (G->h_pin) (void)hipHostFree(G->h_pin);
        if (G->h_chk) (void)hipHostFree(G->h_chk);
        if (G->stream) (void)hipStreamDestroy(G->stream);
        (void)hipGetLastError();
    }
    delete G;
}

extern "C" int sc_gkr_gates_init_batch(uint32_t n, uint32_t dim, const uint64_t *const *mul_idx, const uint64_t *const *mul_vals, const uint64_t *mul_nnz, const uint64_t *const *add_idx,
                                       const uint64_t *const *add_vals, const uint64_t *add_nnz, const uint64_t *const *f2, const uint64_t *const *f3, const uint64_t *const *g,
                                       const uint64_t *const *g2_or_null, const uint64_t *coef_or_null, uint32_t flags, sc_gkr_batch_prover **out) {
    // ---- everything the host can check, before any HIP call (the lowest failing instance decides) ----
    if (out) *out = nullptr;
    if (!mul_idx || !mul_vals || !mul_nnz || !add_idx || !add_vals || !add_nnz || !f2 || !f3 || !g || !out) return sc_internal_fail(SC_ERR_BAD_ARG, "null argument");
    if ((g2_or_null == nullptr) != (coef_or_null == nullptr)) return sc_internal_fail(SC_ERR_BAD_ARG, "g2 and coef come together (two points) or are both NULL (one point)");
    if (n == 0) return sc_internal_fail(SC_ERR_BAD_ARG, "n == 0: a batch handle holds at least one instance");
    if (dim == 0) return sc_internal_fail(SC_ERR_CONSTANT_POLY, "instance 0: Attempt to prove a constant.");
    if (dim > 21) return sc_internal_fail(SC_ERR_BAD_ARG, "instance 0: dim %u: 3*dim index bits do not fit 64-bit indices", dim);
    if (n > 0xffffffffu / 3) return sc_internal_fail(SC_ERR_BAD_ARG, "n %u: a gate handle holds at most %u instances", n, 0xffffffffu / 3);
    const bool dev_in = flags & SC_TABLES_ON_DEVICE;
    const GatesIn in = {n, dim, mul_idx, mul_vals, mul_nnz, add_idx, add_vals, add_nnz, f2, f3, g, g2_or_null, coef_or_null, dev_in};
    uint64_t nnz_max = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (int rc = check_instance(in, i)) return rc;
        nnz_max = std::max(nnz_max, std::max(mul_nnz[i], add_nnz[i]));
    }
    if (sc_device_count() <= 0) return sc_internal_fail(SC_ERR_HIP, "no HIP device visible: libsumcheck_hip has no CPU fallback");
    GkrGates *G = new (std::nothrow) GkrGates();
    if (!G) return sc_internal_fail(SC_ERR_OOM, "out of host memory");
    G->device = sc_internal_device_ref();
    G->n = n;
    G->dim = dim;
    G->dev_in = dev_in;
    G->two_point = g2_or_null != nullptr;
    const size_t N = (size_t)1 << dim;
    auto build = [&]() -> int {
        const uint32_t offs[3] = {0, 2, 3}, idx3[3] = {0, 1, 2};
        const uint64_t *no_tables[3] = {nullptr, nullptr, nullptr};
        sch::Fr two_ones[2] = {sch::kOne, sch::kOne};
        sc_poly_desc d;
        std::memset(&d, 0, sizeof(d));
        d.num_vars = dim;
        d.max_multiplicands = 2;
        d.n_products = 2;
        d.coeffs = two_ones[0].l;
        d.prod_offsets = offs;
        d.prod_indices = idx3;
        d.n_tables = 3;
        d.tables = no_tables;
        build_shared(&d, G->s);
        G->s.unit.push_back(unit_matrix(2, 3));
        G->s.unit.push_back(unit_matrix(1, 3));
        G->fused = scd::policy(scd::kPolGkrGatesFused) != 0 && scd::policy(scd::kPolBatch) != 0 && scd::gkr_batch_shape_fits(dim, nnz_max) && G->s.fits_args &&
                   scd::batch_shape_fits(dim, 3, 2, 3, 2);
        G->chk_flag_off = round_up((size_t)2 * n * sizeof(scd::GkrBatchInst), 256);
        {
            DeviceGate gate_(G->device);
            HIP_TRY(hipSetDevice(G->device));
            HIP_TRY(hipStreamCreateWithFlags(&G->stream, hipStreamNonBlocking));
            if (dev_in) {
                HIP_TRY(hipMalloc(reinterpret_cast<void **>(&G->d_chk), G->chk_flag_off + (size_t)2 * n * 4));
                HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&G->h_chk), G->chk_flag_off + (size_t)2 * n * 4, hipHostMallocDefault));
                HIP_TRY(hipDeviceSynchronize()); // the inputs' producers are waited for, as a copy on their stream would
                if (int rc = check_idx_on_device(G, in)) return rc;
            }
            if (G->fused) {
                const Layout L(in, true, 0);
                G->in_cap = L.used;
                G->work_bytes = round_up((size_t)n * 3 * 2 * (scd::kBatchRoundSlotBytes << dim), 256);
                G->w_off = 0;
                G->rec_off = G->w_off + round_up((size_t)G->s.w_elems * 32, 256);
                G->g_off = G->rec_off + round_up((size_t)n * sizeof(scd::GkrGatesInst), 256);
                G->g2_off = G->g_off + round_up((size_t)n * dim * 32, 256);
                G->coef_off = G->g2_off + round_up((size_t)n * dim * 32, 256);
                G->u_off = G->coef_off + round_up((size_t)n * 64, 256);
                G->msg_off = G->u_off + round_up((size_t)2 * dim * n * 32, 256);
                G->f2u_off = G->msg_off + round_up((size_t)n * 3 * 32, 256);
                G->exp_off = G->f2u_off + round_up((size_t)n * 32, 256);
                G->item_off = G->exp_off + round_up((size_t)n * 3 * 32, 256);
                G->pin_bytes = G->item_off + round_up((size_t)n * 6 * sizeof(scd::GkrRestageItem), 256); // (every array of every instance)
                HIP_TRY(hipMalloc(reinterpret_cast<void **>(&G->d_buf), 2 * G->work_bytes + G->pin_bytes + G->in_cap));
                G->d_in = G->d_buf + 2 * G->work_bytes + G->pin_bytes;
                HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&G->h_pin), G->pin_bytes, hipHostMallocDefault));
                std::memset(G->h_pin, 0, G->pin_bytes);
                instance_weights(G->s, two_ones[0].l, reinterpret_cast<sch::Fr *>(G->h_pin + G->w_off));
                G->rec.assign(n, scd::GkrGatesInst());
                return fused_stage(G, in, L, true);
            }
            G->ones.assign(N, sch::kOne);
            if (dev_in) {
                HIP_TRY(hipMalloc(reinterpret_cast<void **>(&G->d_ones), N * 32));
                HIP_TRY(hipMemcpy(G->d_ones, G->ones.data(), N * 32, hipMemcpyHostToDevice));
            }
        }
        const Tripled T(in, true, dev_in ? reinterpret_cast<const uint64_t *>(G->d_ones) : G->ones[0].l);
        if (in.g2) return sc_gkr_two_point_init_batch(3 * n, dim, T.idx.data(), T.vals.data(), T.nnz.data(), T.f2.data(), T.f3.data(), T.g.data(), T.g2.data(), T.coef.data(), flags, &G->inner);
        return sc_gkr_batch_prover_init(3 * n, dim, T.idx.data(), T.vals.data(), T.nnz.data(), T.f2.data(), T.f3.data(), T.g.data(), flags, &G->inner);
    };
    int rc = build();
    if (rc == SC_OK) {
        *out = gkr_gates_wrap(G);
        if (*out) return SC_OK;
        rc = sc_internal_fail(SC_ERR_OOM, "out of host memory");
    }
    const std::string why = sc_last_error(); // (the frees below may run library calls of their own)
    gkr_gates_destroy(G);
    return sc_internal_fail(rc, "%s", why.c_str());
}

int gkr_gates_prove_round(GkrGates *G, const uint64_t *r_or_null, uint32_t r_shared, uint64_t *out_evals) {
    if (!out_evals) return sc_internal_fail(SC_ERR_BAD_ARG, "null argument");
    // validation, sc_gkr_batch_prove_round's precedence; every check comes before the first change to the handle
    if (G->exhausted) return sc_internal_fail(SC_ERR_NOT_ACTIVE, "Prover is not active");
    if (r_or_null && G->round == 0) return sc_internal_fail(SC_ERR_FIRST_ROUND_HAS_MSG, "first round should be prover first.");
    if (!r_or_null && G->round > 0) return sc_internal_fail(SC_ERR_MISSING_MSG, "verifier message is empty");
    if (G->round + 1 > 2 * G->dim) return sc_internal_fail(SC_ERR_NOT_ACTIVE, "Prover is not active");
    std::vector<sch::Fr> chal;
    if (r_or_null)
        if (int rc = take_challenges(G->n, r_or_null, r_shared, chal)) return rc;
    const uint32_t n = G->n, dim = G->dim, t = G->round, phase = t / dim, r = t % dim;
    if (G->fused) {
        const SharedMeta &s = G->s;
        DeviceGate gate_(G->device);
        HIP_TRY(hipSetDevice(G->device));
        char *const d_up = G->d_buf + 2 * G->work_bytes;
        if (r_or_null) { // challenge t - 1 of every instance -> the handle's device copy, [challenge][instance]; a shared one is expanded
            const size_t off = G->u_off + (size_t)(t - 1) * n * 32;
            sch::Fr *h = reinterpret_cast<sch::Fr *>(G->h_pin + off);
            for (uint32_t i = 0; i < n; ++i) h[i] = challenge_of(chal, i);
            HIP_TRY(hipMemcpyAsync(d_up + off, h, (size_t)n * 32, hipMemcpyHostToDevice, G->stream));
        }
        if (t == dim) { // the phase change: f2(u), T1, T2, f3 -> area B
            scd::BatchGkrGatesArgs P;
            std::memset(&P, 0, sizeof(P));
            P.inst = reinterpret_cast<const scd::GkrGatesInst *>(d_up + G->rec_off);
            P.work_a = reinterpret_cast<int32_t *>(G->d_buf);
            P.work_b = reinterpret_cast<int32_t *>(G->d_buf + G->work_bytes);
            P.u = reinterpret_cast<const uint4 *>(d_up + G->u_off);
            P.f2u = reinterpret_cast<uint4 *>(d_up + G->f2u_off);
            P.n = n;
            P.dim = dim;
            P.g2 = reinterpret_cast<const uint4 *>(d_up + G->g2_off);
            P.coef = reinterpret_cast<const uint4 *>(d_up + G->coef_off);
            HIP_TRY(scd::launch_batch_gkr_gates_phase(2, P, G->stream, G->points()));
        }
        scd::BatchRoundArgs A;
        std::memset(&A, 0, sizeof(A));
        A.work = reinterpret_cast<int32_t *>(G->d_buf + (phase ? G->work_bytes : 0));
        A.Wm = reinterpret_cast<const uint4 *>(d_up + G->w_off);
        A.w_stride = 0; // coefficients of one: the same matrices for every instance
        A.chal = r ? reinterpret_cast<const uint4 *>(d_up + G->u_off + (size_t)(t - 1) * n * 32) : nullptr;
        A.chal_shared = 0;
        A.out = reinterpret_cast<uint4 *>(d_up + G->msg_off);
        A.n = n;
        A.n_tables = 3;
        A.nv = dim;
        A.round = r;
        A.n_combos = s.n_combos;
        A.K = 2;
        A.D = 3;
        HIP_TRY(scd::launch_batch_round(A, s.combo, s.fin, G->stream));
        scd::plan_hit(scd::kPlanBatchGkrGatesOneBlock);
        HIP_TRY(hipMemcpyAsync(G->h_pin + G->msg_off, d_up + G->msg_off, (size_t)n * 96, hipMemcpyDeviceToHost, G->stream));
        HIP_TRY(hipStreamSynchronize(G->stream));
        std::memcpy(out_evals, G->h_pin + G->msg_off, (size_t)n * 96);
    } else {
        // the inner handle is where this one is (every call that moves one moves the other): its own checks have nothing left to refuse
        std::vector<sch::Fr> chal3;
        if (r_or_null && !r_shared) {
            chal3.resize((size_t)3 * n);
            for (uint32_t i = 0; i < n; ++i) chal3[3 * (size_t)i] = chal3[3 * (size_t)i + 1] = chal3[3 * (size_t)i + 2] = chal[i];
        }
        std::vector<sch::Fr> msg((size_t)3 * n * 3);
        if (int rc = sc_gkr_batch_prove_round(G->inner, r_or_null ? (r_shared ? r_or_null : chal3[0].l) : nullptr, r_shared, msg[0].l)) {
            G->exhausted = true; // (the inner handle may have moved part of the way: the handle needs a reset)
            return rc;
        }
        scd::plan_hit(scd::kPlanBatchGkrGatesComposed);
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t e = 0; e < 3; ++e) {
                const sch::Fr sum = sch::add(sch::add(msg[(3 * (size_t)i + 0) * 3 + e], msg[(3 * (size_t)i + 1) * 3 + e]), msg[(3 * (size_t)i + 2) * 3 + e]);
                std::memcpy(out_evals + ((size_t)i * 3 + e) * 4, &sum, 32);
            }
    }
    if (r_or_null) G->randomness.push_back(std::move(chal));
    G->round++;
    return SC_OK;
}

int gkr_gates_finish(GkrGates *G, const uint64_t *r, uint32_t r_shared, uint64_t *out_uv_or_null, uint64_t *out_final_or_null) {
    if (!r) return sc_internal_fail(SC_ERR_BAD_ARG, "null argument");
    if (G->exhausted || G->round != 2 * G->dim) return sc_internal_fail(SC_ERR_NOT_ACTIVE, "finish needs a prover that has answered its last round");
    std::vector<sch::Fr> chal;
    if (int rc = take_challenges(G->n, r, r_shared, chal)) return rc;
    const uint32_t n = G->n, dim = G->dim;
    std::vector<sch::Fr> fin((size_t)n * 3); // f2(u), f3(v), f3(v) T1(v) + T2(v)
    if (G->fused) {
        DeviceGate gate_(G->device);
        HIP_TRY(hipSetDevice(G->device));
        char *const d_up = G->d_buf + 2 * G->work_bytes;
        const size_t off = G->u_off + (size_t)(2 * dim - 1) * n * 32;
        sch::Fr *h = reinterpret_cast<sch::Fr *>(G->h_pin + off);
        for (uint32_t i = 0; i < n; ++i) h[i] = challenge_of(chal, i);
        HIP_TRY(hipMemcpyAsync(d_up + off, h, (size_t)n * 32, hipMemcpyHostToDevice, G->stream));
        // area B's three tables, bound dim - 1 times, bound once more with v_{dim-1}: f3(v), T1(v), T2(v), canonical
        HIP_TRY(scd::launch_batch_rounds_export(reinterpret_cast<const int32_t *>(G->d_buf + G->work_bytes), 0, n, 3, dim, dim - 1, reinterpret_cast<const uint4 *>(d_up + off), 0u,
                                                reinterpret_cast<uint4 *>(d_up + G->exp_off), G->stream));
        HIP_TRY(hipMemcpyAsync(G->h_pin + G->f2u_off, d_up + G->f2u_off, G->exp_off - G->f2u_off + (size_t)n * 96, hipMemcpyDeviceToHost, G->stream));
        HIP_TRY(hipStreamSynchronize(G->stream));
        const sch::Fr *f2u = reinterpret_cast<const sch::Fr *>(G->h_pin + G->f2u_off), *ex = reinterpret_cast<const sch::Fr *>(G->h_pin + G->exp_off);
        for (uint32_t i = 0; i < n; ++i) {
            fin[3 * (size_t)i + 0] = f2u[i];
            fin[3 * (size_t)i + 1] = ex[3 * (size_t)i];
            fin[3 * (size_t)i + 2] = sch::add(sch::mul(ex[3 * (size_t)i], ex[3 * (size_t)i + 1]), ex[3 * (size_t)i + 2]);
        }
    } else {
        std::vector<sch::Fr> chal3, in3((size_t)3 * n * 3);
        if (!r_shared) {
            chal3.resize((size_t)3 * n);
            for (uint32_t i = 0; i < n; ++i) chal3[3 * (size_t)i] = chal3[3 * (size_t)i + 1] = chal3[3 * (size_t)i + 2] = chal[i];
        }
        if (int rc = sc_gkr_batch_prover_finish(G->inner, r_shared ? r : chal3[0].l, r_shared, nullptr, in3[0].l)) {
            G->exhausted = true;
            return rc;
        }
        // inner final values per instance: f1(g,u,v), f2(u), f2(u) f3(v).  a = (MUL, f2, f3), b = (ADD, f2, 1), c = (ADD, 1, f3)
        for (uint32_t i = 0; i < n; ++i) {
            const sch::Fr *a = &in3[(3 * (size_t)i + 0) * 3], *b = a + 3, *c = a + 6;
            fin[3 * (size_t)i + 0] = a[1];
            fin[3 * (size_t)i + 1] = c[2]; // 1(u) f3(v)
            fin[3 * (size_t)i + 2] = sch::add(sch::add(sch::mul(a[0], a[2]), sch::mul(b[0], b[2])), sch::mul(c[0], c[2]));
        }
    }
    G->randomness.push_back(std::move(chal));
    G->exhausted = true;
    if (out_uv_or_null)
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t j = 0; j < 2 * dim; ++j) std::memcpy(out_uv_or_null + ((size_t)i * 2 * dim + j) * 4, &challenge_of(G->randomness[j], i), 32);
    if (out_final_or_null) std::memcpy(out_final_or_null, fin.data(), fin.size() * 32);
    return SC_OK;
}

int gkr_gates_state(GkrGates *G, uint32_t instance, uint64_t *randomness, uint32_t *n_randomness, uint64_t *tables_out, uint32_t *round) {
    if (instance >= G->n) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: the handle holds %u instances", instance, G->n);
    if (tables_out) return sc_internal_fail(SC_ERR_BAD_ARG, "tables_out: a gate handle exports no tables (its plans hold different ones)");
    batch_state_head(G->randomness, instance, G->round, randomness, n_randomness, round);
    return SC_OK;
}

int gkr_gates_reset(GkrGates *G) {
    if (G->inner)
        if (int rc = sc_gkr_batch_prover_reset(G->inner)) return rc;
    // (fused: area A's depth 0 was never overwritten)
    rewind(G);
    return SC_OK;
}

// The handle onto the next layer's inputs, inside what init allocated.  Every check -- the host's, the capacity rule, the index check of
// new device-resident lists over the caller's arrays -- comes before the first write to the handle: an error leaves a proof in progress
// exactly where it was.  [A HIP error behind them leaves the handle exhausted until the next successful call.]
extern "C" int sc_gkr_gates_next_batch(sc_gkr_batch_prover *bp, const uint64_t *const *mul_idx_or_null, const uint64_t *const *mul_vals_or_null, const uint64_t *mul_nnz_or_null,
                                       const uint64_t *const *add_idx_or_null, const uint64_t *const *add_vals_or_null, const uint64_t *add_nnz_or_null, const uint64_t *const *f2,
                                       const uint64_t *const *f3, const uint64_t *const *g, const uint64_t *const *g2_or_null, const uint64_t *coef_or_null, uint32_t flags) {
    if (!bp) return sc_internal_fail(SC_ERR_BAD_ARG, "null prover");
    GkrGates *G = gkr_gates_of(bp);
    if (!G) return sc_internal_fail(SC_ERR_BAD_ARG, "the handle was not built by sc_gkr_gates_init_batch");
    if (!f2 || !f3 || !g) return sc_internal_fail(SC_ERR_BAD_ARG, "null argument");
    if ((g2_or_null == nullptr) != (coef_or_null == nullptr)) return sc_internal_fail(SC_ERR_BAD_ARG, "g2 and coef come together (two points) or are both NULL (one point)");
    const int given = (mul_idx_or_null != nullptr) + (mul_vals_or_null != nullptr) + (mul_nnz_or_null != nullptr) + (add_idx_or_null != nullptr) + (add_vals_or_null != nullptr) +
                      (add_nnz_or_null != nullptr);
    if (given != 0 && given != 6)
        return sc_internal_fail(SC_ERR_BAD_ARG, "mul_idx, mul_vals, mul_nnz, add_idx, add_vals and add_nnz come together (new wiring) or are all NULL (the handle's wiring is kept)");
    const bool wiring = given == 6, dev_in = flags & SC_TABLES_ON_DEVICE;
    if (dev_in != G->dev_in) return sc_internal_fail(SC_ERR_BAD_ARG, "flags: the handle was built over %s arrays, a later layer's are where init's were", G->dev_in ? "device" : "host");
    const uint32_t n = G->n, dim = G->dim;
    const std::vector<const uint64_t *> none(wiring ? 0 : n, nullptr);
    const std::vector<uint64_t> zero(wiring ? 0 : n, 0); // (kept wiring: nothing of the lists to check)
    const GatesIn in = {n, dim, wiring ? mul_idx_or_null : none.data(), wiring ? mul_vals_or_null : none.data(), wiring ? mul_nnz_or_null : zero.data(),
                        wiring ? add_idx_or_null : none.data(), wiring ? add_vals_or_null : none.data(), wiring ? add_nnz_or_null : zero.data(), f2, f3, g, g2_or_null, coef_or_null, dev_in};
    for (uint32_t i = 0; i < n; ++i) {
        if (int rc = check_instance(in, i)) return rc;
        if (wiring && G->fused)
            for (int k = 0; k < 2; ++k) {
                const uint64_t nnz = (k ? in.add_nnz : in.mul_nnz)[i];
                if (!scd::gkr_batch_shape_fits(dim, nnz))
                    return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: %s nnz %llu is beyond the limit of plan batch.gkr_gates_one_block, 64 x 2^dim = %llu: build a new handle", i,
                                            k ? "add" : "mul", (unsigned long long)nnz, (unsigned long long)(scd::kGkrBatchMaxNnzPerCell << dim));
            }
    }
    if (G->fused) {
        const Layout L(in, wiring, G->lists_used);
        if (L.used > G->in_cap)
            return sc_internal_fail(SC_ERR_BAD_ARG, "the layer's distinct arrays take %zu bytes of the handle's copy, init reserved %zu: build a new handle", L.used, G->in_cap);
        DeviceGate gate_(G->device);
        HIP_TRY(hipSetDevice(G->device));
        if (dev_in) {
            HIP_TRY(hipDeviceSynchronize()); // the inputs' producers are waited for, as at init
            if (wiring)
                if (int rc = check_idx_on_device(G, in)) return rc;
        }
        // ---- from here on the handle is the new layer's ----
        rewind(G);
        if (int rc = fused_stage(G, in, L, wiring)) {
            G->exhausted = true;
            return rc;
        }
        return SC_OK;
    }
    if (dev_in && wiring) {
        DeviceGate gate_(G->device);
        HIP_TRY(hipSetDevice(G->device));
        HIP_TRY(hipDeviceSynchronize());
        if (int rc = check_idx_on_device(G, in)) return rc;
    }
    const Tripled T(in, wiring, dev_in ? reinterpret_cast<const uint64_t *>(G->d_ones) : G->ones[0].l);
    const uint64_t *const *idx = wiring ? T.idx.data() : nullptr, *const *vals = wiring ? T.vals.data() : nullptr;
    const uint64_t *nnz = wiring ? T.nnz.data() : nullptr;
    // (the inner call's own errors -- its plan and capacity rules, over inner instances 3 i + k -- leave it, and so this handle, where it was)
    const int rc = in.g2 ? sc_gkr_two_point_next_batch(G->inner, idx, vals, nnz, T.f2.data(), T.f3.data(), T.g.data(), T.g2.data(), T.coef.data(), flags)
                         : sc_gkr_layer_next_batch(G->inner, idx, vals, nnz, T.f2.data(), T.f3.data(), T.g.data(), flags);
    if (rc) {
        const std::string why = sc_last_error();
        return sc_internal_fail(rc, "composed plan (inner instances 3 i + k): %s", why.c_str());
    }
    G->two_point = in.g2 != nullptr;
    rewind(G);
    return SC_OK;
}
