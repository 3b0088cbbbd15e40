// batch_rounds.hip -- sc_batch_prover_*: n x IPForMLSumcheck::{prover_init, prove_round} (reference src/ml_sumcheck/protocol/prover.rs:49-153)
// of one structure behind ONE handle, a round of all n instances per call.  The interactive half of the batched provers (batch.hip is the
// non-interactive one): the caller owns the transcript(s) and hands in every challenge, so a round is launched after its challenges
// are known and nothing on the GPU ever waits for the host.  Three plans, chosen when the handle is built (batch_slices.hpp: bs_plan), same bits:
//   batch.rounds_one_block  k_batch_round (kernels_batch_rounds.hip): one block per instance, one launch per round for the whole batch.  The
//                           per-round sequence is fixed: upload the challenges, one launch, one copy back, one synchronisation.  The
//                           tables live in a device work area as 48-byte LDS slots, every binding depth in a region of its own;
//   batch.rounds_slices     policy "batch_slices" = 1, shapes beyond one block's LDS up to 2^16 entries: the same work area and per-round
//                           sequence, but the rounds whose tables as loaded do not fit one block run as k_batch_round_slices +
//                           k_batch_round_fin (kernels_batch_round_slices.hip: several blocks per instance, their sums through a device
//                           array of partials); from the first round that fits, k_batch_round, counted as batch.rounds_one_block;
//   batch.rounds_serial     n ordinary sc_prover handles inside the batch handle (device-side waits off, no resident kernel) over the
//                           handle's own copy of the tables; a round is a loop of sc_prove_round: shapes beyond one block's LDS
//                           (batch_shape_fits) unless sliced, policy "batch" = 0.
#include "batch_slices.hpp"
#include "prover_internal.hpp"

struct sc_batch_prover {
    int device = 0;
    uint32_t n = 0, nv = 0, U = 0, D = 0, round = 0; // round: rounds proved so far
    bool exhausted = false;
    int plan = scd::kBrSerial; // scd::BatchRoundsPlan; kBrOneBlock and kBrSlices share the work area and everything that reads it
    bool work_area() const { return plan != scd::kBrSerial; }
    std::vector<std::vector<sch::Fr>> randomness; // per challenge received: n elements, or ONE for a shared challenge
    // the descriptors' structure (host copies: a reset checks new descriptors against it)
    uint32_t max_mult = 0, K = 0, flags = 0;
    std::vector<uint32_t> prod_offsets, prod_indices;
    hipStream_t stream = nullptr;
    // ---- batch.rounds_one_block, batch.rounds_slices ----
    SharedMeta s;
    char *d_buf = nullptr;   // device: work area | matrices | table pointers | challenges | messages | export area | staged host tables | partials (sliced rounds)
    char *h_pin = nullptr;   // pinned: matrices | table pointers | challenges | messages | export area | staged host tables
    size_t work_bytes = 0, w_off = 0, ptr_off = 0, chal_off = 0, msg_off = 0, exp_off = 0, stage_off = 0, pin_bytes = 0, exp_bytes = 0; // (offsets into h_pin; d_buf: + work_bytes)
    size_t part_off = 0;     // the partials, into d_buf (behind the mirror of h_pin)
    // ---- batch.rounds_serial ----
    std::vector<sc_prover *> provers;
    char *d_orig = nullptr;  // device: the handle's copy of the tables, [instance][table][2^nv] elements (the n handles borrow it)
    char *d_fin = nullptr;   // device: bind_final's n x U elements
};

namespace {

void batch_prover_destroy(sc_batch_prover *bp) {
    if (!bp) return;
    for (sc_prover *p : bp->provers)
        if (p) sc_prover_free(p);
    bp->provers.clear();
    if (bp->d_buf || bp->h_pin || bp->d_orig || bp->d_fin || bp->stream) {
        DeviceGate gate_(bp->device);
        (void)hipSetDevice(bp->device);
        if (bp->stream) (void)hipStreamSynchronize(bp->stream);
        if (bp->d_buf) (void)hipFree(bp->d_buf);
        if (bp->h_pin) (void)hipHostFree(bp->h_pin);
        if (bp->d_orig) (void)hipFree(bp->d_orig);
        if (bp->d_fin) (void)hipFree(bp->d_fin);
        if (bp->stream) (void)hipStreamDestroy(bp->stream);
        (void)hipGetLastError();
    }
    delete bp;
}

// everything the host can check on n descriptors of a batch: sc_ml_prove_batch's checks, plus canonical coefficients
int check_descs(const sc_poly_desc *descs, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) {
        if (int rc = batch_check_desc(descs, i)) return rc;
        if (int rc = batch_check_structure(descs, i)) return rc;
        for (uint32_t k = 0; k < descs[i].n_products; ++k) {
            sch::Fr c;
            std::memcpy(&c, descs[i].coeffs + 4 * k, 32);
            if (sch::geq_p(c)) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: coefficient %u is not a canonical field element", i, k);
        }
    }
    return SC_OK;
}

// the tables and coefficients of n descriptors into the handle, which is at round 0 afterwards (init and reset; the gate is held)
int load_one_block(sc_batch_prover *bp, const sc_poly_desc *descs) {
    const uint32_t n = bp->n, U = bp->U;
    const SharedMeta &s = bp->s;
    const bool host_tables = !(descs[0].flags & SC_TABLES_ON_DEVICE);
    const size_t table_bytes = (size_t)32 << bp->nv;
    if (!host_tables) HIP_TRY(hipDeviceSynchronize()); // the tables are read in place by the load kernel: their producers are waited for, as a copy would
    sch::Fr *h_w = reinterpret_cast<sch::Fr *>(bp->h_pin + bp->w_off);
    const void **h_ptrs = reinterpret_cast<const void **>(bp->h_pin + bp->ptr_off);
    char *d_up = bp->d_buf + bp->work_bytes;
    for (uint32_t i = 0; i < n; ++i) {
        instance_weights(s, descs[i].coeffs, h_w + (size_t)i * s.w_elems);
        for (uint32_t u = 0; u < U; ++u) {
            if (host_tables) {
                const size_t off = bp->stage_off + ((size_t)i * U + u) * table_bytes;
                std::memcpy(bp->h_pin + off, descs[i].tables[u], table_bytes);
                h_ptrs[(size_t)i * U + u] = d_up + off;
            } else {
                h_ptrs[(size_t)i * U + u] = descs[i].tables[u];
            }
        }
    }
    // one upload: matrices | pointers, and (host tables) the staged tables behind the per-round areas
    HIP_TRY(hipMemcpyAsync(d_up + bp->w_off, bp->h_pin + bp->w_off, bp->chal_off - bp->w_off, hipMemcpyHostToDevice, bp->stream));
    if (host_tables) HIP_TRY(hipMemcpyAsync(d_up + bp->stage_off, bp->h_pin + bp->stage_off, (size_t)n * U * table_bytes, hipMemcpyHostToDevice, bp->stream));
    HIP_TRY(scd::launch_batch_rounds_load(reinterpret_cast<const uint4 *const *>(d_up + bp->ptr_off), n, U, bp->nv, reinterpret_cast<int32_t *>(bp->d_buf), bp->stream));
    HIP_TRY(hipStreamSynchronize(bp->stream)); // nothing of the caller's is read after the call returns
    return SC_OK;
}

int load_serial(sc_batch_prover *bp, const sc_poly_desc *descs) {
    const uint32_t n = bp->n, U = bp->U;
    const bool host_tables = !(descs[0].flags & SC_TABLES_ON_DEVICE);
    const size_t table_bytes = (size_t)32 << bp->nv;
    {
        DeviceGate gate_(bp->device);
        HIP_TRY(hipSetDevice(bp->device));
        if (!host_tables) HIP_TRY(hipDeviceSynchronize());
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t u = 0; u < U; ++u)
                HIP_TRY(hipMemcpyAsync(bp->d_orig + ((size_t)i * U + u) * table_bytes, descs[i].tables[u], table_bytes, host_tables ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, bp->stream));
        HIP_TRY(hipStreamSynchronize(bp->stream)); // (the handles below read the copy on streams of their own)
    }
    std::vector<const uint64_t *> tabs(U);
    for (uint32_t i = 0; i < n; ++i) {
        for (uint32_t u = 0; u < U; ++u) tabs[u] = reinterpret_cast<const uint64_t *>(bp->d_orig + ((size_t)i * U + u) * table_bytes);
        int rc = SC_OK;
        bool same_coeffs = false;
        if (bp->provers[i]) { // a reset: the handle is rewound when its coefficients are the new ones, rebuilt otherwise
            const sc_prover *p = bp->provers[i];
            same_coeffs = true;
            for (uint32_t k = 0; k < bp->K && same_coeffs; ++k) same_coeffs = std::memcmp(&p->prods[k].coeff, descs[i].coeffs + 4 * k, 32) == 0;
        }
        if (same_coeffs) {
            rc = sc_prover_reset(bp->provers[i], tabs.data(), SC_TABLES_ON_DEVICE);
        } else {
            if (bp->provers[i]) sc_prover_free(bp->provers[i]);
            bp->provers[i] = nullptr;
            sc_poly_desc eff = descs[i];
            eff.tables = tabs.data();
            eff.flags = SC_TABLES_ON_DEVICE | SC_TABLES_BORROW | SC_NO_DEVICE_POLLING;
            rc = sc_prover_init(&eff, &bp->provers[i]);
            if (rc == SC_OK) rc = sc_prover_set_resident(bp->provers[i], 0);
        }
        if (rc) return prefix_instance(rc, i);
    }
    return SC_OK;
}

} // namespace

extern "C" int sc_batch_prover_init(const sc_poly_desc *descs, uint32_t n, sc_batch_prover **out) {
    if (!descs || !out) return sc_internal_fail(SC_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    if (n == 0) return sc_internal_fail(SC_ERR_BAD_ARG, "n == 0: a batch handle holds at least one instance");
    if (int rc = check_descs(descs, n)) return rc;
    if (sc_device_count() <= 0) return sc_internal_fail(SC_ERR_HIP, "no HIP device visible: libsumcheck_hip has no CPU fallback");
    const sc_poly_desc &d0 = descs[0];
    sc_batch_prover *bp = new (std::nothrow) sc_batch_prover();
    if (!bp) return sc_internal_fail(SC_ERR_OOM, "out of host memory");
    bp->device = sc_internal_device_ref();
    bp->n = n;
    bp->nv = d0.num_vars;
    bp->U = d0.n_tables;
    bp->max_mult = d0.max_multiplicands;
    bp->D = d0.max_multiplicands + 1;
    bp->K = d0.n_products;
    bp->flags = d0.flags;
    if (bp->K) {
        bp->prod_offsets.assign(d0.prod_offsets, d0.prod_offsets + bp->K + 1);
        bp->prod_indices.assign(d0.prod_indices, d0.prod_indices + d0.prod_offsets[bp->K]);
    }
    if (scd::policy(scd::kPolBatch) != 0 && bp->K > 0) {
        build_shared(&d0, bp->s);
        const SharedMeta &s = bp->s;
        bp->plan = scd::bs_plan(n, s.nv, s.U, (int)s.K, (int)s.D, s.max_mult, s.n_combos, s.fits_args, scd::policy(scd::kPolBatch), scd::policy(scd::kPolBatchSlices));
    }
    const size_t table_bytes = (size_t)32 << bp->nv;
    auto build = [&]() -> int {
        {
            DeviceGate gate_(bp->device);
            HIP_TRY(hipSetDevice(bp->device));
            HIP_TRY(hipStreamCreateWithFlags(&bp->stream, hipStreamNonBlocking));
        }
        if (!bp->work_area()) {
            {
                DeviceGate gate_(bp->device);
                HIP_TRY(hipMalloc(reinterpret_cast<void **>(&bp->d_orig), (size_t)n * bp->U * table_bytes));
                HIP_TRY(hipMalloc(reinterpret_cast<void **>(&bp->d_fin), (size_t)n * bp->U * 32));
            }
            bp->provers.assign(n, nullptr);
            return load_serial(bp, descs);
        }
        SharedMeta &s = bp->s;
        for (uint32_t k = 0; k < s.K; ++k) s.unit.push_back(unit_matrix(s.M[k], s.D));
        const bool host_tables = !(d0.flags & SC_TABLES_ON_DEVICE);
        bp->work_bytes = round_up((size_t)n * bp->U * 2 * (scd::kBatchRoundSlotBytes << bp->nv), 256);
        bp->exp_bytes = std::max((size_t)bp->U * table_bytes, (size_t)n * bp->U * 32); // one instance's tables (state), or every instance's final values
        bp->w_off = 0;
        bp->ptr_off = bp->w_off + round_up((size_t)n * s.w_elems * 32, 256);
        bp->chal_off = bp->ptr_off + round_up((size_t)n * bp->U * sizeof(void *), 256);
        bp->msg_off = bp->chal_off + round_up((size_t)n * 32, 256);
        bp->exp_off = bp->msg_off + round_up((size_t)n * bp->D * 32, 256);
        bp->stage_off = bp->exp_off + round_up(bp->exp_bytes, 256);
        bp->pin_bytes = bp->stage_off + (host_tables ? (size_t)n * bp->U * table_bytes : 0);
        bp->part_off = bp->work_bytes + round_up(bp->pin_bytes, 256);
        const size_t part_bytes = bp->plan == scd::kBrSlices ? (size_t)scd::bs_partials_bytes(n, s.nv, s.U, (int)s.K, (int)s.D, s.n_combos) : 0;
        DeviceGate gate_(bp->device);
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&bp->d_buf), bp->part_off + part_bytes));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&bp->h_pin), bp->pin_bytes, hipHostMallocDefault));
        return load_one_block(bp, descs);
    };
    if (int rc = build()) {
        const std::string why = sc_last_error(); // (the frees below may run library calls of their own)
        batch_prover_destroy(bp);
        return sc_internal_fail(rc, "%s", why.c_str());
    }
    *out = bp;
    return SC_OK;
}

extern "C" void sc_batch_prover_free(sc_batch_prover *bp) { batch_prover_destroy(bp); }

extern "C" int sc_batch_prove_round(sc_batch_prover *bp, const uint64_t *r_or_null, uint32_t r_shared, uint64_t *out_evals) {
    if (!bp || !out_evals) return sc_internal_fail(SC_ERR_BAD_ARG, "null argument");
    // validation, same precedence as sc_prove_round's (prover.rs:78-98); every check comes before the first change to the handle
    if (bp->exhausted) return sc_internal_fail(SC_ERR_NOT_ACTIVE, "Prover is not active");
    if (r_or_null && bp->round == 0) return sc_internal_fail(SC_ERR_FIRST_ROUND_HAS_MSG, "first round should be prover first.");
    if (!r_or_null && bp->round > 0) return sc_internal_fail(SC_ERR_MISSING_MSG, "verifier message is empty");
    if (bp->round + 1 > bp->nv) return sc_internal_fail(SC_ERR_NOT_ACTIVE, "Prover is not active");
    std::vector<sch::Fr> chal;
    if (r_or_null)
        if (int rc = take_challenges(bp->n, r_or_null, r_shared, chal)) return rc;
    const uint32_t n = bp->n, D = bp->D;
    if (bp->work_area()) {
        const SharedMeta &s = bp->s;
        DeviceGate gate_(bp->device);
        HIP_TRY(hipSetDevice(bp->device));
        char *d_up = bp->d_buf + bp->work_bytes;
        if (r_or_null) {
            std::memcpy(bp->h_pin + bp->chal_off, chal.data(), chal.size() * 32);
            HIP_TRY(hipMemcpyAsync(d_up + bp->chal_off, bp->h_pin + bp->chal_off, chal.size() * 32, hipMemcpyHostToDevice, bp->stream));
        }
        scd::BatchRoundArgs A;
        std::memset(&A, 0, sizeof(A));
        A.work = reinterpret_cast<int32_t *>(bp->d_buf);
        A.Wm = reinterpret_cast<const uint4 *>(d_up + bp->w_off);
        A.w_stride = s.w_elems;
        A.chal = reinterpret_cast<const uint4 *>(d_up + bp->chal_off);
        A.chal_shared = chal.size() == 1 && n != 1 ? 1u : 0u;
        A.out = reinterpret_cast<uint4 *>(d_up + bp->msg_off);
        A.n = n;
        A.n_tables = s.U;
        A.nv = s.nv;
        A.round = bp->round;
        A.n_combos = s.n_combos;
        A.K = (int)s.K;
        A.D = (int)s.D;
        if (bp->plan == scd::kBrSlices && scd::bs_round_sliced(s.nv, bp->round, s.U, (int)s.K, (int)s.D, s.max_mult)) {
            HIP_TRY(scd::launch_batch_round_slices(A, reinterpret_cast<uint4 *>(bp->d_buf + bp->part_off), s.combo, s.fin, bp->stream));
            scd::plan_hit(scd::kPlanBatchRoundsSlices);
        } else {
            HIP_TRY(scd::launch_batch_round(A, s.combo, s.fin, bp->stream));
            scd::plan_hit(scd::kPlanBatchRoundsOneBlock);
        }
        HIP_TRY(hipMemcpyAsync(bp->h_pin + bp->msg_off, d_up + bp->msg_off, (size_t)n * D * 32, hipMemcpyDeviceToHost, bp->stream));
        HIP_TRY(hipStreamSynchronize(bp->stream));
        std::memcpy(out_evals, bp->h_pin + bp->msg_off, (size_t)n * D * 32);
    } else {
        scd::plan_hit(scd::kPlanBatchRoundsSerial);
        for (uint32_t i = 0; i < n; ++i) {
            int rc = sc_prove_round(bp->provers[i], r_or_null ? challenge_of(chal, i).l : nullptr, out_evals + (size_t)i * D * 4);
            if (rc) {
                bp->exhausted = true; // (a HIP failure part of the way through the batch: the handle needs a reset)
                return prefix_instance(rc, i);
            }
        }
    }
    if (r_or_null) bp->randomness.push_back(std::move(chal));
    bp->round++;
    return SC_OK;
}

extern "C" int sc_batch_prover_push_randomness(sc_batch_prover *bp, const uint64_t *r, uint32_t r_shared) {
    if (!bp || !r) return sc_internal_fail(SC_ERR_BAD_ARG, "null argument");
    std::vector<sch::Fr> chal(r_shared ? 1 : bp->n);
    std::memcpy(chal.data(), r, chal.size() * 32);
    bp->randomness.push_back(std::move(chal));
    return SC_OK;
}

extern "C" int sc_batch_prover_state(sc_batch_prover *bp, uint32_t instance, uint64_t *randomness, uint32_t *n_randomness, uint64_t *tables_out, uint32_t *round) {
    if (!bp) return sc_internal_fail(SC_ERR_BAD_ARG, "null prover");
    if (instance >= bp->n) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: the handle holds %u instances", instance, bp->n);
    batch_state_head(bp->randomness, instance, bp->round, randomness, n_randomness, round);
    if (!tables_out) return SC_OK;
    if (bp->exhausted) return sc_internal_fail(SC_ERR_NOT_ACTIVE, "tables were consumed by sc_batch_prover_bind_final");
    if (!bp->work_area()) return sc_prover_state(bp->provers[instance], nullptr, nullptr, tables_out, nullptr);
    const uint32_t bound = bp->round > 0 ? bp->round - 1 : 0;
    DeviceGate gate_(bp->device);
    HIP_TRY(hipSetDevice(bp->device));
    return batch_export_out(reinterpret_cast<const int32_t *>(bp->d_buf), instance, 1, bp->U, bp->nv, bound, nullptr, 0, bp->d_buf + bp->work_bytes + bp->exp_off, bp->h_pin + bp->exp_off,
                            tables_out, bp->stream);
}

extern "C" int sc_batch_prover_bind_final(sc_batch_prover *bp, const uint64_t *r, uint32_t r_shared, uint64_t *out_table_values) {
    if (!bp || !r || !out_table_values) return sc_internal_fail(SC_ERR_BAD_ARG, "null argument");
    if (bp->exhausted || bp->round != bp->nv) return sc_internal_fail(SC_ERR_NOT_ACTIVE, "bind_final needs a prover that has finished its last round");
    std::vector<sch::Fr> chal;
    if (int rc = take_challenges(bp->n, r, r_shared, chal)) return rc;
    const uint32_t n = bp->n, U = bp->U;
    if (bp->work_area()) {
        DeviceGate gate_(bp->device);
        HIP_TRY(hipSetDevice(bp->device));
        char *d_up = bp->d_buf + bp->work_bytes;
        std::memcpy(bp->h_pin + bp->chal_off, chal.data(), chal.size() * 32);
        HIP_TRY(hipMemcpyAsync(d_up + bp->chal_off, bp->h_pin + bp->chal_off, chal.size() * 32, hipMemcpyHostToDevice, bp->stream));
        if (int rc = batch_export_out(reinterpret_cast<const int32_t *>(bp->d_buf), 0, n, U, bp->nv, bp->nv - 1, reinterpret_cast<const uint4 *>(d_up + bp->chal_off),
                                      chal.size() == 1 && n != 1 ? 1u : 0u, d_up + bp->exp_off, bp->h_pin + bp->exp_off, out_table_values, bp->stream))
            return rc;
    } else {
        for (uint32_t i = 0; i < n; ++i)
            if (int rc = serial_bind_final(bp->provers[i], bp->device, challenge_of(chal, i).l, bp->d_fin + (size_t)i * U * 32, 0, U, out_table_values + (size_t)i * U * 4)) {
                bp->exhausted = true;
                return prefix_instance(rc, i);
            }
    }
    bp->randomness.push_back(std::move(chal));
    bp->exhausted = true;
    return SC_OK;
}

extern "C" int sc_batch_prover_reset(sc_batch_prover *bp, const sc_poly_desc *descs_or_null) {
    if (!bp) return sc_internal_fail(SC_ERR_BAD_ARG, "null prover");
    if (descs_or_null) {
        const sc_poly_desc *descs = descs_or_null;
        if (int rc = check_descs(descs, bp->n)) return rc;
        // the handle's structure: what its work areas and launches were built for
        sc_poly_desc own;
        std::memset(&own, 0, sizeof(own));
        own.num_vars = bp->nv;
        own.max_multiplicands = bp->max_mult;
        own.n_products = bp->K;
        own.prod_offsets = bp->prod_offsets.data();
        own.prod_indices = bp->prod_indices.data();
        own.n_tables = bp->U;
        own.flags = descs[0].flags;
        if (const char *field = first_structure_difference(own, descs[0]))
            return sc_internal_fail(SC_ERR_BAD_ARG, "instance 0 differs from the handle's structure in %s: a reset does not reallocate", field);
        if (bp->work_area() && !(descs[0].flags & SC_TABLES_ON_DEVICE) && (bp->flags & SC_TABLES_ON_DEVICE))
            return sc_internal_fail(SC_ERR_BAD_ARG, "a handle built over device tables has no staging area for host tables: a reset does not reallocate");
        if (bp->work_area()) {
            DeviceGate gate_(bp->device);
            HIP_TRY(hipSetDevice(bp->device));
            if (int rc = load_one_block(bp, descs)) return rc;
        } else {
            if (int rc = load_serial(bp, descs)) return rc;
        }
    } else if (!bp->work_area()) {
        for (uint32_t i = 0; i < bp->n; ++i) { // the handles borrow the batch handle's own copy of the tables: rewound in place
            if (int rc = sc_prover_reset(bp->provers[i], nullptr, SC_TABLES_ON_DEVICE)) return prefix_instance(rc, i);
        }
    } // (a work area, the same tables: round 0's slots were never overwritten)
    bp->round = 0;
    bp->exhausted = false;
    bp->randomness.clear();
    return SC_OK;
}
