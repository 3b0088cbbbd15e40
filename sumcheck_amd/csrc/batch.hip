// batch.hip -- sc_ml_prove_batch: n independent instances of MLSumcheck::prove (reference src/ml_sumcheck/mod.rs:42-70) of one
// structure, proved concurrently.  Two plans, same bits:
//   batch.one_block  k_batch_proofs (kernels_batch.hip): one block per instance, every round out of LDS; this thread serves whichever
//                    instance's message has appeared -- copy, feed_prover_msg, sample_fr, post the challenge -- and makes no HIP call
//                    while it does (compare run_tail, protocol.hip);
//   batch.serial     instance after instance on one prover handle (rewound onto the next instance's tables; rebuilt where the
//                    coefficients change): shapes beyond the kernel's envelope, n below the measured crossover, policy "batch" = 0,
//                    device-side waits off, the device's tail slot taken -- and the instances whose block gave up waiting.
// sc_gkr_prove_batch: n independent instances of GKRRoundSumcheck::prove (reference src/gkr_round_sumcheck/mod.rs:93-139) of one dim, the
// same two plans over the same work areas, serving loop and give-up protocol (run_batched takes what differs as a BatchJob):
//   batch.gkr_one_block  k_batch_gkr (kernels_batch_gkr.hip): one block per instance builds both phases' tables in LDS and runs the
//                        2 x dim rounds; no PolynomialInfo is fed (mod.rs:108-133) and the challenge behind every message but the last is posted;
//   batch.gkr_serial     instance after instance through sc_gkr_prove's path, on copies of the callers' transcripts.
#include <functional>
#include <unordered_set>

#include "prover_internal.hpp"

int sc_internal_gkr_prove(sc_rng *rng, const uint64_t *f1_idx, const uint64_t *f1_vals, uint64_t nnz, uint32_t dim, const uint64_t *f2, const uint64_t *f3, const uint64_t *g,
                          uint32_t flags, uint64_t *out_proof, uint64_t *out_uv_or_null, bool no_polling); // gkr.hip: sc_gkr_prove, optionally with device-side waits off

namespace {

// ---- the serial plan -------------------------------------------------------------------------------------------------------------------
// sc_ml_prove's steps (protocol.hip) with the handle kept across the instances of the call: the structure is the same by contract, so
// a handle whose coefficients match is rewound onto the next tables (sc_prover_reset), as the kept prover of one-shot proofs is.
struct SerialRunner {
    sc_prover *p = nullptr;
    std::vector<uint64_t> coeffs; // of the instance `p` was built for
    bool no_polling = false;      // every round launched after its challenge (the retry of an instance whose device-side wait expired)
    ~SerialRunner() {
        if (p) sc_prover_free(p); // (back to the pool: the next one-shot proof of this structure finds it)
    }
    int prove(const sc_poly_desc *d, sc_rng *rng_or_null, uint64_t *out_proof, uint64_t *out_rand_or_null) {
        sc_poly_desc eff = *d;
        if ((eff.flags & SC_TABLES_ON_DEVICE) && !(eff.flags & SC_TABLES_BORROW)) eff.flags |= SC_TABLES_BORROW; // read in place: the handle does not outlive the call
        const size_t cw = (size_t)d->n_products * 4;
        if (p && (coeffs.size() != cw || (cw && std::memcmp(coeffs.data(), d->coeffs, cw * 8) != 0))) {
            sc_prover_free(p);
            p = nullptr;
        }
        int rc;
        if (p) {
            rc = sc_prover_reset(p, eff.tables, eff.flags & SC_TABLES_ON_DEVICE);
        } else {
            rc = sc_prover_init(&eff, &p);
            if (rc == SC_OK) coeffs.assign(d->coeffs, d->coeffs + cw);
        }
        if (rc == SC_OK && no_polling) rc = sc_prover_set_polling(p, 0);
        if (rc == SC_OK) rc = sc_ml_prove_handle(p, rng_or_null, out_proof);
        if (rc != SC_OK) {
            if (p) {
                p->pool_key.clear();
                prover_destroy(p);
                p = nullptr;
            }
            return rc;
        }
        if (out_rand_or_null) std::memcpy(out_rand_or_null, p->randomness.data(), (size_t)p->nv * 32);
        return SC_OK;
    }
};

// ---- the batched plan's work areas: process-wide, one call at a time holds them (a concurrent call takes the serial plan: the device
// has one tail slot anyway); obey sc_set_cache_limit / sc_release_caches like the other caches ------------------------------------------
struct BatchArea {
    std::mutex mu;
    int device = -1;
    int n_cus = 0;
    sc_prover owner;            // never built: the identity under which the call holds the device's tail slot, and the stream of the launch probe
    hipStream_t stream = nullptr;
    char *d_buf = nullptr;      // device: ticket (256 B) | table pointers | weight matrices | staged host tables
    size_t d_cap = 0;
    char *h_up = nullptr;       // pinned: what is uploaded behind the ticket, in the same layout (one copy per call)
    size_t up_cap = 0;
    char *h_page = nullptr;     // host-mapped: messages | give-up markers | mailboxes
    char *h_page_dev = nullptr;
    size_t page_cap = 0;
    uint64_t *d_vmail = nullptr; // mailboxes in host-visible device memory (large BAR, policy "vram_mailbox")
    size_t vmail_cap = 0;
    uint32_t gen = 0;           // tags of a launch: gen << 6 | round
    uint64_t occ_key = 0;       // the last shape the occupancy query was made for, and its answer
    int occ_val = 0;
    int large_bar = -1;         // hipDeviceAttributeIsLargeBar, asked once per device
    size_t device_bytes() const { return d_cap + vmail_cap; }
    void free_all() {
        if (device >= 0) (void)hipSetDevice(device);
        if (d_buf) (void)hipFree(d_buf);
        if (h_up) (void)hipHostFree(h_up);
        if (h_page) (void)hipHostFree(h_page);
        if (d_vmail) (void)hipFree(d_vmail);
        if (stream) (void)hipStreamDestroy(stream);
        (void)hipGetLastError();
        d_buf = h_up = h_page = h_page_dev = nullptr;
        d_vmail = nullptr;
        stream = nullptr;
        d_cap = up_cap = page_cap = vmail_cap = 0;
        device = -1;
        n_cus = 0;
        gen = 0;
        occ_key = 0;
        occ_val = 0;
        large_bar = -1;
    }
};
BatchArea g_area;
struct AreaLease {
    bool held;
    AreaLease() : held(g_area.mu.try_lock()) {}
    ~AreaLease() {
        if (!held) return;
        if (g_area.device_bytes() > sc_internal_cache_limit()) g_area.free_all(); // (over the limit: nothing is kept between calls)
        g_area.mu.unlock();
    }
};
// the area on the calling thread's device, with its stream (the caller holds the lease and the device gate)
int area_open(BatchArea &a, int dev) {
    HIP_TRY(hipSetDevice(dev));
    if (a.device != dev) {
        a.free_all();
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, dev));
        HIP_TRY(hipStreamCreateWithFlags(&a.stream, hipStreamNonBlocking));
        a.device = dev;
        a.n_cus = prop.multiProcessorCount;
        a.owner.device = dev;
        a.owner.stream = a.stream;
    }
    return SC_OK;
}
// at least d_bytes of device memory and up_bytes of pinned host memory
int area_reserve(BatchArea &a, size_t d_bytes, size_t up_bytes) {
    if (a.d_cap < d_bytes) {
        if (a.d_buf) (void)hipFree(a.d_buf);
        a.d_buf = nullptr;
        a.d_cap = 0;
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&a.d_buf), d_bytes));
        a.d_cap = d_bytes;
    }
    if (a.up_cap < up_bytes) {
        if (a.h_up) (void)hipHostFree(a.h_up);
        a.h_up = nullptr;
        a.up_cap = 0;
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&a.h_up), up_bytes, hipHostMallocDefault));
        a.up_cap = up_bytes;
    }
    return SC_OK;
}

} // namespace

// ---- what the entry points here and the two batch handles share (prover_internal.hpp) ----
size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
int prefix_instance(int rc, uint32_t i) {
    const std::string why = sc_last_error();
    return sc_internal_fail(rc, "instance %u: %s", i, why.c_str());
}
const sch::Fr &challenge_of(const std::vector<sch::Fr> &c, uint32_t i) { return c.size() == 1 ? c[0] : c[i]; }
int take_challenges(uint32_t n, const uint64_t *r, uint32_t r_shared, std::vector<sch::Fr> &out) {
    out.resize(r_shared ? 1 : n);
    std::memcpy(out.data(), r, out.size() * 32);
    for (size_t i = 0; i < out.size(); ++i)
        if (sch::geq_p(out[i])) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: challenge is not canonical", (uint32_t)i);
    return SC_OK;
}
int serial_bind_final(sc_prover *p, int device, const uint64_t *r, char *d_fin, uint32_t first, uint32_t count, void *h_out) {
    if (int rc = sc_prover_bind_final(p, r, reinterpret_cast<uint64_t *>(d_fin))) return rc;
    DeviceGate gate_(device);
    hipError_t e = hipMemcpyAsync(h_out, d_fin + (size_t)first * 32, (size_t)count * 32, hipMemcpyDeviceToHost, p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    if (e == hipSuccess) return SC_OK;
    (void)hipGetLastError();
    return sc_internal_fail(SC_ERR_HIP, "copying the final table values failed: %s", hipGetErrorString(e));
}
void batch_state_head(const std::vector<std::vector<sch::Fr>> &rand, uint32_t instance, uint32_t round_now, uint64_t *randomness, uint32_t *n_randomness, uint32_t *round) {
    if (randomness)
        for (size_t j = 0; j < rand.size(); ++j) std::memcpy(randomness + 4 * j, &challenge_of(rand[j], instance), 32);
    if (n_randomness) *n_randomness = (uint32_t)rand.size();
    if (round) *round = round_now;
}
int batch_export_out(const int32_t *work, uint32_t first, uint32_t count, uint32_t n_tables, uint32_t nv, uint32_t bound, const uint4 *d_chal_or_null, uint32_t chal_shared, char *d_exp,
                     char *h_exp, void *out, hipStream_t stream) {
    HIP_TRY(scd::launch_batch_rounds_export(work, first, count, n_tables, nv, bound, d_chal_or_null, chal_shared, reinterpret_cast<uint4 *>(d_exp), stream));
    const size_t bytes = (size_t)count * n_tables * ((size_t)32 << (nv - bound - (d_chal_or_null ? 1u : 0u))); // (the launcher has refused a depth beyond nv)
    HIP_TRY(hipMemcpyAsync(h_exp, d_exp, bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    std::memcpy(out, h_exp, bytes);
    return SC_OK;
}

// (the structure every instance shares: SharedMeta, prover_internal.hpp -- also what batch_rounds.hip builds its launches from)
void build_shared(const sc_poly_desc *d, SharedMeta &s) {
    s.nv = d->num_vars;
    s.U = d->n_tables;
    s.K = d->n_products;
    s.max_mult = d->max_multiplicands;
    s.D = d->max_multiplicands + 1;
    std::memset(&s.combo, 0, sizeof(s.combo));
    std::memset(&s.fin, 0, sizeof(s.fin));
    std::vector<Combo> combos;
    std::vector<uint32_t> slot_table, slot_exp;
    uint64_t partial_elems = 0;
    for (uint32_t k = 0; k < s.K; ++k) {
        std::vector<uint32_t> tables, exps;
        for (uint32_t q = d->prod_offsets[k]; q < d->prod_offsets[k + 1]; ++q) {
            const uint32_t t = d->prod_indices[q];
            auto it = std::find(tables.begin(), tables.end(), t);
            if (it == tables.end()) {
                tables.push_back(t);
                exps.push_back(1);
            } else {
                exps[it - tables.begin()]++;
            }
        }
        const uint32_t M = d->prod_offsets[k + 1] - d->prod_offsets[k];
        s.M.push_back(M);
        const uint32_t slot_off = (uint32_t)slot_table.size();
        slot_table.insert(slot_table.end(), tables.begin(), tables.end());
        slot_exp.insert(slot_exp.end(), exps.begin(), exps.end());
        if (k < (uint32_t)scd::kMetaProds) {
            s.fin.prod[k].M = M;
            s.fin.prod[k].partial_off = partial_elems; // (the product's identity in the combination records; nothing is stored there)
            s.fin.prod[k].w_off = s.w_elems;
        }
        for (uint32_t t = 0; t <= M; ++t) {
            Combo c;
            c.t = t;
            c.M = M;
            c.slot_off = slot_off;
            c.n_slots = (uint32_t)tables.size();
            c.partial_off = partial_elems;
            combos.push_back(c);
        }
        partial_elems += (uint64_t)scd::kMaxGrid * (M + 1);
        s.w_elems += 2 * s.D * (M + 1);
    }
    s.n_combos = (int)combos.size();
    s.fits_args = s.K >= 1 && s.K <= (uint32_t)scd::kMetaProds && combos.size() <= (size_t)scd::kMetaCombos && slot_table.size() <= (size_t)scd::kMetaSlots;
    if (s.fits_args) {
        std::copy(combos.begin(), combos.end(), s.combo.combo);
        std::copy(slot_table.begin(), slot_table.end(), s.combo.slot_table);
        std::copy(slot_exp.begin(), slot_exp.end(), s.combo.slot_exp);
    }
}
// the node -> message matrix of a product of M multiplicands in a message of D points, for a coefficient of one: exact Lagrange weights
// (a field inversion per entry), the same for every instance of every batch -- computed once per process
const std::vector<sch::Fr> *unit_matrix(uint32_t M, uint32_t D) {
    static std::mutex mu;
    static std::map<std::pair<uint32_t, uint32_t>, std::vector<sch::Fr>> cache;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find({M, D});
    if (it == cache.end()) {
        it = cache.emplace(std::make_pair(M, D), std::vector<sch::Fr>()).first;
        build_node_matrix(M, D, sch::kOne, it->second);
    }
    return &it->second; // (map nodes do not move)
}
// instance weights: c_k W_k and c_k 2^(5(M-1)) W_k behind it, product after product (FinProd::w_off) -- c x (1 x w) is c x w, bit for bit
void instance_weights(const SharedMeta &s, const uint64_t *coeffs, sch::Fr *out) {
    for (uint32_t k = 0; k < s.K; ++k) {
        sch::Fr c, sc;
        std::memcpy(&c, coeffs + 4 * k, 32);
        sc = c; // coeff * 2^(5(M-1)) in Montgomery form = Montgomery form doubled 5(M-1) times
        for (uint32_t dbl = 0; dbl < 5 * (s.M[k] - 1); ++dbl) sc = sch::add(sc, sc);
        const std::vector<sch::Fr> &w = *s.unit[k];
        for (size_t i = 0; i < w.size(); ++i) *out++ = sch::mul(c, w[i]);
        for (size_t i = 0; i < w.size(); ++i) *out++ = sch::mul(sc, w[i]);
    }
}

namespace {
// The smallest n the batched kernel takes under policy "batch" = 1 (profiles/batch_bench.json).  Measured per call: about
// 70-150 us whatever n (wait for the tables' producers, one upload, the launch, num_vars round trips, the drain of the stream) plus
// 5-10 us per instance, against 65-130 us per instance for the serial plan -- so from n = 2 on the kernel wins everywhere (3x at n = 4),
// and at n = 1 it is level with or ahead of the serial plan except where ONE block has a long first round to itself: config 3's shape at
// 2^8 entries (14 combinations of 16 lanes: 8 passes over the pairs x 4 dependent products; 151 against 131 us).  The measure is
// tail_slices_blocks': passes over a combination's pairs x multiplicands; up to 16 (a GKR phase's shape at 2^10: 131 against 132 us)
// a lone instance runs batched.
uint32_t batch_min_n(const SharedMeta &s) {
    const int L = scd::bt_lanes(s.n_combos);
    const uint64_t pairs = 1ULL << (s.nv - 1), passes = (pairs + (uint64_t)L - 1) / (uint64_t)L;
    return passes * s.max_mult <= 16 ? 1 : 2;
}

bool device_waits_allowed(BatchArea &a) {
    if (scd::policy(scd::kPolPipeline) == 0) return false;
    for (const char *name : {"AMD_SERIALIZE_KERNEL", "HIP_LAUNCH_BLOCKING"}) {
        const char *v = std::getenv(name);
        if (v && std::atoi(v) != 0) return false;
    }
    return launches_are_async(&a.owner);
}

struct GateHold { // the device gate until release()
    const int device;
    bool held = true;
    explicit GateHold(int d) : device(d) { gate_lock(d); }
    void release() {
        if (held) gate_unlock(device);
        held = false;
    }
    ~GateHold() { release(); }
};
struct SlotHold {
    sc_prover *p;
    bool held;
    explicit SlotHold(sc_prover *p_) : p(p_), held(tail_slot_acquire(p_, false)) {}
    ~SlotHold() {
        if (held) tail_slot_release(p);
    }
};

enum { kInFlight = 0, kDone = 1, kGaveUp = 2 };

// What an entry point hands to the batched plan: the shape of the exchange with the host, and the three steps that differ.
struct BatchPages { // where a launch finds the call's pages
    char *d_up;     // device: the uploaded image
    uint32_t *ticket;
    uint64_t *h_msg;
    uint32_t *h_giveup;
    const uint64_t *mail;
    uint32_t mail_local, tag0, max_spins;
};
struct BatchJob {
    uint32_t n = 0, n_rounds = 0, D = 0; // instances; messages per instance (the challenge behind every one but the last is posted); evaluations per message
    bool poly_info = false;              // MLSumcheck::prove feeds PolynomialInfo first (mod.rs:54); GKRRoundSumcheck::prove continues the transcript as it is
    uint32_t max_mult = 0;
    bool inputs_on_device = false;       // read in place: their producers are waited for
    uint64_t occ_key = 0;                // identifies the launch shape of the occupancy query
    int plan = 0;
    const char *plan_name = "", *size_name = "nv"; // (the SC_HOST_TRACE line)
    uint32_t size = 0;
    size_t up_bytes = 0;                 // what is uploaded behind the ticket
    std::function<int(int)> blocks_per_cu;                                        // (device) -> resident blocks per CU of the kernel at this shape
    std::function<int(char *, char *)> fill;                                      // (h_up, d_up): write the image (pointers into it are d_up + offset)
    std::function<int(char *, char *, hipStream_t)> check_on_device;              // optional, behind the upload and in front of the launch: an argument error found on the device
    std::function<hipError_t(const BatchPages &, int, hipStream_t)> launch;      // (pages, grid, stream)
};

// The batched plan.  *took = false: nothing was proved and nothing written (the caller takes the serial plan); otherwise instances
// whose state is kGaveUp are left for the caller to prove again.
int run_batched(const BatchJob &job, sc_rng *const *rngs_or_null, uint64_t *out_proofs, uint64_t *out_rand_or_null, std::vector<uint8_t> &state, bool *took) {
    using clk = std::chrono::steady_clock;
    *took = false;
    const uint32_t n = job.n;
    AreaLease lease;
    if (!lease.held) return SC_OK;
    BatchArea &a = g_area;
    const int dev = sc_internal_device_ref();
    GateHold gate(dev);
    if (int rc = area_open(a, dev)) return rc;
    if (!device_waits_allowed(a)) return SC_OK;
    if (a.occ_key != job.occ_key) {
        a.occ_val = job.blocks_per_cu(dev);
        a.occ_key = job.occ_key;
    }
    const int per_cu = a.occ_val;
    if (per_cu < 1 || a.n_cus < 1) return SC_OK;
    SlotHold slot(&a.owner);
    if (!slot.held) return SC_OK;
    const auto t_begin = clk::now();

    // ---- layout of the call's data ---------------------------------------------------------------------------------------------------
    const size_t msg_words = (size_t)job.D * 8;
    const size_t up_bytes = job.up_bytes, d_bytes = 256 + up_bytes;
    const size_t msg_bytes = round_up((size_t)n * msg_words * 8, 256), giveup_bytes = round_up((size_t)n * 4, 256), mail_bytes = (size_t)n * 128;
    const size_t page_bytes = msg_bytes + giveup_bytes + mail_bytes;
    if (int rc = area_reserve(a, d_bytes, up_bytes)) return rc;
    if (a.page_cap < page_bytes) {
        if (a.h_page) (void)hipHostFree(a.h_page);
        a.h_page = nullptr;
        a.page_cap = 0;
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&a.h_page), page_bytes, hipHostMallocMapped | hipHostMallocCoherent));
        a.page_cap = page_bytes;
        std::memset(a.h_page, 0, page_bytes);
        HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&a.h_page_dev), a.h_page, 0));
    }
    bool vram = false;
    if (scd::policy(scd::kPolVramMailbox) != 0) {
        if (a.large_bar < 0) {
            int lb = 0;
            a.large_bar = hipDeviceGetAttribute(&lb, hipDeviceAttributeIsLargeBar, dev) == hipSuccess && lb ? 1 : 0;
        }
        if (a.large_bar == 1) {
            if (a.vmail_cap < mail_bytes) {
                if (a.d_vmail) (void)hipFree(a.d_vmail);
                a.d_vmail = nullptr;
                a.vmail_cap = 0;
                void *m = nullptr;
                if (hipExtMallocWithFlags(&m, mail_bytes, hipDeviceMallocFinegrained) == hipSuccess && hipMemsetAsync(m, 0, mail_bytes, a.stream) == hipSuccess &&
                    hipStreamSynchronize(a.stream) == hipSuccess) {
                    a.d_vmail = static_cast<uint64_t *>(m);
                    a.vmail_cap = mail_bytes;
                } else if (m) {
                    (void)hipFree(m);
                }
            }
            vram = a.d_vmail != nullptr;
        }
        (void)hipGetLastError();
    }
    if (a.gen >= (1u << 24)) { // (tags only ever grow; after 2^24 launches the pages start over)
        std::memset(a.h_page, 0, a.page_cap);
        if (a.d_vmail) HIP_TRY(hipMemset(a.d_vmail, 0, a.vmail_cap));
        a.gen = 0;
    }
    const uint32_t tag0 = ++a.gen << 6;

    // ---- upload: what the kernel reads behind the ticket, in one copy ------------------------------------------------------------------
    if (job.inputs_on_device) HIP_TRY(hipDeviceSynchronize()); // the inputs are read in place: their producers are waited for, as a copy would
    char *d_up = a.d_buf + 256;
    {
        int rc = job.fill(a.h_up, d_up);
        if (rc) return rc;
    }
    HIP_TRY(hipMemcpyAsync(d_up, a.h_up, up_bytes, hipMemcpyHostToDevice, a.stream));
    HIP_TRY(scd::launch_zero_words(reinterpret_cast<uint32_t *>(a.d_buf), 64, a.stream));
    if (job.check_on_device) {
        int rc = job.check_on_device(a.h_up, d_up, a.stream);
        if (rc) return rc;
    }

    // ---- launch ----------------------------------------------------------------------------------------------------------------------
    uint64_t *h_msg = reinterpret_cast<uint64_t *>(a.h_page);
    uint32_t *h_giveup = reinterpret_cast<uint32_t *>(a.h_page + msg_bytes);
    uint64_t *h_mail = reinterpret_cast<uint64_t *>(a.h_page + msg_bytes + giveup_bytes);
    BatchPages pg;
    pg.d_up = d_up;
    pg.ticket = reinterpret_cast<uint32_t *>(a.d_buf);
    pg.h_msg = reinterpret_cast<uint64_t *>(a.h_page_dev);
    pg.h_giveup = reinterpret_cast<uint32_t *>(a.h_page_dev + msg_bytes);
    pg.mail = vram ? a.d_vmail : reinterpret_cast<const uint64_t *>(a.h_page_dev + msg_bytes + giveup_bytes);
    pg.mail_local = vram ? 1u : 0u;
    pg.tag0 = tag0;
    pg.max_spins = scd::wait_spins_default();
    const int grid = (int)std::min<uint64_t>(n, (uint64_t)per_cu * (uint64_t)a.n_cus);
    static const bool trace = std::getenv("SC_HOST_TRACE") != nullptr; // stderr: one line per batch
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (trace && (hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess)) (void)hipGetLastError();
    if (ev0 && ev1) (void)hipEventRecord(ev0, a.stream);
    HIP_TRY(job.launch(pg, grid, a.stream));
    if (ev0 && ev1) (void)hipEventRecord(ev1, a.stream);
    scd::plan_hit(job.plan);
    *took = true;
    gate.release(); // the loop below makes no HIP calls

    // ---- the host's half: whichever instance has published, in any order -------------------------------------------------------------
    std::vector<sch::Blake2b512Rng> tr(n); // (the callers' transcripts are touched only by instances that complete)
    std::vector<uint32_t> round(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
        if (rngs_or_null) tr[i] = rngs_or_null[i]->rng;
        if (job.poly_info) tr[i].feed_poly_info(job.max_mult, job.n_rounds); // mod.rs:54
    }
    auto post = [&](uint32_t i, uint32_t tag, uint32_t slot_ix, const sch::Fr &vm) { // tail_post_challenge's two forms, into the instance's own slots
        if (vram) {
            volatile uint64_t *slot = a.d_vmail + (size_t)i * 16 + 8 * slot_ix;
            for (int q = 0; q < 8; ++q) slot[q] = ((uint64_t)(uint32_t)(vm.l[q >> 1] >> (32 * (q & 1))) << 32) | tag;
            __atomic_thread_fence(__ATOMIC_SEQ_CST); // (the mapping is write-combining: the fence pushes the eight words out)
        } else {
            uint64_t *slot = h_mail + (size_t)i * 16 + 8 * slot_ix;
            for (int q = 0; q < 8; ++q) __atomic_store_n(slot + q, ((uint64_t)(uint32_t)(vm.l[q >> 1] >> (32 * (q & 1))) << 32) | tag, __ATOMIC_RELEASE);
        }
    };
    uint32_t lo = 0, hi_seen = 0, remaining = n;
    uint64_t idle = 0;
    double hash_us = 0;
    auto t_progress = clk::now();
    bool dead = false;
    uint32_t words[9 * 8];
    while (remaining > 0) {
        // tickets are taken in order: an instance beyond (highest that has shown a message) + grid cannot have started
        const uint32_t end = (uint32_t)std::min<uint64_t>(n, (uint64_t)hi_seen + (uint64_t)grid + 1);
        bool progress = false;
        for (uint32_t i = lo; i < end; ++i) {
            if (state[i] != kInFlight) continue;
            const uint32_t tag = tag0 + round[i];
            const uint64_t *m = h_msg + (size_t)i * msg_words;
            bool all = (uint32_t)(__atomic_load_n(m + msg_words - 1, __ATOMIC_RELAXED) >> 32) == tag;
            for (size_t q = 0; all && q < msg_words; ++q) {
                const uint64_t w = __atomic_load_n(m + q, __ATOMIC_RELAXED);
                all = (uint32_t)(w >> 32) == tag;
                words[q] = (uint32_t)w;
            }
            if (!all) {
                const uint32_t g = __atomic_load_n(h_giveup + i, __ATOMIC_ACQUIRE);
                if (g >= tag0 && g < tag0 + 64) { // its block's wait expired: nothing of this instance is returned from here
                    state[i] = kGaveUp;
                    --remaining;
                    hi_seen = std::max(hi_seen, i + 1);
                    progress = true;
                }
                continue;
            }
            uint64_t *pm = out_proofs + ((size_t)i * job.n_rounds + round[i]) * job.D * 4;
            std::memcpy(pm, words, msg_words * 4);
            const auto h0 = trace ? clk::now() : clk::time_point();
            tr[i].feed_prover_msg(reinterpret_cast<const sch::Fr *>(pm), job.D); // mod.rs:61
            const sch::Fr vm = tr[i].sample_fr();                              // mod.rs:63
            if (trace) hash_us += std::chrono::duration<double, std::micro>(clk::now() - h0).count();
            if (out_rand_or_null) std::memcpy(out_rand_or_null + ((size_t)i * job.n_rounds + round[i]) * 4, &vm, 32);
            if (++round[i] < job.n_rounds) {
                post(i, tag, (round[i] - 1) & 1u, vm);
            } else {
                state[i] = kDone;
                --remaining;
                if (rngs_or_null) rngs_or_null[i]->rng = tr[i];
            }
            hi_seen = std::max(hi_seen, i + 1);
            progress = true;
        }
        while (lo < n && state[lo] != kInFlight) ++lo;
        if (progress) {
            idle = 0;
        } else if ((++idle & 0x3ff) == 0) {
            const auto now = clk::now();
            if (idle == 0x400) t_progress = now; // (the clock is read only once the loop has been idle for a while)
            else if (now - t_progress > publish_timeout()) {
                dead = true;
                break;
            }
        }
    }
    if (dead) { // ask every block to drop what it holds (and what it would take next), so that the stream drains
        for (uint32_t i = 0; i < n; ++i)
            if (state[i] == kInFlight) post(i, (tag0 + round[i]) ^ 0x80000000u, round[i] & 1u, sch::zero()); // (the wait behind the message the host never saw)
    }
    {
        DeviceGate g2(dev);
        (void)hipSetDevice(dev);
        const hipError_t e = hipStreamSynchronize(a.stream); // the kernel has left the GPU before the tail slot is given back
        float ms = 0;
        if (ev0 && ev1 && e == hipSuccess) (void)hipEventElapsedTime(&ms, ev0, ev1);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (trace) {
            uint32_t gave_up = 0;
            for (uint32_t i = 0; i < n; ++i) gave_up += state[i] == kGaveUp;
            std::fprintf(stderr, "[sc] batch: n %u, %s %u, plan %s, grid %d (%d per CU), mailbox %s, total %.1f us, kernel %.1f us, host hash %.1f us, gave up %u\n", n, job.size_name,
                         job.size, job.plan_name, grid, per_cu, vram ? "vram" : "host", std::chrono::duration<double, std::micro>(clk::now() - t_begin).count(), ms * 1e3, hash_us, gave_up);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return sc_internal_fail(SC_ERR_HIP, "hipStreamSynchronize failed after a batch: %s", hipGetErrorString(e));
        }
    }
    if (dead) return sc_internal_fail(SC_ERR_HIP, "a batched instance did not publish its message within the publish timeout");
    return SC_OK;
}

} // namespace

const char *first_structure_difference(const sc_poly_desc &a, const sc_poly_desc &b) {
    if (a.num_vars != b.num_vars) return "num_vars";
    if (a.max_multiplicands != b.max_multiplicands) return "max_multiplicands";
    if (a.n_products != b.n_products) return "n_products";
    if (a.n_tables != b.n_tables) return "n_tables";
    if (a.flags != b.flags) return "flags";
    if (a.n_products) {
        if (std::memcmp(a.prod_offsets, b.prod_offsets, (size_t)(a.n_products + 1) * 4) != 0) return "prod_offsets";
        if (std::memcmp(a.prod_indices, b.prod_indices, (size_t)a.prod_offsets[a.n_products] * 4) != 0) return "prod_indices";
    }
    return nullptr;
}

int batch_check_desc(const sc_poly_desc *descs, uint32_t i) {
    const int rc = validate_desc(&descs[i]); // prover_init panics on a constant before anything is proved (prover.rs:50-52)
    return rc ? prefix_instance(rc, i) : SC_OK;
}
int batch_check_structure(const sc_poly_desc *descs, uint32_t i) {
    if (const char *field = i ? first_structure_difference(descs[0], descs[i]) : nullptr)
        return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u differs from instance 0 in %s: a batch has one structure", i, field);
    return SC_OK;
}

void sc_internal_release_batch_cache() {
    std::lock_guard<std::mutex> lk(g_area.mu);
    g_area.free_all();
}

extern "C" int sc_ml_prove_batch(const sc_poly_desc *descs, uint32_t n, sc_rng *const *rngs_or_null, uint64_t *out_proofs, uint64_t *out_randomness_or_null) {
    if (n == 0) return SC_OK;
    if (!descs || !out_proofs) return sc_internal_fail(SC_ERR_BAD_ARG, "null argument");
    for (uint32_t i = 0; i < n; ++i) {
        if (int rc = batch_check_desc(descs, i)) return rc;
        if (rngs_or_null && !rngs_or_null[i]) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: null rng", i);
        if (int rc = batch_check_structure(descs, i)) return rc;
    }
    if (sc_device_count() <= 0) return sc_internal_fail(SC_ERR_HIP, "no HIP device visible: libsumcheck_hip has no CPU fallback");
    static const bool trace = std::getenv("SC_HOST_TRACE") != nullptr;
    const uint32_t nv = descs[0].num_vars, D = descs[0].max_multiplicands + 1;
    std::vector<uint8_t> state(n, kGaveUp); // (what the serial plan below proves)
    bool took = false;
    const int64_t pol = scd::policy(scd::kPolBatch);
    if (pol != 0 && descs[0].n_products > 0 && !(descs[0].flags & (SC_TABLES_STREAM | SC_NO_DEVICE_POLLING))) {
        SharedMeta s;
        build_shared(&descs[0], s);
        if (s.fits_args && scd::batch_shape_fits(s.nv, s.U, (int)s.K, (int)s.D, s.max_mult) && (pol == 2 || n >= batch_min_n(s))) {
            for (uint32_t k = 0; k < s.K; ++k) s.unit.push_back(unit_matrix(s.M[k], s.D));
            std::fill(state.begin(), state.end(), (uint8_t)kInFlight);
            // the uploaded image: table pointers | per-instance weights | host tables
            const bool host_tables = !(descs[0].flags & SC_TABLES_ON_DEVICE);
            const size_t table_bytes = (size_t)32 << s.nv;
            const size_t ptr_bytes = round_up((size_t)n * s.U * sizeof(void *), 256), w_bytes = round_up((size_t)n * s.w_elems * 32, 256);
            BatchJob job;
            job.n = n;
            job.n_rounds = s.nv;
            job.D = s.D;
            job.poly_info = true;
            job.max_mult = s.max_mult;
            job.inputs_on_device = !host_tables;
            job.occ_key = ((uint64_t)s.nv << 48) | ((uint64_t)s.U << 32) | ((uint64_t)s.K << 16) | s.D;
            job.plan = scd::kPlanBatchOneBlock;
            job.plan_name = "batch.one_block";
            job.size = s.nv;
            job.up_bytes = ptr_bytes + w_bytes + (host_tables ? (size_t)n * s.U * table_bytes : 0);
            job.blocks_per_cu = [&](int dev) { return scd::batch_blocks_per_cu(dev, s.nv, s.U, (int)s.K, (int)s.D); };
            job.fill = [&](char *h_up, char *d_up) -> int {
                const void **h_ptrs = reinterpret_cast<const void **>(h_up);
                sch::Fr *h_w = reinterpret_cast<sch::Fr *>(h_up + ptr_bytes);
                for (uint32_t i = 0; i < n; ++i) {
                    for (uint32_t k = 0; k < s.K; ++k) {
                        sch::Fr c;
                        std::memcpy(&c, descs[i].coeffs + 4 * k, 32);
                        if (sch::geq_p(c)) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: coefficient %u is not a canonical field element", i, k);
                    }
                    instance_weights(s, descs[i].coeffs, h_w + (size_t)i * s.w_elems);
                    for (uint32_t u = 0; u < s.U; ++u) {
                        if (host_tables) {
                            const size_t off = ptr_bytes + w_bytes + ((size_t)i * s.U + u) * table_bytes;
                            std::memcpy(h_up + off, descs[i].tables[u], table_bytes);
                            h_ptrs[(size_t)i * s.U + u] = d_up + off;
                        } else {
                            h_ptrs[(size_t)i * s.U + u] = descs[i].tables[u];
                        }
                    }
                }
                return SC_OK;
            };
            job.launch = [&](const BatchPages &pg, int grid, hipStream_t stream) -> hipError_t {
                scd::BatchArgs A;
                std::memset(&A, 0, sizeof(A));
                A.tables = reinterpret_cast<const uint4 *const *>(pg.d_up);
                A.Wm = reinterpret_cast<const uint4 *>(pg.d_up + ptr_bytes);
                A.w_stride = s.w_elems;
                A.n = n;
                A.n_tables = s.U;
                A.nv = s.nv;
                A.n_combos = s.n_combos;
                A.K = (int)s.K;
                A.D = (int)s.D;
                A.ticket = pg.ticket;
                A.h_msg = pg.h_msg;
                A.h_giveup = pg.h_giveup;
                A.mail = pg.mail;
                A.mail_local = pg.mail_local;
                A.tag0 = pg.tag0;
                A.max_spins = pg.max_spins;
                return scd::launch_batch_proofs(A, s.combo, s.fin, grid, stream);
            };
            int rc = run_batched(job, rngs_or_null, out_proofs, out_randomness_or_null, state, &took);
            if (rc) return rc;
            if (!took) std::fill(state.begin(), state.end(), (uint8_t)kGaveUp);
        }
    }
    // ---- the serial plan: everything (nothing ran batched), or the instances whose block gave up waiting -- those with device-side waits off
    uint32_t todo = 0;
    for (uint32_t i = 0; i < n; ++i) todo += state[i] != kDone;
    if (todo == 0) return SC_OK;
    const auto t0 = std::chrono::steady_clock::now();
    if (!took) scd::plan_hit(scd::kPlanBatchSerial);
    if (descs[0].flags & SC_TABLES_ON_DEVICE) { // read in place: whatever produced the tables is waited for, as a copy would
        const int dev = sc_internal_device_ref();
        DeviceGate gate_(dev);
        HIP_TRY(hipSetDevice(dev));
        HIP_TRY(hipDeviceSynchronize());
    }
    SerialRunner serial;
    serial.no_polling = took;
    for (uint32_t i = 0; i < n; ++i) {
        if (state[i] == kDone) continue;
        int rc = serial.prove(&descs[i], rngs_or_null ? rngs_or_null[i] : nullptr, out_proofs + (size_t)i * nv * D * 4,
                              out_randomness_or_null ? out_randomness_or_null + (size_t)i * nv * 4 : nullptr);
        if (rc) return prefix_instance(rc, i);
        if (took) g_stat[kStatProofRetries].fetch_add(1, std::memory_order_relaxed);
    }
    if (trace)
        std::fprintf(stderr, "[sc] batch: n %u, nv %u, plan batch.serial (%u instances%s), total %.1f us\n", n, nv, todo, took ? ", after an expired device-side wait" : "",
                     std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    return SC_OK;
}

// ---- sc_gkr_prove_batch ---------------------------------------------------------------------------------------------------------------
namespace {
// The smallest n the batched kernel takes under policy "batch" = 1 (profiles/gkr_batch_bench.json; compare batch_min_n).  Measured
// at dim 6 / 8 / 9 with nnz = 2 x 2^dim, device-resident inputs: ONE sc_gkr_prove costs 261 / 337 / 390 us (two initialisations with their
// launches and synchronisations, 2 x dim latency-bound rounds), a batched call of one instance 165 / 207 / 245 us (upload, the index check's
// round trip, the launch, 2 x dim round trips, the drain), and every further instance adds 13 / 17 / 20 us -- the host's one-thread
// transcript at 0.85 us per instance and round.  The kernel is ahead from n = 1 on at every dim of its envelope: there is no crossover.
uint32_t gkr_batch_min_n(uint32_t dim) {
    (void)dim;
    return 1;
}

int check_canonical(const uint64_t *elems, uint32_t n_elems, uint32_t i, const char *what) {
    for (uint32_t k = 0; k < n_elems; ++k) {
        sch::Fr e;
        std::memcpy(&e, elems + 4 * (size_t)k, 32);
        if (sch::geq_p(e)) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: %s[%u] is not a canonical field element", i, what, k);
    }
    return SC_OK;
}

// ---- what sc_gkr_prove_batch and sc_gkr_subclaim_batch (below) share: the callers' arrays, their checks, their place in the uploaded image
// (GkrBatchIn: prover_internal.hpp)
} // namespace
// sc_gkr_prove's checks on instance i (no HIP call); uv_or_null: the subclaim call's points u | v, checked behind g
int gkr_check_instance(const GkrBatchIn &in, uint32_t i, const uint64_t *uv_or_null) {
    if (in.nnz[i] >= (1ULL << 32)) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: nnz too large", i);
    if ((in.nnz[i] && (!in.f1_idx[i] || !in.f1_vals[i])) || !in.f2[i] || !in.f3[i] || !in.g[i]) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: null argument", i);
    if (int rc = check_canonical(in.g[i], in.dim, i, "g")) return rc;
    if (uv_or_null)
        if (int rc = check_canonical(uv_or_null, 2 * in.dim, i, "uv")) return rc;
    if (!in.on_device)
        for (uint64_t k = 0; k < in.nnz[i]; ++k)
            if ((in.f1_idx[i][k] >> (3 * in.dim)) != 0) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: f1 index %llu out of range", i, (unsigned long long)k);
    return SC_OK;
}
namespace {
// host inputs into the image, each distinct array once (one wiring predicate for many data instances is the usual case) -> per instance the
// offsets of idx, vals, f2, f3; empty for device inputs
std::vector<size_t> gkr_stage_inputs(const GkrBatchIn &in, StageMap &st) {
    std::vector<size_t> offs;
    if (in.on_device) return offs;
    const size_t N = (size_t)1 << in.dim;
    offs.resize((size_t)in.n * 4);
    for (uint32_t i = 0; i < in.n; ++i) {
        offs[4 * (size_t)i + 0] = in.nnz[i] ? st.add(in.f1_idx[i], (size_t)in.nnz[i] * 8) : st.base;
        offs[4 * (size_t)i + 1] = in.nnz[i] ? st.add(in.f1_vals[i], (size_t)in.nnz[i] * 32) : st.base;
        offs[4 * (size_t)i + 2] = st.add(in.f2[i], N * 32);
        offs[4 * (size_t)i + 3] = st.add(in.f3[i], N * 32);
    }
    return offs;
}
// instance i's record: its arrays where the kernel reads them (in place, or their staged copies in the image at d_up) and its point(s) at d_g
scd::GkrBatchInst gkr_record(const GkrBatchIn &in, uint32_t i, const std::vector<size_t> &offs, const char *d_up, const char *d_g) {
    scd::GkrBatchInst r;
    r.nnz = in.nnz[i];
    r.g = reinterpret_cast<const uint4 *>(d_g);
    if (in.on_device) {
        r.idx = in.f1_idx[i];
        r.vals = reinterpret_cast<const uint4 *>(in.f1_vals[i]);
        r.f2 = reinterpret_cast<const uint4 *>(in.f2[i]);
        r.f3 = reinterpret_cast<const uint4 *>(in.f3[i]);
    } else {
        r.idx = reinterpret_cast<const uint64_t *>(d_up + offs[4 * (size_t)i + 0]);
        r.vals = reinterpret_cast<const uint4 *>(d_up + offs[4 * (size_t)i + 1]);
        r.f2 = reinterpret_cast<const uint4 *>(d_up + offs[4 * (size_t)i + 2]);
        r.f3 = reinterpret_cast<const uint4 *>(d_up + offs[4 * (size_t)i + 3]);
    }
    return r;
}
} // namespace
// device-resident lists: their indices are checked on the device, in front of the launch (the kernels themselves mask every index they use);
// the flags (zeroed in the image) are at flag_off
int gkr_check_idx_on_device(const scd::GkrBatchInst *d_rec, uint32_t n, uint32_t dim, char *h_up, char *d_up, size_t flag_off, hipStream_t stream) {
    HIP_TRY(scd::launch_batch_gkr_idx_range(d_rec, n, dim, reinterpret_cast<uint32_t *>(d_up + flag_off), stream));
    HIP_TRY(hipMemcpyAsync(h_up + flag_off, d_up + flag_off, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const uint32_t *fl = reinterpret_cast<const uint32_t *>(h_up + flag_off);
    for (uint32_t i = 0; i < n; ++i)
        if (fl[i]) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: f1 has an index out of range", i);
    return SC_OK;
}

extern "C" int sc_gkr_prove_batch(uint32_t n, uint32_t dim, sc_rng *const *rngs, const uint64_t *const *f1_idx, const uint64_t *const *f1_vals, const uint64_t *nnz,
                                  const uint64_t *const *f2, const uint64_t *const *f3, const uint64_t *const *g, uint32_t flags, uint64_t *out_proofs, uint64_t *out_uv_or_null) {
    if (n == 0) return SC_OK;
    // ---- everything the host can check, before any HIP call (sc_gkr_prove's checks, per instance: the lowest failing instance decides) ----
    if (!rngs || !f1_idx || !f1_vals || !nnz || !f2 || !f3 || !g || !out_proofs) return sc_internal_fail(SC_ERR_BAD_ARG, "instance 0: null argument");
    if (dim == 0) return sc_internal_fail(SC_ERR_CONSTANT_POLY, "instance 0: Attempt to prove a constant.");
    if (dim > 21) return sc_internal_fail(SC_ERR_BAD_ARG, "instance 0: dim %u: 3*dim index bits do not fit 64-bit indices", dim);
    const bool dev_in = flags & SC_TABLES_ON_DEVICE;
    const GkrBatchIn in = {n, dim, f1_idx, f1_vals, nnz, f2, f3, g, dev_in};
    uint64_t nnz_max = 0;
    {
        std::unordered_set<const sc_rng *> seen;
        for (uint32_t i = 0; i < n; ++i) {
            if (!rngs[i]) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: null rng", i);
            if (!seen.insert(rngs[i]).second) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: its rng is also an earlier instance's: every instance continues a transcript of its own", i);
            if (int rc = gkr_check_instance(in, i, nullptr)) return rc;
            nnz_max = std::max(nnz_max, nnz[i]);
        }
    }
    if (sc_device_count() <= 0) return sc_internal_fail(SC_ERR_HIP, "no HIP device visible: libsumcheck_hip has no CPU fallback");
    static const bool trace = std::getenv("SC_HOST_TRACE") != nullptr;
    std::vector<uint8_t> state(n, kGaveUp); // (what the serial plan below proves)
    bool took = false;
    const int64_t pol = scd::policy(scd::kPolBatch);
    if (pol != 0 && scd::gkr_batch_shape_fits(dim, nnz_max) && (pol == 2 || n >= gkr_batch_min_n(dim))) {
        // both phases are one product of two tables with a coefficient of one (start_phase{1,2}_sumcheck, mod.rs:45-54, 66-82)
        const uint32_t offs[2] = {0, 2}, idx2[2] = {0, 1};
        sc_poly_desc d;
        std::memset(&d, 0, sizeof(d));
        d.num_vars = dim;
        d.max_multiplicands = 2;
        d.n_products = 1;
        d.coeffs = sch::kOne.l;
        d.prod_offsets = offs;
        d.prod_indices = idx2;
        d.n_tables = 2;
        SharedMeta s;
        build_shared(&d, s);
        s.unit.push_back(unit_matrix(2, 3));
        // the uploaded image: instance records | the matrices | the index check's flags | the points g | host inputs
        const size_t rec_bytes = round_up((size_t)n * sizeof(scd::GkrBatchInst), 256), w_bytes = round_up((size_t)s.w_elems * 32, 256);
        const size_t flag_bytes = round_up((size_t)n * 4, 256), g_bytes = round_up((size_t)n * dim * 32, 256);
        const size_t rec_off = 0, w_off = rec_bytes, flag_off = w_off + w_bytes, g_off = flag_off + flag_bytes;
        StageMap st;
        st.base = g_off + g_bytes;
        const std::vector<size_t> offs_in = gkr_stage_inputs(in, st);
        BatchJob job;
        job.n = n;
        job.n_rounds = 2 * dim;
        job.D = 3;
        job.poly_info = false;
        job.inputs_on_device = dev_in;
        job.occ_key = (1ULL << 63) | dim;
        job.plan = scd::kPlanBatchGkrOneBlock;
        job.plan_name = "batch.gkr_one_block";
        job.size_name = "dim";
        job.size = dim;
        job.up_bytes = st.base + st.bytes;
        job.blocks_per_cu = [&](int dv) { return scd::gkr_batch_blocks_per_cu(dv, dim); };
        job.fill = [&](char *h_up, char *d_up) -> int {
            scd::GkrBatchInst *rec = reinterpret_cast<scd::GkrBatchInst *>(h_up + rec_off);
            instance_weights(s, sch::kOne.l, reinterpret_cast<sch::Fr *>(h_up + w_off));
            std::memset(h_up + flag_off, 0, flag_bytes);
            st.copy_into(h_up);
            for (uint32_t i = 0; i < n; ++i) {
                const size_t gi = g_off + (size_t)i * dim * 32;
                std::memcpy(h_up + gi, g[i], (size_t)dim * 32);
                rec[i] = gkr_record(in, i, offs_in, d_up, d_up + gi);
            }
            return SC_OK;
        };
        if (dev_in)
            job.check_on_device = [&](char *h_up, char *d_up, hipStream_t stream) -> int {
                return gkr_check_idx_on_device(reinterpret_cast<const scd::GkrBatchInst *>(d_up + rec_off), n, dim, h_up, d_up, flag_off, stream);
            };
        job.launch = [&](const BatchPages &pg, int grid, hipStream_t stream) -> hipError_t {
            scd::BatchGkrArgs A;
            std::memset(&A, 0, sizeof(A));
            A.inst = reinterpret_cast<const scd::GkrBatchInst *>(pg.d_up + rec_off);
            A.Wm = reinterpret_cast<const uint4 *>(pg.d_up + w_off);
            A.n = n;
            A.dim = dim;
            A.ticket = pg.ticket;
            A.h_msg = pg.h_msg;
            A.h_giveup = pg.h_giveup;
            A.mail = pg.mail;
            A.mail_local = pg.mail_local;
            A.tag0 = pg.tag0;
            A.max_spins = pg.max_spins;
            return scd::launch_batch_gkr(A, s.combo, s.fin, grid, stream);
        };
        std::fill(state.begin(), state.end(), (uint8_t)kInFlight);
        int rc = run_batched(job, rngs, out_proofs, out_uv_or_null, state, &took);
        if (rc) return rc;
        if (!took) std::fill(state.begin(), state.end(), (uint8_t)kGaveUp);
    }
    // ---- the serial plan: everything (nothing ran batched), or the instances whose block gave up waiting -- those with device-side waits
    // off.  The callers' transcripts are worked on as copies and written back once every instance has been proved.
    uint32_t todo = 0;
    for (uint32_t i = 0; i < n; ++i) todo += state[i] != kDone;
    if (todo == 0) return SC_OK;
    const auto t0 = std::chrono::steady_clock::now();
    if (!took) scd::plan_hit(scd::kPlanBatchGkrSerial);
    std::vector<std::pair<uint32_t, sc_rng>> work;
    work.reserve(todo);
    for (uint32_t i = 0; i < n; ++i) {
        if (state[i] == kDone) continue;
        work.emplace_back(i, *rngs[i]);
        int rc = sc_internal_gkr_prove(&work.back().second, f1_idx[i], f1_vals[i], nnz[i], dim, f2[i], f3[i], g[i], flags, out_proofs + (size_t)i * 2 * dim * 12,
                                       out_uv_or_null ? out_uv_or_null + (size_t)i * 2 * dim * 4 : nullptr, took);
        if (rc) return prefix_instance(rc, i);
        if (took) g_stat[kStatProofRetries].fetch_add(1, std::memory_order_relaxed);
    }
    for (auto &w : work) rngs[w.first]->rng = w.second.rng;
    if (trace)
        std::fprintf(stderr, "[sc] batch: n %u, dim %u, plan batch.gkr_serial (%u instances%s), total %.1f us\n", n, dim, todo, took ? ", after an expired device-side wait" : "",
                     std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    return SC_OK;
}

// ---- sc_poly_evaluate_batch, sc_gkr_subclaim_batch: the oracle queries behind a batch of proofs -------------------------------------------
// What a caller of the two entry points above does next: evaluate every instance at the point its proof ended on.  Two plans, same bits:
//   batch.eval_one_block / batch.gkr_eval_one_block   kernels_batch_eval.hip: the whole batch in one launch (GKR: two, back to back) over the
//                    batch work areas -- one upload (pointers, points, host inputs: every distinct array once), the launch, one copy back,
//                    one synchronisation; the K x M (GKR: two) scalar products per instance that combine the values are host work, as in
//                    sc_poly_evaluate.  No kernel waits for the host: no mailbox, no tail slot;
//   batch.eval_serial / batch.gkr_eval_serial         instance after instance through sc_poly_evaluate / sc_sparse_evaluate inside the call:
//                    shapes beyond the kernels' envelope, policy "batch" = 0, the work areas held by a concurrent call.
namespace {
// The smallest n the kernels take under policy "batch" = 1 (profiles/eval_batch_bench.json; medians, us).  A batched call is one
// upload, one or two launches, one copy back and one synchronisation whatever n: 27-39 us for ONE instance of the c2 / config-3 shapes at
// 2^6 .. 2^10 entries (host or device tables) against 35-78 us for one sc_poly_evaluate, and 65 / 73 / 82 us for one GKR triple at dim 6 / 8 / 9
// against 130 / 144 / 170 us for sc_sparse_evaluate + 2 x sc_poly_evaluate: ahead by more than both spreads from n = 1 on, there is no
// handshake with the host to amortise.  Beyond 2^10 entries a lone table no longer hides behind the call's fixed cost -- ONE block per table
// walks 2^14 entries in 65 us where sc_poly_evaluate's grids take 55 -- so a lone instance above nv = 10 goes to the serial plan (at nv = 12
// the kernel's median is ahead, 37 against 49 us, but not by more than the spreads); at n = 16, the next measured size, the kernel is 13-20x
// ahead there too (a whole call of 16 at nv = 14 costs 67 us, what the loop pays for little more than one instance).
uint32_t eval_batch_min_n(uint32_t nv) { return nv <= 10 ? 1 : 16; }
uint32_t gkr_eval_batch_min_n() { return 1; }

// One batched call over the work areas: `fill` writes the image into pinned memory (pointers into it are d_up + offset), one copy uploads
// it, `launch` enqueues the kernels (it may synchronise to report an argument error found on the device), the image's out_bytes at out_off
// come back, `collect` reads them.  *took = false: the work areas are another call's -- nothing was done.
int run_eval_batched(size_t image_bytes, size_t out_off, size_t out_bytes, bool inputs_on_device, int plan, const std::function<void(char *, char *)> &fill,
                     const std::function<int(char *, char *, hipStream_t)> &launch, const std::function<void(const char *)> &collect, bool *took) {
    *took = false;
    AreaLease lease;
    if (!lease.held) return SC_OK;
    BatchArea &a = g_area;
    const int dev = sc_internal_device_ref();
    GateHold gate(dev);
    if (int rc = area_open(a, dev)) return rc;
    if (int rc = area_reserve(a, 256 + image_bytes, image_bytes)) return rc;
    if (inputs_on_device) HIP_TRY(hipDeviceSynchronize()); // the inputs are read in place: their producers are waited for, as a copy would
    char *d_up = a.d_buf + 256;
    fill(a.h_up, d_up);
    HIP_TRY(hipMemcpyAsync(d_up, a.h_up, out_off, hipMemcpyHostToDevice, a.stream));
    if (int rc = launch(a.h_up, d_up, a.stream)) return rc;
    scd::plan_hit(plan);
    HIP_TRY(hipMemcpyAsync(a.h_up + out_off, d_up + out_off, out_bytes, hipMemcpyDeviceToHost, a.stream));
    HIP_TRY(hipStreamSynchronize(a.stream));
    gate.release();
    collect(a.h_up + out_off);
    *took = true;
    return SC_OK;
}

// sc_poly_evaluate's argument checks on one descriptor of a batch (no HIP call)
int check_eval_desc(const sc_poly_desc *d, uint32_t i) {
    if (d->num_vars > 40) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: num_vars %u too large", i, d->num_vars);
    if (d->n_tables == 0 || !d->tables) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: no tables", i);
    if (d->n_products && (!d->coeffs || !d->prod_offsets || !d->prod_indices)) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: null product arrays", i);
    for (uint32_t k = 0; k < d->n_products; ++k) {
        if (d->prod_offsets[k + 1] <= d->prod_offsets[k]) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: product %u is empty", i, k);
        for (uint32_t q = d->prod_offsets[k]; q < d->prod_offsets[k + 1]; ++q)
            if (d->prod_indices[q] >= d->n_tables)
                return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: product %u refers to table %u >= %u", i, k, d->prod_indices[q], d->n_tables);
        sch::Fr c;
        std::memcpy(&c, d->coeffs + 4 * k, 32);
        if (sch::geq_p(c)) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: coefficient %u is not a canonical field element", i, k);
    }
    for (uint32_t u = 0; u < d->n_tables; ++u)
        if (!d->tables[u]) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: table %u is null", i, u);
    return SC_OK;
}
constexpr size_t kEvalImageMax = (size_t)1 << 30; // a batch whose staged inputs exceed this goes instance by instance
} // namespace

extern "C" int sc_poly_evaluate_batch(const sc_poly_desc *descs, uint32_t n, const uint64_t *points, uint64_t *out_values, uint64_t *out_table_values_or_null) {
    if (n == 0) return SC_OK;
    // ---- everything the host can check, before any HIP call: the lowest failing instance decides --------------------------------------
    if (!descs || !out_values || (descs[0].num_vars && !points)) return sc_internal_fail(SC_ERR_BAD_ARG, "instance 0: null argument");
    const uint32_t nv = descs[0].num_vars, U = descs[0].n_tables, K = descs[0].n_products;
    for (uint32_t i = 0; i < n; ++i) {
        if (int rc = check_eval_desc(&descs[i], i)) return rc;
        if (const char *field = i ? first_structure_difference(descs[0], descs[i]) : nullptr)
            return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u differs from instance 0 in %s: a batch has one structure", i, field);
        if (int rc = check_canonical(points + (size_t)i * nv * 4, nv, i, "point")) return rc;
    }
    if (sc_device_count() <= 0) return sc_internal_fail(SC_ERR_HIP, "no HIP device visible: libsumcheck_hip has no CPU fallback");
    auto combine = [&](uint32_t i, const sch::Fr *tv) { // sum_k c_k prod_j T_j(point): sc_poly_evaluate's K x M host products
        const sc_poly_desc &d = descs[i];
        sch::Fr acc = sch::zero();
        for (uint32_t k = 0; k < K; ++k) {
            sch::Fr pr;
            std::memcpy(&pr, d.coeffs + 4 * k, 32);
            for (uint32_t q = d.prod_offsets[k]; q < d.prod_offsets[k + 1]; ++q) pr = sch::mul(pr, tv[d.prod_indices[q]]);
            acc = sch::add(acc, pr);
        }
        std::memcpy(out_values + 4 * (size_t)i, &acc, 32);
        if (out_table_values_or_null) std::memcpy(out_table_values_or_null + (size_t)i * U * 4, tv, (size_t)U * 32);
    };
    const int64_t pol = scd::policy(scd::kPolBatch);
    const bool host_tables = !(descs[0].flags & SC_TABLES_ON_DEVICE);
    if (pol != 0 && scd::eval_batch_shape_fits(nv) && (uint64_t)n * U < (1ULL << 31) && (pol == 2 || n >= eval_batch_min_n(nv))) {
        // the image: table pointers | points | host tables, each distinct array once | the n x U values
        const size_t table_bytes = (size_t)32 << nv, blocks = (size_t)n * U;
        const size_t ptr_bytes = round_up(blocks * sizeof(void *), 256), pt_bytes = round_up((size_t)n * nv * 32, 256);
        StageMap st;
        st.base = ptr_bytes + pt_bytes;
        std::vector<size_t> tab_off;
        if (host_tables) {
            tab_off.resize(blocks);
            for (uint32_t i = 0; i < n; ++i)
                for (uint32_t u = 0; u < U; ++u) tab_off[(size_t)i * U + u] = st.add(descs[i].tables[u], table_bytes);
        }
        const size_t out_off = round_up(st.base + st.bytes, 256), out_bytes = blocks * 32;
        if (out_off + out_bytes <= kEvalImageMax) {
            bool took = false;
            int rc = run_eval_batched(
                out_off + out_bytes, out_off, out_bytes, !host_tables, scd::kPlanBatchEvalOneBlock,
                [&](char *h_up, char *d_up) {
                    const void **h_ptrs = reinterpret_cast<const void **>(h_up);
                    for (uint32_t i = 0; i < n; ++i)
                        for (uint32_t u = 0; u < U; ++u) h_ptrs[(size_t)i * U + u] = host_tables ? d_up + tab_off[(size_t)i * U + u] : (const void *)descs[i].tables[u];
                    if (nv) std::memcpy(h_up + ptr_bytes, points, (size_t)n * nv * 32);
                    st.copy_into(h_up);
                },
                [&](char *, char *d_up, hipStream_t stream) -> int {
                    scd::EvalBatchArgs A;
                    std::memset(&A, 0, sizeof(A));
                    A.tables = reinterpret_cast<const uint4 *const *>(d_up);
                    A.points = reinterpret_cast<const uint4 *>(d_up + ptr_bytes);
                    A.out = reinterpret_cast<uint4 *>(d_up + out_off);
                    A.nv = nv;
                    A.group_size = U;
                    A.pt_stride = nv;
                    A.out_stride = U;
                    HIP_TRY(scd::launch_batch_eval(A, (uint32_t)blocks, stream));
                    return SC_OK;
                },
                [&](const char *h_out) {
                    for (uint32_t i = 0; i < n; ++i) combine(i, reinterpret_cast<const sch::Fr *>(h_out) + (size_t)i * U);
                },
                &took);
            if (rc) return rc;
            if (took) return SC_OK;
        }
    }
    // ---- the serial plan: sc_poly_evaluate, instance after instance ----------------------------------------------------------------------
    scd::plan_hit(scd::kPlanBatchEvalSerial);
    for (uint32_t i = 0; i < n; ++i) {
        int rc = sc_poly_evaluate(&descs[i], nv ? points + (size_t)i * nv * 4 : nullptr, out_values + 4 * (size_t)i,
                                  out_table_values_or_null ? out_table_values_or_null + (size_t)i * U * 4 : nullptr);
        if (rc) return prefix_instance(rc, i);
    }
    return SC_OK;
}

extern "C" int sc_gkr_subclaim_batch(uint32_t n, uint32_t dim, const uint64_t *const *f1_idx, const uint64_t *const *f1_vals, const uint64_t *nnz, const uint64_t *const *f2,
                                     const uint64_t *const *f3, const uint64_t *const *g, const uint64_t *uv, uint32_t flags, uint64_t *out_evals) {
    if (n == 0) return SC_OK;
    // ---- everything the host can check, before any HIP call: the lowest failing instance decides --------------------------------------
    if (!f1_idx || !f1_vals || !nnz || !f2 || !f3 || !g || !uv || !out_evals) return sc_internal_fail(SC_ERR_BAD_ARG, "instance 0: null argument");
    if (dim == 0) return sc_internal_fail(SC_ERR_BAD_ARG, "instance 0: dim 0: a GKR round has at least one variable per component");
    if (dim > 21) return sc_internal_fail(SC_ERR_BAD_ARG, "instance 0: dim %u: 3*dim index bits do not fit 64-bit indices", dim);
    const bool dev_in = flags & SC_TABLES_ON_DEVICE;
    const GkrBatchIn in = {n, dim, f1_idx, f1_vals, nnz, f2, f3, g, dev_in};
    uint64_t nnz_max = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (int rc = gkr_check_instance(in, i, uv + (size_t)i * 2 * dim * 4)) return rc;
        nnz_max = std::max(nnz_max, nnz[i]);
    }
    if (sc_device_count() <= 0) return sc_internal_fail(SC_ERR_HIP, "no HIP device visible: libsumcheck_hip has no CPU fallback");
    auto finish = [&](uint32_t i, const sch::Fr &a1, const sch::Fr &a2, const sch::Fr &a3) { // f1(g,u,v), f2(u), f3(v), their product (data_structures.rs:53-55)
        const sch::Fr e[4] = {a1, a2, a3, sch::mul(sch::mul(a1, a2), a3)};
        std::memcpy(out_evals + (size_t)i * 16, e, 128);
    };
    const int64_t pol = scd::policy(scd::kPolBatch);
    if (pol != 0 && scd::gkr_eval_batch_shape_fits(dim, nnz_max) && scd::eval_batch_shape_fits(dim) && (pol == 2 || n >= gkr_eval_batch_min_n())) {
        // the image: instance records | the index check's flags | g | u | v per instance | (f2, f3) pointers | host inputs | the n x 3 values
        const size_t rec_bytes = round_up((size_t)n * sizeof(scd::GkrBatchInst), 256), flag_bytes = round_up((size_t)n * 4, 256);
        const size_t pt_bytes = round_up((size_t)n * 3 * dim * 32, 256), ptr_bytes = round_up((size_t)n * 2 * sizeof(void *), 256);
        const size_t flag_off = rec_bytes, pt_off = flag_off + flag_bytes, ptr_off = pt_off + pt_bytes;
        StageMap st;
        st.base = ptr_off + ptr_bytes;
        const std::vector<size_t> offs_in = gkr_stage_inputs(in, st);
        const size_t out_off = round_up(st.base + st.bytes, 256), out_bytes = (size_t)n * 3 * 32;
        if (out_off + out_bytes <= kEvalImageMax) {
            bool took = false;
            int rc = run_eval_batched(
                out_off + out_bytes, out_off, out_bytes, dev_in, scd::kPlanBatchGkrEvalOneBlock,
                [&](char *h_up, char *d_up) {
                    scd::GkrBatchInst *rec = reinterpret_cast<scd::GkrBatchInst *>(h_up);
                    const void **h_ptrs = reinterpret_cast<const void **>(h_up + ptr_off);
                    std::memset(h_up + flag_off, 0, flag_bytes);
                    st.copy_into(h_up);
                    for (uint32_t i = 0; i < n; ++i) {
                        const size_t pi = pt_off + (size_t)i * 3 * dim * 32; // g | u | v
                        std::memcpy(h_up + pi, g[i], (size_t)dim * 32);
                        std::memcpy(h_up + pi + (size_t)dim * 32, uv + (size_t)i * 2 * dim * 4, (size_t)2 * dim * 32);
                        rec[i] = gkr_record(in, i, offs_in, d_up, d_up + pi);
                        h_ptrs[2 * (size_t)i] = rec[i].f2;
                        h_ptrs[2 * (size_t)i + 1] = rec[i].f3;
                    }
                },
                [&](char *h_up, char *d_up, hipStream_t stream) -> int {
                    const scd::GkrBatchInst *d_rec = reinterpret_cast<const scd::GkrBatchInst *>(d_up);
                    if (dev_in)
                        if (int rc = gkr_check_idx_on_device(d_rec, n, dim, h_up, d_up, flag_off, stream)) return rc;
                    uint4 *d_out = reinterpret_cast<uint4 *>(d_up + out_off);
                    HIP_TRY(scd::launch_batch_gkr_eval(d_rec, n, dim, d_out, 3, stream));
                    scd::EvalBatchArgs A; // f2 at u and f3 at v: 2 n tables of dim variables, points inside the instance's g | u | v
                    std::memset(&A, 0, sizeof(A));
                    A.tables = reinterpret_cast<const uint4 *const *>(d_up + ptr_off);
                    A.points = reinterpret_cast<const uint4 *>(d_up + pt_off);
                    A.out = d_out;
                    A.nv = dim;
                    A.group_size = 2;
                    A.pt_stride = 3 * dim;
                    A.pt_base = dim;
                    A.pt_step = dim;
                    A.out_stride = 3;
                    A.out_base = 1;
                    HIP_TRY(scd::launch_batch_eval(A, 2 * n, stream));
                    return SC_OK;
                },
                [&](const char *h_out) {
                    const sch::Fr *v = reinterpret_cast<const sch::Fr *>(h_out);
                    for (uint32_t i = 0; i < n; ++i) finish(i, v[3 * (size_t)i], v[3 * (size_t)i + 1], v[3 * (size_t)i + 2]);
                },
                &took);
            if (rc) return rc;
            if (took) return SC_OK;
        }
    }
    // ---- the serial plan: sc_sparse_evaluate at g | u | v (a host list: a device-resident one is copied, each distinct list once, and its
    // indices checked before anything is written) and sc_poly_evaluate of the one-table polynomials, instance after instance ---------------
    scd::plan_hit(scd::kPlanBatchGkrEvalSerial);
    std::map<const void *, std::vector<uint64_t>> host_copy; // device pointer -> its host copy (indices, values)
    auto on_host = [&](const uint64_t *src, size_t words, const uint64_t **out) -> int {
        if (!dev_in || words == 0) {
            *out = src;
            return SC_OK;
        }
        auto it = host_copy.find(src);
        if (it == host_copy.end() || it->second.size() < words) {
            std::vector<uint64_t> buf(words);
            const int dev = sc_internal_device_ref();
            DeviceGate gate_(dev);
            HIP_TRY(hipSetDevice(dev));
            HIP_TRY(hipMemcpy(buf.data(), src, words * 8, hipMemcpyDeviceToHost)); // (waits for whatever produced the list, as a copy does)
            it = host_copy.insert_or_assign(src, std::move(buf)).first;
        }
        *out = it->second.data();
        return SC_OK;
    };
    if (dev_in)
        for (uint32_t i = 0; i < n; ++i) {
            const uint64_t *idx = nullptr;
            if (int rc = on_host(f1_idx[i], (size_t)nnz[i], &idx)) return rc;
            for (uint64_t k = 0; k < nnz[i]; ++k)
                if ((idx[k] >> (3 * dim)) != 0) return sc_internal_fail(SC_ERR_BAD_ARG, "instance %u: f1 has an index out of range", i);
        }
    const uint32_t offs[2] = {0, 1}, idx0[1] = {0};
    std::vector<uint64_t> guv((size_t)3 * dim * 4);
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t *u = uv + (size_t)i * 2 * dim * 4, *v = u + (size_t)dim * 4, *idx = nullptr, *vals = nullptr;
        std::memcpy(guv.data(), g[i], (size_t)dim * 32);
        std::memcpy(guv.data() + (size_t)dim * 4, u, (size_t)2 * dim * 32);
        int rc = on_host(f1_idx[i], (size_t)nnz[i], &idx);
        if (!rc) rc = on_host(f1_vals[i], (size_t)nnz[i] * 4, &vals);
        if (rc) return rc;
        sch::Fr a[3];
        rc = sc_sparse_evaluate(idx, vals, nnz[i], 3 * dim, guv.data(), a[0].l);
        for (int t = 0; t < 2 && !rc; ++t) {
            const uint64_t *tab[1] = {t == 0 ? f2[i] : f3[i]};
            sc_poly_desc d;
            std::memset(&d, 0, sizeof(d));
            d.num_vars = dim;
            d.max_multiplicands = 1;
            d.n_products = 1;
            d.coeffs = sch::kOne.l; // one x T(point) is T(point), bit for bit
            d.prod_offsets = offs;
            d.prod_indices = idx0;
            d.n_tables = 1;
            d.tables = tab;
            d.flags = dev_in ? (uint32_t)SC_TABLES_ON_DEVICE : 0u;
            rc = sc_poly_evaluate(&d, t == 0 ? u : v, a[1 + t].l, nullptr);
        }
        if (rc) return prefix_instance(rc, i);
        finish(i, a[0], a[1], a[2]);
    }
    return SC_OK;
}
