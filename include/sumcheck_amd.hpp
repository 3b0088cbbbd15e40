// sumcheck_amd.hpp -- header-only C++17 host-side mirror of arkworks-rs/sumcheck's public interface over the C ABI of
// libsumcheck_hip.so (include/sumcheck_hip.h).  Same names, argument meaning and error behaviour as the reference:
//
//   ListOfProductsOfPolynomials, PolynomialInfo      reference src/ml_sumcheck/data_structures.rs:25-110
//   ProverState, ProverMsg, IPForMLSumcheck          reference src/ml_sumcheck/protocol/prover.rs:13-153
//   VerifierMsg, SubClaim                            reference src/ml_sumcheck/protocol/verifier.rs:10-34
//   MLSumcheck                                       reference src/ml_sumcheck/mod.rs:18-101
//   Blake2b512Rng                                    reference src/rng.rs:22-81
//   SparseMultilinearExtension, GKRRoundSumcheck     reference src/gkr_round_sumcheck/mod.rs:22-193
//
// The reference is Rust; this is the compiled-language host layer for an image without a Rust toolchain (the Rust
// binding itself is rust-shim/).  The reference's panic!s surface as sumcheck::Panic carrying the same message;
// verifier rejection as sumcheck::Reject.  All prove_round work happens on the GPU inside the library.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "sumcheck_hip.h"

namespace sumcheck {

struct Panic : std::runtime_error {
    int code;
    Panic(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};
struct Reject : std::runtime_error { // crate::Error::Reject
    explicit Reject(const std::string &m) : std::runtime_error(m) {}
};
inline void check(int rc) {
    if (rc == SC_OK) return;
    const std::string msg = sc_last_error();
    if (rc == SC_ERR_REJECT) throw Reject(msg);
    throw Panic(rc, msg);
}

// BLS12-381 Fr: 4 x u64 Montgomery limbs, the layout of ark_ff::Fp<MontBackend<FrConfig,4>,4>
struct Fr {
    uint64_t l[4] = {0, 0, 0, 0};
    bool operator==(const Fr &o) const { return std::memcmp(l, o.l, 32) == 0; }
    bool operator!=(const Fr &o) const { return !(*this == o); }
    static Fr one() { return Fr{{0x00000001fffffffeULL, 0x5884b7fa00034802ULL, 0x998c4fefecbc4ff5ULL, 0x1824b159acc5056fULL}}; }
    static Fr zero() { return Fr{}; }
    // a valid ark_ff::Fp holds a residue < p; anything else is not a field element (operator+ below relies on it)
    bool is_canonical() const {
        static const uint64_t P[4] = {0xffffffff00000001ULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL, 0x73eda753299d7d48ULL};
        for (int i = 3; i >= 0; --i)
            if (l[i] != P[i]) return l[i] < P[i];
        return false;
    }
    // a + b mod p (host; only extract_sum needs it)
    friend Fr operator+(const Fr &a, const Fr &b) {
        static const uint64_t P[4] = {0xffffffff00000001ULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL, 0x73eda753299d7d48ULL};
        Fr r;
        unsigned __int128 c = 0;
        for (int i = 0; i < 4; ++i) {
            c += (unsigned __int128)a.l[i] + b.l[i];
            r.l[i] = (uint64_t)c;
            c >>= 64;
        }
        bool ge = true;
        for (int i = 3; i >= 0; --i)
            if (r.l[i] != P[i]) {
                ge = r.l[i] > P[i];
                break;
            }
        if (ge) {
            uint64_t borrow = 0;
            for (int i = 0; i < 4; ++i) {
                unsigned __int128 d = (unsigned __int128)r.l[i] - P[i] - borrow;
                r.l[i] = (uint64_t)d;
                borrow = (uint64_t)(d >> 64) & 1;
            }
        }
        return r;
    }
};
static_assert(sizeof(Fr) == 32, "Fr must be 4 x u64");

class Blake2b512Rng { // FeedableRNG + RngCore
  public:
    Blake2b512Rng() : h_(sc_rng_setup()) {}
    static Blake2b512Rng setup() { return Blake2b512Rng(); }
    Blake2b512Rng(Blake2b512Rng &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Blake2b512Rng(const Blake2b512Rng &) = delete;
    ~Blake2b512Rng() {
        if (h_) sc_rng_free(h_);
    }
    void feed(const void *bytes, size_t len) { sc_rng_feed_bytes(h_, static_cast<const uint8_t *>(bytes), len); }
    void feed(const std::string &s) { feed(s.data(), s.size()); }
    void fill_bytes(uint8_t *dest, size_t len) { sc_rng_fill_bytes(h_, dest, len); }
    uint64_t next_u64() {
        uint8_t t[8];
        fill_bytes(t, 8);
        uint64_t x;
        std::memcpy(&x, t, 8);
        return x;
    }
    Fr rand_fr() { // F::rand(rng)
        Fr r;
        sc_rng_sample_fr(h_, r.l);
        return r;
    }
    sc_rng *raw() { return h_; }

  private:
    sc_rng *h_;
};

struct DenseMultilinearExtension {
    size_t num_vars = 0;
    std::vector<Fr> evaluations;
    static DenseMultilinearExtension from_evaluations_vec(size_t num_vars, std::vector<Fr> ev) {
        if (ev.size() != (size_t(1) << num_vars)) throw Panic(SC_ERR_BAD_ARG, "The size of evaluations should be 2^num_vars.");
        return DenseMultilinearExtension{num_vars, std::move(ev)};
    }
    static DenseMultilinearExtension rand(size_t num_vars, Blake2b512Rng &rng) {
        std::vector<Fr> ev(size_t(1) << num_vars);
        for (auto &x : ev) x = rng.rand_fr();
        return DenseMultilinearExtension{num_vars, std::move(ev)};
    }
    const Fr &operator[](size_t i) const { return evaluations[i]; }
    DenseMultilinearExtension fix_variables(const std::vector<Fr> &partial_point) const {
        if (partial_point.size() > num_vars) throw Panic(SC_ERR_BAD_ARG, "invalid partial point dimension");
        DenseMultilinearExtension out{num_vars - partial_point.size(), std::vector<Fr>(size_t(1) << (num_vars - partial_point.size()))};
        check(sc_fix_variables(evaluations[0].l, (uint32_t)num_vars, partial_point.empty() ? nullptr : partial_point[0].l,
                               (uint32_t)partial_point.size(), out.evaluations[0].l, 0));
        return out;
    }
    Fr evaluate(const std::vector<Fr> &point) const {
        if (point.size() != num_vars) throw Panic(SC_ERR_BAD_ARG, "invalid size of partial point");
        return fix_variables(point).evaluations[0];
    }
};

struct PolynomialInfo {
    size_t max_multiplicands = 0, num_variables = 0;
};

class ListOfProductsOfPolynomials {
  public:
    size_t max_multiplicands = 0;
    size_t num_variables;
    std::vector<std::pair<Fr, std::vector<size_t>>> products;
    std::vector<std::shared_ptr<DenseMultilinearExtension>> flattened_ml_extensions;

    explicit ListOfProductsOfPolynomials(size_t nv) : num_variables(nv) {}
    static ListOfProductsOfPolynomials new_(size_t nv) { return ListOfProductsOfPolynomials(nv); }
    PolynomialInfo info() const { return PolynomialInfo{max_multiplicands, num_variables}; }
    // data_structures.rs:71-96: multiplicands shared by pointer are stored once
    void add_product(const std::vector<std::shared_ptr<DenseMultilinearExtension>> &product, const Fr &coefficient) {
        if (product.empty()) throw Panic(SC_ERR_BAD_ARG, "assertion failed: !product.is_empty()");
        max_multiplicands = std::max(max_multiplicands, product.size());
        std::vector<size_t> indexed;
        for (const auto &m : product) {
            if (m->num_vars != num_variables) throw Panic(SC_ERR_BAD_ARG, "product has a multiplicand with wrong number of variables");
            auto it = lookup_.find(m.get());
            if (it != lookup_.end()) {
                indexed.push_back(it->second);
            } else {
                const size_t idx = flattened_ml_extensions.size();
                flattened_ml_extensions.push_back(m);
                lookup_[m.get()] = idx;
                indexed.push_back(idx);
            }
        }
        products.emplace_back(coefficient, std::move(indexed));
    }

    // marshalled view for the C ABI (valid while *this is alive and unchanged)
    struct Desc {
        sc_poly_desc d;
        std::vector<Fr> coeffs;
        std::vector<uint32_t> offsets, indices;
        std::vector<const uint64_t *> tables;
    };
    std::unique_ptr<Desc> desc() const {
        auto D = std::make_unique<Desc>();
        D->offsets.push_back(0);
        for (const auto &pr : products) {
            D->coeffs.push_back(pr.first);
            for (size_t i : pr.second) D->indices.push_back((uint32_t)i);
            D->offsets.push_back((uint32_t)D->indices.size());
        }
        for (const auto &t : flattened_ml_extensions) D->tables.push_back(t->evaluations[0].l);
        std::memset(&D->d, 0, sizeof(D->d));
        D->d.num_vars = (uint32_t)num_variables;
        D->d.max_multiplicands = (uint32_t)max_multiplicands;
        D->d.n_products = (uint32_t)products.size();
        D->d.coeffs = D->coeffs.empty() ? nullptr : D->coeffs[0].l;
        D->d.prod_offsets = D->offsets.data();
        D->d.prod_indices = D->indices.data();
        D->d.n_tables = (uint32_t)D->tables.size();
        D->d.tables = D->tables.data();
        return D;
    }

  private:
    std::unordered_map<const DenseMultilinearExtension *, size_t> lookup_;
};

struct ProverMsg {
    std::vector<Fr> evaluations;
};
struct VerifierMsg {
    Fr randomness;
};
struct SubClaim {
    std::vector<Fr> point;
    Fr expected_evaluation;
};
using Proof = std::vector<ProverMsg>;

class ProverState { // prover.rs:19-33, tables resident in HBM
  public:
    size_t num_vars = 0, max_multiplicands = 0;
    std::vector<std::pair<Fr, std::vector<size_t>>> list_of_products;
    ProverState() = default;
    ProverState(sc_prover *h, const ListOfProductsOfPolynomials &p)
        : num_vars(p.num_variables), max_multiplicands(p.max_multiplicands), list_of_products(p.products), h_(h),
          n_tables_(p.flattened_ml_extensions.size()) {}
    ProverState(ProverState &&o) noexcept { *this = std::move(o); }
    ProverState &operator=(ProverState &&o) noexcept {
        if (h_) sc_prover_free(h_);
        num_vars = o.num_vars;
        max_multiplicands = o.max_multiplicands;
        list_of_products = std::move(o.list_of_products);
        h_ = o.h_;
        n_tables_ = o.n_tables_;
        o.h_ = nullptr;
        return *this;
    }
    ~ProverState() {
        if (h_) sc_prover_free(h_);
    }
    size_t round() const {
        uint32_t r = 0;
        check(sc_prover_state(h_, nullptr, nullptr, nullptr, &r));
        return r;
    }
    std::vector<Fr> randomness() const {
        std::vector<Fr> buf(num_vars + 1);
        uint32_t n = 0;
        check(sc_prover_state(h_, buf[0].l, &n, nullptr, nullptr));
        buf.resize(n);
        return buf;
    }
    std::vector<DenseMultilinearExtension> flattened_ml_extensions() const {
        const size_t r = round();
        const size_t nv = num_vars - (r > 0 ? r - 1 : 0);
        std::vector<Fr> buf(n_tables_ << nv);
        check(sc_prover_state(h_, nullptr, nullptr, buf[0].l, nullptr));
        std::vector<DenseMultilinearExtension> out;
        for (size_t u = 0; u < n_tables_; ++u)
            out.push_back(DenseMultilinearExtension{nv, std::vector<Fr>(buf.begin() + (u << nv), buf.begin() + ((u + 1) << nv))});
        return out;
    }
    sc_prover *raw() { return h_; }
    // library policy (no reference counterpart): false = no kernel of this handle ever waits for the host (a host with HIP streams of its
    // own: see the interference contract in sumcheck_hip.h); patience of the resident kernel behind prove_round called round by round
    void set_polling(bool allow) { check(sc_prover_set_polling(h_, allow ? 1 : 0)); }
    void set_resident(uint32_t patience_polls) { check(sc_prover_set_resident(h_, patience_polls)); }

  private:
    sc_prover *h_ = nullptr;
    size_t n_tables_ = 0;
};

// n x ProverState of ONE structure behind one sc_batch_prover handle: IPForMLSumcheck::prover_init_batch / prove_round_batch.  The caller owns
// the transcript(s) and hands in every challenge: one VerifierMsg per instance, or one for all of them.
class BatchProverState {
  public:
    size_t n = 0, num_vars = 0, max_multiplicands = 0;
    BatchProverState() = default;
    BatchProverState(sc_batch_prover *h, size_t n_, const ListOfProductsOfPolynomials &p)
        : n(n_), num_vars(p.num_variables), max_multiplicands(p.max_multiplicands), h_(h), n_tables_(p.flattened_ml_extensions.size()) {}
    BatchProverState(BatchProverState &&o) noexcept { *this = std::move(o); }
    BatchProverState &operator=(BatchProverState &&o) noexcept {
        if (h_) sc_batch_prover_free(h_);
        n = o.n;
        num_vars = o.num_vars;
        max_multiplicands = o.max_multiplicands;
        h_ = o.h_;
        n_tables_ = o.n_tables_;
        o.h_ = nullptr;
        return *this;
    }
    ~BatchProverState() {
        if (h_) sc_batch_prover_free(h_);
    }
    size_t round() const {
        uint32_t r = 0;
        check(sc_batch_prover_state(h_, 0, nullptr, nullptr, nullptr, &r));
        return r;
    }
    std::vector<Fr> randomness(size_t i) const {
        uint32_t cnt = 0;
        check(sc_batch_prover_state(h_, (uint32_t)i, nullptr, &cnt, nullptr, nullptr));
        std::vector<Fr> buf(std::max<size_t>(cnt, 1));
        check(sc_batch_prover_state(h_, (uint32_t)i, buf[0].l, nullptr, nullptr, nullptr));
        buf.resize(cnt);
        return buf;
    }
    std::vector<DenseMultilinearExtension> flattened_ml_extensions(size_t i) const {
        const size_t r = round();
        const size_t nv = num_vars - (r > 0 ? r - 1 : 0);
        std::vector<Fr> buf(n_tables_ << nv);
        check(sc_batch_prover_state(h_, (uint32_t)i, nullptr, nullptr, buf[0].l, nullptr));
        std::vector<DenseMultilinearExtension> out;
        for (size_t u = 0; u < n_tables_; ++u)
            out.push_back(DenseMultilinearExtension{nv, std::vector<Fr>(buf.begin() + (u << nv), buf.begin() + ((u + 1) << nv))});
        return out;
    }
    // prove_as_subprotocol's final push without a bind (mod.rs:65-67)
    void push_randomness(const std::vector<VerifierMsg> &v_msgs) {
        const std::vector<Fr> r = challenges(v_msgs);
        check(sc_batch_prover_push_randomness(h_, r[0].l, v_msgs.size() == 1 && n != 1 ? 1u : 0u));
    }
    // bind the last variable after the last round: per instance the U table evaluations at its point; the handle is exhausted until reset
    std::vector<std::vector<Fr>> bind_final(const std::vector<VerifierMsg> &v_msgs) {
        const std::vector<Fr> r = challenges(v_msgs);
        std::vector<Fr> flat(n * std::max<size_t>(n_tables_, 1));
        check(sc_batch_prover_bind_final(h_, r[0].l, v_msgs.size() == 1 && n != 1 ? 1u : 0u, flat[0].l));
        std::vector<std::vector<Fr>> out(n);
        for (size_t i = 0; i < n; ++i) out[i].assign(flat.begin() + i * n_tables_, flat.begin() + (i + 1) * n_tables_);
        return out;
    }
    // rewind to round 0 without reallocating: over the tables the handle holds, or over n new polynomials of the same structure
    void reset() { check(sc_batch_prover_reset(h_, nullptr)); }
    void reset(const std::vector<const ListOfProductsOfPolynomials *> &polynomials) {
        if (polynomials.size() != n) throw Panic(SC_ERR_BAD_ARG, "one polynomial per instance of the handle");
        std::vector<std::unique_ptr<ListOfProductsOfPolynomials::Desc>> keep;
        std::vector<sc_poly_desc> descs;
        for (const ListOfProductsOfPolynomials *p : polynomials) {
            if (!p) throw Panic(SC_ERR_BAD_ARG, "null polynomial");
            keep.push_back(p->desc());
            descs.push_back(keep.back()->d);
        }
        check(sc_batch_prover_reset(h_, descs.data()));
    }
    sc_batch_prover *raw() { return h_; }
    // n challenges, or ONE for all instances, as the library takes them
    std::vector<Fr> challenges(const std::vector<VerifierMsg> &v_msgs) const {
        if (v_msgs.size() != n && v_msgs.size() != 1) throw Panic(SC_ERR_BAD_ARG, "one VerifierMsg per instance, or a single one for all");
        std::vector<Fr> r;
        for (const VerifierMsg &m : v_msgs) r.push_back(m.randomness);
        return r;
    }

  private:
    sc_batch_prover *h_ = nullptr;
    size_t n_tables_ = 0;
};

// The library keeps device memory between calls (the last prover it built, the work areas of evaluate / fix_variables, the GKR
// scratch) so that one-shot calls cost what kept state costs; this returns all of it.
inline void release_caches() { check(sc_release_caches()); }
inline void set_cache_limit(uint64_t bytes) { check(sc_set_cache_limit(bytes)); } // what each of those caches may keep; 0 = nothing

struct IPForMLSumcheck {
    static ProverState prover_init(const ListOfProductsOfPolynomials &polynomial) { // prover.rs:49-69
        auto D = polynomial.desc();
        sc_prover *h = nullptr;
        check(sc_prover_init(&D->d, &h));
        return ProverState(h, polynomial);
    }
    static ProverMsg prove_round(ProverState &state, const std::optional<VerifierMsg> &v_msg) { // prover.rs:74-153
        ProverMsg m;
        m.evaluations.resize(state.max_multiplicands + 1);
        check(sc_prove_round(state.raw(), v_msg ? v_msg->randomness.l : nullptr, m.evaluations[0].l));
        return m;
    }
    // n x prover_init of ONE structure behind one handle (sc_batch_prover_init); the tables are copied.  Shapes beyond one block's LDS run n
    // ordinary provers inside the handle (plan batch.rounds_serial) unless sc_set_policy("batch_slices", 1) is in effect when the handle is built
    // (default 0): then, for 1 <= num_vars <= 16, products of at most eight multiplicands and a work area (96 bytes x n x tables x 2^num_vars)
    // of at most 16 GiB, the rounds whose tables do not fit one block give every instance to several blocks (plan batch.rounds_slices: two
    // launches a round) and the later rounds run as within the envelope, with the same bits
    static BatchProverState prover_init_batch(const std::vector<const ListOfProductsOfPolynomials *> &polynomials) {
        std::vector<std::unique_ptr<ListOfProductsOfPolynomials::Desc>> keep;
        std::vector<sc_poly_desc> descs;
        for (const ListOfProductsOfPolynomials *p : polynomials) {
            if (!p) throw Panic(SC_ERR_BAD_ARG, "null polynomial");
            keep.push_back(p->desc());
            descs.push_back(keep.back()->d);
        }
        sc_batch_prover *h = nullptr;
        check(sc_batch_prover_init(descs.data(), (uint32_t)descs.size(), &h));
        return BatchProverState(h, descs.size(), *polynomials[0]);
    }
    // n x prove_round in one library call (sc_batch_prove_round): v_msgs empty on the first call, then one VerifierMsg per instance or ONE
    // for all instances; message i is bit for bit prove_round's
    static std::vector<ProverMsg> prove_round_batch(BatchProverState &state, const std::vector<VerifierMsg> &v_msgs) {
        const size_t Dg = state.max_multiplicands + 1;
        std::vector<Fr> flat(state.n * Dg);
        if (v_msgs.empty()) {
            check(sc_batch_prove_round(state.raw(), nullptr, 0, flat[0].l));
        } else {
            const std::vector<Fr> r = state.challenges(v_msgs);
            check(sc_batch_prove_round(state.raw(), r[0].l, v_msgs.size() == 1 && state.n != 1 ? 1u : 0u, flat[0].l));
        }
        std::vector<ProverMsg> out(state.n);
        for (size_t i = 0; i < state.n; ++i) out[i].evaluations.assign(flat.begin() + i * Dg, flat.begin() + (i + 1) * Dg);
        return out;
    }
    static VerifierMsg sample_round(Blake2b512Rng &rng) { return VerifierMsg{rng.rand_fr()}; } // verifier.rs:128-131
};

struct MLSumcheck {
    static Fr extract_sum(const Proof &proof) { return proof[0].evaluations[0] + proof[0].evaluations[1]; } // mod.rs:26-28
    static std::pair<Proof, ProverState> prove_as_subprotocol(Blake2b512Rng &fs_rng, const ListOfProductsOfPolynomials &polynomial) {
        auto D = polynomial.desc();
        const size_t nv = polynomial.num_variables, Dg = polynomial.max_multiplicands + 1;
        std::vector<Fr> flat(std::max<size_t>(nv, 1) * Dg);
        sc_prover *h = nullptr;
        check(sc_ml_prove(&D->d, fs_rng.raw(), flat[0].l, &h));
        Proof proof(nv);
        for (size_t i = 0; i < nv; ++i) proof[i].evaluations.assign(flat.begin() + i * Dg, flat.begin() + (i + 1) * Dg);
        return {std::move(proof), ProverState(h, polynomial)};
    }
    static Proof prove(const ListOfProductsOfPolynomials &polynomial) { // mod.rs:42-45
        // no state comes back: the library reads device tables in place and keeps the prover for the next proof of this shape
        auto D = polynomial.desc();
        const size_t nv = polynomial.num_variables, Dg = polynomial.max_multiplicands + 1;
        std::vector<Fr> flat(std::max<size_t>(nv, 1) * Dg);
        check(sc_ml_prove(&D->d, nullptr, flat[0].l, nullptr));
        Proof proof(nv);
        for (size_t i = 0; i < nv; ++i) proof[i].evaluations.assign(flat.begin() + i * Dg, flat.begin() + (i + 1) * Dg);
        return proof;
    }
    // n independent proofs of ONE structure (the same num_variables and product lists; tables and coefficients per instance) in one
    // library call (sc_ml_prove_batch): what the reference's caller writes as polys.par_iter().map(MLSumcheck::prove).  Proof i is bit
    // for bit prove(*polynomials[i]) -- with `rngs` (one per polynomial, or empty) prove_as_subprotocol's proof over rngs[i], which is
    // continued accordingly.  challenges_or_null: the sampled challenges, instance-major, num_variables each.
    static std::vector<Proof> prove_batch(const std::vector<const ListOfProductsOfPolynomials *> &polynomials, const std::vector<Blake2b512Rng *> &rngs = {},
                                          std::vector<std::vector<Fr>> *challenges_or_null = nullptr) {
        const size_t n = polynomials.size();
        if (!rngs.empty() && rngs.size() != n) throw Panic(SC_ERR_BAD_ARG, "one rng per polynomial");
        std::vector<Proof> out(n);
        if (n == 0) {
            check(sc_ml_prove_batch(nullptr, 0, nullptr, nullptr, nullptr));
            return out;
        }
        std::vector<std::unique_ptr<ListOfProductsOfPolynomials::Desc>> keep;
        std::vector<sc_poly_desc> descs;
        for (const ListOfProductsOfPolynomials *p : polynomials) {
            if (!p) throw Panic(SC_ERR_BAD_ARG, "null polynomial");
            keep.push_back(p->desc());
            descs.push_back(keep.back()->d);
        }
        std::vector<sc_rng *> raw;
        for (Blake2b512Rng *r : rngs) raw.push_back(r ? r->raw() : nullptr);
        const size_t nv = polynomials[0]->num_variables, Dg = polynomials[0]->max_multiplicands + 1, rows = std::max<size_t>(nv, 1);
        std::vector<Fr> flat(n * rows * Dg), rand(n * rows);
        check(sc_ml_prove_batch(descs.data(), (uint32_t)n, raw.empty() ? nullptr : raw.data(), flat[0].l, rand[0].l));
        for (size_t i = 0; i < n; ++i) {
            out[i].resize(nv);
            for (size_t j = 0; j < nv; ++j) out[i][j].evaluations.assign(flat.begin() + (i * nv + j) * Dg, flat.begin() + (i * nv + j + 1) * Dg);
        }
        if (challenges_or_null) {
            challenges_or_null->assign(n, {});
            for (size_t i = 0; i < n; ++i) (*challenges_or_null)[i].assign(rand.begin() + i * nv, rand.begin() + (i + 1) * nv);
        }
        return out;
    }
    static SubClaim verify_as_subprotocol(Blake2b512Rng &fs_rng, const PolynomialInfo &info, const Fr &claimed_sum, const Proof &proof) {
        const size_t nv = info.num_variables, Dg = info.max_multiplicands + 1;
        if (proof.size() < nv) throw Panic(SC_ERR_BAD_ARG, "proof is incomplete");
        std::vector<Fr> flat(std::max<size_t>(nv, 1) * Dg);
        for (size_t i = 0; i < nv; ++i) {
            if (proof[i].evaluations.size() != Dg) throw Panic(SC_ERR_BAD_ARG, "incorrect number of evaluations");
            std::copy(proof[i].evaluations.begin(), proof[i].evaluations.end(), flat.begin() + i * Dg);
        }
        SubClaim sub;
        sub.point.resize(std::max<size_t>(nv, 1));
        check(sc_ml_verify((uint32_t)nv, (uint32_t)info.max_multiplicands, claimed_sum.l, flat[0].l, (uint64_t)(nv * Dg), fs_rng.raw(), sub.point[0].l,
                           sub.expected_evaluation.l));
        sub.point.resize(nv);
        return sub;
    }
    static SubClaim verify(const PolynomialInfo &info, const Fr &claimed_sum, const Proof &proof) { // mod.rs:73-80
        Blake2b512Rng rng;
        return verify_as_subprotocol(rng, info, claimed_sum, proof);
    }
};

// ListOfProductsOfPolynomials::evaluate (data_structures.rs:99-109): one library call, all tables folded on the GPU
inline Fr evaluate(const ListOfProductsOfPolynomials &poly, const std::vector<Fr> &point) {
    if (point.size() != poly.num_variables) throw Panic(SC_ERR_BAD_ARG, "wrong number of variables");
    auto D = poly.desc();
    Fr out;
    check(sc_poly_evaluate(&D->d, point.empty() ? nullptr : point[0].l, out.l, nullptr));
    return out;
}

// n x ListOfProductsOfPolynomials::evaluate in one library call (sc_poly_evaluate_batch): polynomials of ONE structure, points[i] the
// num_variables-element point of polynomial i (what its proof's subclaim ended on).  Value i is bit for bit evaluate(*polynomials[i],
// points[i]); table_values_or_null: per instance the U table evaluations T_j(point).  After MLSumcheck::prove_batch a caller finishes
// with this one call, not n.
inline std::vector<Fr> evaluate_batch(const std::vector<const ListOfProductsOfPolynomials *> &polynomials, const std::vector<std::vector<Fr>> &points,
                                      std::vector<std::vector<Fr>> *table_values_or_null = nullptr) {
    const size_t n = polynomials.size();
    if (points.size() != n) throw Panic(SC_ERR_BAD_ARG, "one point per polynomial");
    std::vector<Fr> out(n);
    if (table_values_or_null) table_values_or_null->assign(n, {});
    if (n == 0) {
        check(sc_poly_evaluate_batch(nullptr, 0, nullptr, nullptr, nullptr));
        return out;
    }
    std::vector<std::unique_ptr<ListOfProductsOfPolynomials::Desc>> keep;
    std::vector<sc_poly_desc> descs;
    if (!polynomials[0]) throw Panic(SC_ERR_BAD_ARG, "null polynomial");
    const size_t nv = polynomials[0]->num_variables, U = polynomials[0]->flattened_ml_extensions.size();
    std::vector<Fr> pts(std::max<size_t>(n * nv, 1)), tv(std::max<size_t>(n * U, 1));
    for (size_t i = 0; i < n; ++i) {
        if (!polynomials[i]) throw Panic(SC_ERR_BAD_ARG, "null polynomial");
        if (points[i].size() != nv) throw Panic(SC_ERR_BAD_ARG, "assertion failed: point.len() == num_variables");
        keep.push_back(polynomials[i]->desc());
        descs.push_back(keep.back()->d);
        std::copy(points[i].begin(), points[i].end(), pts.begin() + i * nv);
    }
    check(sc_poly_evaluate_batch(descs.data(), (uint32_t)n, pts[0].l, out[0].l, tv[0].l));
    if (table_values_or_null)
        for (size_t i = 0; i < n; ++i) (*table_values_or_null)[i].assign(tv.begin() + i * U, tv.begin() + (i + 1) * U);
    return out;
}

struct SparseMultilinearExtension {
    size_t num_vars = 0;
    std::vector<uint64_t> indices; // distinct
    std::vector<Fr> values;
};

struct GKRProof {
    Proof phase1_sumcheck_msgs, phase2_sumcheck_msgs;
    Fr extract_sum() const { return phase1_sumcheck_msgs[0].evaluations[0] + phase1_sumcheck_msgs[0].evaluations[1]; }
};

// initialize_phase_one (gkr_round_sumcheck/mod.rs:22-42)
inline std::pair<DenseMultilinearExtension, SparseMultilinearExtension> initialize_phase_one(const SparseMultilinearExtension &f1,
                                                                                             const DenseMultilinearExtension &f3,
                                                                                             const std::vector<Fr> &g) {
    const size_t dim = f3.num_vars;
    if (f1.num_vars != 3 * dim || g.size() != dim) throw Panic(SC_ERR_BAD_ARG, "assertion failed: dimensions");
    DenseMultilinearExtension hg{dim, std::vector<Fr>(size_t(1) << dim)};
    SparseMultilinearExtension f1g{2 * dim, std::vector<uint64_t>(std::max<size_t>(f1.indices.size(), 1)), std::vector<Fr>(std::max<size_t>(f1.indices.size(), 1))};
    uint64_t n1 = 0;
    check(sc_gkr_phase_one(f1.indices.data(), f1.values.empty() ? nullptr : f1.values[0].l, f1.indices.size(), (uint32_t)dim, f3.evaluations[0].l,
                           g[0].l, 0, hg.evaluations[0].l, f1g.indices.data(), f1g.values[0].l, &n1));
    f1g.indices.resize(n1);
    f1g.values.resize(n1);
    return {std::move(hg), std::move(f1g)};
}
// initialize_phase_two (gkr_round_sumcheck/mod.rs:57-63)
inline DenseMultilinearExtension initialize_phase_two(const SparseMultilinearExtension &f1_g, const std::vector<Fr> &u) {
    if (u.size() * 2 != f1_g.num_vars) throw Panic(SC_ERR_BAD_ARG, "assertion failed: u.len() * 2 == f1_g.num_vars");
    DenseMultilinearExtension out{u.size(), std::vector<Fr>(size_t(1) << u.size())};
    check(sc_gkr_phase_two(f1_g.indices.data(), f1_g.values.empty() ? nullptr : f1_g.values[0].l, f1_g.indices.size(), (uint32_t)u.size(), u[0].l,
                           0, out.evaluations[0].l));
    return out;
}

// gkr_round_sumcheck/data_structures.rs:22-56
struct GKRRoundSumcheckSubClaim {
    std::vector<Fr> u, v;
    Fr expected_evaluation;
    // expected_evaluation == f1(g, u, v) * f2(u) * f3(v); the three oracle queries run on the GPU
    bool verify_subclaim(const SparseMultilinearExtension &f1, const DenseMultilinearExtension &f2, const DenseMultilinearExtension &f3,
                         const std::vector<Fr> &g) const {
        const size_t dim = u.size();
        if (v.size() != dim || g.size() != dim || f1.num_vars != 3 * dim || f2.num_vars != dim || f3.num_vars != dim)
            throw Panic(SC_ERR_BAD_ARG, "assertion failed: dimensions");
        std::vector<Fr> guv(g);
        guv.insert(guv.end(), u.begin(), u.end());
        guv.insert(guv.end(), v.begin(), v.end());
        Fr a, ab, abc;
        check(sc_sparse_evaluate(f1.indices.data(), f1.values.empty() ? nullptr : f1.values[0].l, f1.indices.size(), (uint32_t)f1.num_vars,
                                 guv.empty() ? nullptr : guv[0].l, a.l));
        const Fr b = f2.evaluate(u), c = f3.evaluate(v);
        check(sc_fr_elementwise(0, a.l, b.l, ab.l, 1));
        check(sc_fr_elementwise(0, ab.l, c.l, abc.l, 1));
        return abc == expected_evaluation;
    }
    // f1(g,u,v), f2(u), f3(v) and their product for n instances of ONE dim in one library call (sc_gkr_subclaim_batch): four elements per
    // instance.  uv[i]: u then v (2 dim elements), as GKRRoundSumcheck::prove_batch returns them.  Pointers may repeat.
    static std::vector<std::array<Fr, 4>> evaluate_subclaims_batch(const std::vector<const SparseMultilinearExtension *> &f1s,
                                                                   const std::vector<const DenseMultilinearExtension *> &f2s,
                                                                   const std::vector<const DenseMultilinearExtension *> &f3s, const std::vector<std::vector<Fr>> &gs,
                                                                   const std::vector<std::vector<Fr>> &uv) {
        const size_t n = f1s.size();
        if (f2s.size() != n || f3s.size() != n || gs.size() != n || uv.size() != n) throw Panic(SC_ERR_BAD_ARG, "one f1, f2, f3, g and (u, v) per instance");
        std::vector<std::array<Fr, 4>> out(n);
        if (n == 0) {
            check(sc_gkr_subclaim_batch(0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr));
            return out;
        }
        if (!f2s[0]) throw Panic(SC_ERR_BAD_ARG, "null polynomial");
        const size_t dim = f2s[0]->num_vars;
        std::vector<const uint64_t *> idx(n), vals(n), p2(n), p3(n), pg(n);
        std::vector<uint64_t> nnz(n);
        std::vector<Fr> flat_uv(std::max<size_t>(n * 2 * dim, 1));
        for (size_t i = 0; i < n; ++i) {
            if (!f1s[i] || !f2s[i] || !f3s[i]) throw Panic(SC_ERR_BAD_ARG, "null polynomial");
            if (f1s[i]->num_vars != 3 * dim || f2s[i]->num_vars != dim || f3s[i]->num_vars != dim || gs[i].size() != dim || uv[i].size() != 2 * dim)
                throw Panic(SC_ERR_BAD_ARG, "assertion failed: dimensions");
            idx[i] = f1s[i]->indices.data();
            vals[i] = f1s[i]->values.empty() ? nullptr : f1s[i]->values[0].l;
            nnz[i] = f1s[i]->indices.size();
            p2[i] = f2s[i]->evaluations[0].l;
            p3[i] = f3s[i]->evaluations[0].l;
            pg[i] = gs[i].empty() ? nullptr : gs[i][0].l;
            std::copy(uv[i].begin(), uv[i].end(), flat_uv.begin() + i * 2 * dim);
        }
        check(sc_gkr_subclaim_batch((uint32_t)n, (uint32_t)dim, idx.data(), vals.data(), nnz.data(), p2.data(), p3.data(), pg.data(), flat_uv[0].l, 0, out[0][0].l));
        return out;
    }
    // verify_subclaim of n subclaims of ONE dim in one library call: element i is subclaims[i].verify_subclaim(*f1s[i], *f2s[i], *f3s[i], gs[i])
    static std::vector<bool> verify_subclaim_batch(const std::vector<GKRRoundSumcheckSubClaim> &subclaims, const std::vector<const SparseMultilinearExtension *> &f1s,
                                                   const std::vector<const DenseMultilinearExtension *> &f2s, const std::vector<const DenseMultilinearExtension *> &f3s,
                                                   const std::vector<std::vector<Fr>> &gs) {
        std::vector<std::vector<Fr>> uv;
        for (const GKRRoundSumcheckSubClaim &c : subclaims) {
            uv.push_back(c.u);
            uv.back().insert(uv.back().end(), c.v.begin(), c.v.end());
        }
        if (f1s.size() != subclaims.size()) throw Panic(SC_ERR_BAD_ARG, "one f1, f2, f3 and g per subclaim");
        const auto ev = evaluate_subclaims_batch(f1s, f2s, f3s, gs, uv);
        std::vector<bool> ok(subclaims.size());
        for (size_t i = 0; i < subclaims.size(); ++i) ok[i] = ev[i][3] == subclaims[i].expected_evaluation;
        return ok;
    }
    // ... of n subclaims of rounds proved in TWO-POINT form (GKRRoundSumcheck::prover_init_batch with g2s and coeffs), from existing calls
    // only: evaluate_subclaims_batch once over the gs and once over the g2s, then (alpha f1(g,u,v) + beta f1(g2,u,v)) f2(u) f3(v) by
    // sc_fr_elementwise.  coeffs[i]: (alpha, beta)
    static std::vector<bool> verify_subclaim_two_point_batch(const std::vector<GKRRoundSumcheckSubClaim> &subclaims, const std::vector<const SparseMultilinearExtension *> &f1s,
                                                             const std::vector<const DenseMultilinearExtension *> &f2s, const std::vector<const DenseMultilinearExtension *> &f3s,
                                                             const std::vector<std::vector<Fr>> &gs, const std::vector<std::vector<Fr>> &g2s, const std::vector<std::array<Fr, 2>> &coeffs) {
        const size_t n = subclaims.size();
        if (f1s.size() != n || g2s.size() != n || coeffs.size() != n) throw Panic(SC_ERR_BAD_ARG, "one f1, f2, f3, g, g2 and (alpha, beta) per subclaim");
        std::vector<std::vector<Fr>> uv;
        for (const GKRRoundSumcheckSubClaim &c : subclaims) {
            uv.push_back(c.u);
            uv.back().insert(uv.back().end(), c.v.begin(), c.v.end());
        }
        const auto e1 = evaluate_subclaims_batch(f1s, f2s, f3s, gs, uv), e2 = evaluate_subclaims_batch(f1s, f2s, f3s, g2s, uv);
        std::vector<bool> ok(n);
        for (size_t i = 0; i < n; ++i) {
            Fr a, b, f1v, t, all;
            check(sc_fr_elementwise(0, coeffs[i][0].l, e1[i][0].l, a.l, 1));
            check(sc_fr_elementwise(0, coeffs[i][1].l, e2[i][0].l, b.l, 1));
            check(sc_fr_elementwise(1, a.l, b.l, f1v.l, 1));
            check(sc_fr_elementwise(0, f1v.l, e1[i][1].l, t.l, 1));
            check(sc_fr_elementwise(0, t.l, e1[i][2].l, all.l, 1));
            ok[i] = all == subclaims[i].expected_evaluation;
        }
        return ok;
    }
    // n subclaims of rounds proved in GATE form (GKRRoundSumcheck::prover_init_batch_gates), from existing calls only: evaluate_subclaims_batch
    // per list and per point, then M f2(u) f3(v) + A (f2(u) + f3(v)) by sc_fr_elementwise, M = alpha mul(g,u,v) + beta mul(g2,u,v) and A
    // likewise (g2s and coeffs empty: one point, M = mul(g,u,v))
    static std::vector<bool> verify_subclaim_gates_batch(const std::vector<GKRRoundSumcheckSubClaim> &subclaims, const std::vector<const SparseMultilinearExtension *> &mul_f1s,
                                                         const std::vector<const SparseMultilinearExtension *> &add_f1s, const std::vector<const DenseMultilinearExtension *> &f2s,
                                                         const std::vector<const DenseMultilinearExtension *> &f3s, const std::vector<std::vector<Fr>> &gs,
                                                         const std::vector<std::vector<Fr>> &g2s = {}, const std::vector<std::array<Fr, 2>> &coeffs = {}) {
        const size_t n = subclaims.size();
        const bool two = !g2s.empty() || !coeffs.empty();
        if (mul_f1s.size() != n || add_f1s.size() != n || (two && (g2s.size() != n || coeffs.size() != n))) throw Panic(SC_ERR_BAD_ARG, "one mul, add, f2, f3, g (and g2, (alpha, beta)) per subclaim");
        std::vector<std::vector<Fr>> uv;
        for (const GKRRoundSumcheckSubClaim &c : subclaims) {
            uv.push_back(c.u);
            uv.back().insert(uv.back().end(), c.v.begin(), c.v.end());
        }
        const auto m1 = evaluate_subclaims_batch(mul_f1s, f2s, f3s, gs, uv), a1 = evaluate_subclaims_batch(add_f1s, f2s, f3s, gs, uv);
        auto m2 = m1, a2 = a1;
        if (two) {
            m2 = evaluate_subclaims_batch(mul_f1s, f2s, f3s, g2s, uv);
            a2 = evaluate_subclaims_batch(add_f1s, f2s, f3s, g2s, uv);
        }
        std::vector<bool> ok(n);
        for (size_t i = 0; i < n; ++i) {
            Fr M = m1[i][0], A = a1[i][0], t, s, all;
            if (two) {
                Fr x, y;
                check(sc_fr_elementwise(0, coeffs[i][0].l, m1[i][0].l, x.l, 1));
                check(sc_fr_elementwise(0, coeffs[i][1].l, m2[i][0].l, y.l, 1));
                check(sc_fr_elementwise(1, x.l, y.l, M.l, 1));
                check(sc_fr_elementwise(0, coeffs[i][0].l, a1[i][0].l, x.l, 1));
                check(sc_fr_elementwise(0, coeffs[i][1].l, a2[i][0].l, y.l, 1));
                check(sc_fr_elementwise(1, x.l, y.l, A.l, 1));
            }
            Fr mt, as;
            check(sc_fr_elementwise(0, M.l, m1[i][1].l, t.l, 1));
            check(sc_fr_elementwise(0, t.l, m1[i][2].l, mt.l, 1));
            check(sc_fr_elementwise(1, m1[i][1].l, m1[i][2].l, s.l, 1));
            check(sc_fr_elementwise(0, A.l, s.l, as.l, 1));
            check(sc_fr_elementwise(1, mt.l, as.l, all.l, 1));
            ok[i] = all == subclaims[i].expected_evaluation;
        }
        return ok;
    }
    bool verify_subclaim_gates(const SparseMultilinearExtension &mul_f1, const SparseMultilinearExtension &add_f1, const DenseMultilinearExtension &f2, const DenseMultilinearExtension &f3,
                               const std::vector<Fr> &g) const {
        return verify_subclaim_gates_batch({*this}, {&mul_f1}, {&add_f1}, {&f2}, {&f3}, {g})[0];
    }
    bool verify_subclaim_two_point(const SparseMultilinearExtension &f1, const DenseMultilinearExtension &f2, const DenseMultilinearExtension &f3, const std::vector<Fr> &g,
                                   const std::vector<Fr> &g2, const Fr &alpha, const Fr &beta) const {
        return verify_subclaim_two_point_batch({*this}, {&f1}, {&f2}, {&f3}, {g}, {g2}, {std::array<Fr, 2>{alpha, beta}})[0];
    }
};

// n x the two prover states of GKRRoundSumcheck::prove of ONE dim behind one sc_gkr_batch_prover handle (GKRRoundSumcheck::prover_init_batch):
// the interactive rounds under the caller's transcript.  2 dim calls of prove_round -- phase one's messages, then phase two's --, then finish.
class GKRBatchProverState {
  public:
    size_t n = 0, dim = 0;
    struct Final { // per instance, from finish: the subclaim's oracle values at no extra pass
        std::vector<Fr> u, v;
        Fr f1_guv, f2_u, f2u_f3v; // f1(g,u,v), f2(u), f2(u) f3(v); f1_guv * f2u_f3v is the verifier's expected evaluation
    };
    GKRBatchProverState() = default;
    GKRBatchProverState(sc_gkr_batch_prover *h, size_t n_, size_t dim_) : n(n_), dim(dim_), h_(h) {}
    GKRBatchProverState(GKRBatchProverState &&o) noexcept { *this = std::move(o); }
    GKRBatchProverState &operator=(GKRBatchProverState &&o) noexcept {
        if (h_) sc_gkr_batch_prover_free(h_);
        n = o.n;
        dim = o.dim;
        h_ = o.h_;
        o.h_ = nullptr;
        return *this;
    }
    ~GKRBatchProverState() {
        if (h_) sc_gkr_batch_prover_free(h_);
    }
    // one message per instance.  v_msgs: empty exactly on the first call; afterwards one VerifierMsg per instance, or a single one for all
    std::vector<ProverMsg> prove_round(const std::vector<VerifierMsg> &v_msgs = {}) {
        std::vector<Fr> r, flat(std::max<size_t>(n, 1) * 3);
        if (!v_msgs.empty()) r = challenges(v_msgs);
        check(sc_gkr_batch_prove_round(h_, r.empty() ? nullptr : r[0].l, v_msgs.size() == 1 && n != 1 ? 1u : 0u, flat[0].l));
        std::vector<ProverMsg> out;
        for (size_t i = 0; i < n; ++i) out.push_back(ProverMsg{std::vector<Fr>(flat.begin() + 3 * i, flat.begin() + 3 * i + 3)});
        return out;
    }
    // the last challenge v_{dim-1}, after 2 dim rounds; the handle is exhausted until reset
    std::vector<Final> finish(const std::vector<VerifierMsg> &v_msgs) {
        const std::vector<Fr> r = challenges(v_msgs);
        std::vector<Fr> uv(std::max<size_t>(n * 2 * dim, 1)), fin(std::max<size_t>(n, 1) * 3);
        check(sc_gkr_batch_prover_finish(h_, r[0].l, v_msgs.size() == 1 && n != 1 ? 1u : 0u, uv[0].l, fin[0].l));
        std::vector<Final> out(n);
        for (size_t i = 0; i < n; ++i) {
            out[i].u.assign(uv.begin() + i * 2 * dim, uv.begin() + i * 2 * dim + dim);
            out[i].v.assign(uv.begin() + i * 2 * dim + dim, uv.begin() + (i + 1) * 2 * dim);
            out[i].f1_guv = fin[3 * i];
            out[i].f2_u = fin[3 * i + 1];
            out[i].f2u_f3v = fin[3 * i + 2];
        }
        return out;
    }
    size_t round() const {
        uint32_t r = 0;
        check(sc_gkr_batch_prover_state(h_, 0, nullptr, nullptr, nullptr, &r));
        return r;
    }
    std::vector<Fr> randomness(size_t i) const { // u followed by the v's received so far
        std::vector<Fr> buf(std::max<size_t>(2 * dim, 1));
        uint32_t cnt = 0;
        check(sc_gkr_batch_prover_state(h_, (uint32_t)i, buf[0].l, &cnt, nullptr, nullptr));
        buf.resize(cnt);
        return buf;
    }
    std::vector<DenseMultilinearExtension> tables(size_t i) const { // the current phase's two tables, canonical
        const size_t t = round(), pr = t > dim ? t - dim : t, nv = dim - (pr > 0 ? pr - 1 : 0);
        std::vector<Fr> buf(size_t(2) << nv);
        check(sc_gkr_batch_prover_state(h_, (uint32_t)i, nullptr, nullptr, buf[0].l, nullptr));
        return {DenseMultilinearExtension{nv, std::vector<Fr>(buf.begin(), buf.begin() + (size_t(1) << nv))},
                DenseMultilinearExtension{nv, std::vector<Fr>(buf.begin() + (size_t(1) << nv), buf.end())}};
    }
    void reset() { check(sc_gkr_batch_prover_reset(h_)); }
    // the argument arrays sc_gkr_gates_init_batch and sc_gkr_gates_next_batch share (lists null: the wiring is kept)
    struct GatesArgs {
        std::vector<const uint64_t *> idx[2], vals[2], p2, p3, pg, pg2;
        std::vector<uint64_t> nnz[2];
        bool two = false;
        GatesArgs(size_t n, size_t dim, const std::vector<const SparseMultilinearExtension *> *mul_f1s, const std::vector<const SparseMultilinearExtension *> *add_f1s,
                  const std::vector<const DenseMultilinearExtension *> &f2s, const std::vector<const DenseMultilinearExtension *> &f3s, const std::vector<std::vector<Fr>> &gs,
                  const std::vector<std::vector<Fr>> &g2s, const std::vector<std::array<Fr, 2>> &coeffs)
            : p2(n + 1), p3(n + 1), pg(n + 1), pg2(n + 1) {
            two = !g2s.empty() || !coeffs.empty();
            if (f2s.size() != n || f3s.size() != n || gs.size() != n || (two && (g2s.size() != n || coeffs.size() != n))) throw Panic(SC_ERR_BAD_ARG, "one f2, f3 and g (and g2, (alpha, beta)) per instance");
            const std::vector<const SparseMultilinearExtension *> *lists[2] = {mul_f1s, add_f1s};
            for (int k = 0; k < 2; ++k) {
                idx[k].assign(n + 1, nullptr);
                vals[k].assign(n + 1, nullptr);
                nnz[k].assign(n + 1, 0);
                if (lists[k] && lists[k]->size() != n) throw Panic(SC_ERR_BAD_ARG, "one mul and one add list per instance");
            }
            for (size_t i = 0; i < n; ++i) {
                if (!f2s[i] || !f3s[i]) throw Panic(SC_ERR_BAD_ARG, "null polynomial");
                if (f2s[i]->num_vars != dim || f3s[i]->num_vars != dim || gs[i].size() != dim || (two && g2s[i].size() != dim)) throw Panic(SC_ERR_BAD_ARG, "assertion failed: dimensions");
                for (int k = 0; k < 2 && lists[k]; ++k) {
                    const SparseMultilinearExtension *f1 = (*lists[k])[i];
                    if (!f1) throw Panic(SC_ERR_BAD_ARG, "null polynomial");
                    if (f1->num_vars != 3 * dim) throw Panic(SC_ERR_BAD_ARG, "assertion failed: dimensions");
                    idx[k][i] = f1->indices.data();
                    vals[k][i] = f1->values.empty() ? nullptr : f1->values[0].l;
                    nnz[k][i] = f1->indices.size();
                }
                p2[i] = f2s[i]->evaluations[0].l;
                p3[i] = f3s[i]->evaluations[0].l;
                pg[i] = gs[i].empty() ? nullptr : gs[i][0].l;
                if (two) pg2[i] = g2s[i].empty() ? nullptr : g2s[i][0].l;
            }
        }
    };
    // next_layer for a handle of GKRRoundSumcheck::prover_init_batch_gates (sc_gkr_gates_next_batch): mul_f1s and add_f1s both empty keeps both
    // lists, both given is new wiring; g2s and coeffs (both or neither) choose the layer's form.  An argument error leaves a proof in progress where it was.
    void next_layer_gates(const std::vector<const DenseMultilinearExtension *> &f2s, const std::vector<const DenseMultilinearExtension *> &f3s, const std::vector<std::vector<Fr>> &gs,
                          const std::vector<const SparseMultilinearExtension *> &mul_f1s = {}, const std::vector<const SparseMultilinearExtension *> &add_f1s = {},
                          const std::vector<std::vector<Fr>> &g2s = {}, const std::vector<std::array<Fr, 2>> &coeffs = {}) {
        const bool keep = mul_f1s.empty() && add_f1s.empty();
        GatesArgs a(n, dim, keep ? nullptr : &mul_f1s, keep ? nullptr : &add_f1s, f2s, f3s, gs, g2s, coeffs);
        check(sc_gkr_gates_next_batch(h_, keep ? nullptr : a.idx[0].data(), keep ? nullptr : a.vals[0].data(), keep ? nullptr : a.nnz[0].data(), keep ? nullptr : a.idx[1].data(),
                                      keep ? nullptr : a.vals[1].data(), keep ? nullptr : a.nnz[1].data(), a.p2.data(), a.p3.data(), a.pg.data(), a.two ? a.pg2.data() : nullptr,
                                      a.two ? coeffs[0][0].l : nullptr, 0));
    }
    // the handle onto the next layer's inputs (sc_gkr_layer_next_batch): nothing is allocated; afterwards round 0, as prover_init_batch over
    // these inputs would leave it.  f1s empty: the wiring the handle holds is kept.  Pointers may repeat; an argument error leaves the handle where it was.
    void next_layer(const std::vector<const DenseMultilinearExtension *> &f2s, const std::vector<const DenseMultilinearExtension *> &f3s, const std::vector<std::vector<Fr>> &gs,
                    const std::vector<const SparseMultilinearExtension *> &f1s = {}) {
        const bool keep = f1s.empty();
        if (f2s.size() != n || f3s.size() != n || gs.size() != n || (!keep && f1s.size() != n)) throw Panic(SC_ERR_BAD_ARG, "one f2, f3 and g per instance, and one f1 or none at all");
        std::vector<const uint64_t *> idx(n + 1), vals(n + 1), p2(n + 1), p3(n + 1), pg(n + 1);
        std::vector<uint64_t> nnz(n + 1);
        for (size_t i = 0; i < n; ++i) {
            if (!f2s[i] || !f3s[i] || (!keep && !f1s[i])) throw Panic(SC_ERR_BAD_ARG, "null polynomial");
            if (f2s[i]->num_vars != dim || f3s[i]->num_vars != dim || gs[i].size() != dim || (!keep && f1s[i]->num_vars != 3 * dim)) throw Panic(SC_ERR_BAD_ARG, "assertion failed: dimensions");
            if (!keep) {
                idx[i] = f1s[i]->indices.data();
                vals[i] = f1s[i]->values.empty() ? nullptr : f1s[i]->values[0].l;
                nnz[i] = f1s[i]->indices.size();
            }
            p2[i] = f2s[i]->evaluations[0].l;
            p3[i] = f3s[i]->evaluations[0].l;
            pg[i] = gs[i].empty() ? nullptr : gs[i][0].l;
        }
        check(sc_gkr_layer_next_batch(h_, keep ? nullptr : idx.data(), keep ? nullptr : vals.data(), keep ? nullptr : nnz.data(), p2.data(), p3.data(), pg.data(), 0));
    }
    // ... onto a layer in TWO-POINT form (sc_gkr_two_point_next_batch), whichever form the handle was built in: per instance a second point
    // g2s[i] and coeffs[i] = (alpha, beta); alpha eq(g, .) + beta eq(g2, .) stands where eq(g, .) stands.  The overload above returns the
    // handle to the one-point form.
    void next_layer(const std::vector<const DenseMultilinearExtension *> &f2s, const std::vector<const DenseMultilinearExtension *> &f3s, const std::vector<std::vector<Fr>> &gs,
                    const std::vector<std::vector<Fr>> &g2s, const std::vector<std::array<Fr, 2>> &coeffs, const std::vector<const SparseMultilinearExtension *> &f1s = {}) {
        const bool keep = f1s.empty();
        if (f2s.size() != n || f3s.size() != n || gs.size() != n || g2s.size() != n || coeffs.size() != n || (!keep && f1s.size() != n))
            throw Panic(SC_ERR_BAD_ARG, "one f2, f3, g, g2 and (alpha, beta) per instance, and one f1 or none at all");
        std::vector<const uint64_t *> idx(n + 1), vals(n + 1), p2(n + 1), p3(n + 1), pg(n + 1), pg2(n + 1);
        std::vector<uint64_t> nnz(n + 1);
        for (size_t i = 0; i < n; ++i) {
            if (!f2s[i] || !f3s[i] || (!keep && !f1s[i])) throw Panic(SC_ERR_BAD_ARG, "null polynomial");
            if (f2s[i]->num_vars != dim || f3s[i]->num_vars != dim || gs[i].size() != dim || g2s[i].size() != dim || (!keep && f1s[i]->num_vars != 3 * dim))
                throw Panic(SC_ERR_BAD_ARG, "assertion failed: dimensions");
            if (!keep) {
                idx[i] = f1s[i]->indices.data();
                vals[i] = f1s[i]->values.empty() ? nullptr : f1s[i]->values[0].l;
                nnz[i] = f1s[i]->indices.size();
            }
            p2[i] = f2s[i]->evaluations[0].l;
            p3[i] = f3s[i]->evaluations[0].l;
            pg[i] = gs[i].empty() ? nullptr : gs[i][0].l;
            pg2[i] = g2s[i].empty() ? nullptr : g2s[i][0].l;
        }
        check(sc_gkr_two_point_next_batch(h_, keep ? nullptr : idx.data(), keep ? nullptr : vals.data(), keep ? nullptr : nnz.data(), p2.data(), p3.data(), pg.data(), pg2.data(),
                                          n ? coeffs[0][0].l : nullptr, 0));
    }
    sc_gkr_batch_prover *raw() { return h_; }
    std::vector<Fr> challenges(const std::vector<VerifierMsg> &v_msgs) const {
        if (v_msgs.size() != n && v_msgs.size() != 1) throw Panic(SC_ERR_BAD_ARG, "one VerifierMsg per instance, or a single one for all");
        std::vector<Fr> r;
        for (const VerifierMsg &m : v_msgs) r.push_back(m.randomness);
        return r;
    }

  private:
    sc_gkr_batch_prover *h_ = nullptr;
};

struct GKRRoundSumcheck {
    // verifier_init{max_multiplicands: 2} + (feed, verify_round) x dim + check_and_generate_subclaim (mod.rs:157-166, 173-182)
    static std::pair<std::vector<Fr>, Fr> verify_phase(Blake2b512Rng &rng, const Proof &msgs, size_t dim, const Fr &asserted_sum) {
        if (msgs.size() < dim) throw Panic(SC_ERR_BAD_ARG, "proof is incomplete");
        std::vector<Fr> rs;
        for (size_t i = 0; i < dim; ++i) {
            if (msgs[i].evaluations.empty()) throw Panic(SC_ERR_BAD_ARG, "incorrect number of evaluations");
            sc_rng_feed_prover_msg(rng.raw(), msgs[i].evaluations[0].l, (uint32_t)msgs[i].evaluations.size());
            rs.push_back(rng.rand_fr());
        }
        Fr expected = asserted_sum;
        if (!expected.is_canonical()) throw Panic(SC_ERR_BAD_ARG, "claimed sum is not a canonical field element");
        for (size_t i = 0; i < dim; ++i) {
            const auto &ev = msgs[i].evaluations;
            if (ev.size() != 3) throw Panic(SC_ERR_BAD_ARG, "incorrect number of evaluations");
            for (const Fr &e : ev) // the raw-limb sum below is only a field addition on canonical operands
                if (!e.is_canonical()) throw Panic(SC_ERR_BAD_ARG, "proof element is not a canonical field element");
            if (ev[0] + ev[1] != expected) throw Reject("Prover message is not consistent with the claim.");
            check(sc_interpolate_uni_poly(ev[0].l, 3, rs[i].l, expected.l));
        }
        return {rs, expected};
    }
    static GKRRoundSumcheckSubClaim verify(Blake2b512Rng &rng, size_t f2_num_vars, const GKRProof &proof, const Fr &claimed_sum) { // mod.rs:147-192
        auto p1 = verify_phase(rng, proof.phase1_sumcheck_msgs, f2_num_vars, claimed_sum);
        auto p2 = verify_phase(rng, proof.phase2_sumcheck_msgs, f2_num_vars, p1.second);
        return GKRRoundSumcheckSubClaim{std::move(p1.first), std::move(p2.first), p2.second};
    }
    static GKRProof prove(Blake2b512Rng &rng, const SparseMultilinearExtension &f1, const DenseMultilinearExtension &f2,
                          const DenseMultilinearExtension &f3, const std::vector<Fr> &g) { // gkr_round_sumcheck/mod.rs:93-139
        const size_t dim = f2.num_vars;
        if (f1.num_vars != 3 * dim || f3.num_vars != dim || g.size() != dim) throw Panic(SC_ERR_BAD_ARG, "assertion failed: dimensions");
        std::vector<Fr> flat(2 * std::max<size_t>(dim, 1) * 3);
        check(sc_gkr_prove(rng.raw(), f1.indices.data(), f1.values.empty() ? nullptr : f1.values[0].l, f1.indices.size(), (uint32_t)dim,
                           f2.evaluations[0].l, f3.evaluations[0].l, g[0].l, 0, flat[0].l, nullptr));
        GKRProof pr;
        for (size_t i = 0; i < dim; ++i) {
            pr.phase1_sumcheck_msgs.push_back(ProverMsg{std::vector<Fr>(flat.begin() + 3 * i, flat.begin() + 3 * i + 3)});
            pr.phase2_sumcheck_msgs.push_back(ProverMsg{std::vector<Fr>(flat.begin() + 3 * (dim + i), flat.begin() + 3 * (dim + i) + 3)});
        }
        return pr;
    }
    // the oracle queries behind prove_batch, in one library call (GKRRoundSumcheckSubClaim::evaluate_subclaims_batch)
    static std::vector<std::array<Fr, 4>> evaluate_subclaims_batch(const std::vector<const SparseMultilinearExtension *> &f1s,
                                                                   const std::vector<const DenseMultilinearExtension *> &f2s,
                                                                   const std::vector<const DenseMultilinearExtension *> &f3s, const std::vector<std::vector<Fr>> &gs,
                                                                   const std::vector<std::vector<Fr>> &uv) {
        return GKRRoundSumcheckSubClaim::evaluate_subclaims_batch(f1s, f2s, f3s, gs, uv);
    }
    // n independent GKRRoundSumcheck::prove of ONE dim in one library call (sc_gkr_prove_batch): proof i is bit for bit
    // prove(*rngs[i], *f1s[i], *f2s[i], *f3s[i], gs[i]), and rngs[i] is continued accordingly.  Pointers may repeat (one wiring predicate f1
    // for many data instances) -- except the rngs, which are all distinct.  uv_or_null: per instance the sampled u then v (2 dim elements).
    static std::vector<GKRProof> prove_batch(const std::vector<Blake2b512Rng *> &rngs, const std::vector<const SparseMultilinearExtension *> &f1s,
                                             const std::vector<const DenseMultilinearExtension *> &f2s, const std::vector<const DenseMultilinearExtension *> &f3s,
                                             const std::vector<std::vector<Fr>> &gs, std::vector<std::vector<Fr>> *uv_or_null = nullptr) {
        const size_t n = rngs.size();
        if (f1s.size() != n || f2s.size() != n || f3s.size() != n || gs.size() != n) throw Panic(SC_ERR_BAD_ARG, "one f1, f2, f3 and g per rng");
        std::vector<GKRProof> out(n);
        if (n == 0) {
            check(sc_gkr_prove_batch(0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr));
            return out;
        }
        if (!f2s[0]) throw Panic(SC_ERR_BAD_ARG, "null polynomial");
        const size_t dim = f2s[0]->num_vars, rows = std::max<size_t>(dim, 1);
        std::vector<sc_rng *> raw(n);
        std::vector<const uint64_t *> idx(n), vals(n), p2(n), p3(n), pg(n);
        std::vector<uint64_t> nnz(n);
        for (size_t i = 0; i < n; ++i) {
            if (!f1s[i] || !f2s[i] || !f3s[i]) throw Panic(SC_ERR_BAD_ARG, "null polynomial");
            if (f1s[i]->num_vars != 3 * dim || f2s[i]->num_vars != dim || f3s[i]->num_vars != dim || gs[i].size() != dim) throw Panic(SC_ERR_BAD_ARG, "assertion failed: dimensions");
            raw[i] = rngs[i] ? rngs[i]->raw() : nullptr;
            idx[i] = f1s[i]->indices.data();
            vals[i] = f1s[i]->values.empty() ? nullptr : f1s[i]->values[0].l;
            nnz[i] = f1s[i]->indices.size();
            p2[i] = f2s[i]->evaluations[0].l;
            p3[i] = f3s[i]->evaluations[0].l;
            pg[i] = gs[i].empty() ? nullptr : gs[i][0].l;
        }
        std::vector<Fr> flat(n * 2 * rows * 3), uv(n * 2 * rows);
        check(sc_gkr_prove_batch((uint32_t)n, (uint32_t)dim, raw.data(), idx.data(), vals.data(), nnz.data(), p2.data(), p3.data(), pg.data(), 0, flat[0].l, uv[0].l));
        for (size_t i = 0; i < n; ++i) {
            const Fr *m = flat.data() + i * 2 * dim * 3;
            for (size_t j = 0; j < dim; ++j) {
                out[i].phase1_sumcheck_msgs.push_back(ProverMsg{std::vector<Fr>(m + 3 * j, m + 3 * j + 3)});
                out[i].phase2_sumcheck_msgs.push_back(ProverMsg{std::vector<Fr>(m + 3 * (dim + j), m + 3 * (dim + j) + 3)});
            }
        }
        if (uv_or_null) {
            uv_or_null->assign(n, {});
            for (size_t i = 0; i < n; ++i) (*uv_or_null)[i].assign(uv.begin() + i * 2 * dim, uv.begin() + (i + 1) * 2 * dim);
        }
        return out;
    }
    // n x the interactive prover of ONE dim behind one handle (sc_gkr_batch_prover_init): the caller owns the transcript.  Pointers may repeat.
    // Plans: dim <= 9 runs one block per instance; with policy "batch_slices" = 1 set when the handle is built, dim 10 .. 16 (nnz <= 64 x 2^dim, at most 16 GiB) gives every instance to many blocks (plan batch.gkr_rounds_slices: same bits); other shapes take the serial plan.
    static GKRBatchProverState prover_init_batch(const std::vector<const SparseMultilinearExtension *> &f1s, const std::vector<const DenseMultilinearExtension *> &f2s,
                                                 const std::vector<const DenseMultilinearExtension *> &f3s, const std::vector<std::vector<Fr>> &gs) {
        const size_t n = f1s.size();
        if (f2s.size() != n || f3s.size() != n || gs.size() != n) throw Panic(SC_ERR_BAD_ARG, "one f1, f2, f3 and g per instance");
        const size_t dim = n && f2s[0] ? f2s[0]->num_vars : 0;
        std::vector<const uint64_t *> idx(n + 1), vals(n + 1), p2(n + 1), p3(n + 1), pg(n + 1);
        std::vector<uint64_t> nnz(n + 1);
        for (size_t i = 0; i < n; ++i) {
            if (!f1s[i] || !f2s[i] || !f3s[i]) throw Panic(SC_ERR_BAD_ARG, "null polynomial");
            if (f1s[i]->num_vars != 3 * dim || f2s[i]->num_vars != dim || f3s[i]->num_vars != dim || gs[i].size() != dim) throw Panic(SC_ERR_BAD_ARG, "assertion failed: dimensions");
            idx[i] = f1s[i]->indices.data();
            vals[i] = f1s[i]->values.empty() ? nullptr : f1s[i]->values[0].l;
            nnz[i] = f1s[i]->indices.size();
            p2[i] = f2s[i]->evaluations[0].l;
            p3[i] = f3s[i]->evaluations[0].l;
            pg[i] = gs[i].empty() ? nullptr : gs[i][0].l;
        }
        sc_gkr_batch_prover *h = nullptr;
        check(sc_gkr_batch_prover_init((uint32_t)n, (uint32_t)dim, idx.data(), vals.data(), nnz.data(), p2.data(), p3.data(), pg.data(), 0, &h));
        return GKRBatchProverState(h, n, dim);
    }
    // ... in TWO-POINT form (sc_gkr_two_point_init_batch): the handle proves alpha W(g) + beta W(g2) = sum (alpha f1(g,x,y) + beta f1(g2,x,y)) f2(x) f3(y),
    // the claim a GKR layer below the output layer starts from.  g2s[i]: the second point; coeffs[i]: (alpha, beta).  finish's f1_guv is
    // alpha f1(g,u,v) + beta f1(g2,u,v); everything else is as above.
    static GKRBatchProverState prover_init_batch(const std::vector<const SparseMultilinearExtension *> &f1s, const std::vector<const DenseMultilinearExtension *> &f2s,
                                                 const std::vector<const DenseMultilinearExtension *> &f3s, const std::vector<std::vector<Fr>> &gs,
                                                 const std::vector<std::vector<Fr>> &g2s, const std::vector<std::array<Fr, 2>> &coeffs) {
        const size_t n = f1s.size();
        if (f2s.size() != n || f3s.size() != n || gs.size() != n || g2s.size() != n || coeffs.size() != n) throw Panic(SC_ERR_BAD_ARG, "one f1, f2, f3, g, g2 and (alpha, beta) per instance");
        const size_t dim = n && f2s[0] ? f2s[0]->num_vars : 0;
        std::vector<const uint64_t *> idx(n + 1), vals(n + 1), p2(n + 1), p3(n + 1), pg(n + 1), pg2(n + 1);
        std::vector<uint64_t> nnz(n + 1);
        for (size_t i = 0; i < n; ++i) {
            if (!f1s[i] || !f2s[i] || !f3s[i]) throw Panic(SC_ERR_BAD_ARG, "null polynomial");
            if (f1s[i]->num_vars != 3 * dim || f2s[i]->num_vars != dim || f3s[i]->num_vars != dim || gs[i].size() != dim || g2s[i].size() != dim) throw Panic(SC_ERR_BAD_ARG, "assertion failed: dimensions");
            idx[i] = f1s[i]->indices.data();
            vals[i] = f1s[i]->values.empty() ? nullptr : f1s[i]->values[0].l;
            nnz[i] = f1s[i]->indices.size();
            p2[i] = f2s[i]->evaluations[0].l;
            p3[i] = f3s[i]->evaluations[0].l;
            pg[i] = gs[i].empty() ? nullptr : gs[i][0].l;
            pg2[i] = g2s[i].empty() ? nullptr : g2s[i][0].l;
        }
        sc_gkr_batch_prover *h = nullptr;
        check(sc_gkr_two_point_init_batch((uint32_t)n, (uint32_t)dim, idx.data(), vals.data(), nnz.data(), p2.data(), p3.data(), pg.data(), pg2.data(), n ? coeffs[0][0].l : nullptr, 0, &h));
        return GKRBatchProverState(h, n, dim);
    }
    // prover_init_batch for layers of multiplication AND addition gates (sc_gkr_gates_init_batch):
    //     W_out[z] = sum over mul_f1 of v f2[x] f3[y] + sum over add_f1 of v (f2[x] + f3[y]),
    // claimed at gs[i], or -- g2s and coeffs non-empty -- as alpha W_out(g) + beta W_out(g2).  The handle is driven as any other; its finish
    // returns f2(u), f3(v) and f3(v) T1(v) + T2(v) in f1_guv, f2_u, f2u_f3v -- the LAST is the value the verifier compares; tables() is
    // refused; later layers come through GKRBatchProverState::next_layer_gates.  Plans batch.gkr_gates_one_block / batch.gkr_gates_composed: same bits.
    static GKRBatchProverState prover_init_batch_gates(const std::vector<const SparseMultilinearExtension *> &mul_f1s, const std::vector<const SparseMultilinearExtension *> &add_f1s,
                                                       const std::vector<const DenseMultilinearExtension *> &f2s, const std::vector<const DenseMultilinearExtension *> &f3s,
                                                       const std::vector<std::vector<Fr>> &gs, const std::vector<std::vector<Fr>> &g2s = {},
                                                       const std::vector<std::array<Fr, 2>> &coeffs = {}) {
        const size_t n = f2s.size();
        const size_t dim = n && f2s[0] ? f2s[0]->num_vars : 0;
        GKRBatchProverState::GatesArgs a(n, dim, &mul_f1s, &add_f1s, f2s, f3s, gs, g2s, coeffs);
        sc_gkr_batch_prover *h = nullptr;
        check(sc_gkr_gates_init_batch((uint32_t)n, (uint32_t)dim, a.idx[0].data(), a.vals[0].data(), a.nnz[0].data(), a.idx[1].data(), a.vals[1].data(), a.nnz[1].data(), a.p2.data(),
                                      a.p3.data(), a.pg.data(), a.two ? a.pg2.data() : nullptr, a.two ? coeffs[0][0].l : nullptr, 0, &h));
        return GKRBatchProverState(h, n, dim);
    }
    // evaluate_layers_batch for layers of multiplication AND addition gates (sc_gkr_gates_layers_eval_batch): mul_layers[k][i] and add_layers[k][i]
    // are the two lists of layer k of instance i; out[k][i][z] = sum over mul of v A[x] B[y] + sum over add of v (A[x] + B[y]), (A, B) = (f2s[i], f3s[i])
    // for layer 0 and out[k-1][i] on both sides afterwards.  What prover_init_batch_gates and next_layer_gates take as f2s and f3s.
    static std::vector<std::vector<DenseMultilinearExtension>> evaluate_layers_batch_gates(const std::vector<std::vector<const SparseMultilinearExtension *>> &mul_layers,
                                                                                          const std::vector<std::vector<const SparseMultilinearExtension *>> &add_layers,
                                                                                          const std::vector<const DenseMultilinearExtension *> &f2s,
                                                                                          const std::vector<const DenseMultilinearExtension *> &f3s) {
        const size_t n = f2s.size(), n_layers = mul_layers.size();
        if (f3s.size() != n || add_layers.size() != n_layers) throw Panic(SC_ERR_BAD_ARG, "one f2 and one f3 per instance, one mul and one add list per layer");
        std::vector<std::vector<DenseMultilinearExtension>> out(n_layers);
        if (n == 0 || n_layers == 0) return out;
        if (!f2s[0]) throw Panic(SC_ERR_BAD_ARG, "null polynomial");
        const size_t dim = f2s[0]->num_vars, total = n * n_layers;
        std::vector<const uint64_t *> idx[2], vals[2], p2(n), p3(n);
        std::vector<uint64_t> nnz[2];
        std::vector<uint64_t *> po(total);
        for (size_t i = 0; i < n; ++i) {
            if (!f2s[i] || !f3s[i]) throw Panic(SC_ERR_BAD_ARG, "null polynomial");
            if (f2s[i]->num_vars != dim || f3s[i]->num_vars != dim) throw Panic(SC_ERR_BAD_ARG, "assertion failed: dimensions");
            p2[i] = f2s[i]->evaluations[0].l;
            p3[i] = f3s[i]->evaluations[0].l;
        }
        for (int q = 0; q < 2; ++q) {
            const auto &layers = q ? add_layers : mul_layers;
            idx[q].resize(total);
            vals[q].resize(total);
            nnz[q].resize(total);
            for (size_t k = 0; k < n_layers; ++k) {
                if (layers[k].size() != n) throw Panic(SC_ERR_BAD_ARG, "one list per layer and instance");
                for (size_t i = 0; i < n; ++i) {
                    const SparseMultilinearExtension *f1 = layers[k][i];
                    if (!f1) throw Panic(SC_ERR_BAD_ARG, "null polynomial");
                    if (f1->num_vars != 3 * dim) throw Panic(SC_ERR_BAD_ARG, "assertion failed: dimensions");
                    idx[q][k * n + i] = f1->indices.data();
                    vals[q][k * n + i] = f1->values.empty() ? nullptr : f1->values[0].l;
                    nnz[q][k * n + i] = f1->indices.size();
                }
            }
        }
        for (size_t k = 0; k < n_layers; ++k) {
            out[k].resize(n);
            for (size_t i = 0; i < n; ++i) {
                out[k][i].num_vars = dim;
                out[k][i].evaluations.resize(size_t(1) << dim);
                po[k * n + i] = out[k][i].evaluations[0].l;
            }
        }
        check(sc_gkr_gates_layers_eval_batch((uint32_t)n, (uint32_t)dim, (uint32_t)n_layers, idx[0].data(), vals[0].data(), nnz[0].data(), idx[1].data(), vals[1].data(), nnz[1].data(),
                                             p2.data(), p3.data(), 0, po.data()));
        return out;
    }
    // The values of a circuit's layers for n instances of ONE dim in one library call (sc_gkr_layers_eval_batch): f1_layers[k][i] is the
    // wiring of layer k of instance i, layer 0 next to the inputs (f2s[i], f3s[i]).  out[0][i][z] = sum over f1_layers[0][i]'s non-zeros
    // (z | x << dim | y << 2 dim, v) of v f2s[i][x] f3s[i][y]; out[k][i] the same over f1_layers[k][i] with out[k-1][i] on both sides.
    // Pointers may repeat across instances and layers.  What prover_init_batch and GKRBatchProverState::next_layer take as f2s and f3s.
    static std::vector<std::vector<DenseMultilinearExtension>> evaluate_layers_batch(const std::vector<std::vector<const SparseMultilinearExtension *>> &f1_layers,
                                                                                    const std::vector<const DenseMultilinearExtension *> &f2s,
                                                                                    const std::vector<const DenseMultilinearExtension *> &f3s) {
        const size_t n = f2s.size(), n_layers = f1_layers.size();
        if (f3s.size() != n) throw Panic(SC_ERR_BAD_ARG, "one f2 and one f3 per instance");
        std::vector<std::vector<DenseMultilinearExtension>> out(n_layers);
        if (n == 0 || n_layers == 0) return out;
        if (!f2s[0]) throw Panic(SC_ERR_BAD_ARG, "null polynomial");
        const size_t dim = f2s[0]->num_vars, total = n * n_layers;
        std::vector<const uint64_t *> idx(total), vals(total), p2(n), p3(n);
        std::vector<uint64_t> nnz(total);
        std::vector<uint64_t *> po(total);
        for (size_t i = 0; i < n; ++i) {
            if (!f2s[i] || !f3s[i]) throw Panic(SC_ERR_BAD_ARG, "null polynomial");
            if (f2s[i]->num_vars != dim || f3s[i]->num_vars != dim) throw Panic(SC_ERR_BAD_ARG, "assertion failed: dimensions");
            p2[i] = f2s[i]->evaluations[0].l;
            p3[i] = f3s[i]->evaluations[0].l;
        }
        for (size_t k = 0; k < n_layers; ++k) {
            if (f1_layers[k].size() != n) throw Panic(SC_ERR_BAD_ARG, "one f1 per layer and instance");
            out[k].resize(n);
            for (size_t i = 0; i < n; ++i) {
                const SparseMultilinearExtension *f1 = f1_layers[k][i];
                if (!f1) throw Panic(SC_ERR_BAD_ARG, "null polynomial");
                if (f1->num_vars != 3 * dim) throw Panic(SC_ERR_BAD_ARG, "assertion failed: dimensions");
                idx[k * n + i] = f1->indices.data();
                vals[k * n + i] = f1->values.empty() ? nullptr : f1->values[0].l;
                nnz[k * n + i] = f1->indices.size();
                out[k][i].num_vars = dim;
                out[k][i].evaluations.resize(size_t(1) << dim);
                po[k * n + i] = out[k][i].evaluations[0].l;
            }
        }
        check(sc_gkr_layers_eval_batch((uint32_t)n, (uint32_t)dim, (uint32_t)n_layers, idx.data(), vals.data(), nnz.data(), p2.data(), p3.data(), 0, po.data()));
        return out;
    }
};

} // namespace sumcheck
