// evaluate_batch, GKRRoundSumcheck::evaluate_subclaims_batch and GKRRoundSumcheckSubClaim::verify_subclaim_batch of include/sumcheck_amd.hpp
// (sc_poly_evaluate_batch, sc_gkr_subclaim_batch through the C ABI) against the single-instance calls, instance by instance.  Without a
// HIP device the library has no CPU fallback: the mirror's Panic carries the library's text, which is what this program then reports
// (tests/test_eval_batch_host.py runs it both ways).
#include <cstdio>
#include <string>

#include "sumcheck_amd.hpp"

using namespace sumcheck;

int main() {
    Blake2b512Rng rng = Blake2b512Rng::setup();
    rng.feed("eval batch mirror");
    const size_t nv = 5, dim = 4, n = 6;
    // ---- n polynomials of one structure: c0 * A B C + c1 * B B, tables per instance --------------------------------------------------
    std::vector<ListOfProductsOfPolynomials> polys;
    std::vector<std::vector<Fr>> points;
    for (size_t i = 0; i < n; ++i) {
        auto A = std::make_shared<DenseMultilinearExtension>(DenseMultilinearExtension::rand(nv, rng));
        auto B = std::make_shared<DenseMultilinearExtension>(DenseMultilinearExtension::rand(nv, rng));
        auto Cc = std::make_shared<DenseMultilinearExtension>(DenseMultilinearExtension::rand(nv, rng));
        ListOfProductsOfPolynomials p(nv);
        p.add_product({A, B, Cc}, rng.rand_fr());
        p.add_product({B, B}, rng.rand_fr());
        polys.push_back(std::move(p));
        std::vector<Fr> pt;
        for (size_t k = 0; k < nv; ++k) pt.push_back(rng.rand_fr());
        points.push_back(pt);
    }
    // ---- n GKR rounds of one dim, one wiring predicate shared by all of them -----------------------------------------------------------
    SparseMultilinearExtension f1;
    f1.num_vars = 3 * dim;
    for (size_t k = 0; k < (size_t(2) << dim); ++k) { // (a repeated index now and then: summed)
        f1.indices.push_back((k * 2654435761ull) & ((uint64_t(1) << (3 * dim)) - 1));
        f1.values.push_back(rng.rand_fr());
    }
    SparseMultilinearExtension f1_distinct; // sc_sparse_evaluate's contract: distinct indices
    f1_distinct.num_vars = 3 * dim;
    for (size_t k = 0; k < (size_t(2) << dim); ++k) {
        f1_distinct.indices.push_back(k * 97);
        f1_distinct.values.push_back(rng.rand_fr());
    }
    std::vector<DenseMultilinearExtension> f2, f3;
    std::vector<std::vector<Fr>> gs, uv;
    for (size_t i = 0; i < n; ++i) {
        f2.push_back(DenseMultilinearExtension::rand(dim, rng));
        f3.push_back(DenseMultilinearExtension::rand(dim, rng));
        std::vector<Fr> g, w;
        for (size_t k = 0; k < dim; ++k) g.push_back(rng.rand_fr());
        for (size_t k = 0; k < 2 * dim; ++k) w.push_back(rng.rand_fr());
        gs.push_back(g);
        uv.push_back(w);
    }
    try {
        int failed = 0;
        if (!evaluate_batch({}, {}).empty() || !GKRRoundSumcheck::evaluate_subclaims_batch({}, {}, {}, {}, {}).empty() ||
            !GKRRoundSumcheckSubClaim::verify_subclaim_batch({}, {}, {}, {}, {}).empty()) {
            std::printf("FAILED: an empty batch returned values\n");
            return 1;
        }
        std::vector<const ListOfProductsOfPolynomials *> pp;
        for (const auto &p : polys) pp.push_back(&p);
        std::vector<std::vector<Fr>> tv;
        const std::vector<Fr> got = evaluate_batch(pp, points, &tv);
        for (size_t i = 0; i < n; ++i) {
            bool same = got[i] == evaluate(polys[i], points[i]) && tv[i].size() == 3;
            for (size_t u = 0; same && u < 3; ++u) same = tv[i][u] == polys[i].flattened_ml_extensions[u]->evaluate(points[i]);
            if (!same) {
                std::printf("  FAILED: polynomial %zu differs from evaluate\n", i);
                ++failed;
            }
        }
        std::vector<const SparseMultilinearExtension *> p1;
        std::vector<const DenseMultilinearExtension *> p2, p3;
        for (size_t i = 0; i < n; ++i) {
            p1.push_back(i % 2 ? &f1 : &f1_distinct);
            p2.push_back(&f2[i]);
            p3.push_back(&f3[i]);
        }
        const auto ev = GKRRoundSumcheck::evaluate_subclaims_batch(p1, p2, p3, gs, uv);
        std::vector<GKRRoundSumcheckSubClaim> claims;
        for (size_t i = 0; i < n; ++i) {
            const std::vector<Fr> u(uv[i].begin(), uv[i].begin() + dim), v(uv[i].begin() + dim, uv[i].end());
            bool same = ev[i][1] == f2[i].evaluate(u) && ev[i][2] == f3[i].evaluate(v);
            Fr ab, abc;
            check(sc_fr_elementwise(0, ev[i][0].l, ev[i][1].l, ab.l, 1));
            check(sc_fr_elementwise(0, ab.l, ev[i][2].l, abc.l, 1));
            same = same && abc == ev[i][3];
            if (i % 2 == 0) { // distinct indices: f1(g, u, v) is sc_sparse_evaluate's
                std::vector<Fr> guv(gs[i]);
                guv.insert(guv.end(), uv[i].begin(), uv[i].end());
                Fr a;
                check(sc_sparse_evaluate(f1_distinct.indices.data(), f1_distinct.values[0].l, f1_distinct.indices.size(), (uint32_t)(3 * dim), guv[0].l, a.l));
                same = same && a == ev[i][0];
            }
            if (!same) {
                std::printf("  FAILED: GKR instance %zu differs from the single-instance queries\n", i);
                ++failed;
            }
            claims.push_back(GKRRoundSumcheckSubClaim{u, v, i == 3 ? ev[i][1] : ev[i][3]}); // instance 3: a wrong expectation
        }
        const std::vector<bool> ok = GKRRoundSumcheckSubClaim::verify_subclaim_batch(claims, p1, p2, p3, gs);
        for (size_t i = 0; i < n; ++i)
            if (ok[i] != (i != 3) || (i % 2 == 0 && ok[i] != claims[i].verify_subclaim(f1_distinct, f2[i], f3[i], gs[i]))) {
                std::printf("  FAILED: verify_subclaim_batch, instance %zu\n", i);
                ++failed;
            }
        if (failed) return 1;
        std::printf("ALL TESTS PASSED\n");
        return 0;
    } catch (const Panic &p) {
        std::printf("PANIC %d: %s\n", p.code, p.what());
        return p.code == SC_ERR_HIP && std::string(p.what()).find("no CPU fallback") != std::string::npos ? 3 : 2;
    }
}
