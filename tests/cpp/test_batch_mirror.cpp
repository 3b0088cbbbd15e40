// MLSumcheck::prove_batch of include/sumcheck_amd.hpp (sc_ml_prove_batch through the C ABI): a batch of small instances of one structure
// against MLSumcheck::prove instance by instance.  Without a HIP device the library has no CPU fallback: the mirror's Panic carries the
// library's text, which is what this program then reports (tests/test_batch_host.py runs it both ways).
#include <cstdio>
#include <memory>
#include <string>

#include "sumcheck_amd.hpp"

using namespace sumcheck;

int main() {
    Blake2b512Rng rng = Blake2b512Rng::setup();
    const size_t nv = 5, n = 6;
    std::vector<ListOfProductsOfPolynomials> polys;
    for (size_t i = 0; i < n; ++i) {
        ListOfProductsOfPolynomials poly(nv);
        std::vector<std::shared_ptr<DenseMultilinearExtension>> t;
        for (int j = 0; j < 3; ++j) t.push_back(std::make_shared<DenseMultilinearExtension>(DenseMultilinearExtension::rand(nv, rng)));
        poly.add_product({t[0], t[1], t[2]}, rng.rand_fr());
        poly.add_product({t[1], t[1]}, rng.rand_fr());
        polys.push_back(std::move(poly));
    }
    std::vector<const ListOfProductsOfPolynomials *> ptrs;
    for (const auto &p : polys) ptrs.push_back(&p);
    try {
        if (!MLSumcheck::prove_batch({}).empty()) {
            std::printf("FAILED: an empty batch returned proofs\n");
            return 1;
        }
        std::vector<std::vector<Fr>> challenges;
        const std::vector<Proof> got = MLSumcheck::prove_batch(ptrs, {}, &challenges);
        int failed = 0;
        for (size_t i = 0; i < n; ++i) {
            const Proof want = MLSumcheck::prove(polys[i]);
            bool same = got[i].size() == want.size() && challenges[i].size() == nv;
            for (size_t j = 0; same && j < want.size(); ++j) same = got[i][j].evaluations == want[j].evaluations;
            if (!same) {
                std::printf("  FAILED: instance %zu differs from MLSumcheck::prove\n", i);
                ++failed;
            }
        }
        if (failed) return 1;
        std::printf("ALL TESTS PASSED\n");
        return 0;
    } catch (const Panic &p) {
        std::printf("PANIC %d: %s\n", p.code, p.what());
        return p.code == SC_ERR_HIP && std::string(p.what()).find("no CPU fallback") != std::string::npos ? 3 : 2;
    }
}
