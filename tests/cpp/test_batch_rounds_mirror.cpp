// IPForMLSumcheck::prover_init_batch / prove_round_batch and BatchProverState of include/sumcheck_amd.hpp (sc_batch_prover_* through the C
// ABI) against the single-instance prover_init / prove_round, instance by instance and round by round.  Without a HIP device the library
// has no CPU fallback: the mirror's Panic carries the library's text, which is what this program then reports
// (tests/test_batch_rounds_host.py runs it both ways).
#include <cstdio>
#include <string>

#include "sumcheck_amd.hpp"

using namespace sumcheck;

int main() {
    Blake2b512Rng rng = Blake2b512Rng::setup();
    rng.feed("batch rounds mirror");
    const size_t nv = 5, n = 6;
    // ---- n polynomials of one structure: c0 * A B C + c1 * B B, tables per instance --------------------------------------------------
    std::vector<ListOfProductsOfPolynomials> polys;
    for (size_t i = 0; i < n; ++i) {
        auto A = std::make_shared<DenseMultilinearExtension>(DenseMultilinearExtension::rand(nv, rng));
        auto B = std::make_shared<DenseMultilinearExtension>(DenseMultilinearExtension::rand(nv, rng));
        auto Cc = std::make_shared<DenseMultilinearExtension>(DenseMultilinearExtension::rand(nv, rng));
        ListOfProductsOfPolynomials p(nv);
        p.add_product({A, B, Cc}, rng.rand_fr());
        p.add_product({B, B}, rng.rand_fr());
        polys.push_back(std::move(p));
    }
    std::vector<const ListOfProductsOfPolynomials *> pp;
    for (const auto &p : polys) pp.push_back(&p);
    // the argument checks come before any HIP call: the same with and without a device
    try {
        (void)IPForMLSumcheck::prover_init_batch({});
        std::printf("FAILED: a handle over no instance\n");
        return 1;
    } catch (const Panic &p) {
        if (p.code != SC_ERR_BAD_ARG) {
            std::printf("FAILED: n == 0 gave status %d\n", p.code);
            return 1;
        }
    }
    try {
        int failed = 0;
        BatchProverState st = IPForMLSumcheck::prover_init_batch(pp);
        std::vector<ProverState> single;
        for (const auto &p : polys) single.push_back(IPForMLSumcheck::prover_init(p));
        for (int pass = 0; pass < 2; ++pass) { // pass 0: a challenge per instance; pass 1 (after a reset): one shared challenge
            std::vector<VerifierMsg> vm;
            if (pass == 1) {
                st.reset();
                single.clear();
                for (const auto &p : polys) single.push_back(IPForMLSumcheck::prover_init(p));
            }
            for (size_t j = 0; j < nv; ++j) {
                const std::vector<ProverMsg> got = IPForMLSumcheck::prove_round_batch(st, vm);
                for (size_t i = 0; i < n; ++i) {
                    const std::optional<VerifierMsg> one = j == 0 ? std::nullopt : std::optional<VerifierMsg>(vm[vm.size() == 1 ? 0 : i]);
                    if (!(got[i].evaluations == IPForMLSumcheck::prove_round(single[i], one).evaluations)) {
                        std::printf("  FAILED: pass %d, round %zu, instance %zu differs from prove_round\n", pass, j + 1, i);
                        ++failed;
                    }
                }
                vm.clear();
                for (size_t i = 0; i < (pass == 0 ? n : 1); ++i) vm.push_back(VerifierMsg{rng.rand_fr()});
            }
            if (st.round() != nv || st.randomness(n - 1).size() != nv - 1) {
                std::printf("  FAILED: pass %d, round / randomness after the last round\n", pass);
                ++failed;
            }
            const auto tabs = st.flattened_ml_extensions(n - 1), want = single[n - 1].flattened_ml_extensions();
            for (size_t u = 0; u < want.size(); ++u)
                if (!(tabs[u].evaluations == want[u].evaluations)) {
                    std::printf("  FAILED: pass %d, bound table %zu of the last instance\n", pass, u);
                    ++failed;
                }
            if (pass == 1) { // the last variable: the tables' values at the point
                const std::vector<std::vector<Fr>> tv = st.bind_final(vm);
                std::vector<Fr> point = st.randomness(0);
                for (size_t i = 0; i < n; ++i)
                    for (size_t u = 0; u < 3; ++u)
                        if (!(tv[i][u] == polys[i].flattened_ml_extensions[u]->evaluate(point))) {
                            std::printf("  FAILED: bind_final, instance %zu, table %zu\n", i, u);
                            ++failed;
                        }
                try {
                    (void)IPForMLSumcheck::prove_round_batch(st, vm);
                    std::printf("  FAILED: a round after bind_final\n");
                    ++failed;
                } catch (const Panic &p) {
                    if (p.code != SC_ERR_NOT_ACTIVE) ++failed;
                }
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
