// GKRRoundSumcheck::prover_init_batch and GKRBatchProverState of include/sumcheck_amd.hpp (sc_gkr_batch_prover_* through the C ABI)
// against GKRRoundSumcheck::prove: the handle is driven by n Blake2b transcripts of the caller's -- feed the message, sample the
// challenge, as mod.rs:111-133 does -- and has to reproduce every proof, (u, v) and the verifier's expected evaluation.  Without a HIP
// device the library has no CPU fallback: the mirror's Panic carries the library's text, which is what this program then reports.
#include <cstdio>
#include <string>

#include "sumcheck_amd.hpp"

using namespace sumcheck;

int main() {
    Blake2b512Rng rng = Blake2b512Rng::setup();
    rng.feed("gkr batch rounds mirror");
    const size_t dim = 4, n = 5, N = size_t(1) << dim;
    // ---- n instances of one dim; instances 3 and 4 share the wiring predicate of instance 0 -------------------------------------------
    std::vector<SparseMultilinearExtension> f1(n);
    std::vector<DenseMultilinearExtension> f2, f3;
    std::vector<std::vector<Fr>> gs(n);
    for (size_t i = 0; i < n; ++i) {
        f1[i].num_vars = 3 * dim;
        for (size_t k = 0; k < 2 * N + i; ++k) { // distinct indices, in no particular order
            f1[i].indices.push_back((k * 2654435761ULL + 977 * i) % (1ULL << (3 * dim)));
            f1[i].values.push_back(rng.rand_fr());
        }
        std::sort(f1[i].indices.begin(), f1[i].indices.end());
        f1[i].indices.erase(std::unique(f1[i].indices.begin(), f1[i].indices.end()), f1[i].indices.end());
        f1[i].values.resize(f1[i].indices.size());
        f2.push_back(DenseMultilinearExtension::rand(dim, rng));
        f3.push_back(DenseMultilinearExtension::rand(dim, rng));
        for (size_t j = 0; j < dim; ++j) gs[i].push_back(rng.rand_fr());
    }
    std::vector<const SparseMultilinearExtension *> p1;
    std::vector<const DenseMultilinearExtension *> p2, p3;
    for (size_t i = 0; i < n; ++i) {
        p1.push_back(&f1[i >= 3 ? 0 : i]);
        p2.push_back(&f2[i]);
        p3.push_back(&f3[i]);
    }
    // the argument checks come before any HIP call: the same with and without a device
    try {
        (void)GKRRoundSumcheck::prover_init_batch({}, {}, {}, {});
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
        GKRBatchProverState st = GKRRoundSumcheck::prover_init_batch(p1, p2, p3, gs);
        for (int pass = 0; pass < 2; ++pass) { // pass 1: after a reset, the same transcripts again
            if (pass == 1) st.reset();
            std::vector<Blake2b512Rng> mine, theirs;
            for (size_t i = 0; i < n; ++i) {
                mine.push_back(Blake2b512Rng::setup());
                theirs.push_back(Blake2b512Rng::setup());
                mine[i].feed("layer " + std::to_string(i));
                theirs[i].feed("layer " + std::to_string(i));
            }
            std::vector<GKRProof> want;
            for (size_t i = 0; i < n; ++i) want.push_back(GKRRoundSumcheck::prove(theirs[i], *p1[i], *p2[i], *p3[i], gs[i]));
            std::vector<VerifierMsg> vm;
            for (size_t t = 0; t < 2 * dim; ++t) {
                const std::vector<ProverMsg> got = st.prove_round(vm);
                vm.clear();
                for (size_t i = 0; i < n; ++i) {
                    const ProverMsg &w = t < dim ? want[i].phase1_sumcheck_msgs[t] : want[i].phase2_sumcheck_msgs[t - dim];
                    if (!(got[i].evaluations == w.evaluations)) {
                        std::printf("  FAILED: pass %d, round %zu, instance %zu differs from GKRRoundSumcheck::prove\n", pass, t + 1, i);
                        ++failed;
                    }
                    sc_rng_feed_prover_msg(mine[i].raw(), got[i].evaluations[0].l, 3);
                    vm.push_back(VerifierMsg{mine[i].rand_fr()});
                }
                if (st.round() != t + 1 || st.randomness(n - 1).size() != t) {
                    std::printf("  FAILED: pass %d, round / randomness after call %zu\n", pass, t + 1);
                    ++failed;
                }
            }
            if (st.tables(0).size() != 2 || st.tables(0)[0].evaluations.size() != 2) {
                std::printf("  FAILED: pass %d, the tables before finish\n", pass);
                ++failed;
            }
            const std::vector<GKRBatchProverState::Final> fin = st.finish(vm);
            for (size_t i = 0; i < n; ++i) {
                Blake2b512Rng vr = Blake2b512Rng::setup();
                vr.feed("layer " + std::to_string(i));
                const GKRRoundSumcheckSubClaim sub = GKRRoundSumcheck::verify(vr, dim, want[i], want[i].extract_sum());
                Fr prod;
                check(sc_fr_elementwise(0, fin[i].f1_guv.l, fin[i].f2u_f3v.l, prod.l, 1));
                if (!(fin[i].u == sub.u) || !(fin[i].v == sub.v) || !(prod == sub.expected_evaluation) || !(fin[i].f2_u == p2[i]->evaluate(sub.u))) {
                    std::printf("  FAILED: pass %d, finish of instance %zu against the verifier's subclaim\n", pass, i);
                    ++failed;
                }
                if (!(mine[i].rand_fr() == theirs[i].rand_fr())) {
                    std::printf("  FAILED: pass %d, the transcript of instance %zu after the proof\n", pass, i);
                    ++failed;
                }
            }
            try {
                (void)st.prove_round(vm);
                std::printf("  FAILED: a round after finish\n");
                ++failed;
            } catch (const Panic &p) {
                if (p.code != SC_ERR_NOT_ACTIVE) ++failed;
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
