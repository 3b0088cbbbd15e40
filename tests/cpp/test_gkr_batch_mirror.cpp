// GKRRoundSumcheck::prove_batch of include/sumcheck_amd.hpp (sc_gkr_prove_batch through the C ABI): a batch of small instances of one dim,
// one wiring predicate shared by all of them, against GKRRoundSumcheck::prove instance by instance -- proofs, (u, v) and the transcripts'
// next sample.  Without a HIP device the library has no CPU fallback: the mirror's Panic carries the library's text, which is what this
// program then reports (tests/test_gkr_batch_host.py runs it both ways).
#include <cstdio>
#include <string>

#include "sumcheck_amd.hpp"

using namespace sumcheck;

static Blake2b512Rng fed(size_t i) {
    Blake2b512Rng r = Blake2b512Rng::setup();
    r.feed("gkr batch mirror " + std::to_string(i));
    return r;
}

int main() {
    Blake2b512Rng rng = Blake2b512Rng::setup();
    const size_t dim = 4, n = 5;
    SparseMultilinearExtension f1;
    f1.num_vars = 3 * dim;
    for (size_t k = 0; k < (size_t(2) << dim); ++k) { // (a repeated index now and then: summed)
        f1.indices.push_back((k * 2654435761ull) & ((uint64_t(1) << (3 * dim)) - 1));
        f1.values.push_back(rng.rand_fr());
    }
    std::vector<DenseMultilinearExtension> f2, f3;
    std::vector<std::vector<Fr>> gs;
    for (size_t i = 0; i < n; ++i) {
        f2.push_back(DenseMultilinearExtension::rand(dim, rng));
        f3.push_back(DenseMultilinearExtension::rand(dim, rng));
        std::vector<Fr> g;
        for (size_t k = 0; k < dim; ++k) g.push_back(rng.rand_fr());
        gs.push_back(g);
    }
    try {
        if (!GKRRoundSumcheck::prove_batch({}, {}, {}, {}, {}).empty()) {
            std::printf("FAILED: an empty batch returned proofs\n");
            return 1;
        }
        std::vector<Blake2b512Rng> rngs, twins;
        for (size_t i = 0; i < n; ++i) {
            rngs.push_back(fed(i));
            twins.push_back(fed(i));
        }
        std::vector<Blake2b512Rng *> rp;
        std::vector<const SparseMultilinearExtension *> p1;
        std::vector<const DenseMultilinearExtension *> p2, p3;
        for (size_t i = 0; i < n; ++i) {
            rp.push_back(&rngs[i]);
            p1.push_back(&f1);
            p2.push_back(&f2[i]);
            p3.push_back(&f3[i]);
        }
        std::vector<std::vector<Fr>> uv;
        const std::vector<GKRProof> got = GKRRoundSumcheck::prove_batch(rp, p1, p2, p3, gs, &uv);
        int failed = 0;
        for (size_t i = 0; i < n; ++i) {
            const GKRProof want = GKRRoundSumcheck::prove(twins[i], f1, f2[i], f3[i], gs[i]);
            bool same = got[i].phase1_sumcheck_msgs.size() == dim && got[i].phase2_sumcheck_msgs.size() == dim && uv[i].size() == 2 * dim;
            for (size_t j = 0; same && j < dim; ++j)
                same = got[i].phase1_sumcheck_msgs[j].evaluations == want.phase1_sumcheck_msgs[j].evaluations &&
                       got[i].phase2_sumcheck_msgs[j].evaluations == want.phase2_sumcheck_msgs[j].evaluations;
            same = same && rngs[i].rand_fr() == twins[i].rand_fr();
            if (!same) {
                std::printf("  FAILED: instance %zu differs from GKRRoundSumcheck::prove\n", i);
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
