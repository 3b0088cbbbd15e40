// The gate form through include/sumcheck_amd.hpp (sc_gkr_gates_init_batch / sc_gkr_gates_next_batch through the C ABI): one handle is built
// over layer A of multiplication and addition gates in two-point form and proves it (pass 0), is put onto layer B with new wiring in
// one-point form (pass 1), onto layer A's tables with B's wiring KEPT in two-point form (pass 2) and onto layer A again (pass 3: pass 0's
// bits).  The program prints what it proved over -- both layers' lists, tables, points and coefficients, every challenge -- and every
// message and finish's three values, as lines of "key: hex words"; tests/test_gpu_gkr_gates.py computes the oracle's walks over the printed
// inputs and compares.  The verifier's helper runs on pass 0's and pass 1's values.  Without a HIP device the library has no CPU fallback:
// the mirror's Panic carries the library's text, which is what this program then reports.
#include <cstdio>
#include <string>

#include "sumcheck_amd.hpp"

using namespace sumcheck;

static void row(const std::string &key, const uint64_t *w, size_t n) {
    std::printf("%s:", key.c_str());
    for (size_t k = 0; k < n; ++k) std::printf(" %llx", (unsigned long long)w[k]);
    std::printf("\n");
}
static void row(const std::string &key, const std::vector<Fr> &v) { row(key, v.empty() ? nullptr : v[0].l, 4 * v.size()); }

struct Layer {
    std::vector<SparseMultilinearExtension> mul, add;
    std::vector<DenseMultilinearExtension> f2, f3;
    std::vector<std::vector<Fr>> gs, g2s;
    std::vector<std::array<Fr, 2>> coeffs;
    std::vector<const SparseMultilinearExtension *> pm, pa;
    std::vector<const DenseMultilinearExtension *> p2, p3;
};

int main() {
    Blake2b512Rng rng = Blake2b512Rng::setup();
    rng.feed("gkr gates mirror");
    const size_t dim = 4, n = 3, N = size_t(1) << dim;
    Layer L[2];
    for (int l = 0; l < 2; ++l) {
        Layer &y = L[l];
        y.mul.resize(n);
        y.add.resize(n);
        y.gs.resize(n);
        y.g2s.resize(n);
        y.coeffs.resize(n);
        for (size_t i = 0; i < n; ++i) {
            for (int k = 0; k < 2; ++k) {
                SparseMultilinearExtension &f1 = k ? y.add[i] : y.mul[i];
                f1.num_vars = 3 * dim;
                const size_t nnz = l == 0 ? 2 * N + i + k : (i == (size_t)(1 + k) ? 0 : N - 1 + i); // layer B: shorter lists, an empty one on either side
                for (size_t e = 0; e < nnz; ++e) {
                    f1.indices.push_back((e * 2654435761ULL + 977 * i + 31 * l + 7 * k) % (1ULL << (3 * dim)));
                    f1.values.push_back(rng.rand_fr());
                }
            }
            y.f2.push_back(DenseMultilinearExtension::rand(dim, rng));
            y.f3.push_back(DenseMultilinearExtension::rand(dim, rng));
            for (size_t j = 0; j < dim; ++j) y.gs[i].push_back(rng.rand_fr());
            for (size_t j = 0; j < dim; ++j) y.g2s[i].push_back(rng.rand_fr());
            y.coeffs[i] = {rng.rand_fr(), rng.rand_fr()};
        }
        for (size_t i = 0; i < n; ++i) {
            y.pm.push_back(&y.mul[i]);
            y.pa.push_back(&y.add[i]);
            y.p2.push_back(&y.f2[i]);
            y.p3.push_back(&y.f3[i]);
            const std::string name = std::string(l == 0 ? "A" : "B"), at = " " + std::to_string(i);
            row(name + " mul idx" + at, y.mul[i].indices.data(), y.mul[i].indices.size());
            row(name + " mul vals" + at, y.mul[i].values);
            row(name + " add idx" + at, y.add[i].indices.data(), y.add[i].indices.size());
            row(name + " add vals" + at, y.add[i].values);
            row(name + " f2" + at, y.f2[i].evaluations);
            row(name + " f3" + at, y.f3[i].evaluations);
            row(name + " g" + at, y.gs[i]);
            row(name + " g2" + at, y.g2s[i]);
            row(name + " coef" + at, y.coeffs[i][0].l, 8);
        }
    }
    const uint64_t shape[2] = {dim, n};
    row("dim", shape, 1);
    row("n", shape + 1, 1);
    try {
        GKRBatchProverState st = GKRRoundSumcheck::prover_init_batch_gates(L[0].pm, L[0].pa, L[0].p2, L[0].p3, L[0].gs, L[0].g2s, L[0].coeffs);
        for (int pass = 0; pass < 4; ++pass) {
            const Layer &A = L[0], &B = L[1];
            if (pass == 1) st.next_layer_gates(B.p2, B.p3, B.gs, B.pm, B.pa);                         // new wiring, one point
            if (pass == 2) st.next_layer_gates(A.p2, A.p3, A.gs, {}, {}, A.g2s, A.coeffs);            // B's wiring kept, A's tables and points
            if (pass == 3) st.next_layer_gates(A.p2, A.p3, A.gs, A.pm, A.pa, A.g2s, A.coeffs);        // pass 0 again
            if (st.round() != 0 || !st.randomness(0).empty()) {
                std::printf("FAILED: pass %d does not start at round 0\n", pass);
                return 1;
            }
            Blake2b512Rng chal = Blake2b512Rng::setup();
            chal.feed("challenges"); // (the same for passes 0 and 3: the two proofs have to agree)
            if (pass == 1) chal.feed("of layer B");
            if (pass == 2) chal.feed("of the kept wiring");
            std::vector<Fr> all_chal, all_msgs;
            std::vector<VerifierMsg> vm;
            for (size_t t = 0; t < 2 * dim; ++t) {
                const std::vector<ProverMsg> got = st.prove_round(vm);
                vm.clear();
                for (size_t i = 0; i < n; ++i) {
                    all_msgs.insert(all_msgs.end(), got[i].evaluations.begin(), got[i].evaluations.end());
                    vm.push_back(VerifierMsg{chal.rand_fr()});
                    all_chal.push_back(vm.back().randomness);
                }
            }
            const std::vector<GKRBatchProverState::Final> fin = st.finish(vm);
            std::vector<Fr> triple;
            for (size_t i = 0; i < n; ++i) {
                triple.push_back(fin[i].f1_guv);  // on a gate handle: f2(u)
                triple.push_back(fin[i].f2_u);    //                   f3(v)
                triple.push_back(fin[i].f2u_f3v); //                   f3(v) T1(v) + T2(v), what the verifier compares
            }
            const std::string p = "pass " + std::to_string(pass);
            row(p + " challenges", all_chal);
            row(p + " messages", all_msgs);
            row(p + " final", triple);
            if (pass <= 1) { // the verifier's helper accepts the third value at (u, v), and rejects it with one bit flipped
                const Layer &y = L[pass];
                std::vector<GKRRoundSumcheckSubClaim> claims(n);
                for (size_t i = 0; i < n; ++i) {
                    claims[i].u = fin[i].u;
                    claims[i].v = fin[i].v;
                    claims[i].expected_evaluation = fin[i].f2u_f3v;
                }
                claims[n - 1].expected_evaluation.l[0] ^= 1;
                const std::vector<bool> ok = pass == 0 ? GKRRoundSumcheckSubClaim::verify_subclaim_gates_batch(claims, y.pm, y.pa, y.p2, y.p3, y.gs, y.g2s, y.coeffs)
                                                       : GKRRoundSumcheckSubClaim::verify_subclaim_gates_batch(claims, y.pm, y.pa, y.p2, y.p3, y.gs);
                for (size_t i = 0; i < n; ++i)
                    if (ok[i] != (i + 1 != n)) {
                        std::printf("FAILED: the gate subclaim of instance %zu in pass %d\n", i, pass);
                        return 1;
                    }
            }
        }
        // the older next call refuses a gate handle, and the mirror refuses a g2 without coefficients
        try {
            st.next_layer(L[1].p2, L[1].p3, L[1].gs);
            std::printf("FAILED: sc_gkr_layer_next_batch took a gate handle\n");
            return 1;
        } catch (const Panic &p) {
            if (p.code != SC_ERR_BAD_ARG) return 1;
        }
        try {
            st.next_layer_gates(L[1].p2, L[1].p3, L[1].gs, {}, {}, L[1].g2s);
            std::printf("FAILED: g2 without coefficients\n");
            return 1;
        } catch (const Panic &p) {
            if (p.code != SC_ERR_BAD_ARG) return 1;
        }
        std::printf("DONE\n");
        return 0;
    } catch (const Panic &p) {
        std::printf("PANIC %d: %s\n", p.code, p.what());
        return p.code == SC_ERR_HIP && std::string(p.what()).find("no CPU fallback") != std::string::npos ? 3 : 2;
    }
}
