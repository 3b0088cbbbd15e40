"""GPU tests of the batched interactive rounds (sc_batch_prover_*: IPForMLSumcheck.prover_init_batch / prove_round_batch): one prove_round
of n small provers per call, the caller's challenges.  Every message of every round of every instance is compared bit for bit with the
oracle's (cref.Prover(desc).prove_round(r) on H.desc_from(...)), bound tables and randomness with its .state(); none sampled, none skipped."""
import ctypes as C

import numpy as np
import pytest
import torch

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib
from tests import fe_model as fm
from tests import helpers as H
from tests.test_gpu_batch import C2, C3, ENVELOPE, GKR, SIX, SQUARED, TWO, make_batch

pytestmark = pytest.mark.gpu
P = fm.P
VM = sc.VerifierMsg


def plans():
    p = _lib.plan_stats()
    return p["batch.rounds_one_block"], p["batch.rounds_serial"]


def challenges(n, nv, seed):
    """(nv, n, 4): challenge [j][i] follows message j of instance i -- all distinct, so a mixed-up index cannot pass"""
    return cref.synth_table(seed, 77, n * nv).reshape(nv, n, 4)


def v_msgs(chal_j):
    return [VM(chal_j[i]) for i in range(chal_j.shape[0])]


class Oracle:
    """n reference provers advanced round by round"""

    def __init__(self, descs):
        self.provers = [cref.Prover(d, threads=1) for d in descs]

    def round(self, chal_j):
        """chal_j: None, or (n, 4) -> (n, D, 4)"""
        return np.stack([p.prove_round(None if chal_j is None else chal_j[i]) for i, p in enumerate(self.provers)])

    def state(self, i):
        return self.provers[i].state()


def assert_state(st, orc, i, where):
    rand, tabs, rnd = orc.state(i)
    assert st.round == rnd, where
    assert np.array_equal(st.randomness(i), rand), f"{where}: randomness of instance {i}"
    got = st.flattened_ml_extensions(i)
    assert len(got) == tabs.shape[0]
    for u, t in enumerate(got):
        assert np.array_equal(np.asarray(t.evaluations), tabs[u]), f"{where}: bound table {u} of instance {i}"


def run_rounds(st, descs, chal, shared=False, check_state=True):
    """every round of the handle against fresh reference provers; chal (nv, n, 4); shared: instance 0's challenge for all, passed once"""
    n, nv = len(descs), descs[0].num_vars
    orc = Oracle(descs)
    msgs = []
    for j in range(nv):
        cj = None if j == 0 else (np.repeat(chal[j - 1][:1], n, axis=0) if shared else chal[j - 1])
        want = orc.round(cj)
        got = sc.IPForMLSumcheck.prove_round_batch(st, None if j == 0 else (VM(cj[0]) if shared else v_msgs(cj)))
        got = np.stack([m.evaluations for m in got])
        bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
        assert np.array_equal(got, want), f"round {j + 1}: messages differ from the oracle's, first for instance {bad[:1]}"
        msgs.append(got)
        if check_state and (j + 1) in (1, 2, nv):
            for i in sorted({0, n - 1}):
                assert_state(st, orc, i, f"after round {j + 1}")
    return np.stack(msgs, axis=1), orc  # (n, nv, D, 4)


def _parity_cases():
    for name, (shapes, nv_max) in ENVELOPE.items():
        for nv in (1, 2, 5, nv_max):
            for n in (1, 2, 7, 1000):
                if n == 1000 and nv > 5:
                    continue
                yield pytest.param(shapes, nv, n, id=f"{name}-nv{nv}-n{n}")


@pytest.mark.parametrize("shapes,nv,n", list(_parity_cases()))
def test_every_round_equals_the_oracle(shapes, nv, n):
    """every shape of the envelope from one variable (a single round, no bind) to the largest one block's LDS holds; 1000 blocks in a grid"""
    polys, descs = make_batch(n, nv, shapes, 51000 + 97 * nv + n)
    b0, s0 = plans()
    st = sc.IPForMLSumcheck.prover_init_batch(polys)
    run_rounds(st, descs, challenges(n, nv, 52000 + nv + n))
    st.close()
    b1, s1 = plans()
    assert b1 == b0 + nv and s1 == s0, "every round of a batch within the envelope is one launch of the batched kernel"


def test_a_shared_challenge_equals_the_same_challenge_n_times():
    n, nv = 7, 6
    polys, descs = make_batch(n, nv, TWO, 53000)
    chal = challenges(n, nv, 53001)
    st = sc.IPForMLSumcheck.prover_init_batch(polys)
    shared, _ = run_rounds(st, descs, chal, shared=True)
    st.reset()
    orc = Oracle(descs)
    for j in range(nv):
        cj = None if j == 0 else np.repeat(chal[j - 1][:1], n, axis=0)
        want = orc.round(cj)
        got = np.stack([m.evaluations for m in sc.IPForMLSumcheck.prove_round_batch(st, None if j == 0 else v_msgs(cj))])
        assert np.array_equal(got, want) and np.array_equal(got, shared[:, j]), f"round {j + 1}"
    st.close()


def raw(v):
    assert 0 <= v < P
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


@pytest.mark.parametrize("shapes", [GKR, [[0]]], ids=["gkr", "single"])
@pytest.mark.parametrize("entry", [P - 1, 1, (P - 1) * fm.R256 % P], ids=["p-1", "one", "field-minus-one"])
def test_lazy_sums_at_the_bound(shapes, entry):
    """512 pairs a block with EVERY entry at one value and every challenge p - 1: the lazy sums of batch_round.hpp at kLazySumMaxP's rule
    (entries stored as LDS slots: the magnitudes are k_batch_proofs').  n = 2, all rounds against the oracle.
    These cases pin ROUND 0 only: every slope of a constant table is 0, so a bind adds exactly 0 and the entries never go lazy -- later
    rounds see the same canonical values.  Entries at the ends of their lazy range: tests/test_gpu_lazy_entries.py."""
    n, nv = 2, 10
    nt = max(max(s) for s in shapes) + 1
    polys, descs = [], []
    for i in range(n):
        tabs = [np.tile(raw(entry), (1 << nv, 1)) for _ in range(nt)]
        coefs = cref.synth_table(54000 + i, 1000, len(shapes))
        descs.append(H.desc_from(nv, shapes, tabs, coefs))
        polys.append(H.hip_poly_from(nv, shapes, tabs, coefs, device="cuda:0")[0])
    torch.cuda.synchronize()
    chal = np.tile(raw(P - 1), (nv, n, 1))
    b0, s0 = plans()
    st = sc.IPForMLSumcheck.prover_init_batch(polys)
    run_rounds(st, descs, chal)
    st.close()
    assert plans() == (b0 + nv, s0)


def test_the_callers_transcripts_give_prove_batchs_proofs():
    """one Python Blake2b512Rng per instance around the batched rounds = MLSumcheck.prove_batch = the oracle's ml_prove"""
    n, nv = 16, 6
    polys, descs = make_batch(n, nv, TWO, 55000)
    rngs = [sc.Blake2b512Rng.setup() for _ in range(n)]
    for r in rngs:
        r.feed(polys[0].info())
    st = sc.IPForMLSumcheck.prover_init_batch(polys)
    proof, vm = [], None
    for _ in range(nv):
        msgs = sc.IPForMLSumcheck.prove_round_batch(st, vm)
        vm = []
        for i, m in enumerate(msgs):
            rngs[i].feed(m)
            vm.append(sc.IPForMLSumcheck.sample_round(rngs[i]))
        proof.append(np.stack([m.evaluations for m in msgs]))
    st.push_randomness(vm)
    proof = np.stack(proof, axis=1)
    batch = sc.MLSumcheck.prove_batch(polys)
    for i in range(n):
        wp, wr = cref.ml_prove(descs[i], threads=1)
        assert np.array_equal(proof[i], wp), f"instance {i}: the interactive rounds differ from the oracle's proof"
        assert np.array_equal(np.stack([m.evaluations for m in batch[i]]), wp), f"instance {i}: prove_batch"
        assert np.array_equal(st.randomness(i), wr), f"instance {i}: randomness"
    st.close()


def test_bind_final_gives_the_table_values_at_the_point():
    n, nv = 5, 7
    polys, descs = make_batch(n, nv, TWO, 56000)
    chal = challenges(n, nv, 56001)
    st = sc.IPForMLSumcheck.prover_init_batch(polys)
    run_rounds(st, descs, chal, check_state=False)
    tv = st.bind_final(v_msgs(chal[nv - 1]))
    for i in range(n):
        point = chal[:, i]
        _, want_tv = polys[i].evaluate_with_tables(point)
        assert np.array_equal(tv[i], want_tv), f"instance {i}: sc_poly_evaluate's table values"
        for u, t in enumerate(descs[i].tables):
            assert np.array_equal(tv[i, u], cref.fix_variables(t, point)[0]), f"instance {i}, table {u}: the oracle's fix_variables"
        assert np.array_equal(st.randomness(i), point)
    with pytest.raises(sc.SumcheckError) as e:
        sc.IPForMLSumcheck.prove_round_batch(st, v_msgs(chal[0]))
    assert e.value.code == _lib.SC_ERR_NOT_ACTIVE
    with pytest.raises(sc.SumcheckError) as e:
        st.bind_final(v_msgs(chal[0]))
    assert e.value.code == _lib.SC_ERR_NOT_ACTIVE
    st.close()


def test_misuse_maps_to_status_codes_and_leaves_the_handle_where_it_was():
    n, nv = 5, 3
    polys, descs = make_batch(n, nv, C2, 57000)
    chal = challenges(n, nv, 57001)
    orc = Oracle(descs)
    st = sc.IPForMLSumcheck.prover_init_batch(polys)

    def ok(cj):
        got = np.stack([m.evaluations for m in sc.IPForMLSumcheck.prove_round_batch(st, None if cj is None else v_msgs(cj))])
        assert np.array_equal(got, orc.round(cj))

    with pytest.raises(sc.SumcheckError) as e:  # a challenge on the first call
        sc.IPForMLSumcheck.prove_round_batch(st, v_msgs(chal[0]))
    assert e.value.code == _lib.SC_ERR_FIRST_ROUND_HAS_MSG and e.value.msg == "first round should be prover first."
    assert st.round == 0
    ok(None)
    with pytest.raises(sc.SumcheckError) as e:  # NULL on a later call
        sc.IPForMLSumcheck.prove_round_batch(st, None)
    assert e.value.code == _lib.SC_ERR_MISSING_MSG and e.value.msg == "verifier message is empty"
    assert st.round == 1
    bad = chal[0].copy()
    bad[3] = raw(P - 1) + np.array([1, 0, 0, 0], dtype=np.uint64)  # p itself
    with pytest.raises(sc.SumcheckError) as e:  # a non-canonical challenge for instance 3 of 5
        sc.IPForMLSumcheck.prove_round_batch(st, v_msgs(bad))
    assert e.value.code == _lib.SC_ERR_BAD_ARG and e.value.msg.startswith("instance 3: challenge is not canonical"), e.value.msg
    assert st.round == 1 and st.randomness(0).shape == (0, 4)
    ok(chal[0])
    ok(chal[1])
    assert_state(st, orc, 4, "after the misuse")
    with pytest.raises(sc.SumcheckError) as e:  # a call after the last round
        sc.IPForMLSumcheck.prove_round_batch(st, v_msgs(chal[2]))
    assert e.value.code == _lib.SC_ERR_NOT_ACTIVE and e.value.msg == "Prover is not active"
    assert st.round == nv
    st.close()


def test_the_serial_plan_gives_the_same_bits():
    """beyond one block's LDS, and policy batch = 0 within it: n ordinary provers inside the handle"""
    n = 3
    polys, descs = make_batch(n, 10, C2, 58000)
    b0, s0 = plans()
    st = sc.IPForMLSumcheck.prover_init_batch(polys)
    chal = challenges(n, 10, 58001)
    run_rounds(st, descs, chal)
    tv = st.bind_final(v_msgs(chal[9]))
    for i in range(n):
        assert np.array_equal(tv[i], polys[i].evaluate_with_tables(chal[:, i])[1])
    st.reset()
    run_rounds(st, descs, challenges(n, 10, 58002), check_state=False)
    st.close()
    assert plans() == (b0, s0 + 20)
    polys, descs = make_batch(n, 6, C2, 58100)
    with _lib.policy(batch=0):
        b0, s0 = plans()
        st = sc.IPForMLSumcheck.prover_init_batch(polys)
        serial, _ = run_rounds(st, descs, challenges(n, 6, 58101))
        st.close()
        assert plans() == (b0, s0 + 6)
    st = sc.IPForMLSumcheck.prover_init_batch(polys)
    batched, _ = run_rounds(st, descs, challenges(n, 6, 58101))
    st.close()
    assert np.array_equal(serial, batched) and plans() == (b0 + 6, s0 + 6)


def test_reset_with_the_same_and_with_new_tables_and_two_handles_in_turn():
    n, nv = 4, 6
    polys_a, descs_a = make_batch(n, nv, SQUARED, 59000)
    polys_b, descs_b = make_batch(n, nv, SQUARED, 59100)
    b0, s0 = plans()
    st = sc.IPForMLSumcheck.prover_init_batch(polys_a)
    run_rounds(st, descs_a, challenges(n, nv, 59001))
    st.reset()  # the same tables, other challenges
    assert st.round == 0 and st.randomness(0).shape == (0, 4)
    run_rounds(st, descs_a, challenges(n, nv, 59002))
    st.reset(polys_b)  # new tables and coefficients
    run_rounds(st, descs_b, challenges(n, nv, 59003))
    st.reset()  # ... which are the handle's tables now
    run_rounds(st, descs_b, challenges(n, nv, 59004), check_state=False)
    # two handles advanced alternately, round by round, with a one-shot proof of a third polynomial in between
    st2 = sc.IPForMLSumcheck.prover_init_batch(polys_a)
    st.reset()
    third, third_desc = make_batch(1, 8, C2, 59200)
    want_third = cref.ml_prove(third_desc[0], threads=1)[0]
    o1, o2 = Oracle(descs_b), Oracle(descs_a)
    c1, c2 = challenges(n, nv, 59005), challenges(n, nv, 59006)
    for j in range(nv):
        for s, o, c in ((st, o1, c1), (st2, o2, c2)):
            cj = None if j == 0 else c[j - 1]
            got = np.stack([m.evaluations for m in sc.IPForMLSumcheck.prove_round_batch(s, None if j == 0 else v_msgs(cj))])
            assert np.array_equal(got, o.round(cj)), f"round {j + 1}"
            if s is st:
                assert np.array_equal(np.stack([m.evaluations for m in sc.MLSumcheck.prove(third[0])]), want_third)
    assert_state(st, o1, n - 1, "first handle")
    assert_state(st2, o2, 0, "second handle")
    st.close()
    st2.close()
    assert plans() == (b0 + 6 * nv, s0)


def test_host_tables_and_device_tables_give_identical_output():
    n, nv = 7, 5
    out = []
    for device in ("cuda:0", None):
        polys, descs = make_batch(n, nv, C3, 60000, device=device)
        st = sc.IPForMLSumcheck.prover_init_batch(polys)
        msgs, _ = run_rounds(st, descs, challenges(n, nv, 60001))
        out.append(msgs)
        if device is None:  # a handle built over host tables takes either kind on reset
            polys_d, _ = make_batch(n, nv, C3, 60000, device="cuda:0")
            st.reset(polys_d)
            again, _ = run_rounds(st, descs, challenges(n, nv, 60001), check_state=False)
            assert np.array_equal(again, msgs)
        st.close()
    assert np.array_equal(out[0], out[1])
