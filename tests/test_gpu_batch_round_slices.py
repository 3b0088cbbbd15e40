"""GPU tests of the sliced rounds of the batched interactive provers (policy "batch_slices" = 1, plan batch.rounds_slices:
k_batch_round_slices + k_batch_round_fin, sumcheck_amd/csrc/kernels_batch_round_slices.hip).  An instance beyond one block's LDS is given to
several blocks for its first nv - nv_max + 1 rounds and handed over to k_batch_round on the same work area.  Every message of every round of
every instance is compared bit for bit with cref.Prover(desc).prove_round(r), bound tables and randomness with its .state() -- after rounds 1
and 2, after the last sliced round (the hand-over), after the round behind it and after the last; nothing is sampled.  The counters prove
which kernels ran."""
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
DEV = "cuda:0"
SINGLE = [[0]]
EIGHT = [[0, 1, 2, 3, 4, 5, 6, 7]]
NV_MAX = {**{name: nv_max for name, (_, nv_max) in ENVELOPE.items()}, "single": 11, "eight": 8}  # the largest num_vars one block holds
SHAPES = {**{name: shapes for name, (shapes, _) in ENVELOPE.items()}, "single": SINGLE, "eight": EIGHT}
assert SHAPES["c2"] is C2 and SHAPES["gkr"] is GKR and SHAPES["two"] is TWO and SHAPES["squared"] is SQUARED and SHAPES["c3"] is C3 and SHAPES["six"] is SIX


def plans():
    p = _lib.plan_stats()
    return p.get("batch.rounds_slices"), p["batch.rounds_one_block"], p["batch.rounds_serial"]


def expect(before, name, nv, times=1):
    """the counters after `times` full passes over a sliced handle of the named shape: rounds 0 .. nv - nv_max sliced, the rest one block"""
    sliced = nv - NV_MAX[name] + 1
    return (before[0] + times * sliced, before[1] + times * (nv - sliced), before[2])


def challenges(n, nv, seed):
    """(nv, n, 4): challenge [j][i] follows message j of instance i -- all distinct, so a mixed-up index cannot pass"""
    return cref.synth_table(seed, 77, n * nv).reshape(nv, n, 4)


def v_msgs(chal_j):
    return [VM(chal_j[i]) for i in range(chal_j.shape[0])]


def raw(v):
    assert 0 <= v < P
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


class Oracle:
    """n reference provers advanced round by round"""

    def __init__(self, descs):
        self.provers = [cref.Prover(d, threads=1) for d in descs]

    def round(self, chal_j):
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


def run_rounds(st, descs, chal, name, shared=False, check_state=True, orc=None):
    """every round of the handle against reference provers; the state of instances 0 and n - 1 after rounds 1, 2, the last sliced round (the
    hand-over into k_batch_round), the round behind it and the last"""
    n, nv = len(descs), descs[0].num_vars
    orc = orc or Oracle(descs)
    handover = nv - NV_MAX[name] + 1  # rounds proved when the last sliced round has run
    msgs = []
    for j in range(nv):
        cj = None if j == 0 else (np.repeat(chal[j - 1][:1], n, axis=0) if shared else chal[j - 1])
        want = orc.round(cj)
        got = sc.IPForMLSumcheck.prove_round_batch(st, None if j == 0 else (VM(cj[0]) if shared else v_msgs(cj)))
        got = np.stack([m.evaluations for m in got])
        bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
        assert np.array_equal(got, want), f"round {j + 1}: messages differ from the oracle's, first for instance {bad[:1]}"
        msgs.append(got)
        if check_state and (j + 1) in (1, 2, handover, handover + 1, nv):
            for i in sorted({0, n - 1}):
                assert_state(st, orc, i, f"after round {j + 1}")
    return np.stack(msgs, axis=1), orc  # (n, nv, D, 4)


PARITY = [("c2", 10, 3), ("c2", 12, 2), ("single", 12, 1), ("single", 16, 2), ("gkr", 11, 7), ("gkr", 16, 1), ("squared", 10, 2), ("c3", 9, 2), ("c3", 11, 2),
          ("six", 9, 2), ("eight", 9, 1), ("eight", 12, 1), ("c2", 10, 300)]


@pytest.mark.parametrize("name,nv,n", PARITY, ids=[f"{a}-nv{b}-n{c}" for a, b, c in PARITY])
def test_every_round_equals_the_oracle(name, nv, n):
    """the smallest sizes that can go wrong: one variable beyond every envelope (c2 at nv 10 is the shape test_the_serial_plan_gives_the_same_bits
    pins under the default policy), several beyond, the largest tables (nv 16: six sliced rounds of a single table, eight of the GKR shape), a
    table twice in one product, ten tables in four products, products of six and eight, and more blocks than are resident (n 300)"""
    polys, descs = make_batch(n, nv, SHAPES[name], 81000 + 97 * nv + n)
    with _lib.policy(batch_slices=1):
        before = plans()
        st = sc.IPForMLSumcheck.prover_init_batch(polys)
        run_rounds(st, descs, challenges(n, nv, 82000 + nv + n), name)
        st.close()
        assert plans() == expect(before, name, nv), "rounds 0 .. nv - nv_max as the two sliced launches, the rest as k_batch_round, none serial"


def test_a_shared_challenge_equals_the_same_challenge_n_times():
    n, nv = 5, 11
    polys, descs = make_batch(n, nv, GKR, 83000)
    chal = challenges(n, nv, 83001)
    with _lib.policy(batch_slices=1):
        before = plans()
        st = sc.IPForMLSumcheck.prover_init_batch(polys)
        shared, _ = run_rounds(st, descs, chal, "gkr", shared=True)
        st.reset()
        orc = Oracle(descs)
        for j in range(nv):
            cj = None if j == 0 else np.repeat(chal[j - 1][:1], n, axis=0)
            want = orc.round(cj)
            got = np.stack([m.evaluations for m in sc.IPForMLSumcheck.prove_round_batch(st, None if j == 0 else v_msgs(cj))])
            assert np.array_equal(got, want) and np.array_equal(got, shared[:, j]), f"round {j + 1}"
        st.close()
        assert plans() == expect(before, "gkr", nv, times=2)


# ---- entries at the ends of their lazy range (tests/test_gpu_lazy_entries.py's tables) -------------------------------------------------------
def sinking(nv, s, t):
    m = 1 + t % 7
    c = m * sum(s) + t if t % 2 == 0 else P - 1 - t
    tab = H.sinking_table_limbs(nv, s, m, c)
    H.assert_entries_match(tab, H.sinking_entry(s, m, c), seed=t)
    return tab


def selector(nv, s, sel, t, flip):
    m = 1 + t % 7
    c = m * sum(s) + t
    tab = H.selector_table_limbs(nv, s, sel, m, c, flip)
    H.assert_entries_match(tab, H.selector_entry(s, sel, m, c, flip), seed=t)
    return tab


def range_end_rounds(name, nv, tabs, chal):
    """all rounds of len(tabs) instances over the given tables, then bind_final"""
    shapes, n = SHAPES[name], len(tabs)
    coefs = [cref.synth_table(84000 + i, 1000, len(shapes)) for i in range(n)]
    descs = [H.desc_from(nv, shapes, tabs[i], coefs[i]) for i in range(n)]
    polys = [H.hip_poly_from(nv, shapes, tabs[i], coefs[i], device=DEV)[0] for i in range(n)]
    torch.cuda.synchronize()
    with _lib.policy(batch_slices=1):
        before = plans()
        st = sc.IPForMLSumcheck.prover_init_batch(polys)
        run_rounds(st, descs, chal, name)
        tv = st.bind_final(v_msgs(chal[nv - 1]))
        for i in range(n):
            for u, t in enumerate(descs[i].tables):
                assert np.array_equal(tv[i, u], cref.fix_variables(t, chal[:, i])[0]), f"bind_final: instance {i}, table {u}"
        st.close()
        assert plans() == expect(before, name, nv)


def test_a_single_table_sinking_to_minus_fifteen_p():
    """[[0]] at nv = 16, n = 3: instance 0 sinking (entries at -k p after k binds: -15 p in the last round, through six sliced rounds and ten
    of k_batch_round), instance 1 a selector whose slopes peak in the last sliced round, instance 2 random under instance 0's challenges"""
    nv = 16
    s0, r0 = fm.sinking_challenges(nv, 85000)
    s1, r1 = fm.sinking_challenges(nv, 85001)
    tabs = [[sinking(nv, s0, 0)], [selector(nv, s1, nv - NV_MAX["single"], 0, False)], [cref.synth_table(85002, 0, 1 << nv)]]
    range_end_rounds("single", nv, tabs, np.stack([H.mont_challenges(r0), H.mont_challenges(r1), H.mont_challenges(r0)], axis=1))


def test_selector_slopes_peak_in_the_last_sliced_and_the_first_one_block_round():
    """c2 at nv = 12: round sel + 1 of a selector has every slope at +-(sel + 1) p.  sel = nv - nv_max = 3 is the last sliced round, sel + 1 the
    first round of k_batch_round on the tables the slices stored; both orientations in one product"""
    nv, sel = 12, 12 - NV_MAX["c2"]
    s0, r0 = fm.sinking_challenges(nv, 86000)
    s1, r1 = fm.sinking_challenges(nv, 86001)
    tabs = [[selector(nv, s0, sel, 0, False), selector(nv, s0, sel + 1, 1, True), selector(nv, s0, sel, 2, True)],
            [selector(nv, s1, sel + 1, 0, True), selector(nv, s1, sel, 1, False), selector(nv, s1, sel + 1, 2, False)]]
    range_end_rounds("c2", nv, tabs, np.stack([H.mont_challenges(r0), H.mont_challenges(r1)], axis=1))


def test_every_factor_of_a_product_of_eight_a_selector_at_the_deepest_bind():
    """EIGHT at nv = 16, n = 2, every table a selector at sel = 15: the last round's pair is (entry at -15 p, p - 1) in every factor at once,
    instance 0 all up, instance 1 all down -- every factor of an eight-fold product at the deepest bind the exact model admits, lines at 67 p
    (tests/test_fe_model_host.py: test_every_factor_a_selector_products_of_up_to_eight_stay_inside_every_box, k = 15)"""
    nv, sel = 16, 15
    s0, r0 = fm.sinking_challenges(nv, 87000)
    s1, r1 = fm.sinking_challenges(nv, 87001)
    tabs = [[selector(nv, s0, sel, t, False) for t in range(8)], [selector(nv, s1, sel, t, True) for t in range(8)]]
    range_end_rounds("eight", nv, tabs, np.stack([H.mont_challenges(r0), H.mont_challenges(r1)], axis=1))


@pytest.mark.parametrize("name", ["gkr", "single"])
@pytest.mark.parametrize("entry", [P - 1, 1, (P - 1) * fm.R256 % P], ids=["p-1", "one", "field-minus-one"])
def test_lazy_sums_at_the_bound(name, entry):
    """every entry at one value and every challenge p - 1, nv = 12, n = 2: every block's partial and every sum of partials sits at its extreme
    (a constant table's slopes are 0, so the entries stay what they were: this pins the sums, the range ends are the tests above)"""
    n, nv, shapes = 2, 12, SHAPES[name]
    nt = max(max(s) for s in shapes) + 1
    polys, descs = [], []
    for i in range(n):
        tabs = [np.tile(raw(entry), (1 << nv, 1)) for _ in range(nt)]
        coefs = cref.synth_table(88000 + i, 1000, len(shapes))
        descs.append(H.desc_from(nv, shapes, tabs, coefs))
        polys.append(H.hip_poly_from(nv, shapes, tabs, coefs, device=DEV)[0])
    torch.cuda.synchronize()
    with _lib.policy(batch_slices=1):
        before = plans()
        st = sc.IPForMLSumcheck.prover_init_batch(polys)
        run_rounds(st, descs, np.tile(raw(P - 1), (nv, n, 1)), name)
        st.close()
        assert plans() == expect(before, name, nv)


# ---- the handle's life cycle --------------------------------------------------------------------------------------------------------------
def test_reset_with_the_same_and_with_new_tables_and_two_handles_in_turn():
    n, nv = 3, 10
    polys_a, descs_a = make_batch(n, nv, SQUARED, 89000)
    polys_b, descs_b = make_batch(n, nv, SQUARED, 89100)
    with _lib.policy(batch_slices=1):
        before = plans()
        st = sc.IPForMLSumcheck.prover_init_batch(polys_a)
        run_rounds(st, descs_a, challenges(n, nv, 89001), "squared")
        st.reset()  # the same tables, other challenges: round 0's slots were never overwritten
        assert st.round == 0 and st.randomness(0).shape == (0, 4)
        run_rounds(st, descs_a, challenges(n, nv, 89002), "squared")
        st.reset(polys_b)  # new tables and coefficients
        run_rounds(st, descs_b, challenges(n, nv, 89003), "squared")
        st2 = sc.IPForMLSumcheck.prover_init_batch(polys_a)
    # (the key is read when a handle is built: the rounds below run sliced without it)
    st.reset()
    o1, o2 = Oracle(descs_b), Oracle(descs_a)
    c1, c2 = challenges(n, nv, 89005), challenges(n, nv, 89006)
    for j in range(nv):  # two sliced handles advanced alternately, round by round
        for s, o, c in ((st, o1, c1), (st2, o2, c2)):
            cj = None if j == 0 else c[j - 1]
            got = np.stack([m.evaluations for m in sc.IPForMLSumcheck.prove_round_batch(s, None if j == 0 else v_msgs(cj))])
            assert np.array_equal(got, o.round(cj)), f"round {j + 1}"
    assert_state(st, o1, n - 1, "first handle")
    assert_state(st2, o2, 0, "second handle")
    st.close()
    st2.close()
    assert plans() == expect(before, "squared", nv, times=5)


def test_bind_final_gives_the_table_values_at_the_point():
    n, nv = 3, 11
    polys, descs = make_batch(n, nv, TWO, 90000)
    chal = challenges(n, nv, 90001)
    with _lib.policy(batch_slices=1):
        st = sc.IPForMLSumcheck.prover_init_batch(polys)
    run_rounds(st, descs, chal, "two", check_state=False)
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
    st.close()


def test_host_tables_and_device_tables_give_identical_output():
    n, nv = 2, 9
    out = []
    for device in (DEV, None):
        polys, descs = make_batch(n, nv, C3, 91000, device=device)
        with _lib.policy(batch_slices=1):
            before = plans()
            st = sc.IPForMLSumcheck.prover_init_batch(polys)
            msgs, _ = run_rounds(st, descs, challenges(n, nv, 91001), "c3")
            out.append(msgs)
            if device is None:  # a handle built over host tables takes either kind on reset
                polys_d, _ = make_batch(n, nv, C3, 91000, device=DEV)
                st.reset(polys_d)
                again, _ = run_rounds(st, descs, challenges(n, nv, 91001), "c3", check_state=False)
                assert np.array_equal(again, msgs)
            st.close()
            assert plans() == expect(before, "c3", nv, times=1 if device else 2)
    assert np.array_equal(out[0], out[1])


def test_a_bad_challenge_at_a_sliced_round_leaves_the_handle_where_it_was():
    n, nv = 5, 10
    polys, descs = make_batch(n, nv, C2, 92000)
    chal = challenges(n, nv, 92001)
    orc = Oracle(descs)
    with _lib.policy(batch_slices=1):
        before = plans()
        st = sc.IPForMLSumcheck.prover_init_batch(polys)

    def ok(cj):
        got = np.stack([m.evaluations for m in sc.IPForMLSumcheck.prove_round_batch(st, None if cj is None else v_msgs(cj))])
        assert np.array_equal(got, orc.round(cj))

    with pytest.raises(sc.SumcheckError) as e:  # a challenge on the first call
        sc.IPForMLSumcheck.prove_round_batch(st, v_msgs(chal[0]))
    assert e.value.code == _lib.SC_ERR_FIRST_ROUND_HAS_MSG and st.round == 0
    ok(None)
    with pytest.raises(sc.SumcheckError) as e:  # NULL on a later call
        sc.IPForMLSumcheck.prove_round_batch(st, None)
    assert e.value.code == _lib.SC_ERR_MISSING_MSG and st.round == 1
    bad = chal[0].copy()
    bad[3] = raw(P - 1) + np.array([1, 0, 0, 0], dtype=np.uint64)  # p itself, for instance 3 of 5, at round 1: a sliced round
    with pytest.raises(sc.SumcheckError) as e:
        sc.IPForMLSumcheck.prove_round_batch(st, v_msgs(bad))
    assert e.value.code == _lib.SC_ERR_BAD_ARG and e.value.msg.startswith("instance 3: challenge is not canonical"), e.value.msg
    assert st.round == 1 and st.randomness(0).shape == (0, 4)
    assert plans() == (before[0] + 1, before[1], before[2]), "the refused call launched nothing"
    for j in range(1, nv):
        ok(chal[j - 1])
    assert_state(st, orc, 3, "after the misuse")
    with pytest.raises(sc.SumcheckError) as e:  # a call after the last round
        sc.IPForMLSumcheck.prove_round_batch(st, v_msgs(chal[nv - 1]))
    assert e.value.code == _lib.SC_ERR_NOT_ACTIVE and st.round == nv
    st.close()
    assert plans() == expect(before, "c2", nv)


def test_the_default_policy_and_batch_zero_keep_the_serial_plan():
    """without the key c2 at nv = 10 counts batch.rounds_serial only, and so it does with batch_slices = 1 under batch = 0"""
    n, nv = 2, 10
    polys, descs = make_batch(n, nv, C2, 93000)
    chal = challenges(n, nv, 93001)
    assert _lib.get_policy("batch") != 0
    for pol in ({}, {"batch_slices": 1, "batch": 0}):
        with _lib.policy(**pol):
            p0 = _lib.plan_stats()
            st = sc.IPForMLSumcheck.prover_init_batch(polys)
            orc = Oracle(descs)
            for j in range(nv):
                cj = None if j == 0 else chal[j - 1]
                got = np.stack([m.evaluations for m in sc.IPForMLSumcheck.prove_round_batch(st, None if j == 0 else v_msgs(cj))])
                assert np.array_equal(got, orc.round(cj)), f"round {j + 1}"
            st.close()
            p1 = _lib.plan_stats()
        assert p1["batch.rounds_serial"] == p0["batch.rounds_serial"] + nv and p1["batch.rounds_one_block"] == p0["batch.rounds_one_block"]
        assert p1.get("batch.rounds_slices", 0) == p0.get("batch.rounds_slices", 0)
