"""Lagging single-table products (sumcheck_amd/csrc/lag_index.hpp, policy "lag_single").  A table that only products of ONE multiplicand
name skips the big rounds 2 .. j - 1: round 1 leaves its class sums behind, its products' rows bind the class table, and k_fix_deep binds
the table with every challenge it missed in front of round j -- or earlier, when anything else reads the handle's tables
(materialize_lagging).  Every message and the final randomness are compared bit for bit with the oracle (cref.ml_prove / cref.Prover), the
bound tables with its .state(); the plan counters say which path ran.

Sizes: a round is big above 2^14 pairs, so nv = 18 .. 21 have 3 .. 6 big rounds: the catch-up round j = min(lag_single + 2, last big round)
is round 3, 4, 5 (the last big round) and 5 (not the last).  Shapes whose latency-bound tail takes over from 2^15 or 2^16 pairs reach the
tail before round j at some of these sizes: the tail's launch then catches the table up (big.lag_materialize instead of big.lag_catch_up)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib, sharded
from tests import fe_model as fm
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VM = sc.VerifierMsg
C3 = [[0, 1, 2, 3], [4, 5, 6], [7, 8], [9]]
SHAPES = {"pair-single": [[0, 1], [2]], "config3": C3, "two-singles": [[0], [1]], "single": [[0]], "two-coefficients": [[0, 1], [2], [2]]}
N_LAG = {"pair-single": 1, "config3": 1, "two-singles": 2, "single": 1, "two-coefficients": 1}  # lagging TABLES
INELIGIBLE = {"shared": [[0, 1], [1]], "square": [[0, 0]]}
LAG = ("big.lag_class_round", "big.lag_catch_up", "big.lag_materialize")


@pytest.fixture(autouse=True)
def three_skipped_rounds():
    """the sizes below are chosen for lag_single = 3 (catch-up before round 5 where five big rounds exist); the library's default is
    exercised by every other big-round test of the suite, and test_every_lag_single_value_gives_the_same_proof walks 0 .. 4"""
    with _lib.policy(lag_single=3):
        yield


def n_tables(shapes):
    return max(max(sh) for sh in shapes) + 1


@functools.lru_cache(maxsize=None)
def case(nv, name):
    """tables, coefficients and the oracle's proof and randomness, computed once per (size, shape)"""
    shapes = {**SHAPES, **INELIGIBLE}[name]
    tabs, coefs = H.random_case(None, nv, shapes, n_tables(shapes), 0x1A6 + nv)
    proof, rand = cref.ml_prove(H.desc_from(nv, shapes, tabs, coefs), threads=cref.max_threads())
    return shapes, tabs, coefs, proof, rand


def moved_since(before):
    after = _lib.plan_stats()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def catch_up_round(nv, skip=3):
    return min(skip + 2, nv - 15)


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("nv", [18, 19, 20, 21])
def test_proofs_with_a_lagging_table_equal_the_oracles(nv, name):
    """borrowed tables: a proof, state.reset(), the same proof again on the handle; then the same on a copying handle (reset with the tables)"""
    shapes, tabs, coefs, want, want_rand = case(nv, name)
    poly, _ = H.hip_poly_from(nv, shapes, tabs, coefs, device=DEV)
    torch.cuda.synchronize()
    before = _lib.plan_stats()
    proofs = 0
    for borrow in (True, False):
        st = sc.IPForMLSumcheck.prover_init(poly, borrow=borrow)
        for again in range(2):
            if again and borrow:
                st.reset()
            elif again:  # a copying handle takes its tables again
                ptrs = (C.c_void_p * len(poly.flattened_ml_extensions))(*[m.data_ptr() for m in poly.flattened_ml_extensions])
                _lib.check(sc.lib().sc_prover_reset(st._h, ptrs, _lib.SC_TABLES_ON_DEVICE))
            got = st.prove()
            proofs += 1
            assert np.array_equal(got, want), f"borrow={borrow}, proof {again + 1}: messages differ from the oracle's"
            assert np.array_equal(st.randomness[:nv - 1], want_rand[:nv - 1]), "randomness differs from the oracle's"
        st.close()
    moved = moved_since(before)
    print(f"\nnv {nv} {name}: plans {moved}")
    j = catch_up_round(nv)
    cls, fix = moved.get(LAG[0], 0), moved.get(LAG[1], 0) + moved.get(LAG[2], 0)
    # Rounds 2 .. j - 1 are class rounds -- unless the tail has taken over by then: lists of single-table products alone enter k_tail_slices
    # at 2^16 pairs, round nv - 16, so their class rounds are 2 .. min(j, nv - 16) - 1 and the tail's launch catches the tables up.  (At
    # nv = 18 that leaves none: the table "lags" by zero challenges and nothing is counted; the interactive test below pins these shapes.)
    per_proof = max((min(j, nv - 16) if name in ("single", "two-singles") else j) - 2, 0)
    assert cls == per_proof * proofs, f"class rounds: {cls}"
    assert fix == (N_LAG[name] * proofs if per_proof else 0), "every lagging table is caught up exactly once per proof"


@pytest.mark.parametrize("name", ["single", "two-singles"])
def test_lists_of_single_table_products_reach_the_catch_up_round(name):
    """[[0]] and [[0], [1]] at nv = 21 through sc_prove_round with the resident kernel off, so that every round is a launch of its own: rounds
    2 .. 4 have class rows ONLY, and round 5 follows k_fix_deep with every slot of the launch reading in place -- a binding round without a
    single binding slot (RoundArgs::binding).  The tables after round 5 are the oracle's."""
    nv = 21
    shapes, tabs, coefs, _, _ = case(nv, name)
    chal = cref.synth_table(0x1A7, 9, nv)
    want, otabs = oracle_rounds(nv, shapes, tabs, coefs, chal, 5)
    poly, _ = H.hip_poly_from(nv, shapes, tabs, coefs, device=DEV)
    torch.cuda.synchronize()
    before = _lib.plan_stats()
    with _lib.policy(resident=0):
        st = sc.IPForMLSumcheck.prover_init(poly)
        for j in range(nv):
            got = sc.IPForMLSumcheck.prove_round(st, None if j == 0 else VM(chal[j - 1])).evaluations
            assert np.array_equal(got, want[j]), f"round {j + 1}"
            if j + 1 == 5:
                for u, t in enumerate(st.flattened_ml_extensions):
                    assert np.array_equal(t.evaluations, otabs[u]), f"table {u} after round 5"
        st.close()
    moved = moved_since(before)
    assert moved.get(LAG[0], 0) == 3 and moved.get(LAG[1], 0) == N_LAG[name] and moved.get(LAG[2], 0) == 0, moved


@pytest.mark.parametrize("name", list(INELIGIBLE))
def test_a_table_that_a_longer_product_names_does_not_lag(name):
    nv = 20
    shapes, tabs, coefs, want, _ = case(nv, name)
    poly, _ = H.hip_poly_from(nv, shapes, tabs, coefs, device=DEV)
    torch.cuda.synchronize()
    before = _lib.plan_stats()
    st = sc.IPForMLSumcheck.prover_init(poly, borrow=True)
    got = st.prove()
    st.close()
    moved = moved_since(before)
    assert np.array_equal(got, want)
    assert not any(moved.get(k, 0) for k in LAG), moved


def test_every_lag_single_value_gives_the_same_proof():
    """nv = 21, six big rounds: lag_single = v skips v rounds (catch-up before round v + 2); 0 switches lagging off"""
    nv, name = 21, "pair-single"
    shapes, tabs, coefs, want, _ = case(nv, name)
    poly, _ = H.hip_poly_from(nv, shapes, tabs, coefs, device=DEV)
    torch.cuda.synchronize()
    st = sc.IPForMLSumcheck.prover_init(poly, borrow=True)
    for v in (0, 1, 2, 3, 4):
        with _lib.policy(lag_single=v):
            before = _lib.plan_stats()
            st.reset()
            got = st.prove()
            moved = moved_since(before)
        assert np.array_equal(got, want), f"lag_single = {v}"
        assert moved.get(LAG[0], 0) == v and moved.get(LAG[1], 0) + moved.get(LAG[2], 0) == (1 if v else 0), (v, moved)
    st.close()


def oracle_rounds(nv, shapes, tabs, coefs, chal, export_after):
    """every message of the oracle's prover under the given challenges, and its tables after round `export_after`"""
    op = cref.Prover(H.desc_from(nv, shapes, tabs, coefs), threads=cref.max_threads())
    want, otabs = [], None
    for j in range(nv):
        want.append(op.prove_round(None if j == 0 else chal[j - 1]))
        if j + 1 == export_after:
            otabs = op.state()[1]
    op.close()
    return want, otabs


def test_interactive_rounds_export_the_bound_tables_mid_lag():
    """sc_prove_round on config 3's shape at nv = 20 (catch-up before round 5): the tables exported after round 3, a skipped round, are the
    bound ones (materialize_lagging, two challenges behind), and the rounds go on to the end"""
    nv, name = 20, "config3"
    shapes, tabs, coefs, _, _ = case(nv, name)
    chal = cref.synth_table(0x1A7, 7, nv)
    want, otabs = oracle_rounds(nv, shapes, tabs, coefs, chal, 3)
    poly, _ = H.hip_poly_from(nv, shapes, tabs, coefs, device=DEV)
    torch.cuda.synchronize()
    before = _lib.plan_stats()
    st = sc.IPForMLSumcheck.prover_init(poly)
    for j in range(nv):
        got = sc.IPForMLSumcheck.prove_round(st, None if j == 0 else VM(chal[j - 1])).evaluations
        assert np.array_equal(got, want[j]), f"round {j + 1}"
        if j + 1 == 3:
            for u, t in enumerate(st.flattened_ml_extensions):
                assert np.array_equal(t.evaluations, otabs[u]), f"table {u} after round 3"
    st.close()
    moved = moved_since(before)
    assert moved.get(LAG[0], 0) == 2 and moved.get(LAG[2], 0) == 1 and moved.get(LAG[1], 0) == 0, moved


def test_partial_rounds_take_over_mid_lag():
    """the same handle driven through sc_prove_round for rounds 1 .. 3 and through sc_prove_round_partial (a sharded round's lanes) from
    round 4 on: the partial round catches the table up first"""
    nv, name = 20, "config3"
    shapes, tabs, coefs, _, _ = case(nv, name)
    chal = cref.synth_table(0x1A7, 8, nv)
    want, _ = oracle_rounds(nv, shapes, tabs, coefs, chal, 0)
    before = _lib.plan_stats()
    eng = sharded.HipShardEngine(nv, shapes, coefs, tabs, DEV, borrow=True)
    for j in range(nv):
        r = None if j == 0 else chal[j - 1]
        got = eng.round_full(r) if j < 3 else sharded.wide_reduce(eng.round_partial(r).cpu().numpy().view(np.uint64))
        assert np.array_equal(got, want[j]), f"round {j + 1}"
    moved = moved_since(before)
    del eng
    assert moved.get(LAG[0], 0) == 2 and moved.get(LAG[2], 0) == 1 and moved.get(LAG[1], 0) == 0, moved


def range_end_tables(nv, s, kind):
    m, c = 3, 3 * sum(s) + 2
    if kind == "sinking":
        tab = H.sinking_table_limbs(nv, s, m, c)
        H.assert_entries_match(tab, H.sinking_entry(s, m, c))
    else:
        tab = H.selector_table_limbs(nv, s, 3, m, c, kind == "selector-flipped")
        H.assert_entries_match(tab, H.selector_entry(s, 3, m, c, kind == "selector-flipped"))
    return tab


@pytest.mark.parametrize("chal_kind", ["sinking", "0-1-p-1"])
@pytest.mark.parametrize("kind", ["sinking", "selector", "selector-flipped"])
def test_range_end_tables_as_the_lagging_table(kind, chal_kind):
    """[[0, 1], [2]] at nv = 20, table 2 -- the lagging one -- a sinking or a selector table (tests/test_gpu_lazy_entries.py) under the
    challenges chosen for it: every level of k_fix_deep settles entries at the ends of the lazily bound range exactly as the rounds would
    have.  A second run binds 0, 1 and p - 1 first.  Messages of every round, and every table after round 5 (the table caught up, four binds)"""
    nv, shapes = 20, [[0, 1], [2]]
    s, r = fm.sinking_challenges(nv, 0x1A8)
    if chal_kind == "0-1-p-1":
        r = [0, 1, fm.P - 1] + list(r[3:])
    chal = H.mont_challenges(r)
    tabs = [cref.synth_table(0x1A9, 0, 1 << nv), cref.synth_table(0x1A9, 1, 1 << nv), range_end_tables(nv, s, kind)]
    coefs = cref.synth_table(0x1A9, 1000, len(shapes))
    want, otabs = oracle_rounds(nv, shapes, tabs, coefs, chal, 5)
    poly, _ = H.hip_poly_from(nv, shapes, tabs, coefs, device=DEV)
    torch.cuda.synchronize()
    before = _lib.plan_stats()
    with _lib.policy(resident=0):  # (every round a launch of its own: round 5 is the catch-up round, not the resident tail's first)
        st = sc.IPForMLSumcheck.prover_init(poly)
        for j in range(nv):
            got = sc.IPForMLSumcheck.prove_round(st, None if j == 0 else VM(chal[j - 1])).evaluations
            assert np.array_equal(got, want[j]), f"round {j + 1}"
            if j + 1 == 5:
                for u, t in enumerate(st.flattened_ml_extensions):
                    assert np.array_equal(t.evaluations, otabs[u]), f"table {u} after round 5"
        st.close()
    moved = moved_since(before)
    assert moved.get(LAG[0], 0) == 3 and moved.get(LAG[1], 0) == 1 and moved.get(LAG[2], 0) == 0, moved
