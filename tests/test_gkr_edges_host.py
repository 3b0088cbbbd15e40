"""Without a GPU: the inputs of tests/test_gpu_gkr_edges.py are what they claim to be, and the C oracle those tests compare with agrees with
the big-integer oracle (oracle/pyoracle.py) at the values they rely on -- g, u, f2, f3 from {0, 1, p - 1}, zero-valued entries of f1(g, ., .),
repeated indices, 8192 terms of p - 1 in one cell."""
import numpy as np
import pytest

import sumcheck_amd as sc
from oracle import cref
from oracle import pyoracle as po
from sumcheck_amd import _lib
from tests import gkr_edge_cases as E
from tests import helpers as H
from tests.test_gpu_gkr_batch_rounds import EDGE, P, raw


def canonical(a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
    below = np.zeros(a.shape[0], dtype=bool)   # limb by limb from the top: strictly below p
    equal = np.ones(a.shape[0], dtype=bool)
    for k in (3, 2, 1, 0):
        pk = np.uint64((P >> (64 * k)) & 0xFFFFFFFFFFFFFFFF)
        below |= equal & (a[:, k] < pk)
        equal &= a[:, k] == pk
    return bool(below.all())


def test_the_direct_evaluation_has_a_plan_counter_next_to_the_list_forms():
    names = list(_lib.plan_stats())
    i = names.index("gkr.list_form")
    assert names[i + 1] == E.EQ_DIRECT and names[i + 2] == E.COEFF and len(names) == sc.lib().sc_plan_count()
    assert {E.GROUPED, E.COUNTED, E.LIST, E.EQ_DIRECT, E.COEFF} <= set(names)


def test_the_route_formulas_at_their_switches():
    assert not E.table_pays(127, 11) and E.table_pays(128, 11) and not E.table_pays(4096, 21)
    assert E.table_pays(1 << 17, 19) and E.table_pays(1 << 18, 21) and not E.table_pays(1 << 17, 21)
    assert E.geometry(11) == (0, 2048) and E.geometry(12) == (1, 2048) and E.geometry(21) == (10, 2048) and E.geometry(4) == (0, 16)
    assert E.cap(8192, 11) == 8192 and E.cap(300000, 12) == 9408 and E.cap(1 << 18, 21) == 8256
    assert (8 << 10) * 8 == 64 << 10  # dim 21: eight uint64 lanes of 1024 cells, the whole of a workgroup's 64 KiB


@pytest.mark.parametrize("name", E.NAMES)
def test_every_input_is_a_legal_one_and_holds_its_preconditions(name):
    c = E.build(name)  # (the builder asserts the facts its expected route rests on)
    assert c.idx.dtype == np.uint64 and int(c.idx.max()) >> (3 * c.dim) == 0
    assert all(canonical(a) for a in (c.vals, c.f2, c.f3, c.g, c.u))
    oi, ov = c.oracle_f1()
    assert np.array_equal(oi, np.unique(c.idx)) and canonical(ov)
    assert np.unique(oi >> np.uint64(c.dim)).shape[0] == c.n1
    assert c.expect["prove"][E.COEFF] == 1
    sparse = E.EQ_DIRECT in c.expect["phase_one"]
    assert sparse == (not E.table_pays(c.idx.shape[0], c.dim)), "the fold over g evaluates eq per entry exactly when 2^dim > 8 nnz + 1024"
    assert (E.EQ_DIRECT in c.expect["phase_two"]) == (not E.table_pays(c.n1, c.dim)), "... and the fold over u when 2^dim > 8 n1 + 1024"
    assert c.expect["prove"].get(E.EQ_DIRECT, 0) == sparse + (E.LIST in c.expect["prove"] and not E.table_pays(c.n1, c.dim))


@pytest.mark.parametrize("name", list(E.PHASE_TWO_CASES))
def test_the_phase_two_inputs_likewise(name):
    c = E.build(name)
    assert int(c.idx.max()) >> (2 * c.dim) == 0 and canonical(c.vals) and canonical(c.u)
    oi, ov = c.oracle_f1g()
    assert np.array_equal(oi, np.unique(c.idx)) and canonical(ov) and oi.shape[0] in (1, 3)


def test_the_named_ends_are_in_the_inputs():
    for name, dim in (("sparse-dim13-nnz64-shuffled", 13), ("sparse-dim17-nnz64", 17), ("sparse-dim21-nnz4096-shuffled", 21)):
        idx = E.build(name).idx
        assert int(idx.min()) == 0 and int(idx.max()) == (1 << (3 * dim)) - 1
    assert E.build("sparse-dim11-nnz1-top").idx.tolist() == [(1 << 33) - 1]
    c = E.build("one-cell-8192-extreme")
    assert np.array_equal(c.vals, np.tile(raw(P - 1), (8192, 1))) and np.unique(c.idx).shape[0] == 1
    z = int(c.idx[0]) & 2047
    assert cref.mont_to_ints(c.g) == [(z >> j) & 1 for j in range(11)] and set(cref.mont_to_ints(c.f3)) == {1}


# ---- the C oracle against big integers at these values -------------------------------------------------------------------------------------
def as_dict(idx, vals):
    return dict(zip((int(i) for i in idx), cref.mont_to_ints(vals)))


def check_oracles_agree(dim, idx, vals, f2, f3, g, u, prove=True):
    """cref on the list as given (repeated indices included) == pyoracle on the merged map"""
    mi, mv = H.merge_repeated(idx, vals)
    f1 = as_dict(mi, mv)
    I = cref.mont_to_ints
    ph, pf1g = po.initialize_phase_one(f1, 3 * dim, I(f3), I(g))
    wh, wi, wv = cref.gkr_phase_one(idx, vals, dim, f3, g)
    assert I(wh) == ph and [int(i) for i in wi] == sorted(pf1g) and I(wv) == [pf1g[k] for k in sorted(pf1g)], "initialize_phase_one"
    assert 0 in I(wv) or not prove, "a zero-valued entry of f1(g, ., .) is kept"
    assert I(cref.gkr_phase_two(wi, wv, dim, u)) == po.initialize_phase_two(pf1g, dim, I(u)), "initialize_phase_two"
    if prove:
        want, wuv = cref.gkr_prove(idx, vals, dim, f2, f3, g)
        m1, m2, pu, pv = po.gkr_prove(po.Blake2b512Rng(), f1, I(f2), I(f3), I(g))
        assert [I(m) for m in want[0]] == m1 and [I(m) for m in want[1]] == m2 and I(wuv[0]) == pu and I(wuv[1]) == pv, "gkr_prove"


@pytest.mark.parametrize("dim", [3, 4])
@pytest.mark.parametrize("mixed", [False, True], ids=["boolean", "mixed"])
def test_c_oracle_equals_big_integers_on_points_and_tables_from_the_ends(dim, mixed):
    c = E.edge_values_case(dim, mixed, False, shuffled=True)
    rep = np.concatenate([c.idx, c.idx[:7], c.idx[:3]])  # ... and with repeated indices
    vals = np.concatenate([c.vals, c.vals[7:14], np.tile(EDGE[2], (3, 1))])
    check_oracles_agree(dim, c.idx, c.vals, c.f2, c.f3, c.g, c.u)
    check_oracles_agree(dim, rep, vals, c.f2, c.f3, c.g, c.u)


@pytest.mark.parametrize("count", [8192, 8193])
def test_c_oracle_equals_big_integers_on_one_cell_of_p_minus_one(count):
    c = E.one_cell_case(count, True, True)
    check_oracles_agree(c.dim, c.idx, c.vals, c.f2, c.f3, c.g, c.u, prove=False)
    total = cref.mont_to_ints(raw(P - 1).reshape(1, 4))[0] * count % P
    wh, wi, wv = cref.gkr_phase_one(c.idx, c.vals, c.dim, c.f3, c.g)
    x0, y0 = (int(c.idx[1]) >> 11) & 2047, int(c.idx[1]) >> 22
    assert cref.mont_to_ints(wh[x0:x0 + 1]) == [total] and cref.mont_to_ints(wv[wi == np.uint64(x0 | (y0 << 11))]) == [total]
    p2 = E.full_cell_phase_two(count, True)
    oi, ov = p2.oracle_f1g()
    assert cref.mont_to_ints(cref.gkr_phase_two(p2.idx, p2.vals, 11, p2.u)) == po.initialize_phase_two(as_dict(oi, ov), 11, cref.mont_to_ints(p2.u))
