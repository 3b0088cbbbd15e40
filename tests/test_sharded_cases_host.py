"""Without a GPU: what tests/test_gpu_sharded_edges.py leans on.

  * tests/sharded_cases.py restates sharded_tail_m (protocol.hip) with the constants as the sources have them; here the restated rule meets a
    table written out by hand: every case of the GPU file and the five shapes of tests/test_gpu_sharded.py's whole-proof tests;
  * every case lies on the side of its edge that it claims (its `why`);
  * the C oracle (oracle/oracle.c through cref.ml_prove) against the big-integer oracle (oracle/pyoracle.py) on every case of nv <= 8, and on
    the extreme-value inputs of F: neither oracle alone carries a mistake into the GPU tests;
  * F's inputs are what they are meant to be: every rank's round-1 message at node 0 is p - 1 (none from the all-zero shard)."""
import os

import numpy as np
import pytest

from oracle import cref
from oracle import pyoracle as po
from tests import sharded_cases as SC

I = cref.mont_to_ints


def test_the_constants_are_the_sources():
    assert (SC.GLOG_DEFAULT, SC.GLOG_MIN, SC.GLOG_MAX) == (15, 1, 15)
    assert (SC.TAIL_CLAMP_LO, SC.TAIL_CLAMP_HI) == (SC.GLOG_MIN, SC.GLOG_MAX), "sharded_tail_m clamps to the range sc_set_policy accepts"
    assert (SC.K_SMALL_ROUND_PAIRS, SC.K_P2P_MAX_RANKS, SC.K_P2P_WORDS) == (1 << 14, 16, 64)
    assert (SC.STREAMED_LOCAL_ROUNDS, SC.STREAM_MIN_NV) == (2, 11)


# (G, nv_local, glog, streamed) -> (nl, m), by hand
BY_HAND = [
    # A
    ((2, 16, 15, False), (2, 14)), ((2, 16, 1, False), (16, 0)), ((2, 16, 10, False), (7, 9)), ((2, 16, 14, False), (3, 13)), ((2, 16, 2, False), (15, 1)),
    # B
    ((8, 6, 2, False), (6, 0)), ((8, 6, 3, False), (6, 0)), ((8, 6, 4, False), (5, 1)),
    # C
    ((2, 1, 15, False), (1, 0)), ((8, 1, 15, False), (1, 0)), ((16, 1, 15, False), (1, 0)), ((4, 2, 15, False), (1, 1)), ((4, 2, 1, False), (2, 0)),
    # D, and the same shards resident
    ((2, 11, 15, True), (2, 9)), ((2, 11, 3, True), (9, 2)), ((2, 11, 15, False), (1, 10)), ((2, 11, 3, False), (9, 2)),
    # E, F
    ((16, 4, 15, False), (1, 3)), ((16, 4, 1, False), (4, 0)), ((4, 6, 1, False), (6, 0)),
    # G
    ((2, 18, 15, False), (4, 14)), ((2, 18, 12, False), (7, 11)),
    # H (each phase: dim = 9 over 4 ranks)
    ((4, 7, 2, False), (7, 0)), ((4, 7, 15, False), (1, 6)),
    # the whole-proof tests of tests/test_gpu_sharded.py: (G, nv) = (2, 13), (4, 19), (2, 20), (8, 6), (8, 12); the streamed ones (2, 14), (4, 15)
    ((2, 12, 15, False), (1, 11)), ((4, 17, 15, False), (4, 13)), ((2, 19, 15, False), (5, 14)), ((8, 3, 15, False), (1, 2)), ((8, 9, 15, False), (1, 8)),
    ((2, 13, 15, True), (2, 11)), ((4, 13, 15, True), (2, 11)),
    # one rank: no tail at all; a streamed shard of one variable keeps its one round
    ((1, 18, 15, False), (18, 0)), ((1, 18, 1, False), (18, 0)), ((2, 1, 15, True), (1, 0)),
]


def test_the_restated_rule_against_a_table_written_by_hand():
    for args, want in BY_HAND:
        assert SC.cut(*args) == want, args
    by_hand = {a: w for a, w in BY_HAND}
    for name in list(SC.CASES) + list(SC.GKR):
        f = SC.case_facts(name)
        streamed = name in SC.CASES and SC.CASES[name].chunk is not None
        assert by_hand[(f["G"], f["nv_local"], f["glog"], streamed)] == (f["nl"], f["m"]), f"{name} is not in the table"
    for (G, nv), want in SC.EXISTING.items():
        assert SC.cut(G, nv - SC.log2(G), SC.GLOG_DEFAULT) == want == by_hand[(G, nv - SC.log2(G), 15, False)], (G, nv)
    # out-of-range policies cannot be set; the rule clamps them all the same
    assert SC.cut(2, 16, 0) == SC.cut(2, 16, 1) and SC.cut(2, 16, 99) == SC.cut(2, 16, 15)


@pytest.mark.parametrize("name", list(SC.CASES) + list(SC.GKR))
def test_every_case_rests_on_the_inequality_it_states(name):
    f = SC.case_facts(name)
    why = SC.GKR_WHY[name] if name in SC.GKR else SC.CASES[name].why
    assert eval(why, {"__builtins__": {}}, dict(f)) is True, (why, f)  # noqa: S307 (the expressions are this repository's own)
    assert f["nl"] + f["tail"] == f["nv"] and f["nl"] >= 1 and f["words"] == 8 * f["D"]
    if name in SC.P2P:
        assert f["words"] <= SC.K_P2P_WORDS, "a peer-to-peer inbox slot holds the message"
    assert f["gather_bytes"] == (f["U"] * 32) << f["m"]
    if name in SC.CASES:
        c = SC.CASES[name]
        seen = [t for sh in c.shapes for t in sh]
        assert sorted(set(seen), key=seen.index) == list(range(SC.n_tables(c.shapes))), "tables named in first-occurrence order: the oracle's descriptor is the wrapper's"
        assert 1 <= c.glog <= 15 and f["G"] <= SC.K_P2P_MAX_RANKS
        if c.chunk is not None:
            assert f["nv_local"] >= SC.STREAM_MIN_NV and c.chunk <= f["nv_local"], "the shard really streams"


def test_the_case_table_covers_what_the_issue_lists():
    F = {n: SC.case_facts(n) for n in list(SC.CASES) + list(SC.GKR)}
    assert [(F[n]["m"], F[n]["nl"]) for n in SC.LADDER_ORDER] == [(14, 2), (0, 16), (9, 7), (13, 3), (1, 15), (14, 2)]
    assert all(F[a]["m"] != F[b]["m"] for a, b in zip(SC.LADDER_ORDER, SC.LADDER_ORDER[1:])), "every step of the ladder rebuilds the tail prover"
    assert [F[n]["m"] for n in ("B-2", "B-3", "B-4")] == [0, 0, 1]
    assert any(f["m"] == 0 and f["k"] >= f["glog"] for f in F.values()) and any(f["nv_local"] == 1 for f in F.values())
    assert F["E-seven"]["words"] == SC.K_P2P_WORDS and F["E-seven"]["nl"] == 6
    assert {F[n]["G"] for n in SC.F_NAMES} == {SC.K_P2P_MAX_RANKS} and len(SC.F_NAMES) == 8
    assert set(SC.P2P) <= set(SC.CASES), "every peer-to-peer case has a host-transport twin that counts its exchanges"
    assert 0 <= SC.HOLE_RANK < 16


# ---- the two oracles against each other ------------------------------------------------------------------------------------------------------
SMALL_CASES = [n for n, c in SC.CASES.items() if c.nv <= 8]


def test_the_small_cases_are_the_ones_meant():
    assert set(SC.F_NAMES) <= set(SMALL_CASES) and {"C-2x1", "C-8x1", "C-16x1", "C-4x2-15", "C-4x2-1", "E-16-15", "E-16-1", "E-seven"} <= set(SMALL_CASES)


@pytest.mark.parametrize("name", SMALL_CASES)
def test_c_oracle_equals_big_integers_on_every_small_case(name):
    c = SC.CASES[name]
    tabs, coefs = SC.inputs(name)
    got, grand = SC.oracle_proof(c.nv, c.shapes, tabs, coefs)
    itabs = [I(t) for t in tabs]
    poly = po.ListOfProductsOfPolynomials(c.nv)
    for k, sh in enumerate(c.shapes):
        poly.add_product([itabs[t] for t in sh], I(coefs[k].reshape(1, 4))[0])
    msgs, st = po.ml_prove_as_subprotocol(po.Blake2b512Rng(), poly)
    assert [I(got[j]) for j in range(c.nv)] == msgs
    assert I(grand) == st.randomness


def _stored(row):
    return sum(int(row[k]) << (64 * k) for k in range(4))


@pytest.mark.parametrize("name", SC.F_NAMES)
def test_extreme_inputs_are_what_they_claim(name):
    """per rank: the shard's own round-1 message (its contribution to the first all-reduce), from the big-integer oracle"""
    c = SC.CASES[name]
    (tab,), coefs = SC.inputs(name)
    assert I(coefs) == [1]
    n_loc = (1 << c.nv) // c.G
    if c.tables == "drawn":
        assert {_stored(r) for r in tab} == {0, 1, SC.P - 1}
        return
    raw = c.tables.startswith("raw")
    for g in range(c.G):
        shard = tab[g * n_loc:(g + 1) * n_loc]
        hole = c.tables.endswith("hole") and g == SC.HOLE_RANK
        assert [_stored(r) for r in shard[1:]] == [0] * (n_loc - 1)
        assert _stored(shard[0]) == (0 if hole else SC.P - 1 if raw else _stored(cref.ints_to_mont([SC.P - 1])[0]))
        poly = po.ListOfProductsOfPolynomials(c.nv - SC.log2(c.G))
        ishard = I(shard)
        poly.add_product([ishard] * len(c.shapes[0]), 1)
        msg = po.prove_round(po.prover_init(poly), None)
        if hole:
            assert msg == [0] * len(msg)
        elif not raw:
            assert msg[0] == SC.P - 1 and msg[1] == 0, "the element p - 1: (p - 1)^3 = p - 1"
        elif c.shapes == SC.ONE:
            assert _stored(cref.ints_to_mont([msg[0]])[0]) == SC.P - 1 and msg[1] == 0, "the rank's lanes at node 0 are the limbs of p - 1"
    if c.tables.endswith("hole"):
        assert not tab[SC.HOLE_RANK * n_loc:(SC.HOLE_RANK + 1) * n_loc].any()


# ---- the policy's range ------------------------------------------------------------------------------------------------------------------------
def test_shard_gather_log2_refuses_0_and_16_and_accepts_1_and_15():
    """sc_set_policy touches no device: checked wherever the library loads (where it does not, tests/test_gpu_sharded_edges.py checks the same)"""
    from sumcheck_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        pytest.fail(f"{_lib.SO_PATH} is missing: the suite runs on a built tree")
    L = _lib.lib()
    old = _lib.get_policy("shard_gather_log2")
    try:
        assert old == SC.GLOG_DEFAULT, "no test leaves the policy moved"
        for bad in (SC.GLOG_MIN - 1, SC.GLOG_MAX + 1):
            assert L.sc_set_policy(b"shard_gather_log2", bad) == _lib.SC_ERR_BAD_ARG
            assert f"{SC.GLOG_MIN}..{SC.GLOG_MAX}" in L.sc_last_error().decode()
            assert _lib.get_policy("shard_gather_log2") == old
        for good in (SC.GLOG_MIN, SC.GLOG_MAX):
            assert L.sc_set_policy(b"shard_gather_log2", good) == 0 and _lib.get_policy("shard_gather_log2") == good
    finally:
        _lib.set_policy("shard_gather_log2", old)
