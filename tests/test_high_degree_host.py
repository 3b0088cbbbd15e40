"""Without a GPU: what tests/test_gpu_high_degree.py leans on.

  * the C oracle (oracle/oracle.c through cref) against the big-integer oracle (oracle/pyoracle.py) on products of 14 to 40 multiplicands and on
    a 33rd power -- whole Fiat-Shamir proofs, and both verifiers (and the library's host-side one) accepting them;
  * the shape builders of tests/high_degree_cases.py against the thresholds the GPU tests' expected plans rest on: sum of (M_k + 1) against
    kMetaCombos = 24, K D (D + 2) 32 bytes against 48 KiB, the table count against kMaxSmallTables = 32."""
import numpy as np
import pytest

import sumcheck_amd as sc
from oracle import cref
from oracle import pyoracle as po
from tests import helpers as H
from tests import high_degree_cases as HD

I = cref.mont_to_ints


@pytest.mark.parametrize("name", ["14", "24", "34", "40", "0^33"])
def test_c_oracle_equals_big_integers_on_long_products(name):
    nv = 3
    shapes, nt = HD.EXPONENT_SHAPES[name] if name in HD.EXPONENT_SHAPES else HD.one_product(int(name))
    tabs, coefs = HD.synth_case(nv, shapes, 0x4D0 + len(shapes[0]))
    d = H.desc_from(nv, shapes, tabs, coefs)
    assert d.max_multiplicands == HD.max_mult(shapes) and len(d.tables) == nt
    itabs = [I(t) for t in tabs]
    poly = po.ListOfProductsOfPolynomials(nv)
    for k, sh in enumerate(shapes):
        poly.add_product([itabs[i] for i in sh], I(coefs[k])[0])
    assert poly.info() == (d.max_multiplicands, nv)
    want_py = po.ml_prove(poly)
    proof, rand = cref.ml_prove(d, threads=2)
    assert [I(m) for m in proof] == want_py, "the C oracle's proof is not the big-integer oracle's"
    # both verifiers accept it, end on the same point and expect the polynomial's value there
    claim = po.extract_sum(want_py)
    point_py, exp_py = po.ml_verify(poly.info(), claim, want_py)
    ok, point, exp = cref.ml_verify((d.max_multiplicands, nv), cref.ints_to_mont([claim])[0], proof)
    assert ok and I(point) == point_py and I(exp.reshape(1, 4)) == [exp_py] and np.array_equal(point, rand)
    assert poly.evaluate(point_py) == exp_py and I(cref.poly_evaluate(d, point).reshape(1, 4)) == [exp_py]
    # ... and so does the library's host-side verifier, whose interpolation changes its arithmetic at 20 and at 33 points
    msgs = [sc.ProverMsg(m) for m in proof]
    sub = sc.MLSumcheck.verify(sc.PolynomialInfo(d.max_multiplicands, nv), sc.MLSumcheck.extract_sum(msgs), msgs)
    assert np.array_equal(sub.point, point) and np.array_equal(sub.expected_evaluation, exp)
    for j in range(nv):
        got = sc.interpolate_uni_poly(proof[j], rand[j])
        assert np.array_equal(got, cref.interpolate_uni_poly(proof[j], rand[j])) and I(got.reshape(1, 4)) == [po.interpolate_uni_poly(want_py[j], point_py[j])]


def test_the_ladder_crosses_every_threshold_by_degree_alone():
    """one product: K = 1, so only M moves the shape across has_meta (D <= 24) and across the finalize's 48 KiB (D (D + 2) 32)"""
    assert HD.K_META_COMBOS == 24 and HD.K_FIN_LDS_MAX == 49152 and HD.K_MAX_SMALL_TABLES == 32
    for M in HD.LADDER:
        shapes, nt = HD.one_product(M)
        assert len(shapes) == 1 and HD.max_mult(shapes) == M and HD.n_tables(shapes) == nt == min(M, 32) and HD.n_combos(shapes) == M + 1
        assert HD.n_slots(shapes) == nt <= HD.K_META_SLOTS, "has_meta is decided by the combinations alone"
        assert HD.has_meta(shapes) == (M <= 23) == HD.tail_shape_ok(shapes), "M + 1 <= 24; and below 24 the node sums fit LDS anyway"
        assert not HD.tail_slices_ok(shapes), "more than twelve multiplicands never take the slices"
        assert HD.small_plan(shapes) == ("small.launched" if M <= 23 else "small.combos_table")
        assert HD.finalize_plan(shapes) == ("finalize.multi_block" if M <= 37 else "finalize.no_lds")
    assert {23, 24} <= set(HD.LADDER) and {37, 38} <= set(HD.LADDER) and set(HD.PLAIN_LAUNCHES) == {23, 24, 37, 38}
    assert {19, 20} <= set(HD.LADDER) and {32, 33} <= set(HD.LADDER), "the verifier's tiers: 20 and 33 evaluation points are D = 20 and D = 33"
    # the two bounds themselves, at K = 1
    assert 24 * 26 * 32 == 19968 and 38 * 40 * 32 == 48640 <= 49152 < 39 * 41 * 32 == 51168
    assert HD.fin_lds_bytes(HD.one_product(37)[0]) == 48640 and HD.fin_lds_bytes(HD.one_product(38)[0]) == 51168
    assert HD.big_rounds(HD.LADDER_NV) == 0 and (1 << (HD.LADDER_NV - 1)) <= 2048, "nv = 11: every round is latency-bound, and within k_tail_rounds' 2048 pairs"


def test_the_big_round_shapes_are_generic_products_where_they_should_be():
    assert HD.big_rounds(HD.BIG_NV) == 2
    for name, (shapes, nt) in HD.BIG_SHAPES.items():
        assert HD.n_tables(shapes) == nt <= HD.K_MAX_SMALL_TABLES, name
        assert len(shapes[0]) > HD.K_MAX_WIDE_M, "the first product is beyond the trees: k_sum_generic"
    assert sorted(HD.BIG_SHAPES["24-over-16"][0][0].count(t) for t in range(16)) == [1] * 8 + [2] * 8
    assert sorted(HD.BIG_SHAPES["38-over-32"][0][0].count(t) for t in range(32)) == [1] * 26 + [2] * 6
    mixed = HD.BIG_SHAPES["mixed-D21"][0]
    assert [len(sh) for sh in mixed] == [20, 2, 1, 9] and HD.degree(mixed) == 21
    assert HD.K_MAX_FUSED_M < 9 <= HD.K_MAX_WIDE_M, "the ninth power is a wide16 product, the pair and the single are trees"
    assert HD.n_combos(mixed) == 36 > HD.K_META_COMBOS and HD.fin_lds_bytes(mixed) == 4 * 21 * 23 * 32 == 61824 > HD.K_FIN_LDS_MAX
    assert HD.finalize_plan(mixed) == "finalize.no_lds" and HD.finalize_plan(HD.BIG_SHAPES["14-distinct"][0]) == "finalize.multi_block"
    assert HD.finalize_plan(HD.BIG_SHAPES["38-over-32"][0]) == "finalize.no_lds" and HD.tail_shape_ok(HD.BIG_SHAPES["14-distinct"][0])


def test_the_exponent_and_many_table_shapes():
    for name, (shapes, nt) in HD.EXPONENT_SHAPES.items():
        assert HD.n_tables(shapes) == nt and HD.max_mult(shapes) == 33 and HD.n_slots(shapes) == nt and not HD.has_meta(shapes), name
    shapes, nt = HD.FORTY_TABLES
    assert nt == 40 > HD.K_MAX_SMALL_TABLES and HD.small_plan(shapes) == "small.ptrs" and not HD.tail_shape_ok(shapes)
    assert HD.finalize_plan(shapes) == "finalize.no_lds"  # D = 41


def test_the_extreme_tables_hold_what_they_claim():
    P = HD.EXTREMES[2] + 1
    tabs = HD.extreme_tables(5, 3, 7)
    seen = set()
    for t in tabs:
        assert t.shape == (32, 4) and t.dtype == np.uint64
        seen |= {sum(int(e[k]) << (64 * k) for k in range(4)) for e in t}
    assert seen == {0, 1, P - 1}
    top = HD.extreme_tables(4, 2, 7, all_top=True)
    assert all(np.array_equal(t, np.tile(H.raw_limbs(P - 1), (16, 1))) for t in top)
    assert I(HD.extreme_challenges(5)) == [0, 1, P - 1, 0, 1]
