"""Launch plans that the suite used to reach once, at a size where the code that can go wrong never runs (sumcheck_amd/csrc/protocol.hip:
launch_round; kernels.hip: launch_finalize):

  A  the single-block finalizes (more than kMetaProds = 16 products: k_finalize<true, false>; node sums beyond 48 KB: k_finalize<false,
     false>) in BIG rounds -- finalize_sums' `nblocks > 8` branch, which enumerates the valid (product, node) pairs, walks them in passes
     of the block's 16 wavefronts and keeps 12 loads in flight per lane (1024 partial blocks: a second batch with a clamped tail);
  B  more than kMaxSmallTables = 32 tables: the handle keeps its bound tables in the reference layout, and every binding big round is the
     chain instantiation of the merged round kernel reading a table it stored itself;
  C  a lagging table (tests/test_gpu_lagging_tables.py) on such a handle: k_fix_deep<false, 1..5>, deep_store<false>, class rows between
     canonical rows;
  D  sc_set_policy("wide_tree", 0): k_prod_round_fe with a repeated factor next to per-product trees, and k_sum_generic from 9 factors on.

Every message is compared bit for bit with the oracle's (cref.Prover under fixed challenges, the Fiat-Shamir proof with cref.Prover and
cref.Rng in ml_prove's order), the bound tables with its .state().  The plan counters are read around every round: each test states which
moved and by how much, so that a change of a threshold cannot move it onto another path unnoticed.

Sizes: a round is big above kSmallRoundPairs = 2^14 pairs, so nv has nv - 15 big rounds; round j runs over 2^(nv - j) pairs and binds
challenge j - 1 first."""
import functools

import numpy as np
import pytest
import torch

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib
from tests import fe_model as fm
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VM = sc.VerifierMsg
SEED = 0x1B0
LAG = ("big.lag_class_round", "big.lag_catch_up", "big.lag_materialize")

MIXED = [[0], [1, 1], [0, 1, 2], [0, 1, 2, 3], [3, 3, 3]]
SHAPES = {
    "18-pairs": [[0, 1]] * 9 + [[1, 2]] * 9,                 # K = 18 > kMetaProds; D = 3: 18 * 3 * 5 * 32 = 8640 bytes of node sums
    "44-quads": [[0, 1, 2, 3]] * 22 + [[1, 2, 3]] * 22,      # D = 5: 44 * 5 * 7 * 32 = 49 280 bytes > kFinLdsMax = 49 152
    "17-mixed": (MIXED * 4)[:17],                            # D = 5; sum of M + 1 = 3 * 18 + 2 + 3 = 59 valid pairs: 3 passes of 16 and one of 11
    "33-tables": [[3 * i, 3 * i + 1, 3 * i + 2] for i in range(10)] + [[30, 31], [32]],
    "narrow": [[0, 1, 2, 3, 4], [5, 5, 1], [2, 3, 4, 0], [0, 0, 0, 0, 0, 0]],
    "nine": [[0, 1, 2, 3, 4, 5, 6, 7, 8], [0, 1]],
}


def n_tables(shapes):
    return max(max(sh) for sh in shapes) + 1


def n_big(nv):
    return nv - 15


def moved_since(before):
    after = _lib.plan_stats()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


@functools.lru_cache(maxsize=None)
def tables_of(nv, name):
    """tables and coefficients, once per (size, shape); add_product flattens these shapes in table order, as the oracle's descriptor does"""
    shapes = SHAPES[name]
    seen = [t for sh in shapes for t in sh]
    assert sorted(set(seen), key=seen.index) == list(range(n_tables(shapes)))
    tabs, coefs = H.random_case(None, nv, shapes, n_tables(shapes), SEED + nv)
    return shapes, tabs, coefs


def oracle_rounds(nv, shapes, tabs, coefs, chal, export_after, last=None):
    """the oracle's messages under the given challenges -> (messages, {round: its tables after that round}); stops after round `last`"""
    op = cref.Prover(H.desc_from(nv, shapes, tabs, coefs), threads=cref.max_threads())
    want, otabs = [], {}
    for j in range(last or nv):
        want.append(op.prove_round(None if j == 0 else chal[j - 1]))
        if j + 1 in export_after:
            otabs[j + 1] = op.state()[1]
    op.close()
    return want, otabs


def oracle_proof(nv, shapes, tabs, coefs, export_after=()):
    """the oracle's Fiat-Shamir proof, round by round in cref.ml_prove's order (PolynomialInfo, then message -> challenge)
    -> (proof, challenges, {round: tables})"""
    desc = H.desc_from(nv, shapes, tabs, coefs)
    op, rng = cref.Prover(desc, threads=cref.max_threads()), cref.Rng()
    rng.feed_poly_info(desc.max_multiplicands, nv)
    proof, rand, otabs, r = [], [], {}, None
    for j in range(nv):
        proof.append(op.prove_round(r))
        rng.feed_prover_msg(proof[-1])
        r = rng.sample_fr()
        rand.append(r)
        if j + 1 in export_after:
            otabs[j + 1] = op.state()[1]
    op.close()
    return np.stack(proof), np.stack(rand), otabs


@pytest.fixture(scope="module", autouse=True)
def free_the_tables():
    """the synthetic tables are shared between the tests of this file and dropped behind its last one"""
    yield
    tables_of.cache_clear()


# The oracle's answers are computed INSIDE every test that compares with them, never shared: tests/conftest.py credits a launch plan to a
# test only when that test itself called the oracle, and the tests below are what the coverage report should name for their plans.
def interactive_case(nv, name, export_after):
    shapes, tabs, coefs = tables_of(nv, name)
    chal = cref.synth_table(SEED + 1, nv, nv)
    want, otabs = oracle_rounds(nv, shapes, tabs, coefs, chal, export_after)
    return chal, want, otabs


def proof_case(nv, name):
    shapes, tabs, coefs = tables_of(nv, name)
    return oracle_proof(nv, shapes, tabs, coefs)[0]


def device_poly(nv, name):
    shapes, tabs, coefs = tables_of(nv, name)
    poly, _ = H.hip_poly_from(nv, shapes, tabs, coefs, device=DEV)
    torch.cuda.synchronize()
    return poly


def assert_tables(st, otabs, what):
    got = st.flattened_ml_extensions
    assert len(got) == len(otabs)
    for u, t in enumerate(got):
        assert np.array_equal(t.evaluations, otabs[u]), f"table {u} {what}"


def drive(st, nv, chal, want, otabs, last=None):
    """rounds 1 .. last through sc_prove_round, every message and the tables after the rounds of `otabs` against the oracle's
    -> the plan counters that each round's call moved (the exports in between are outside: the caller's own snapshot spans them)"""
    per_round = []
    for j in range(last or nv):
        before = _lib.plan_stats()
        got = sc.IPForMLSumcheck.prove_round(st, None if j == 0 else VM(chal[j - 1])).evaluations
        per_round.append(moved_since(before))
        assert np.array_equal(got, want[j]), f"round {j + 1}"
        if j + 1 in otabs:
            assert_tables(st, otabs[j + 1], f"after round {j + 1}")
    return per_round


# ---- A: the single-block finalizes with many partial blocks ------------------------------------------------------------------------------
@pytest.mark.parametrize("nv,name,fin", [(17, "18-pairs", "finalize.one_block"), (19, "18-pairs", "finalize.one_block"),
                                         (19, "44-quads", "finalize.no_lds"), (17, "17-mixed", "finalize.one_block")])
def test_single_block_finalize_in_big_rounds(nv, name, fin):
    """More than kMaxRoundProds = 12 products: every big round is K per-product tree launches of grid_for_pairs = 2^(nv - j) / 256 blocks --
    1024, 512, 256, 128 at nv = 19; 256, 128 at nv = 17 -- and one launch of the single-block finalize over that many partials per node.
    (The counters cannot see a block count: round 1 of nv = 19 has 1024 blocks -- the second batch of 12 loads and its clamped tail -- only
    while kBlock = 256 and kMaxGrid = 1024 (kernels.h, grid_for_pairs); with a lower cap this test would still pass, on one batch.)
    Three or four tables of products of at most four factors: the bound tables are F29 (one big.store_f29 per launch of a binding round).
    More than kMetaCombos = 24 combinations: no persistent kernel, so every later round is a launch with the same finalize.
    Interactive rounds under fixed challenges with the tables after round 3 and after the last round, then a Fiat-Shamir proof."""
    shapes = SHAPES[name]
    K = len(shapes)
    chal, want, otabs = interactive_case(nv, name, (3, nv))
    poly = device_poly(nv, name)
    with _lib.policy(resident=0):
        st = sc.IPForMLSumcheck.prover_init(poly, borrow=True)
        before = _lib.plan_stats()
        per_round = drive(st, nv, chal, want, otabs)
        total = moved_since(before)
        print(f"\nnv {nv} {name}: interactive {total}")
        for j in range(n_big(nv)):
            expect = {"big.per_product_tree": K, fin: 1}
            if j > 0:
                expect["big.store_f29"] = K
            assert per_round[j] == expect, f"round {j + 1}: {per_round[j]}"
        for j in range(n_big(nv), nv):
            assert per_round[j].get(fin, 0) == 1 and not any(k.startswith("big.") for k in per_round[j]), f"round {j + 1}: {per_round[j]}"
        assert total.get(fin, 0) == nv and "finalize.multi_block" not in total, total

        before = _lib.plan_stats()
        st.reset()
        got = st.prove()
        total = moved_since(before)
        st.close()
    assert np.array_equal(got, proof_case(nv, name)), "the Fiat-Shamir proof differs from the oracle's"
    assert total.get(fin, 0) == nv and "finalize.multi_block" not in total, total
    assert total.get("big.per_product_tree", 0) == K * n_big(nv) and total.get("big.store_f29", 0) == K * (n_big(nv) - 1), total


# ---- B: canonical bound tables through every big round -----------------------------------------------------------------------------------
NV_B = 19
# 12 products of at most three factors: one merged launch per big round (k_round_tree_split), 33 tables: canonical bound tables, and from
# 2^14 pairs on k_fix_multi + k_sum_combos_ptrs (no persistent kernel, no pipelined round: more tables than their arguments hold).
# Blocks per product row: min(2^(19 - j) / 256, 384 | 256 | 192 | 192) = 384, 256, 192, 128 in rounds 1 .. 4; K D (D + 2) 32 = 9216 bytes and
# K <= 16: the multi-block finalize, which keeps the node sums of every round of more than 8 blocks -- so rounds 2, 3 and 4 all take node 1
# from the claim identity.
ROUND1 = {"big.merged.round1": 1, "finalize.multi_block": 1}
BIND_CANONICAL = {"big.merged.bind_chain": 1, "big.claim_identity": 1, "big.store_canonical": 1, "finalize.multi_block": 1}
SMALL_PTRS = {"small.ptrs": 1, "finalize.multi_block": 1}
PROOF_B = {"big.merged.round1": 1, "big.merged.bind_chain": 3, "big.claim_identity": 3, "big.store_canonical": 3, "small.ptrs": NV_B - 4,
           "finalize.multi_block": NV_B}


def test_canonical_tables_through_every_big_round():
    """lag_single = 0: rounds 3 and 4 read canonical tables that rounds 2 and 3 stored, round 5 (the first k_sum_combos_ptrs) those of round
    4.  The tables after rounds 2, 3, 4 and after the last round; then, on the same handle, reset + prove, rounds with one export after round
    3, reset + prove."""
    nv, name = NV_B, "33-tables"
    chal, want, otabs = interactive_case(nv, name, (2, 3, 4, nv))
    proof = proof_case(nv, name)
    poly = device_poly(nv, name)
    with _lib.policy(lag_single=0, resident=0):
        st = sc.IPForMLSumcheck.prover_init(poly, borrow=True)
        before = _lib.plan_stats()
        per_round = drive(st, nv, chal, want, otabs)
        total = moved_since(before)
        print(f"\nnv {nv} {name}: interactive {total}")
        assert per_round[0] == ROUND1, per_round[0]
        for j in (1, 2, 3):
            assert per_round[j] == BIND_CANONICAL, f"round {j + 1}: {per_round[j]}"
        for j in range(4, nv):  # 15 rounds
            assert per_round[j] == SMALL_PTRS, f"round {j + 1}: {per_round[j]}"
        assert total == PROOF_B, total  # (nothing else moved: no big.merged.bind, no big.store_f29, no lagging)

        before = _lib.plan_stats()
        st.reset()
        got = st.prove()
        assert np.array_equal(got, proof), "reset + prove"
        assert moved_since(before) == PROOF_B

        before = _lib.plan_stats()
        st.reset()
        drive(st, nv, chal, want, {3: otabs[3]})
        st.reset()
        got = st.prove()
        assert np.array_equal(got, proof), "rounds with an export after round 3, reset + prove"
        assert moved_since(before) == {k: 2 * v for k, v in PROOF_B.items()}
        st.close()


# ---- C: a lagging table on a canonical handle --------------------------------------------------------------------------------------------
def test_lagging_table_on_a_canonical_handle():
    """the library's lag_single = 2 at nv = 19 (four big rounds): table 32 lags through rounds 2 and 3, whose rows for [32] bind its class
    table between eleven canonical rows, and k_fix_deep<false, 3> binds it with three challenges in front of round 4"""
    nv, name = NV_B, "33-tables"
    assert _lib.get_policy("lag_single") == 2
    chal, want, otabs = interactive_case(nv, name, (4,))
    poly = device_poly(nv, name)
    with _lib.policy(resident=0):
        st = sc.IPForMLSumcheck.prover_init(poly, borrow=True)
        before = _lib.plan_stats()
        per_round = drive(st, nv, chal, want, otabs)
        total = moved_since(before)
        st.close()
    print(f"\nnv {nv} {name}: lagging {total}")
    assert per_round[1] == per_round[2] == {**BIND_CANONICAL, LAG[0]: 1}, per_round[1:3]
    assert per_round[3] == {**BIND_CANONICAL, LAG[1]: 1}, per_round[3]
    assert total == {**PROOF_B, LAG[0]: 2, LAG[1]: 1}, total


def test_export_one_challenge_behind_on_a_canonical_handle():
    """the tables exported after round 2, a class round: materialize_lagging with ONE level (k_fix_deep<false, 1> stores from deep_first);
    nothing lags afterwards and the rounds go on to the end"""
    nv, name = NV_B, "33-tables"
    chal, want, otabs = interactive_case(nv, name, (2,))
    poly = device_poly(nv, name)
    with _lib.policy(resident=0):
        st = sc.IPForMLSumcheck.prover_init(poly, borrow=True)
        before = _lib.plan_stats()
        per_round = drive(st, nv, chal, want, otabs)
        total = moved_since(before)
        st.close()
    assert per_round[1] == {**BIND_CANONICAL, LAG[0]: 1}, per_round[1]
    assert per_round[2] == per_round[3] == BIND_CANONICAL, per_round[2:4]
    assert total == {**PROOF_B, LAG[0]: 1, LAG[2]: 1}, total


def extreme_table(nv):
    """0, 1 and p - 1 as STORED values, chosen by index bits: bits 4-5 name the level L = 1 .. 4 at which an entry's pair differs (in index
    bit L - 1; below it the entries are equal and bind to themselves, lo + r * 0), bits 6-7 the pair (lo, hi) = (0, 1), (1, 0), (0, p - 1),
    (p - 1, 0): hi - lo = 1, -1, p - 1, -(p - 1) at each of the first four binds.  With lag_single = 2 only the first THREE are levels of
    k_fix_deep<false, 3>; the fourth is round 5's k_fix_multi (small.ptrs), no coverage of a deep level 4.  (The layout has period 256: the
    check below of the first 256 entries covers it.)"""
    x = np.arange(1 << nv, dtype=np.int64)
    bit = (x >> ((x >> 4) & 3)) & 1
    lo, hi = np.array([0, 1, 0, 2]), np.array([1, 0, 2, 0])
    combo = (x >> 6) & 3
    vals = np.stack([H.raw_limbs(v) for v in (0, 1, fm.P - 1)])
    tab = np.ascontiguousarray(vals[np.where(bit == 1, hi[combo], lo[combo])])
    pairs = [(0, 1), (1, 0), (0, fm.P - 1), (fm.P - 1, 0)]
    for level in range(1, 5):
        for c, (a, b) in enumerate(pairs):
            for low in range(16):
                e = tab[((level - 1) << 4) | (c << 6) | low]
                assert sum(int(e[k]) << (64 * k) for k in range(4)) == (b if (low >> (level - 1)) & 1 else a)
    return tab


@pytest.mark.parametrize("first", ["0-1-p-1", "p-1-p-1-p-1"])
def test_extreme_values_in_the_lagging_canonical_table(first):
    """table 32 of 0, 1 and p - 1 (extreme_table) under the challenges 0, 1, p - 1 -- or p - 1 three times -- and random ones after them:
    k_fix_deep<false, 3> reduces after every level as rounds 2 .. 4 would have.  Every message, and every table after round 4"""
    nv, name = NV_B, "33-tables"
    shapes, tabs, coefs = tables_of(nv, name)
    tabs = list(tabs[:32]) + [extreme_table(nv)]
    chal = np.concatenate([H.mont_challenges([0, 1, fm.P - 1] if first == "0-1-p-1" else [fm.P - 1] * 3), cref.synth_table(SEED + 2, nv, nv - 3)])
    want, otabs = oracle_rounds(nv, shapes, tabs, coefs, chal, (4,))
    poly, _ = H.hip_poly_from(nv, shapes, tabs, coefs, device=DEV)
    torch.cuda.synchronize()
    with _lib.policy(resident=0):
        st = sc.IPForMLSumcheck.prover_init(poly, borrow=True)
        before = _lib.plan_stats()
        drive(st, nv, chal, want, otabs)
        total = moved_since(before)
        st.close()
    assert total == {**PROOF_B, LAG[0]: 2, LAG[1]: 1}, total


@pytest.fixture(scope="module")
def six_big_rounds():
    """33 tables at nv = 21 (2.2 GB), synthesised and put on the device once for the two tests below, which compute the oracle's answers
    themselves; freed behind them"""
    nv, name = 21, "33-tables"
    shapes, tabs, coefs = tables_of.__wrapped__(nv, name)  # (not kept in the cache: the fixture owns them)
    poly, _ = H.hip_poly_from(nv, shapes, tabs, coefs, device=DEV)
    torch.cuda.synchronize()
    box = {"poly": poly, "case": (nv, shapes, tabs, coefs)}
    del poly, tabs
    yield box
    box.clear()
    torch.cuda.empty_cache()


def test_every_lag_single_value_on_a_canonical_handle(six_big_rounds):
    """nv = 21, six big rounds, one borrowed handle: lag_single = v skips v rounds and k_fix_deep<false, v + 1> runs in front of round v + 2
    (five levels at v = 4, the only size at which <false, 4> and <false, 5> run); 0 switches lagging off.  No tail kernel takes over on 33
    tables, so the catch-up is never a materialize."""
    nv = 21
    proof = oracle_proof(*six_big_rounds["case"])[0]
    st = sc.IPForMLSumcheck.prover_init(six_big_rounds["poly"], borrow=True)
    for v in (0, 1, 2, 3, 4):
        with _lib.policy(lag_single=v):
            before = _lib.plan_stats()
            st.reset()
            got = st.prove()
            moved = moved_since(before)
        assert np.array_equal(got, proof), f"lag_single = {v}"
        assert moved.get(LAG[0], 0) == v and moved.get(LAG[1], 0) == (1 if v else 0) and moved.get(LAG[2], 0) == 0, (v, moved)
        # five binding big rounds, all canonical; 15 rounds from 2^14 pairs on
        assert moved.get("big.merged.bind_chain", 0) == 5 and moved.get("big.store_canonical", 0) == 5 and moved.get("small.ptrs", 0) == nv - 6, (v, moved)
        assert not moved.get("big.merged.bind", 0) and not moved.get("big.store_f29", 0), (v, moved)
    st.close()


def test_five_levels_behind_on_a_canonical_handle(six_big_rounds):
    """lag_single = 4 through sc_prove_round under fixed challenges: rounds 2 .. 5 are class rounds, k_fix_deep<false, 5> runs in front of
    round 6, and every table after round 6 is the oracle's.  Seven rounds: the first latency-bound one reads what round 6 left."""
    nv = 21
    chal = cref.synth_table(SEED + 1, nv, nv)
    want, otabs = oracle_rounds(*six_big_rounds["case"], chal, (6,), last=7)
    with _lib.policy(lag_single=4, resident=0):
        st = sc.IPForMLSumcheck.prover_init(six_big_rounds["poly"], borrow=True)
        before = _lib.plan_stats()
        per_round = drive(st, nv, chal, want, otabs, last=7)
        total = moved_since(before)
        st.close()
    for j in (1, 2, 3, 4):
        assert per_round[j].get(LAG[0], 0) == 1 and per_round[j].get("big.merged.bind_chain", 0) == 1, f"round {j + 1}: {per_round[j]}"
    assert per_round[5].get(LAG[1], 0) == 1 and per_round[5].get("big.store_canonical", 0) == 1, per_round[5]
    assert per_round[6] == SMALL_PTRS, per_round[6]
    assert total.get(LAG[0], 0) == 4 and total.get(LAG[1], 0) == 1 and total.get(LAG[2], 0) == 0, total


# ---- D: wide_tree = 0 through three big rounds -------------------------------------------------------------------------------------------
NV_D = 18


def test_node_by_node_products_next_to_trees():
    """[0,1,2,3,4] and the sixth power of table 0 run node by node (k_prod_round_fe; slot.exp = 6), [5,5,1] and [2,3,4,0] as per-product
    trees; a product beyond four factors keeps the handle's tables canonical.  In a binding round the first launch binds tables 0 .. 4, the
    second table 5 (and reads table 1 as the first left it), the third and fourth read only.  Per big round: two launches of each kind, and
    in rounds 2 and 3 one big.store_canonical per tree launch.  K D (D + 2) 32 = 4 * 7 * 9 * 32 bytes: the multi-block finalize."""
    nv, name = NV_D, "narrow"
    chal, want, otabs = interactive_case(nv, name, (2, 3))
    with _lib.policy(wide_tree=0, resident=0):
        poly = device_poly(nv, name)
        st = sc.IPForMLSumcheck.prover_init(poly, borrow=True)
        before = _lib.plan_stats()
        per_round = drive(st, nv, chal, want, otabs)
        total = moved_since(before)
        print(f"\nnv {nv} {name}: interactive {total}")
        for j in range(3):
            expect = {"big.node_by_node": 2, "big.per_product_tree": 2, "finalize.multi_block": 1}
            if j > 0:
                expect["big.store_canonical"] = 2
            assert per_round[j] == expect, f"round {j + 1}: {per_round[j]}"
        assert total.get("big.node_by_node", 0) == 6 and total.get("big.per_product_tree", 0) == 6 and total.get("big.store_canonical", 0) == 4, total
        assert "big.wide" not in total and "big.store_f29" not in total, total

        before = _lib.plan_stats()
        st.reset()
        got = st.prove()
        total = moved_since(before)
        st.close()
    assert np.array_equal(got, proof_case(nv, name)), "the Fiat-Shamir proof differs from the oracle's"
    assert total.get("big.node_by_node", 0) == 6 and total.get("big.per_product_tree", 0) == 6 and total.get("big.store_canonical", 0) == 4, total
    assert "big.wide" not in total and "big.store_f29" not in total, total


def test_generic_sum_below_thirteen_factors():
    """nine factors with wide_tree = 0: k_fix_multi binds every table up front in rounds 2 and 3 (big.bind_pass), k_sum_generic sums the
    product, and [0, 1] is a tree launch that reads in place (nothing stored: no big.store_*)"""
    nv, name = NV_D, "nine"
    chal, want, otabs = interactive_case(nv, name, (2, 3))
    with _lib.policy(wide_tree=0, resident=0):
        poly = device_poly(nv, name)
        st = sc.IPForMLSumcheck.prover_init(poly, borrow=True)
        per_round = drive(st, nv, chal, want, otabs)
        for j in range(3):
            expect = {"big.generic": 1, "big.per_product_tree": 1, "finalize.multi_block": 1}
            if j > 0:
                expect["big.bind_pass"] = 1
            assert per_round[j] == expect, f"round {j + 1}: {per_round[j]}"
        before = _lib.plan_stats()
        st.reset()
        got = st.prove()
        total = moved_since(before)
        st.close()
    assert np.array_equal(got, proof_case(nv, name)), "the Fiat-Shamir proof differs from the oracle's"
    assert total.get("big.generic", 0) == 3 and total.get("big.bind_pass", 0) == 2 and "big.wide16" not in total, total
