"""Lazily bound table entries at the ENDS of their range.  The carry-free kernels never reduce an entry between binds: after k binds it lies in
(-(k + 1) p, p), and `lazy_sum_needs_reduce`, `tail_worst_p`, `tail_slices_blocks`' refusal and `k_batch_round`'s
`worst_p = round + 1` rest on that range.  Constant tables never move (every slope is 0) and random ones sink by about p / 2 a bind, so
neither comes near an end.  The tables here do, with challenges chosen for them (tests/fe_model.py: sinking_challenges): every entry of a
sinking table is at -k p after k binds, and round sel + 1 of a selector table has every slope at +-(sel + 1) p.

Only a caller who chooses the challenges can do this: sc_prove_round and sc_batch_prove_round (and prove_as_subprotocol with an RNG of the
caller's own).  The Fiat-Shamir entry points (sc_ml_prove, sc_ml_prove_batch, sc_gkr_prove_batch) derive their challenges from the messages
and cannot be driven here, but they run the SAME round bodies -- bt_* of batch_round.hpp, and k_tail_slices as the resident kernel -- so the
interactive entry points are the way in to those too.

Every message of every round is compared bit for bit with cref.Prover(desc).prove_round(r), the bound tables with its .state(); nothing is
sampled.  The plan counters (sc_plan_name's names) prove which kernel ran."""
import time

import numpy as np
import pytest
import torch

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib
from tests import fe_model as fm
from tests import helpers as H
from tests.test_gpu_batch import C2, C3, GKR, SIX

pytestmark = pytest.mark.gpu
P = fm.P
VM = sc.VerifierMsg
DEV = "cuda:0"


def sinking(nv, s, t):
    """table number t of a sinking instance: m = 1 .. 7, even t at the low end (c as small as it may be), odd t starting just below p"""
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


def n_tables(shapes):
    return max(max(sh) for sh in shapes) + 1


def poly_of(nv, shapes, tabs, coefs):
    poly, _ = H.hip_poly_from(nv, shapes, tabs, coefs, device=DEV)
    torch.cuda.synchronize()
    return poly


# ---- k_batch_round ---------------------------------------------------------------------------------------------------------------------------
BATCH_SHAPES = [([[0]], 11), ([[0], [1]], 10), (GKR, 10), (C2, 9), (C3, 8), (SIX, 8)]
BATCH_SEL = 3


def batch_plans():
    p = _lib.plan_stats()
    return p["batch.rounds_one_block"], p["batch.rounds_serial"]


@pytest.mark.parametrize("shapes,nv", BATCH_SHAPES, ids=["single-nv11", "two-singles-nv10", "gkr-nv10", "c2-nv9", "c3-nv8", "six-nv8"])
def test_batched_rounds_on_sinking_and_selector_tables(shapes, nv):
    """k_batch_round at the envelope's largest sizes, n = 3: instance 0 every table sinking (entries at -k p in round k + 1: the lower end,
    against worst_p = round + 1), instance 1 every table a selector with sel = 3 (every slope of round 4 at +-4 p; a product's tables
    alternate in orientation, so two slopes have opposite signs), instance 2 random tables under instance 0's challenges."""
    nt = n_tables(shapes)
    s0, r0 = fm.sinking_challenges(nv, 61000 + nv)
    s1, r1 = fm.sinking_challenges(nv, 62000 + nv)
    tabs = [[sinking(nv, s0, t) for t in range(nt)],
            [selector(nv, s1, BATCH_SEL, t, flip=t % 2 == 1) for t in range(nt)],
            [cref.synth_table(63000 + nv, t, 1 << nv) for t in range(nt)]]
    chal = np.stack([H.mont_challenges(r0), H.mont_challenges(r1), H.mont_challenges(r0)], axis=1)  # (nv, n, 4): chal[j][i] follows message j + 1
    batched_rounds(nv, shapes, tabs, chal)


def batched_rounds(nv, shapes, tabs, chal):
    """all nv rounds of len(tabs) instances as one k_batch_round launch a round: every message against the oracle's, the bound tables after
    rounds 1, 2 and nv, bind_final"""
    n = len(tabs)
    coefs = [cref.synth_table(64000 + i, 1000, len(shapes)) for i in range(n)]
    descs = [H.desc_from(nv, shapes, tabs[i], coefs[i]) for i in range(n)]
    polys = [poly_of(nv, shapes, tabs[i], coefs[i]) for i in range(n)]
    provers = [cref.Prover(d, threads=1) for d in descs]
    with _lib.policy(batch=2):
        b0, s0_ = batch_plans()
        st = sc.IPForMLSumcheck.prover_init_batch(polys)
        for j in range(nv):
            cj = None if j == 0 else chal[j - 1]
            want = np.stack([p.prove_round(None if cj is None else cj[i]) for i, p in enumerate(provers)])
            got = sc.IPForMLSumcheck.prove_round_batch(st, None if cj is None else [VM(cj[i]) for i in range(n)])
            got = np.stack([m.evaluations for m in got])
            bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
            assert bad.size == 0, f"round {j + 1}: instances {bad.tolist()} differ from the oracle's message"
            if (j + 1) in (1, 2, nv):
                for i in range(n):
                    rand, otabs, rnd = provers[i].state()
                    assert st.round == rnd and np.array_equal(st.randomness(i), rand)
                    for u, t in enumerate(st.flattened_ml_extensions(i)):
                        assert np.array_equal(np.asarray(t.evaluations), otabs[u]), f"after round {j + 1}: bound table {u} of instance {i}"
        tv = st.bind_final([VM(chal[nv - 1][i]) for i in range(n)])
        for i in range(n):
            for u, t in enumerate(descs[i].tables):
                assert np.array_equal(tv[i, u], cref.fix_variables(t, chal[:, i])[0]), f"bind_final: instance {i}, table {u}"
        st.close()
        assert batch_plans() == (b0 + nv, s0_), "every round must be one launch of k_batch_round"


EIGHT = [[0, 1, 2, 3, 4, 5, 6, 7]]


@pytest.mark.parametrize("shapes", [SIX, EIGHT], ids=["six-nv8", "eight-nv8"])
def test_batched_rounds_with_every_table_a_selector_in_the_last_round(shapes):
    """k_batch_round where its envelope ends (products of six and of eight at nv = 8), EVERY table a selector at sel = 7: the last round's pair
    is (entry at -7 p, p - 1) in every factor at once -- instance 0 all up, instance 1 all down, so no factor of a product is near 0.  fe_line
    out to nodes 3 / -2 (-23 p) and 4 / -3 (-31 p) in all six / eight factors, the running product at 31 * 31 / 70.66 = 13.6 p (the model:
    tests/test_fe_model_host.py, k = 7)"""
    nv, sel, nt = 8, 7, n_tables(shapes)
    s0, r0 = fm.sinking_challenges(nv, 61500 + nt)
    s1, r1 = fm.sinking_challenges(nv, 62500 + nt)
    tabs = [[selector(nv, s0, sel, t, flip=False) for t in range(nt)], [selector(nv, s1, sel, t, flip=True) for t in range(nt)]]
    batched_rounds(nv, shapes, tabs, np.stack([H.mont_challenges(r0), H.mont_challenges(r1)], axis=1))


# ---- sc_prove_round: lazy big rounds, then the resident k_tail_slices ---------------------------------------------------------------------------
def interactive(nv, shapes, tabs, chal, lazy_big_binds, resident="resident.slices"):
    """all nv rounds of one interactive prover over device tables against the oracle's (computed first: the resident kernel waits for its
    challenges), then the bound tables; the counters: `lazy_big_binds` big rounds stored their bound tables in the internal format, and the
    rest of the proof ran in ONE resident kernel of the given kind (None: in no resident kernel at all)"""
    coefs = cref.synth_table(65000 + nv, 1000, len(shapes))
    t0 = time.perf_counter()
    op = cref.Prover(H.desc_from(nv, shapes, tabs, coefs), threads=cref.max_threads())
    want = [op.prove_round(None if j == 0 else chal[j - 1]) for j in range(nv)]
    _, otabs, _ = op.state()
    op.close()
    t1 = time.perf_counter()
    poly = poly_of(nv, shapes, tabs, coefs)
    before = _lib.plan_stats()
    st = sc.IPForMLSumcheck.prover_init(poly)
    bad = []
    for j in range(nv):
        got = sc.IPForMLSumcheck.prove_round(st, None if j == 0 else VM(chal[j - 1])).evaluations
        if not np.array_equal(got, want[j]):
            bad.append(j + 1)
    after = _lib.plan_stats()
    moved = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    print(f"\nnv {nv} {shapes}: oracle {t1 - t0:.2f} s, device {time.perf_counter() - t1:.2f} s, plans {moved}")
    assert not bad, f"rounds {bad} differ from the oracle's"
    for u, t in enumerate(st.flattened_ml_extensions):
        assert np.array_equal(t.evaluations, otabs[u]), f"bound table {u} after the last round"
    st.close()
    assert moved.get("big.store_f29", 0) == lazy_big_binds, "the big rounds must bind lazily, in the internal format"
    if resident is None:
        assert moved.get("resident.slices", 0) == 0 and moved.get("resident.rounds", 0) == 0, "no kernel may wait for the host"
        return moved
    other = "resident.rounds" if resident == "resident.slices" else "resident.slices"
    assert moved.get(resident, 0) == 1 and moved.get(other, 0) == 0, f"the tail must run as one {resident} kernel"
    return moved


@pytest.mark.parametrize("nv", [22, 23])
def test_a_sinking_table_through_lazy_big_rounds_into_the_resident_slices(nv):
    """[[0]]: the tail starts at 2^16 pairs, after nv - 18 lazy big binds and with one more of its own in front of its first sums -- 256 RAW
    entries a block, counted by tail_worst_p as if at -(nv - 17) p, then -(nv - 16) p, ...  (Since bound tables are packed the big rounds
    settle every entry into +-1.104 p, so the tail's own binds sink from there: -1 p, -2 p, ...; the rule's count is an upper bound.)
    tail_slices_blocks' refusal (33 terms of worst_p p a lane) is NOT reached by this shape on a device that holds 256 blocks: a lane then has
    4 terms a round, and 5 * worst_p passes 282 only beyond validate_desc's 40 variables -- there is no nv at which the counter flips."""
    s, r = fm.sinking_challenges(nv, 66000 + nv)
    tab = H.sinking_table_limbs(nv, s, 1, sum(s))
    H.assert_entries_match(tab, H.sinking_entry(s, 1, sum(s)))
    interactive(nv, [[0]], [tab], H.mont_challenges(r), lazy_big_binds=nv - 18)


def test_products_of_sinking_and_selector_tables_into_the_resident_slices():
    """[[0, 1], [2]] at nv = 20: four big rounds, the tail from 2^15 pairs.  Table 0 sinking from just below p, table 1 a selector whose slopes
    peak in the last big round (sel = 3: 4 p), table 2 one the other way round that peaks in the tail's first round (sel = 4: -5 p)"""
    nv, shapes = 20, [[0, 1], [2]]
    s, r = fm.sinking_challenges(nv, 67000)
    tabs = [sinking(nv, s, 1), selector(nv, s, 3, 0, False), selector(nv, s, 4, 2, True)]
    interactive(nv, shapes, tabs, H.mont_challenges(r), lazy_big_binds=3)


def test_the_claim_identity_shape_with_selectors_at_the_last_big_and_first_tail_round():
    """[[0, 1, 2, 3], [4, 5, 6], [1, 1], [2]] at nv = 19: big rounds 2 to 4 take node 1 from the claim (kSkip1) and bind lazily, the tail starts at
    2^14 pairs.  Selectors of both orientations at sel = 3 (the last big round's slopes) and sel = 4 (the tail's first), the rest sinking"""
    nv, shapes = 19, [[0, 1, 2, 3], [4, 5, 6], [1, 1], [2]]
    s, r = fm.sinking_challenges(nv, 68000)
    tabs = [sinking(nv, s, 0), selector(nv, s, 3, 1, False), selector(nv, s, 4, 2, True), sinking(nv, s, 3),
            selector(nv, s, 3, 4, True), selector(nv, s, 4, 5, False), sinking(nv, s, 6)]
    moved = interactive(nv, shapes, tabs, H.mont_challenges(r), lazy_big_binds=3)
    assert moved.get("big.claim_identity", 0) > 0, "the big rounds must take node 1 from the claim"


def test_a_product_of_five_through_the_wide_tree_with_selector_slopes_in_its_last_big_round():
    """[[0, 1, 2, 3, 4]] at nv = 18: the big rounds run in k_prod_tree_wide, whose fifth factor is a half of its own -- its line is the REDUCED
    combination fe_comb5 of two raw lazy entries (wide_tree.hpp), not fe_line.  Selectors of both orientations peak in the last big round
    (sel = 2: +-3 p), that factor among them; the tail starts at 2^14 pairs"""
    nv, shapes = 18, [[0, 1, 2, 3, 4]]
    s, r = fm.sinking_challenges(nv, 68500)
    tabs = [sinking(nv, s, 0), selector(nv, s, 2, 1, True), sinking(nv, s, 3), selector(nv, s, 3, 2, False), selector(nv, s, 2, 4, False)]
    moved = interactive(nv, shapes, tabs, H.mont_challenges(r), lazy_big_binds=2)
    assert moved.get("big.wide", 0) > 0, "the big rounds must run in the tree kernel for five to eight multiplicands"


# ---- every factor of a product at its range end at once, through the resident k_tail_slices ------------------------------------------------------
ALL_NV = 15  # the tail takes the proof from round 1 (2^14 pairs): entries at -k p after k binds, k = 14 in the last round -- the smallest such shape
ORIENT = {"up": lambda t: False, "down": lambda t: True, "alt": lambda t: t % 2 == 1}


def all_selectors(nv, nt, sel, orient):
    """nt selector tables at the same sel in the given orientation, and the challenges that sink them"""
    s, r = fm.sinking_challenges(nv, 72000 + 100 * nv + sel)
    return [selector(nv, s, sel, t, ORIENT[orient](t)) for t in range(nt)], H.mont_challenges(r)


@pytest.mark.parametrize("orient", ["up", "down", "alt"])
@pytest.mark.parametrize("sel", [10, 13, 14])
@pytest.mark.parametrize("M", [3, 4, 6, 8, 9, 10, 11, 12])
def test_every_factor_a_selector_through_the_resident_slices(M, sel, orient):
    """one product of M distinct tables at nv = 15, every table a selector at the same sel: in round sel + 1 every factor's pair is (entry at
    -sel p, p - 1), or the other way round -- no factor near 0.  sel = 10: 16 pairs, the largest sum lazy_sum_needs_reduce leaves lazy; sel = 13
    and 14: the widest lines, -(n (sel + 1) - 1) p at the outermost node, n = ceil(M / 2) -- 59 p for M = 8 and, were the entries left lazy,
    89 p for M = 12, where a chain of fe_muls grows by 89 / 70.66 a factor and leaves int32 (tests/test_fe_model_host.py); k_tail_slices<12>
    makes its entries canonical in the bind that could put a line beyond 70 p (kernels.h: line_needs_canonical)"""
    tabs, chal = all_selectors(ALL_NV, M, sel, orient)
    interactive(ALL_NV, [list(range(M))], tabs, chal, lazy_big_binds=0)  # (k_tail_slices<12> from nine multiplicands on: launch_tail_slices)


@pytest.mark.parametrize("shapes", [[[0] * 12], [[0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2]]], ids=["0^12", "0^4-1^4-2^4"])
def test_powers_of_selectors_through_the_resident_slices(shapes):
    """the exponent loop of the same chain: twelve multiplicands from one table and from three, sel = 14"""
    tabs, chal = all_selectors(ALL_NV, n_tables(shapes), 14, "up")
    interactive(ALL_NV, shapes, tabs, chal, lazy_big_binds=0)


def test_a_product_of_twelve_selectors_beside_a_product_of_two():
    """[[0 .. 11], [0, 1]] at sel = 13: two products under kSlots = 12, 13 + 3 combinations sharing a block's lanes"""
    tabs, chal = all_selectors(ALL_NV, 12, 13, "down")
    interactive(ALL_NV, [list(range(12)), [0, 1]], tabs, chal, lazy_big_binds=0)


def test_a_product_of_twelve_selectors_at_the_smallest_nv_that_overflows():
    """nv = 14, sel = 13: the last round of a tail of 2^13 pairs -- 13 lazy binds put the line at -83 p and limb 8 of the running product
    outside int32 in the model"""
    tabs, chal = all_selectors(14, 12, 13, "up")
    interactive(14, [list(range(12))], tabs, chal, lazy_big_binds=0)


@pytest.mark.parametrize("policy,resident", [({"tail_slices": 0}, "resident.rounds"), ({"pipeline": 0}, None)], ids=["tail_rounds", "launches"])
def test_a_product_of_twelve_selectors_on_the_paths_that_rebuild_canonical_tables(policy, resident):
    """M = 12, sel = 14 again where no entry is ever lazy: k_tail_rounds (tables through memory, canonical) and plain launches (no kernel
    waits for the host).  The same inputs and the same oracle messages as the resident-slices case: what tells a wrong kernel from a wrong test"""
    tabs, chal = all_selectors(ALL_NV, 12, 14, "up")
    with _lib.policy(**policy):
        interactive(ALL_NV, [list(range(12))], tabs, chal, lazy_big_binds=0, resident=resident)


# ---- whole-table consumers at the sinking point ------------------------------------------------------------------------------------------------
def family_tables(nv, s):
    return [sinking(nv, s, 0), sinking(nv, s, 1), selector(nv, s, nv // 2, 2, False), selector(nv, s, 1, 3, True)]


@pytest.mark.parametrize("device", [DEV, None], ids=["device", "host"])
def test_fix_variables_at_the_sinking_point(device):
    nv = 12
    s, r = fm.sinking_challenges(nv, 69000)
    point = H.mont_challenges(r)
    for tab in family_tables(nv, s):
        src = torch.from_numpy(tab.view(np.int64)).to(device) if device else tab
        mle = sc.DenseMultilinearExtension(nv, src)
        for k in (nv, nv - 5):
            got = mle.fix_variables(point[:k]).evaluations
            got = got.cpu().numpy().view(np.uint64) if device else got
            assert np.array_equal(got.reshape(-1, 4), cref.fix_variables(tab, point[:k])), f"k = {k}"


def test_poly_evaluate_at_the_sinking_point():
    nv, shapes = 16, [[0, 1, 2], [1, 3], [0]]
    s, r = fm.sinking_challenges(nv, 70000)
    point = H.mont_challenges(r)
    tabs = family_tables(nv, s)
    coefs = cref.synth_table(70001, 1000, len(shapes))
    desc = H.desc_from(nv, shapes, tabs, coefs)
    value, tv = poly_of(nv, shapes, tabs, coefs).evaluate_with_tables(point)
    for u, t in enumerate(desc.tables):
        assert np.array_equal(tv[u], cref.fix_variables(t, point)[0]), f"table {u}"
    assert np.array_equal(value, cref.poly_evaluate(desc, point))


def test_evaluate_batch_at_the_sinking_points_both_plans():
    nv, shapes, n = 14, [[0, 1, 2], [1, 3], [0]], 2
    polys, descs, points = [], [], []
    for i in range(n):
        s, r = fm.sinking_challenges(nv, 71000 + i)
        tabs = family_tables(nv, s)
        coefs = cref.synth_table(71100 + i, 1000, len(shapes))
        descs.append(H.desc_from(nv, shapes, tabs, coefs))
        polys.append(poly_of(nv, shapes, tabs, coefs))
        points.append(H.mont_challenges(r))
    points = np.stack(points)
    want_v = [cref.poly_evaluate(d, pt) for d, pt in zip(descs, points)]
    want_t = [np.stack([cref.fix_variables(t, pt).reshape(4) for t in d.tables]) for d, pt in zip(descs, points)]
    for pol, name in ((2, "batch.eval_one_block"), (0, "batch.eval_serial")):
        with _lib.policy(batch=pol):
            before = _lib.plan_stats()[name]
            got, tv = sc.ListOfProductsOfPolynomials.evaluate_batch(polys, points, return_table_values=True)
            assert _lib.plan_stats()[name] == before + 1, name
        for i in range(n):
            assert np.array_equal(tv[i], want_t[i]), f"{name}: table values of instance {i}"
            assert np.array_equal(got[i], want_v[i]), f"{name}: value of instance {i}"
