"""Products of 14 to 40 multiplicands on every path that takes them.

The library accepts any max_multiplicands; beyond twelve factors no tree kernel applies and the node-by-node code is alone responsible:
k_sum_generic in the big rounds, combo_product (saturated arithmetic) inside k_sum_combos*, k_tail_rounds and the resident kernel, and the
finalize step with D = M + 1 up to 41 -- `idx / (D * D)`, one block per valid (product, node) pair, the weights at t (M + 1), nodes up to
+-20, 5 (M - 1) doublings of the coefficient.  Every host-side switch that reads D is crossed here by raising the degree of ONE product:

  sum of (M_k + 1) <= kMetaCombos = 24   M = 23 | 24   the persistent kernels (k_tail_rounds, the resident kernel) and small.launched against
                                                        small.combos_table
  K D (D + 2) 32 <= 48 KiB               M = 37 | 38   finalize.multi_block against finalize.no_lds
  more than kMaxSmallTables = 32 tables  40 tables     small.ptrs
  the verifier's interpolation tiers     D = 20, 33    sc_ml_verify on proofs the GPU produced

tests/high_degree_cases.py builds the shapes and states these inequalities; tests/test_high_degree_host.py checks them, and the C oracle
against big integers at these degrees, without a GPU.  Every comparison below is bit for bit with the oracle: every message of every round,
the bound tables after rounds 1, 2 and nv, whole Fiat-Shamir proofs and their challenges; every test names the plan counters it moves."""
import threading

import numpy as np
import pytest
import torch

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib, sharded
from tests import helpers as H
from tests import high_degree_cases as HD
from tests.test_gpu_sharded import _thread_rank

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VM = sc.VerifierMsg
SEED = 0x4D00
EXPORT = lambda nv: (1, 2, nv)  # noqa: E731  the rounds after which the bound tables are compared


def moved_since(before):
    after = _lib.plan_stats()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def none_moved(moved, *prefixes):
    return not any(k.startswith(p) for k in moved for p in prefixes)


def oracle_rounds(desc, chal, export_after):
    """the oracle's messages under the given challenges -> (messages, {round: its tables after that round})"""
    nv = desc.num_vars
    op = cref.Prover(desc, threads=cref.max_threads())
    want, otabs = [], {}
    for j in range(nv):
        want.append(op.prove_round(None if j == 0 else chal[j - 1]))
        if j + 1 in export_after:
            otabs[j + 1] = op.state()[1]
    op.close()
    return want, otabs


def drive(st, nv, chal, want, otabs):
    """rounds 1 .. nv through sc_prove_round: every message, and the tables after the rounds of `otabs`, against the oracle's
    -> the plan counters each round's call moved"""
    per_round = []
    for j in range(nv):
        before = _lib.plan_stats()
        got = sc.IPForMLSumcheck.prove_round(st, None if j == 0 else VM(chal[j - 1])).evaluations
        per_round.append(moved_since(before))
        assert np.array_equal(got, want[j]), f"round {j + 1}"
        if j + 1 in otabs:
            tabs = st.flattened_ml_extensions
            assert len(tabs) == len(otabs[j + 1])
            for u, t in enumerate(tabs):
                assert np.array_equal(t.evaluations, otabs[j + 1][u]), f"table {u} after round {j + 1}"
    assert st.round == nv and np.array_equal(st.randomness, chal[: nv - 1])
    return per_round


def rounds_then_proof(nv, shapes, tabs, coefs, chal, proof=True):
    """One borrowed handle over device tables: the interactive rounds under `chal` against cref.Prover, then reset and the whole
    Fiat-Shamir proof against cref.ml_prove -> (counters of the interactive pass, per round, counters of the proof)"""
    desc = H.desc_from(nv, shapes, tabs, coefs)
    want, otabs = oracle_rounds(desc, chal, EXPORT(nv))
    poly, _ = H.hip_poly_from(nv, shapes, tabs, coefs, device=DEV)
    torch.cuda.synchronize()
    st = sc.IPForMLSumcheck.prover_init(poly, borrow=True)
    before = _lib.plan_stats()
    per_round = drive(st, nv, chal, want, otabs)
    inter = moved_since(before)
    whole = None
    if proof:
        pwant, prand = cref.ml_prove(desc, threads=cref.max_threads())
        before = _lib.plan_stats()
        st.reset()
        got = st.prove()
        whole = moved_since(before)
        assert np.array_equal(got, pwant), "the Fiat-Shamir proof differs from the oracle's"
        assert np.array_equal(st.randomness, prand)
    st.close()
    print(f"\nnv {nv} D {HD.degree(shapes)} K {len(shapes)} U {HD.n_tables(shapes)}: interactive {inter}; proof {whole}")
    return inter, per_round, whole


# ---- 1: the degree ladder in the latency-bound rounds ------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", HD.LADDER)
def test_degree_ladder_in_the_latency_bound_rounds(M):
    """nv = 11: every round has at most 2^10 pairs.  Up to M = 23 the round metadata fits a kernel argument (M + 1 <= kMetaCombos): the
    interactive rounds may be served by the resident k_tail_rounds and a whole proof is ONE launch of k_tail_rounds -- never of k_tail_slices,
    which takes at most twelve multiplicands.  From M = 24 on no persistent kernel applies: launches round by round, each with its finalize
    (k_finalize_mb while D (D + 2) 32 <= 48 KiB, M <= 37; k_finalize<false, false> beyond)."""
    nv = HD.LADDER_NV
    shapes, _ = HD.one_product(M)
    tabs, coefs = HD.synth_case(nv, shapes, SEED + M)
    inter, _, whole = rounds_then_proof(nv, shapes, tabs, coefs, cref.synth_table(SEED + 1, M, nv))
    assert HD.tail_shape_ok(shapes) == (M <= 23) and not HD.tail_slices_ok(shapes)
    for moved in (inter, whole):
        assert none_moved(moved, "tail.slices", "resident.slices", "big."), moved
    if M <= 23:
        assert whole == {"tail.rounds": 1}, whole  # the whole proof is one launch
    else:
        fin = HD.finalize_plan(shapes)
        for moved in (inter, whole):
            assert none_moved(moved, "tail.", "resident."), moved
            assert moved.get(fin, 0) == nv and {k for k in moved if k.startswith("finalize.")} == {fin}, moved
        assert inter.get("small.combos_table", 0) == nv and "small.launched" not in inter, inter
        assert whole.get("small.combos_table", 0) + whole.get("small.pipelined", 0) == nv and "small.launched" not in whole, whole


@pytest.mark.parametrize("M", HD.PLAIN_LAUNCHES)
def test_degree_thresholds_as_plain_launches(M):
    """pipeline = 0: no device-side wait, so every round of either pass is k_fix_multi + a sum kernel + a finalize, launched after its
    challenge.  M = 23 | 24: k_sum_combos_meta against k_sum_combos; M = 37 | 38: k_finalize_mb (38 blocks for the one product, then the
    message from 38 x 38 weights out of LDS) against the finalize without LDS."""
    nv = HD.LADDER_NV
    shapes, _ = HD.one_product(M)
    tabs, coefs = HD.synth_case(nv, shapes, SEED + M)
    with _lib.policy(pipeline=0):
        inter, per_round, whole = rounds_then_proof(nv, shapes, tabs, coefs, cref.synth_table(SEED + 2, M, nv))
    small, fin = HD.small_plan(shapes), HD.finalize_plan(shapes)
    assert small == ("small.launched" if M <= 23 else "small.combos_table") and fin == ("finalize.multi_block" if M <= 37 else "finalize.no_lds")
    for j, moved in enumerate(per_round):
        assert moved == {small: 1, fin: 1}, f"round {j + 1}: {moved}"
    assert inter == whole == {small: nv, fin: nv}, (inter, whole)


# ---- 2: the same through the big rounds --------------------------------------------------------------------------------------------------
def assert_big_round_plans(name, per_round, inter, whole):
    mixed = name == "mixed-D21"
    per_pass = {"big.generic": 2, "big.bind_pass": 1}
    if mixed:
        per_pass.update({"big.wide16": 2, "big.per_product_tree": 4})
    for moved in (inter, whole):
        if moved is None:
            continue
        assert {k: v for k, v in moved.items() if k.startswith("big.")} == per_pass, moved
    trees = {"big.wide16": 1, "big.per_product_tree": 2} if mixed else {}
    big = [{k: v for k, v in m.items() if k.startswith("big.")} for m in per_round]
    assert big[0] == {"big.generic": 1, **trees}, big[0]
    assert big[1] == {"big.generic": 1, "big.bind_pass": 1, **trees}, big[1]
    assert not any(big[2:]), big[2:]


@pytest.mark.parametrize("name", list(HD.BIG_SHAPES))
def test_generic_products_through_the_big_rounds(name):
    """nv = 17: rounds 1 and 2 (2^16 and 2^15 pairs) are big.  A product beyond twelve multiplicands is k_sum_generic over tables that
    k_fix_multi bound up front in round 2 (big.bind_pass); repeated tables run the exponent loop (24 over 16: squares; 38 over 32).  The
    mixed list puts k_sum_generic's unscaled sums beside the sums of two trees and of a wide16 product, which carry 2^(-5(M - 1)), in ONE
    finalize (D = 21, K = 4: 61 824 bytes of node sums, without LDS).  No merged launch, no plain wide tree, nothing lags."""
    nv = HD.BIG_NV
    shapes, _ = HD.BIG_SHAPES[name]
    tabs, coefs = HD.synth_case(nv, shapes, SEED + 0x100 + len(shapes[0]))
    # the 38-factor oracle alone is 1.6 s a pass: the interactive pass covers its rounds
    inter, per_round, whole = rounds_then_proof(nv, shapes, tabs, coefs, cref.synth_table(SEED + 3, len(shapes[0]), nv), proof=name != "38-over-32")
    assert_big_round_plans(name, per_round, inter, whole)
    fin = HD.finalize_plan(shapes)
    assert per_round[0].get(fin, 0) == 1 and per_round[1].get(fin, 0) == 1, per_round[:2]


def test_fourteen_factors_through_the_big_rounds_without_the_wide_trees():
    """wide_tree = 0 changes nothing for a product beyond twelve: the same launches, the same bits"""
    nv, name = HD.BIG_NV, "14-distinct"
    shapes, _ = HD.BIG_SHAPES[name]
    tabs, coefs = HD.synth_case(nv, shapes, SEED + 0x100 + len(shapes[0]))
    with _lib.policy(wide_tree=0):
        inter, per_round, whole = rounds_then_proof(nv, shapes, tabs, coefs, cref.synth_table(SEED + 4, 14, nv))
    assert_big_round_plans(name, per_round, inter, whole)


# ---- 3: exponents, many tables, extremes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HD.EXPONENT_SHAPES))
def test_long_exponent_loops(name):
    """one table to the 33rd power, and a 20th power times a 13th: combo_product's `first` hand-over and its slot_exp loop far beyond the
    exponent 10 other tests reach.  D = 34: no persistent kernel, k_finalize_mb (34 x 36 x 32 bytes)."""
    nv = 12
    shapes, _ = HD.EXPONENT_SHAPES[name]
    tabs, coefs = HD.synth_case(nv, shapes, SEED + 0x200 + len(name))
    inter, _, whole = rounds_then_proof(nv, shapes, tabs, coefs, cref.synth_table(SEED + 5, len(name), nv))
    for moved in (inter, whole):
        assert none_moved(moved, "tail.", "resident.", "big."), moved
        assert moved.get("finalize.multi_block", 0) == nv and "finalize.no_lds" not in moved and "finalize.one_block" not in moved, moved
        assert "small.launched" not in moved, moved


def test_forty_factors_over_forty_tables():
    """more than kMaxSmallTables tables: the pointers go through device memory (k_sum_combos_ptrs) in every round of either pass, the bound
    tables stay in the reference layout, nothing is pipelined and no persistent kernel applies; D = 41 finalizes without LDS"""
    nv = 10
    shapes, _ = HD.FORTY_TABLES
    tabs, coefs = HD.synth_case(nv, shapes, SEED + 0x300)
    inter, per_round, whole = rounds_then_proof(nv, shapes, tabs, coefs, cref.synth_table(SEED + 6, 40, nv))
    for j, moved in enumerate(per_round):
        assert moved == {"small.ptrs": 1, "finalize.no_lds": 1}, f"round {j + 1}: {moved}"
    assert inter == whole == {"small.ptrs": nv, "finalize.no_lds": nv}, (inter, whole)


@pytest.mark.parametrize("pipeline", [1, 0], ids=["default", "plain-launches"])
@pytest.mark.parametrize("M,all_top", [(20, False), (38, False), (20, True), (38, True)], ids=["M20", "M38", "M20-all-p-1", "M38-all-p-1"])
def test_extreme_entries_and_challenges(M, all_top, pipeline):
    """every STORED table entry from {0, 1, p - 1} -- or every one p - 1 -- and the challenges 0, 1, p - 1 in turn: the lines at nodes up to
    +-10 (M = 20) and +-19 (M = 38) through entries at both ends of the field, and the products of up to 38 such values, in the saturated
    arithmetic; then a Fiat-Shamir proof over the same tables"""
    nv = 12
    shapes, nt = HD.one_product(M)
    tabs = HD.extreme_tables(nv, nt, SEED + M, all_top)
    coefs = cref.synth_table(SEED + 7, 1000, 1)
    with _lib.policy(pipeline=pipeline):
        inter, _, whole = rounds_then_proof(nv, shapes, tabs, coefs, HD.extreme_challenges(nv))
    for moved in (inter, whole):
        assert none_moved(moved, "tail.slices", "resident.slices", "big."), moved
        if not pipeline:
            assert moved == {HD.small_plan(shapes): nv, HD.finalize_plan(shapes): nv}, moved
        elif not HD.tail_shape_ok(shapes):  # M = 38: launches round by round, each with the finalize without LDS
            assert none_moved(moved, "tail.", "resident.") and {k: v for k, v in moved.items() if k.startswith("finalize.")} == {HD.finalize_plan(shapes): nv}, moved


# ---- 4: the verifier on real proofs ------------------------------------------------------------------------------------------------------
def flip_one_limb(proof, j, t, limb=0):
    bad = [sc.ProverMsg(m.evaluations.copy()) for m in proof]
    bad[j].evaluations[t, limb] ^= np.uint64(1)
    return bad


@pytest.mark.parametrize("M", HD.LADDER)
def test_verifier_on_proofs_from_the_gpu(M):
    """MLSumcheck.prove -> MLSumcheck.verify for D = 15 .. 41: the reference's interpolate_uni_poly switches its arithmetic at 20 and at 33
    evaluation points (u64, u128, field elements).  The proof is the oracle's, the verifier accepts it, the subclaim is the oracle's, the
    polynomial has the expected value at the subclaim's point (the reference's own test), and every round's interpolation equals the
    oracle's.  At D = 21 and D = 34 one flipped bit in a middle round's message is rejected."""
    nv = HD.LADDER_NV
    shapes, _ = HD.one_product(M)
    tabs, coefs = HD.synth_case(nv, shapes, SEED + M)
    desc = H.desc_from(nv, shapes, tabs, coefs)
    pwant, prand = cref.ml_prove(desc, threads=cref.max_threads())
    poly, _ = H.hip_poly_from(nv, shapes, tabs, coefs, device=DEV)
    torch.cuda.synchronize()
    proof = sc.MLSumcheck.prove(poly)
    assert np.array_equal(np.stack([m.evaluations for m in proof]), pwant), "the Fiat-Shamir proof differs from the oracle's"
    claim = sc.MLSumcheck.extract_sum(proof)
    sub = sc.MLSumcheck.verify(poly.info(), claim, proof)
    ok, opoint, oexp = cref.ml_verify((M, nv), claim, pwant)
    assert ok and np.array_equal(sub.point, opoint) and np.array_equal(sub.point, prand) and np.array_equal(sub.expected_evaluation, oexp)
    value = poly.evaluate(sub.point)
    assert np.array_equal(value, sub.expected_evaluation) and np.array_equal(value, cref.poly_evaluate(desc, sub.point))
    for j in range(nv):
        assert np.array_equal(sc.interpolate_uni_poly(proof[j].evaluations, prand[j]), cref.interpolate_uni_poly(pwant[j], prand[j])), f"round {j + 1}"
    if M + 1 in (21, 34):
        j, t = nv // 2, (M + 1) // 2
        bad = flip_one_limb(proof, j, t)
        with pytest.raises(sc.SumcheckError, match="Prover message is not consistent with the claim"):
            sc.MLSumcheck.verify(poly.info(), claim, bad)
        assert not cref.ml_verify((M, nv), claim, np.stack([m.evaluations for m in bad]))[0], "the oracle's verifier rejects it too"
        with pytest.raises(sc.SumcheckError, match="Prover message is not consistent with the claim"):
            sc.MLSumcheck.verify(poly.info(), claim, flip_one_limb(proof, j, 0, limb=3))  # ... and in node 0, where the round's own check sees it


# ---- 5: the other entry points, fourteen multiplicands each ------------------------------------------------------------------------------
FOURTEEN = [list(range(14))]


def test_resident_kernel_on_fourteen_factors():
    """nv = 13: from round 2 on (2^11 pairs) the interactive rounds are served by the resident kernel -- k_tail_rounds, D = 15 node sums a
    round in flat mode and through finalize_body; the slices never take more than twelve multiplicands.  Back to back, with the tables
    exported in between (the kernel is asked to leave and started again), and once more after a reset."""
    nv = 13
    tabs, coefs = HD.synth_case(nv, FOURTEEN, SEED + 0x500)
    chal = cref.synth_table(SEED + 8, 14, nv)
    desc = H.desc_from(nv, FOURTEEN, tabs, coefs)
    want, otabs = oracle_rounds(desc, chal, (1, 2, nv - 4, nv))
    poly, _ = H.hip_poly_from(nv, FOURTEEN, tabs, coefs, device=DEV)
    torch.cuda.synchronize()
    st = sc.IPForMLSumcheck.prover_init(poly, borrow=True)
    before = _lib.plan_stats()
    drive(st, nv, chal, want, {})
    back_to_back = moved_since(before)
    st.reset()
    before = _lib.plan_stats()
    drive(st, nv, chal, want, otabs)
    with_exports = moved_since(before)
    st.close()
    print(f"\nresident, M = 14: back to back {back_to_back}; with exports {with_exports}")
    for moved in (back_to_back, with_exports):
        assert moved.get("resident.rounds", 0) >= 1 and none_moved(moved, "resident.slices", "tail."), moved
    assert with_exports["resident.rounds"] >= 3, "the exports after rounds 2 and nv - 4 make the kernel leave; the next round starts it again"


def test_streamed_handle_on_fourteen_factors():
    """nv = 13, chunks of 2^11 entries: rounds 1 and 2 walk the host tables in four chunks, k_sum_generic over per-chunk pointer sets and a
    D = 15 message accumulated per chunk; the tables after rounds 1, 2, 3, proofs twice on the rewound handle, the inputs only read"""
    nv, chunk = 13, 11
    tabs, coefs = HD.synth_case(nv, FOURTEEN, SEED + 0x600)
    chal = cref.synth_table(SEED + 9, 14, nv)
    desc = H.desc_from(nv, FOURTEEN, tabs, coefs)
    want, otabs = oracle_rounds(desc, chal, (1, 2, 3, nv))
    pwant, prand = cref.ml_prove(desc, threads=cref.max_threads())
    poly, mles = H.hip_poly_from(nv, FOURTEEN, [t.copy() for t in tabs], coefs)
    before = _lib.plan_stats()
    st = sc.IPForMLSumcheck.prover_init(poly, streamed_chunk_log2=chunk)
    per_round = drive(st, nv, chal, want, otabs)
    assert per_round[0].get("big.streamed", 0) == 1 and per_round[1].get("big.streamed", 0) == 1 and not any("big.streamed" in m for m in per_round[2:]), per_round
    for _ in range(2):
        st.reset()
        assert np.array_equal(st.prove(sc.Blake2b512Rng.setup()), pwant)
    assert np.array_equal(st.randomness, prand)
    st.close()
    print(f"\nstreamed, M = 14: {moved_since(before)}")
    for m, t in zip(mles, tabs):
        assert np.array_equal(m.evaluations, t)


def test_sharded_proof_on_fourteen_factors():
    """two thread ranks over the host transport at nv = 13: every local round's partial message is D x 8 = 120 widened lanes (104 at most in
    any other test), all-reduced by the caller's transport; the proof and its challenges are the unsharded oracle's on both ranks, twice"""
    G, nv = 2, 13
    tabs, coefs = HD.synth_case(nv, FOURTEEN, SEED + 0x700)
    want, wrand = cref.ml_prove(H.desc_from(nv, FOURTEEN, tabs, coefs), threads=cref.max_threads())
    ex = sharded.ThreadExchange(G)
    out = [None] * G
    before = _lib.plan_stats()
    ts = [threading.Thread(target=_thread_rank, args=(r, G, nv, FOURTEEN, tabs, coefs, ex.comm, 0, out)) for r in range(G)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=600)
    moved = moved_since(before)
    for r in range(G):
        assert not isinstance(out[r], Exception), out[r]
        for proof, rand in out[r]:
            assert np.array_equal(proof, want), f"rank {r}"
            assert np.array_equal(rand, wrand), f"rank {r}"
    print(f"\nsharded, M = 14: {moved}")
    assert moved.get("sharded.host", 0) > 0 and none_moved(moved, "sharded.rccl", "sharded.p2p"), moved


def batch_of(n, nv, shapes, seed, device=None):
    polys, descs, keep = [], [], []
    for i in range(n):
        tabs, coefs = HD.synth_case(nv, shapes, seed + i)
        poly, mles = H.hip_poly_from(nv, shapes, tabs, coefs, device=device)
        polys.append(poly)
        descs.append(H.desc_from(nv, shapes, tabs, coefs))
        keep.append(mles)
    return polys, descs, keep


def test_batched_entry_points_take_the_serial_plan_on_fourteen_factors():
    """n = 3 at nv = 6 under batch = 2 (the batched kernels for every n that fits): fourteen multiplicands are beyond kMaxFusedM, so
    sc_ml_prove_batch proves instance after instance and the batch handle runs three ordinary provers -- with the oracle's bits"""
    n, nv = 3, 6
    polys, descs, _keep = batch_of(n, nv, FOURTEEN, SEED + 0x800)
    want = [cref.ml_prove(d, threads=2) for d in descs]
    chal = cref.synth_table(SEED + 10, 77, n * nv).reshape(nv, n, 4)  # challenge [j][i] follows message j of instance i
    with _lib.policy(batch=2):
        before = _lib.plan_stats()
        got, rand = sc.MLSumcheck.prove_batch(polys, return_randomness=True)
        moved = moved_since(before)
        assert moved.get("batch.serial", 0) == 1 and "batch.one_block" not in moved, moved
        for i in range(n):
            assert np.array_equal(np.stack([m.evaluations for m in got[i]]), want[i][0]), f"instance {i}"
            assert np.array_equal(rand[i], want[i][1]), f"instance {i}"
        before = _lib.plan_stats()
        st = sc.IPForMLSumcheck.prover_init_batch(polys)
        provers = [cref.Prover(d, threads=1) for d in descs]
        for j in range(nv):
            msgs = sc.IPForMLSumcheck.prove_round_batch(st, None if j == 0 else [VM(chal[j - 1][i]) for i in range(n)])
            for i, p in enumerate(provers):
                assert np.array_equal(msgs[i].evaluations, p.prove_round(None if j == 0 else chal[j - 1][i])), f"round {j + 1}, instance {i}"
            if j + 1 in EXPORT(nv):
                for i, p in enumerate(provers):
                    orand, otabs, ornd = p.state()
                    assert st.round == ornd and np.array_equal(st.randomness(i), orand)
                    for u, t in enumerate(st.flattened_ml_extensions(i)):
                        assert np.array_equal(np.asarray(t.evaluations), otabs[u]), f"table {u} of instance {i} after round {j + 1}"
        st.close()
        moved = moved_since(before)
    assert moved.get("batch.rounds_serial", 0) == nv and "batch.rounds_one_block" not in moved and "batch.rounds_slices" not in moved, moved


@pytest.mark.parametrize("batch", [2, 0], ids=["batched", "serial"])
def test_evaluate_batch_on_forty_factors(batch):
    """sc_poly_evaluate_batch on 40 factors over 32 tables at nv = 6: the 40 scalar products per instance (eight tables enter twice) on the
    library's host side; the values and every table's evaluation are the oracle's"""
    n, nv = 3, 6
    shapes, nt = HD.one_product(40)
    polys, descs, _keep = batch_of(n, nv, shapes, SEED + 0x900, device=DEV)
    torch.cuda.synchronize()
    points = cref.synth_table(SEED + 11, 5, n * nv).reshape(n, nv, 4)
    with _lib.policy(batch=batch):
        before = _lib.plan_stats()
        vals, tvals = sc.ListOfProductsOfPolynomials.evaluate_batch(polys, points, return_table_values=True)
        moved = moved_since(before)
    for i, d in enumerate(descs):
        assert np.array_equal(vals[i], cref.poly_evaluate(d, points[i])), f"instance {i}"
        assert np.array_equal(polys[i].evaluate(points[i]), vals[i]), f"instance {i}: evaluate_batch against evaluate"
        for u in range(nt):
            assert np.array_equal(tvals[i, u], cref.fix_variables(d.tables[u], points[i]).reshape(4)), f"instance {i}, table {u}"
    assert moved.get("batch.eval_one_block" if batch else "batch.eval_serial", 0) == 1 and ("batch.eval_serial" if batch else "batch.eval_one_block") not in moved, moved
