"""Sums at the top limb's bound, end to end.  The LDS-resident kernels add a combination's products lazily; the int32 top limb of ONE
accumulator holds 282 products of magnitude p (kernels.h: kLazySumMaxP).  Random tables sit far inside that (a sum of n products is about
n p / 2); these tables put EVERY product at the end of fe_mul's window (1 - p), or at the largest canonical value, in the shapes whose
blocks hold 256 and more pairs.  Each proof is compared bit for bit with the oracle's (cref.ml_prove / cref.gkr_prove) and verified."""
import numpy as np
import pytest
import torch

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib
from tests import fe_model as fm
from tests import helpers as H
from tests import test_gpu_gkr_batch as G

pytestmark = pytest.mark.gpu
P = fm.P
N_INST = 2


def raw(v: int) -> np.ndarray:
    """the table entry whose stored (Montgomery) limbs are the integer v"""
    assert 0 <= v < P
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


ONE = 1                          # raw limbs 1
C261 = (1 << fm.K) % P           # raw limbs 2^261 mod p: fe_mul(1, C261) = fe_mul(C261, 1 - p) = 1 - p, the lower end of fe_mul's window
MINUS_ONE = (P - 1) * fm.R256 % P  # the field's p - 1 as the tables store it: 0.79 p
assert fm.value(fm.fe_mul(fm.limbs_of(C261), fm.limbs_of(ONE))) == 1 - P
assert fm.value(fm.fe_mul(fm.limbs_of(C261), fm.limbs_of(1 - P))) == 1 - P


def const_table(nv, v, live=None):
    t = np.zeros((1 << nv, 4), dtype=np.uint64)
    t[:(1 << nv) if live is None else live] = raw(v)
    return t


def tables_for(case, nv):
    n = 1 << nv
    if case == "all-1-p":
        return [const_table(nv, ONE), const_table(nv, C261), const_table(nv, C261)]
    if case == "all-p-1":
        return [const_table(nv, MINUS_ONE)] * 3
    if case == "half-1-p":  # the first half of the pairs at the bound, the second half 0: the lanes differ
        return [const_table(nv, ONE, n // 2), const_table(nv, C261, n // 2), const_table(nv, C261, n // 2)]
    if case == "half-p-1":
        return [const_table(nv, MINUS_ONE, n // 2)] * 3
    if case == "alt":  # entries alternate between p - 1 and 0, the other table the other way round: every slope is +-(p - 1)
        a, b = const_table(nv, P - 1), const_table(nv, P - 1)
        a[1::2] = 0
        b[0::2] = 0
        return [a, b, a]
    if case == "random":
        return [cref.synth_table(fm.SEED, 70 + s, n) for s in range(3)]
    raise ValueError(case)


CASES = [
    ([[0, 1]], 10, "all-1-p"), ([[0, 1]], 10, "all-p-1"), ([[0, 1]], 10, "half-1-p"), ([[0, 1]], 10, "half-p-1"),
    ([[0, 1]], 9, "all-1-p"), ([[0, 1]], 9, "all-p-1"), ([[0, 1]], 9, "half-1-p"), ([[0, 1]], 9, "half-p-1"),
    ([[0]], 10, "all-p-1"), ([[0]], 11, "random"), ([[0]], 11, "all-p-1"),
    ([[0], [1]], 10, "all-p-1"),
    ([[0, 1, 2]], 9, "all-1-p"),
]


def _ml_case(shapes, nv, case, n_inst):
    nt = max(max(s) for s in shapes) + 1
    polys, wants, evals = [], [], []
    for i in range(n_inst):
        tabs = tables_for(case, nv)[:nt]
        if case == "random" and i:
            tabs = [cref.synth_table(fm.SEED + i, 70 + s, 1 << nv) for s in range(nt)]
        coefs = cref.synth_table(fm.SEED + 13 * i, 1000, len(shapes))
        wants.append(cref.ml_prove(H.desc_from(nv, shapes, tabs, coefs), threads=1))
        polys.append(H.hip_poly_from(nv, shapes, tabs, coefs, device="cuda:0")[0])
    torch.cuda.synchronize()
    return polys, wants


def _verify(poly, proof):
    sub = sc.MLSumcheck.verify(poly.info(), sc.MLSumcheck.extract_sum(proof), proof)
    assert np.array_equal(poly.evaluate(sub.point), sub.expected_evaluation), "the verifier's subclaim does not hold"


@pytest.mark.parametrize("shapes,nv,case", CASES, ids=lambda x: str(x).replace(" ", ""))
def test_batched_proofs_with_every_product_at_the_bound(shapes, nv, case):
    polys, wants = _ml_case(shapes, nv, case, N_INST)
    with _lib.policy(batch=2):
        before = _lib.plan_stats()["batch.one_block"]
        got, rand = sc.MLSumcheck.prove_batch(polys, return_randomness=True)
        assert _lib.plan_stats()["batch.one_block"] == before + 1, "the shape must run in the batched kernel"
    for i, (wp, wr) in enumerate(wants):
        gp = np.stack([m.evaluations for m in got[i]])
        bad = np.nonzero((gp != wp).any(axis=(1, 2)))[0] if gp.shape == wp.shape else None
        assert np.array_equal(gp, wp), f"instance {i}: proof differs from the oracle's, first in round {None if bad is None else bad[:1]}"
        assert np.array_equal(rand[i], wr), f"instance {i}: randomness differs from the oracle's"
        _verify(polys[i], got[i])


@pytest.mark.parametrize("v2,v3", [(MINUS_ONE, MINUS_ONE), (ONE, C261), (C261, C261)], ids=["p-1", "one-c261", "c261"])
def test_batched_gkr_rounds_with_constant_tables(v2, v3):
    """k_batch_gkr holds 2^9 entries per table: 256 products of two, each inside (-p, 2^251] whatever the tables hold -- the sum stays
    below kLazySumMaxP p.  Constant f2, f3 at the largest canonical value and at fe_mul's window's end, f1 dense (eight terms a cell)."""
    dim, N = 9, 1 << 9
    b = G.make_batch(N_INST, dim, 52000, nnz=8 * N)
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")
    f2, f3 = const_table(dim, v2), const_table(dim, v3)
    b["raw"] = [(idx, vals, f2, f3, g) for idx, vals, _, _, g in b["raw"]]
    b["f2s"] = [sc.DenseMultilinearExtension(dim, td(f2)) for _ in range(N_INST)]
    b["f3s"] = [sc.DenseMultilinearExtension(dim, td(f3)) for _ in range(N_INST)]
    torch.cuda.synchronize()
    want = G.oracle_all(b)
    with _lib.policy(batch=2):
        before = _lib.plan_stats()["batch.gkr_one_block"]
        G.assert_batch_equals(b, want)
        assert _lib.plan_stats()["batch.gkr_one_block"] == before + 1


@pytest.mark.parametrize("case", ["all-1-p", "all-p-1", "alt"])
def test_one_proof_through_the_tail_slices_with_256_pairs_a_block(case):
    """nv = 17, a product of two: k_tail_slices takes the proof from its first round, 2^16 pairs over 256 blocks.  Constant tables put
    nodes 0 and 1 at the bound (the slopes are 0); alternating ones node inf: every product of two slopes is -(p - 1)^2 / 2^261 - [0, p)"""
    nv, shapes = 17, [[0, 1]]
    tabs = tables_for(case, nv)[:2]
    coefs = cref.synth_table(fm.SEED, 1000, 1)
    want, _ = cref.ml_prove(H.desc_from(nv, shapes, tabs, coefs), threads=cref.max_threads())
    poly, _ = H.hip_poly_from(nv, shapes, tabs, coefs, device="cuda:0")
    before = _lib.plan_stats()["tail.slices8"]
    proof = sc.MLSumcheck.prove(poly)
    assert _lib.plan_stats()["tail.slices8"] > before, "the proof must run through k_tail_slices"
    assert np.array_equal(np.stack([m.evaluations for m in proof]), want)
    _verify(poly, proof)


def test_a_single_table_through_lazy_big_rounds_into_the_tail_slices():
    """[[0]] at nv = 22, random entries: five big rounds bind the table in the internal format (fe_mul_bind and a carry pass, no
    reduction: an entry sinks by about p / 2 a round), then k_tail_slices takes 2^16 pairs, 256 a block, each a RAW entry of about -3 p"""
    nv, shapes = 22, [[0]]
    tabs = [cref.synth_table(fm.SEED, 90, 1 << nv)]
    coefs = cref.synth_table(fm.SEED, 1000, 1)
    want, _ = cref.ml_prove(H.desc_from(nv, shapes, tabs, coefs), threads=cref.max_threads())
    poly, _ = H.hip_poly_from(nv, shapes, tabs, coefs, device="cuda:0")
    before = _lib.plan_stats()
    proof = sc.MLSumcheck.prove(poly)
    after = _lib.plan_stats()
    assert after["tail.slices8"] > before["tail.slices8"], "the proof must end in k_tail_slices"
    assert after["big.store_f29"] > before["big.store_f29"], "the big rounds must hand the tail tables in the internal format"
    got = np.stack([m.evaluations for m in proof])
    bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
    assert bad.size == 0, f"rounds {bad.tolist()} differ from the oracle's"
    _verify(poly, proof)
