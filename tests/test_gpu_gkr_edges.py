"""The single-instance GKR round (sumcheck_amd/csrc/gkr.hip: sc_gkr_phase_one, sc_gkr_phase_two, sc_gkr_prove) where its route changes, at its
largest dims and at the ends of the range -- the inputs are tests/gkr_edge_cases.py's, which states for each why it runs where it does:

  a  the sparse switch at dim 11: 127 non-zeros take the list form with eq evaluated per entry (k_sparse_scale_direct), 128 are bucketed;
  b  sparse lists at dims 13, 17 and 21: that kernel with k up to 21 and 63-bit sort keys, index 0 and index 2^(3 dim) - 1 among them;
  c  12000 non-zeros on 4 (x, y): phase one folds with the eq table, phase two -- n1 = 4 -- with the direct evaluation;
  d  dense lists at dims 17, 19 and 21 (bucket widths 6, 8 and 10 bits; 21 is the last dim: 64 KiB of LDS per workgroup, kMaxBuckets buckets);
  e  a bucket at exactly its cap (taken) and one entry over (refused by k_bucket_skew and k_bucket_accumulate: the list form, same bits), for
     both arms of the cap, max(8192, 64 (n / nb + 1)), and for phase two alone;
  f  8192 terms with the limbs of p - 1 in one LDS cell, and 8193 of them through the list form's reduce_by_key;
  g  g, u from {0, 1, p - 1}, f2 and f3 from {0, 1, p - 1}, values half of them 0, 1 or p - 1: most of eq is 0, and f1(g, ., .) comes back with
     its zero-valued entries where the oracle lists them.

Every case: initialize_phase_one (h_g, and f1(g, ., .) as indices and values), initialize_phase_two under the case's u, and
GKRRoundSumcheck.prove (all 2 dim messages; (u, v) through verify), each bit for bit against oracle/cref.py, from host arrays and from
device-resident tensors.  Around each call the gkr.* plan counters are read: the case names the ones that move and by how much, and no other may."""
import contextlib

import numpy as np
import pytest
import torch

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib
from tests import gkr_edge_cases as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def gkr_plans():
    return {k: v for k, v in _lib.plan_stats().items() if k.startswith("gkr.")}


@contextlib.contextmanager
def moves(expect, what):
    before = gkr_plans()
    yield
    after = gkr_plans()
    got = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    assert got == expect, f"{what}: the gkr.* plans that moved"


def to_dev(a):
    return torch.from_numpy(np.array(a).view(np.int64)).to(DEV)  # (a copy: the case's arrays are read-only)


def to_host(a):
    return a.cpu().numpy().view(np.uint64) if torch.is_tensor(a) else a


def reversed_list(f1_g):
    if f1_g.on_device:
        return sc.SparseMultilinearExtension(f1_g.num_vars, f1_g.indices.flip(0).contiguous(), f1_g.values.flip(0).contiguous())
    return sc.SparseMultilinearExtension(f1_g.num_vars, f1_g.indices[::-1].copy(), f1_g.values[::-1].copy())


@pytest.mark.parametrize("name", E.NAMES)
def test_gkr_round_at_its_edges(name):
    c = E.build(name)
    dim = c.dim
    oi, ov = c.oracle_f1()
    wh, wi, wv = cref.gkr_phase_one(oi, ov, dim, c.f3, c.g)
    assert wi.shape[0] == c.n1
    w2 = cref.gkr_phase_two(wi, wv, dim, c.u)
    want, wuv = cref.gkr_prove(oi, ov, dim, c.f2, c.f3, c.g, threads=cref.max_threads())
    with _lib.policy(gkr_direct=c.gkr_direct):
        for where in ("host", "device"):
            put = to_dev if where == "device" else (lambda a: a)
            f1 = sc.SparseMultilinearExtension(3 * dim, put(c.idx), put(c.vals))
            m2, m3 = sc.DenseMultilinearExtension(dim, put(c.f2)), sc.DenseMultilinearExtension(dim, put(c.f3))
            with moves(c.expect["phase_one"], f"{name}, {where}, initialize_phase_one"):
                h_g, f1_g = sc.initialize_phase_one(f1, m3, c.g)
            assert f1_g.indices.shape[0] == c.n1, where
            assert np.array_equal(to_host(f1_g.indices).reshape(-1), wi) and np.array_equal(to_host(f1_g.values).reshape(-1, 4), wv), f"{where}: f1(g, ., .)"
            assert np.array_equal(to_host(h_g.evaluations), wh), f"{where}: h_g"
            back = reversed_list(f1_g) if c.shuffled else f1_g
            with moves(c.expect["phase_two"], f"{name}, {where}, initialize_phase_two"):
                f1_gu = sc.initialize_phase_two(back, c.u)
            assert np.array_equal(to_host(f1_gu.evaluations), w2), f"{where}: f1(g, u, .)"
            with moves(c.expect["prove"], f"{name}, {where}, prove"):
                proof = sc.GKRRoundSumcheck.prove(sc.Blake2b512Rng.setup(), f1, m2, m3, c.g)
            assert np.array_equal(np.stack([m.evaluations for m in proof.phase1_sumcheck_msgs]), want[0]), f"{where}: phase one's messages"
            assert np.array_equal(np.stack([m.evaluations for m in proof.phase2_sumcheck_msgs]), want[1]), f"{where}: phase two's messages"
            sub = sc.GKRRoundSumcheck.verify(sc.Blake2b512Rng.setup(), dim, proof, proof.extract_sum())
            assert np.array_equal(sub.u, wuv[0]) and np.array_equal(sub.v, wuv[1]), f"{where}: (u, v)"
            for t, h in ((f1.indices, c.idx), (f1.values, c.vals), (m2.evaluations, c.f2), (m3.evaluations, c.f3)):  # the inputs are only read
                assert np.array_equal(to_host(t).reshape(h.shape), h), where


@pytest.mark.parametrize("name", list(E.PHASE_TWO_CASES))
def test_phase_two_with_one_cell_at_its_fullest(name):
    """initialize_phase_two on a list that repeats one (x, y) 8192 times (or 8193), every term the limbs of p - 1; the oracle takes the merged list"""
    c = E.build(name)
    oi, ov = c.oracle_f1g()
    assert oi.shape[0] < c.idx.shape[0]
    want = cref.gkr_phase_two(oi, ov, c.dim, c.u)
    for where in ("host", "device"):
        put = to_dev if where == "device" else (lambda a: a)
        f1_g = sc.SparseMultilinearExtension(2 * c.dim, put(c.idx), put(c.vals))
        with moves(c.expect, f"{name}, {where}"):
            got = sc.initialize_phase_two(f1_g, c.u)
        assert np.array_equal(to_host(got.evaluations), want), where
