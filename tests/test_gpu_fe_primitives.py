"""Every primitive of the carry-free arithmetic, one lane per element through sc_debug_fe_op (kernels_selftest.hip), against the exact
integer model (tests/fe_model.py) on the operand vectors of DESIGN 4.6: the limb and value ranges the call sites can reach, not the
canonical tables whole proofs feed.  Every element of every op is compared."""
import random

import numpy as np
import pytest
import torch

from tests import fe_model as fm
from tests import helpers as H

pytestmark = pytest.mark.gpu
P = fm.P
DEV = "cuda:0"


run_op, dev_limbs, dev_words, as_fr = H.fe_run_op, H.fe_dev_limbs, H.fe_dev_words, H.fe_as_fr


def col(rows, k):
    return [r[k] for r in rows]


def assert_limbs_equal(got, want, what):
    want = np.asarray(want, dtype=np.int64)
    bad = np.nonzero((got.astype(np.int64) != want).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} elements differ, first at {bad[0]}: got {got[bad[0]].tolist()}, want {want[bad[0]].tolist()}"


# ---- exact products ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [fm.OP_MUL, fm.OP_MUL_CHAIN], ids=["plain", "chain"])
def test_fe_mul(op):
    rows = fm.operand_sets([fm.BOX_MUL_A, fm.BOX_MUL_B], random.Random(fm.SEED + op))
    rows += [[b, a] for a, b in rows[:200] if fm.in_box(b, fm.BOX_MUL_A) and fm.in_box(a, fm.BOX_MUL_B)]
    want = [fm.fe_mul(a, b) for a, b in rows]
    assert all(fm.fits_i32(w) for w in want)
    got = run_op(op, len(rows), dev_limbs(col(rows, 0)), dev_limbs(col(rows, 1)))
    assert_limbs_equal(got, want, "fe_mul")


@pytest.mark.parametrize("op", [fm.OP_MUL_U, fm.OP_MUL_U_CHAIN], ids=["plain", "chain"])
def test_fe_mul_u(op):
    rows = fm.operand_sets([fm.BOX_MUL_A, fm.BOX_FEU], random.Random(fm.SEED + op))
    want = [fm.fe_mul(a, u) for a, u in rows]
    got = run_op(op, len(rows), dev_limbs(col(rows, 0)), dev_limbs(col(rows, 1)))
    assert_limbs_equal(got, want, "fe_mul_u")


@pytest.mark.parametrize("op", [fm.OP_MUL2, fm.OP_MUL2_CHAIN], ids=["plain", "chain"])
def test_fe_mul2_sum(op):
    rows = fm.operand_sets([fm.BOX_MUL2] * 4, random.Random(fm.SEED + op))
    want = [fm.fe_mul2_sum(*r) for r in rows]
    got = run_op(op, len(rows), *(dev_limbs(col(rows, k)) for k in range(4)))
    assert_limbs_equal(got, want, "fe_mul2_sum")


@pytest.mark.parametrize("op", [fm.OP_BIND, fm.OP_BIND_CHAIN], ids=["plain", "chain"])
@pytest.mark.parametrize("r_std", [1, P - 1, (P - 1) // 2, 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA9876543211122334455667788 % P, 0], ids=["one", "minus-one", "half", "random", "zero"])
def test_fe_mul_bind(op, r_std):
    rows = col(fm.operand_sets([fm.BOX_BIND_D], random.Random(fm.SEED + op), 1000), 0)
    want = [fm.fe_mul_bind(d, r_std) for d in rows]
    r_mont = r_std * fm.R256 % P
    got = run_op(op, len(rows), dev_limbs(rows), params=[(r_mont >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)])
    assert_limbs_equal(got, want, "fe_mul_bind")
    assert all(abs(w[8]) < (1 << 24) for w in want)


def test_feu_shl5_fe_mul_u():
    """the LDS-resident kernels' bind product: fe_mul_u<true>(d, feu_shl5(r))"""
    rng = random.Random(fm.SEED + 13)
    ds = col(fm.operand_sets([fm.BOX_MUL_A], rng), 0)
    edge = [0, 1, P - 1, P, (1 << 256) - 1, 1 << 255, (1 << 251) - 1, fm.R256]
    xs = [edge[i % len(edge)] if i < 8 * len(edge) else rng.randrange(1 << 256) for i in range(len(ds))]
    want = [fm.fe_shl5_mul_u(d, x) for d, x in zip(ds, xs)]
    got = run_op(fm.OP_SHL5_MUL_U, len(ds), dev_limbs(ds), dev_words(xs))
    assert_limbs_equal(got, want, "feu_shl5 + fe_mul_u")


# ---- carries and conversions -------------------------------------------------------------------------------------------------------------
def test_fe_normalize():
    rows = col(fm.operand_sets([fm.BOX_NORM], random.Random(fm.SEED)), 0)
    got = run_op(fm.OP_NORMALIZE, len(rows), dev_limbs(rows))
    assert_limbs_equal(got, [fm.limbs_of(fm.value(r)) for r in rows], "fe_normalize")


def test_fe_carry_pass():
    rows = col(fm.operand_sets([fm.BOX_CARRY], random.Random(fm.SEED + 1)), 0)
    got = run_op(fm.OP_CARRY_PASS, len(rows), dev_limbs(rows)).astype(np.int64)
    for r, g in zip(rows, got):
        assert fm.value(g) == fm.value(r), (r, g.tolist())
    assert (got[:, 0] >= 0).all() and (got[:, 0] < fm.T29).all()
    assert (got[:, 1:8] >= -4).all() and (got[:, 1:8] < fm.T29 + 4).all()


def test_fe_to_fr():
    rows = fm.to_fr_vectors(random.Random(fm.SEED + 2))
    got = run_op(fm.OP_TO_FR, len(rows), dev_limbs(rows))
    bad = [(r, as_fr(g)) for r, g in zip(rows, got) if as_fr(g) != fm.value(r) % P]
    assert not bad, f"{len(bad)} of {len(rows)} differ, first: limbs {bad[0][0]} -> {bad[0][1]:#x}"


def test_fe_from_fr_and_round_trip():
    rng = random.Random(fm.SEED + 3)
    vals = [0, 1, P - 1, P, P + 1, 2 * P, 2 * P - 1, (1 << 256) - 1, 1 << 255, fm.MASK, 1 << 232, (1 << 232) - 1] + [1 << (29 * i) for i in range(9)]
    vals += [rng.randrange(1 << 256) for _ in range(fm.N_RANDOM)]
    got = run_op(fm.OP_FROM_FR, len(vals), dev_words(vals))
    assert_limbs_equal(got, [fm.limbs_of(v) for v in vals], "fe_from_fr")
    got = run_op(fm.OP_ROUND_TRIP, len(vals), dev_words(vals))
    assert [as_fr(g) for g in got] == [v % P for v in vals]


def test_wide_fold_cell():
    rows = fm.fold_cell_vectors(random.Random(fm.SEED + 4))
    got = run_op(fm.OP_FOLD_CELL, len(rows), torch.zeros((1, 9), dtype=torch.int32, device=DEV), aux_tail=rows)
    assert [as_fr(g) for g in got] == [fm.wide_fold(r) for r in rows]


# ---- lazy lines and combinations -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", fm.LINE_NODES)
def test_fe_line(nv):
    rows = fm.operand_sets([fm.BOX_LINE, fm.BOX_LINE], random.Random(fm.SEED + 5), 1000)
    got = run_op(fm.OP_LINE, len(rows), dev_limbs(col(rows, 0)), dev_limbs(col(rows, 1)), params=[nv]).astype(np.int64)
    for (lo, hi), g in zip(rows, got):
        lo_v, hi_v = fm.value(lo), fm.value(hi)
        want = hi_v - lo_v if nv == fm.NODE_INF else lo_v + nv * (hi_v - lo_v)
        assert fm.value(g) == want, (nv, lo, hi, g.tolist())
    if nv == fm.NODE_INF:  # the slope of two entries: within (-2^29 - 8, 2^29 + 8), fe_mul's second operand
        assert (np.abs(got[:, :8]) <= fm.BOX_MUL_B["hi"]).all()
    else:  # "limbs re-tightened to [-4, 2^29 + 4)"
        assert (got[:, :8] >= -4).all() and (got[:, :8] < fm.T29 + 4).all()


def _check_reduced_combination(got, rows, expect):
    got = got.astype(np.int64)
    for r, g in zip(rows, got):
        v = fm.value(g)
        assert (v - expect(r)) % P == 0 and abs(v) < 2 * P, (r, g.tolist())
    assert (got[:, :8] >= 0).all() and (got[:, :8] < fm.T29).all()


@pytest.mark.parametrize("m,t", fm.WIDE_VALUE_CASES)
def test_fe_comb5_through_wide_value(m, t):
    rows = fm.operand_sets([fm.BOX_COMB5] * 5, random.Random(fm.SEED + 10 * m + t), 600)
    flat = [sum(r, []) for r in rows]
    got = run_op(fm.OP_WIDE_VALUE, len(rows), dev_limbs(flat), params=[m, t])
    x = fm.node_value(t)
    if m == 1:  # (the single factor's line from its two values, as WideNodes forms it: (1 - x) lo + x hi)
        _check_reduced_combination(got, rows, lambda r: (1 - x) * fm.value(r[0]) + x * fm.value(r[1]))
    else:
        _check_reduced_combination(got, rows, lambda r: fm.wide_expected(m, t, r))


@pytest.mark.parametrize("m,t", fm.WIDE_EXT_CASES)
def test_wide_ext(m, t):
    rows = fm.operand_sets([fm.BOX_WIDE_EXT] * 9, random.Random(fm.SEED + 20 * m + t), 300)
    flat = [sum(r, []) for r in rows]
    got = run_op(fm.OP_WIDE_EXT, len(rows), dev_limbs(flat), params=[m, t])
    _check_reduced_combination(got, rows, lambda r: fm.wide_expected(m, t, r))


# ---- the lazy sum of a combination's products ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["1-p", "p-1", "half", "random"])
@pytest.mark.parametrize("per_lane,L", [(4, 64), (8, 64), (16, 64), (8, 32), (1, 64)], ids=lambda x: str(x))
def test_accumulate(regime, per_lane, L):
    """bt_combo_sum (the lane loop and shuffle tree of bt_sum_publish) over per_lane x L products of a combination, four combinations a block:
    256 products of magnitude p fit one top limb; 512 and 1024 need the rule's reduction"""
    rng = random.Random(fm.SEED + per_lane + L)
    terms = fm.product_regimes()
    pairs, groups = per_lane * L, 256 // L
    prods = []
    for g in range(groups):
        for pr in range(pairs):
            if regime == "random":
                prods.append(fm.fe_mul(fm.limbs_of(rng.randrange(P)), fm.limbs_of(rng.randrange(P))))
            elif regime == "half":  # the first half of the pairs at the bound, the second half 0: the lanes differ
                prods.append(terms["1-p" if g % 2 == 0 else "p-1"] if pr < pairs // 2 else [0] * 9)
            else:
                prods.append(terms[regime])
    got = run_op(fm.OP_ACCUM, 256, dev_limbs(prods), params=[per_lane, L, 1]).astype(np.int64)
    for g in range(groups):
        total = sum(fm.value(p) for p in prods[g * pairs:(g + 1) * pairs])
        lane0 = got[g * L]
        if pairs <= fm.LAZY_SUM_MAX_P:
            assert fm.value(lane0) == total, (g, lane0.tolist())  # (no reduction: the lazy sum itself)
        else:
            assert (fm.value(lane0) - total) % P == 0 and 0 <= fm.value(lane0) < L * P, (g, lane0.tolist())
        assert (lane0[:8] >= -4).all() and (lane0[:8] < fm.T29 + 4).all()
