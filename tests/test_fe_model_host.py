"""The exact model of the carry-free arithmetic (tests/fe_model.py) against the Python oracle, and the operand vectors against the
preconditions they are meant to sit on.  No GPU."""
import random

import pytest

from oracle import pyoracle as po
from tests import fe_model as fm

P = fm.P


def test_constants():
    assert po.P == P and fm.R256 == po.R
    assert fm.PH == 7597479 and (1 << 31) // fm.PH == fm.LAZY_SUM_MAX_P == 282
    assert fm.LAZY_SUM_MAX_P * (fm.PH + 1) < (1 << 31) <= (fm.LAZY_SUM_MAX_P + 1) * fm.PH  # 282 terms of magnitude p fit the top limb, 283 do not
    assert [fm.node_value(t) for t in range(9)] == [0, 1, fm.NODE_INF, -1, 2, -2, 3, -3, 4]
    assert fm.limbs_of(1 - P)[8] == -(fm.PH + 1) and fm.limbs_of(P - 1)[8] == fm.PH


def test_limbs_round_trip():
    rng = random.Random(fm.SEED)
    for _ in range(200):
        v = rng.randint(-(1 << 262), 1 << 262)
        l = fm.limbs_of(v)
        assert fm.value(l) == v and all(0 <= x <= fm.MASK for x in l[:8])


def test_fe_mul_is_the_field_product_in_its_window():
    """on canonical inputs: model fe_mul = a b 2^-261 (mod p), inside (a b / 2^261 - p, a b / 2^261]"""
    rng = random.Random(fm.SEED + 1)
    inv = pow(1 << fm.K, -1, P)
    edge = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, fm.R256, P - fm.R256]
    pairs = [(a, b) for a in edge for b in edge] + [(rng.randrange(P), rng.randrange(P)) for _ in range(500)]
    for a, b in pairs:
        got = fm.value(fm.fe_mul(fm.limbs_of(a), fm.limbs_of(b)))
        assert got % P == a * b * inv % P
        assert a * b - P * (1 << fm.K) < got * (1 << fm.K) <= a * b
    # two R-form values: the R-form product times 2^-5, as fe_device.hpp states; with the 2^5 on one side, the oracle's Montgomery product
    for _ in range(100):
        x, y = rng.randrange(P), rng.randrange(P)
        xm, ym = x * po.R % P, y * po.R % P
        assert po.from_mont_limbs(po.to_mont_limbs(x)) == x
        assert fm.value(fm.fe_mul(fm.limbs_of(xm), fm.limbs_of(ym))) * 32 % P == x * y * po.R % P
        assert fm.value(fm.fe_shl5_mul_u(fm.limbs_of(xm), ym)) % P == x * y * po.R % P


def test_fe_mul2_and_bind_models():
    rng = random.Random(fm.SEED + 2)
    inv = pow(1 << fm.K, -1, P)
    for _ in range(200):
        a, b, c, d = (rng.randrange(P) for _ in range(4))
        got = fm.value(fm.fe_mul2_sum(*(fm.limbs_of(x) for x in (a, b, c, d))))
        assert got % P == (a * b + c * d) * inv % P
        r = rng.randrange(P)
        dl = [rng.randint(-(fm.T29 + 16), fm.T29 + 16) for _ in range(9)]
        t = fm.fe_mul_bind(dl, r)
        assert fm.value(t) % P == fm.value(dl) * r % P
        assert abs(t[8]) < (1 << 24)  # fe_mul_bind's comment: |T| < 2^230 + p (1 + 2^-29)


def test_wide_weights_reproduce_a_polynomial():
    """the extension weights are derived from the definition: a random polynomial of degree m, extended from its own nodes"""
    rng = random.Random(fm.SEED + 3)
    for m, t in fm.WIDE_VALUE_CASES + fm.WIDE_EXT_CASES:
        coef = [rng.randrange(-50, 50) for _ in range(m + 1)]
        f = lambda x: sum(c * x ** i for i, c in enumerate(coef))
        vals = []
        for s in range(max(m, 2) + 1):
            vals.append(fm.limbs_of(coef[m] if s == 2 else f(fm.node_value(s))))
        if m == 1:
            vals[2] = fm.limbs_of(coef[1])
        assert fm.wide_expected(m, t, vals) == f(fm.node_value(t)), (m, t)


def test_wide_fold_model():
    assert fm.wide_fold([P & 0xFFFFFFFF] + [(P >> (32 * j)) & 0xFFFFFFFF for j in range(1, 8)]) == 0
    assert fm.wide_fold([(1 << 63) - 1] * 8) == sum(((1 << 63) - 1) << (32 * j) for j in range(8)) % P


@pytest.mark.parametrize("name", ["BOX_MUL_A", "BOX_MUL_B", "BOX_FEU", "BOX_MUL2", "BOX_BIND_D", "BOX_CARRY", "BOX_NORM", "BOX_TO_FR", "BOX_LINE",
                                  "BOX_COMB5", "BOX_WIDE_EXT"])
def test_vectors_sit_inside_their_box_and_on_its_bounds(name):
    bx = getattr(fm, name)
    rows = fm.operand_sets([bx], random.Random(fm.SEED), 300)
    flat = [r[0] for r in rows]
    assert all(fm.in_box(v, bx) and fm.fits_i32(v) for v in flat)
    for i in range(8):
        assert any(v[i] == bx["hi"] for v in flat) and any(v[i] == bx["lo"] for v in flat)
    assert any(v[8] == bx["top_hi"] for v in flat) and any(v[8] == bx["top_lo"] for v in flat)
    if bx["value_bound"] is not None:
        vals = {fm.value(v) for v in flat}
        assert {0, 1, -1, bx["value_bound"] - 1, 1 - bx["value_bound"]} <= vals
        assert all(k * P in vals and -k * P in vals for k in (1, bx["max_p"]))


def test_product_columns_fit_int64_at_the_box_corners():
    """the precondition behind the limb bounds: no column of a product leaves a signed 64-bit accumulator (fe_device.hpp: Bounds)"""
    pl = max(fm.limbs_of(P))
    carry = 1 << 35
    a, b = fm.BOX_MUL_A["hi"], fm.BOX_MUL_B["hi"]
    assert 9 * a * b + 8 * fm.MASK * pl + carry < (1 << 63)
    assert 18 * fm.BOX_MUL2["hi"] ** 2 + 8 * fm.MASK * pl + carry < (1 << 63)
    assert 9 * fm.BOX_BIND_D["hi"] * fm.MASK + 2 * fm.MASK * pl + carry < (1 << 63)
    # fe_comb5: |w| < 2^8 on five values; wide_ext: |w| < 2^23 on nine
    assert 5 * (1 << 8) * (8 * fm.PH + 8 + (1 << 30)) < (1 << 63) and 9 * (1 << 23) * (1 << 30) < (1 << 63)


def test_to_fr_vectors_cover_every_quotient_step():
    rows = fm.to_fr_vectors(random.Random(fm.SEED))
    tops = {r[8] for r in rows}
    assert all(fm.in_box(r, fm.BOX_TO_FR) and fm.fits_i32(r) for r in rows)
    for k in range(1, fm.LAZY_SUM_MAX_P + 1):
        assert {k * (fm.PH + 1) - 1, k * (fm.PH + 1), -k * fm.PH, -k * fm.PH - 1} <= tops, k


def test_fold_cell_vectors():
    rows = fm.fold_cell_vectors(random.Random(fm.SEED))
    assert [(1 << 63) - 1] * 8 in rows and all(0 <= l < (1 << 63) for r in rows for l in r)


def test_accumulate_terms_are_fe_mul_extremes():
    """1 - p is the lower end of fe_mul's window on canonical operands: 1 (as raw limbs) times 2^261 mod p"""
    t = fm.product_regimes()
    assert fm.fe_mul(fm.limbs_of(1), fm.limbs_of((1 << fm.K) % P)) == t["1-p"]
    assert fm.value(t["p-1"]) == P - 1 and t["1-p"][8] == -(fm.PH + 1)
    # 256 of either fit ONE int32 top limb, 512 do not: the rule (kernels.h: lazy_sum_needs_reduce)
    assert 256 * (fm.PH + 1) < (1 << 31) < 512 * fm.PH
