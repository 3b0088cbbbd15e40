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


# ---- lazy table entries at the ends of their range: the model's binds on the sinking and selector tables -------------------------
NV = 10
SEL = 6
FORMS = ["f29", "lds"]


def test_carry_pass_model_keeps_the_value_and_tightens_limbs_0_to_7():
    rng = random.Random(fm.SEED + 4)
    bx = fm.BOX_CARRY
    for a in fm.corners_of(bx) + fm.random_limbs(rng, 500, bx["lo"], bx["hi"], bx["top_lo"], bx["top_hi"]):
        r = fm.carry_pass(a)
        assert fm.value(r) == fm.value(a)
        assert 0 <= r[0] <= fm.MASK and all(-4 <= x < fm.T29 + 4 for x in r[1:8])
        assert r[8] - a[8] in range(-4, 4)


def _bind(form, lo, hi, r_std):
    return fm.bind_f29(lo, hi, r_std) if form == "f29" else fm.bind_lds(lo, hi, fm.to_mont(r_std))


def _rounds(form, ints, r_std):
    """the table after 0, 1, ..., len(r_std) binds, as limbs -- every difference a bind takes checked against the multipliers' boxes"""
    tab = [fm.limbs_of(v) for v in ints]
    out = [tab]
    for r in r_std:
        for i in range(len(tab) // 2):
            d = fm.fe_sub(tab[2 * i + 1], tab[2 * i])
            assert fm.in_box(d, fm.BOX_BIND_D) and fm.in_box(d, fm.BOX_MUL_A), "a bind's difference leaves fe_mul_bind's / fe_mul_u's box"
        tab = [_bind(form, tab[2 * i], tab[2 * i + 1], r) for i in range(len(tab) // 2)]
        out.append(tab)
    return out


def _in_line_box_limbs(e):
    """BOX_LINE as limb ranges: what fe_line, and fe_mul as its second operand, take from a table"""
    return fm.in_box(e, fm.BOX_LINE) and fm.in_box(e, fm.BOX_MUL_B)


def _family(delta=fm.DELTA):
    s, r = fm.sinking_challenges(NV, fm.SEED + 5, delta)
    return s, r


@pytest.mark.parametrize("delta", [fm.DELTA, fm.DELTA_WIDE], ids=["d232", "d240"])
def test_generated_entries_and_challenges_are_canonical_and_non_zero(delta):
    s, r = _family(delta)
    assert all(0 < x < P for x in r) and len(set(r)) == NV
    assert all(x * (P - sj) % P == delta for x, sj in zip(r, s))
    for m, c in ((1, sum(s)), (1, sum(s) + 1), (7, 7 * sum(s) + 12345), (1, P - 1), (3, P - 2)):
        t = fm.sinking_table(NV, s, m, c)
        assert len(t) == 1 << NV and all(0 <= v < P for v in t) and (min(t) > 0 or c == m * sum(s))
        assert t[0] == c and t[-1] == c - m * sum(s) and t[5] == c - m * (s[0] + s[2])
        for flip in (False, True):
            u = fm.selector_table(NV, s, SEL, m, c, flip)
            assert len(u) == 1 << NV and all(0 <= v < P for v in u)
            assert all(u[x] == P - 1 for x in range(1 << NV) if ((x >> SEL) & 1) != flip)
            assert u[((1 << NV) - 1) ^ (0 if flip else 1 << SEL)] == c - m * (sum(s) - s[SEL])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("delta", [fm.DELTA, fm.DELTA_WIDE], ids=["d232", "d240"])
@pytest.mark.parametrize("m", [1, 7])
def test_sinking_entries_attain_the_lower_end_after_every_bind(form, delta, m):
    """after k binds every entry is EXACTLY its start + k (m delta - p): in [-k p, -k p + 2^242) wherever k m delta + c < 2^242 (every k for
    delta = 2^232), never outside (-(k + 1) p, p), its limbs inside what fe_line and fe_mul take"""
    s, r = _family(delta)
    c = m * sum(s) + 1
    ints = fm.sinking_table(NV, s, m, c)
    reached = 0
    for k, tab in enumerate(_rounds(form, ints, r)):
        for y, e in enumerate(tab):
            v = fm.value(e)
            assert v == ints[y << k] + k * (m * delta - P), (k, y)
            assert -(k + 1) * P < v < P and _in_line_box_limbs(e)
            if k * m * delta + c < (1 << 242):
                assert -k * P <= v < -k * P + (1 << 242), (k, y)
        reached = k if k * m * delta + c < (1 << 242) else reached
    assert reached == (NV if delta == fm.DELTA else (3 if m == 1 else 0))


@pytest.mark.parametrize("form", FORMS)
def test_a_table_that_starts_at_the_high_end_stays_below_p(form):
    s, r = _family()
    ints = fm.sinking_table(NV, s, 1, P - 1)
    for k, tab in enumerate(_rounds(form, ints, r)):
        vs = [fm.value(e) for e in tab]
        assert max(vs) == P - 1 + k * (fm.DELTA - P) and all(-(k + 1) * P < v < P for v in vs) and all(_in_line_box_limbs(e) for e in tab)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("flip", [False, True], ids=["up", "down"])
def test_selector_slopes_and_the_lines_through_them(form, flip):
    """round sel + 1 of a selector table: every slope beyond (sel + 0.5) p; fe_line at every node a fused product takes, step by step --
    intermediates below 1.5 * 2^30 a limb, results with limbs 0..7 carry-passed and limb 8 inside fe_mul's second operand"""
    s, r = _family()
    ints = fm.selector_table(NV, s, SEL, 1, sum(s) + 1, flip)
    tab = _rounds(form, ints, r[:SEL])[SEL]
    widest = 0
    for i in range(len(tab) // 2):
        lo, hi = tab[2 * i], tab[2 * i + 1]
        slope = fm.value(hi) - fm.value(lo)
        assert (slope <= -(SEL + 0.5) * P) if flip else (slope >= (SEL + 0.5) * P)
        assert _in_line_box_limbs(lo) and _in_line_box_limbs(hi)
        for x in fm.LINE_NODES:
            res, seen = fm.fe_line(lo, hi, x)
            assert all(abs(l) < 3 << 29 for t in seen for l in t)
            if x == fm.NODE_INF:
                assert fm.value(res) == slope and fm.in_box(res, fm.BOX_MUL_B)
                continue
            assert fm.value(res) == fm.value(lo) + x * slope
            assert all(-4 <= l < fm.T29 + 4 for l in res[:8]) and fm.in_box(res, fm.BOX_MUL_B)
            widest = max(widest, abs(fm.value(res)))
    # node 4 of a (sel + 1) p slope from -sel p: 22 p for sel = 6 -- beyond the +-16 p of the ENTRIES' box, which is no bound on the line
    assert (3 * SEL + 3.9) * P < widest < (4 * SEL + 7) * P and widest < (fm.T29 + 16) // (fm.PH + 1) * P


@pytest.mark.parametrize("form", FORMS)
def test_the_models_binds_are_the_oracles_fix_variables_mod_p(form):
    s, r = _family()
    rinv = pow(fm.R256, -1, P)
    tables = [fm.sinking_table(NV, s, 1, sum(s)), fm.sinking_table(NV, s, 5, P - 1), fm.selector_table(NV, s, SEL, 1, sum(s) + 9),
              fm.selector_table(NV, s, 3, 2, P - 1, True)]
    for ints in tables:
        std = [v * rinv % P for v in ints]
        for k, tab in enumerate(_rounds(form, ints, r)):  # (past round sel + 1 a selector table's slopes are arbitrary: the same binds)
            want = po.dense_fix_variables(std, r[:k])
            assert [fm.value(e) * rinv % P for e in tab] == want, k
            assert all(-(k + 1) * P < fm.value(e) < P for e in tab)


def test_the_array_builders_give_the_formulas_entries():
    import numpy as np
    from tests import helpers as H
    s, _ = _family()
    as_ints = lambda a: [sum(int(row[k]) << (64 * k) for k in range(4)) for row in a]
    assert as_ints(H.sinking_table_limbs(NV, s, 3, P - 1)) == fm.sinking_table(NV, s, 3, P - 1)
    for sel, flip in ((0, False), (SEL, True), (NV - 1, False)):
        assert as_ints(H.selector_table_limbs(NV, s, sel, 2, 2 * sum(s), flip)) == fm.selector_table(NV, s, sel, 2, 2 * sum(s), flip)
    nv = 18
    s, r = fm.sinking_challenges(nv, fm.SEED + 6)
    t = H.sinking_table_limbs(nv, s, 5, 5 * sum(s) + 77)
    assert t.shape == (1 << nv, 4) and t.dtype == np.uint64
    H.assert_entries_match(t, H.sinking_entry(s, 5, 5 * sum(s) + 77))
    u = H.selector_table_limbs(nv, s, 11, 1, P - 1, True)
    H.assert_entries_match(u, H.selector_entry(s, 11, 1, P - 1, True))
    with pytest.raises(AssertionError):
        H.assert_entries_match(u, H.selector_entry(s, 11, 1, P - 1, False))
    assert H.mont_challenges(r).shape == (nv, 4) and as_ints(H.mont_challenges(r[:2])) == [x * fm.R256 % P for x in r[:2]]


# ---- every factor of a product at its range end at once: the product loop on all-selector pairs, in closed form ------------------
import functools

LAMBDA = (1 << fm.K) / P  # 70.66: a factor of magnitude L p scales a running product by L / LAMBDA (and fe_mul's window adds up to p)
ORIENTS = ["up", "down", "alt"]
K_TAIL_MAX = 15           # a tail of 2^14 pairs whose first round binds on the way in: 15 binds behind its last round (2^14 = kSmallRoundPairs)


@pytest.mark.parametrize("form", FORMS)
def test_the_selector_pairs_closed_form_is_what_the_binds_leave(form):
    """selector_pair against the tables bound round by round, both orientations; and with the entries made canonical after k0 binds
    (what the rule of k_tail_slices<12> does): the stored integers are a sinking table again, c + k0 m delta, and sink from there"""
    s, r = _family()
    for sel, m, flip in ((0, 1, False), (3, 7, True), (SEL, 2, False), (NV - 1, 5, True)):
        ints = fm.selector_table(NV, s, sel, m, m * sum(s) + 3, flip)
        for k0 in sorted({0, sel // 2, sel}):
            tab = _rounds(form, ints, r[:k0])[k0]
            if k0:
                tab = [fm.limbs_of(fm.value(e) % P) for e in tab]
                assert all(0 <= fm.value(e) < P for e in tab)
            tab = _rounds(form, [fm.value(e) for e in tab], r[k0:sel])[sel - k0]
            for i in range(len(tab) // 2):
                start = ints[(2 * i + (1 if flip else 0)) << sel]
                lo, hi = fm.selector_pair(sel, m, start, flip, lazy=sel if k0 == 0 else sel - k0)
                assert (fm.value(tab[2 * i]), fm.value(tab[2 * i + 1])) == (fm.value(lo), fm.value(hi)), (sel, k0, i)
                assert _in_line_box_limbs(tab[2 * i]) and _in_line_box_limbs(tab[2 * i + 1])


def test_product_chain_is_the_field_product_and_names_what_it_leaves():
    rng = random.Random(fm.SEED + 7)
    vals = [fm.limbs_of(rng.randrange(P)) for _ in range(12)]
    prod, peak, left = fm.product_chain(vals)
    want = 1
    for v in vals:
        want = want * fm.value(v) % P
    assert fm.value(prod) % P == want * pow(1 << fm.K, -11, P) % P and not left and peak < 2 * P
    wide = [fm.limbs_of(-89 * P + 5)] * 12  # node -5 of an all-selector product of twelve after 14 binds
    assert fm.product_chain(wide, strict=False)[2] == {"mul_b", "int32"}
    with pytest.raises(AssertionError):
        fm.product_chain(wide)
    assert fm.product_chain([fm.limbs_of(P), fm.limbs_of(142 * P)], strict=False)[2] == {"mul_a"}  # 2^30 / PH = 141.3


def test_line_reach_n_is_half_the_degree_rounded_up():
    assert [fm.line_reach_n(M) for M in range(1, 13)] == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6]
    assert fm.LINE_REACH_MAX_P == (1 << fm.K) // P == (fm.T29 + 16) // (fm.PH + 1)  # |value| < 70 p: limb 8 inside BOX_MUL_B


@functools.lru_cache(maxsize=None)
def _scan(M, k, lazy, mult=None):
    """every node the product takes, the three orientations, the pairs whose entries started lowest and highest -> (widest |line|, peak
    |running product|, largest |final product| -- all in p --, what any chain left)"""
    line = peak = final = 0
    left = set()
    for orient in ORIENTS:
        for low in (True, False):
            for t in range((sum(mult) if mult else M) + 1):
                vals = fm.all_selector_values(len(mult) if mult else M, k, orient, t, lazy, low, mult)
                assert all(-4 <= l < fm.T29 + 4 for v in vals for l in v[:8]) or fm.node_value(t) == fm.NODE_INF
                line = max(line, max(abs(fm.value(v)) for v in vals))
                prod, pk, lf = fm.product_chain(vals, strict=False)
                peak, final, left = max(peak, pk), max(final, abs(fm.value(prod))), left | lf
    return line / P, peak / P, final / P, frozenset(left)


def _final_bounds(L, M):
    """|prod'| <= |prod| L / LAMBDA + 1 (fe_mul's window), M - 1 times from L: L rho^(M-1) +- (1 - rho^(M-1)) / (1 - rho), rho = L / LAMBDA"""
    rho = L / LAMBDA
    geo = (1 - rho ** (M - 1)) / (1 - rho)
    return L * rho ** (M - 1) - geo, L * rho ** (M - 1) + geo


@pytest.mark.parametrize("M", range(2, 9))
def test_every_factor_a_selector_products_of_up_to_eight_stay_inside_every_box(M):
    """k = 0 .. 15 binds (no tail of such a product has more: K_TAIL_MAX), entries AT -k p: every line is within (n (k + 2) - 1) p < 69 p, so
    the running product only shrinks towards LAMBDA / (LAMBDA - L) and never leaves fe_mul's second operand"""
    n = fm.line_reach_n(M)
    for k in range(K_TAIL_MAX + 1):
        line, peak, final, left = _scan(M, k, k)
        assert not left, (k, sorted(left))
        assert not fm.line_needs_canonical(n, k + 2), "the rule of the wide tail would never fire for a product of up to eight"
        # entries at -k p, not -(k + 1) p: one n short of the bound (node n from canonical entries: n p; the slope itself: (k + 1) p)
        assert line <= max(n * (k + 2) - 1, k + 2) and abs(line - max(n * (k + 1) - 1, n, k + 1)) < 0.01
        assert peak <= max(line * line / LAMBDA + 1, 2) and final <= peak
        lo, hi = _final_bounds(line, M)
        assert lo <= final <= hi, (k, final, lo, hi)
    if M >= 7:  # round 15 of a proof in 15 variables, the widest the GPU tests reach: lines at 59 p, the product of 7 at 59 (59 / 70.66)^6 = 19.9 p
        line, _, final, _ = _scan(M, 14, 14)
        assert abs(line - 59) < 0.01 and abs(final - 59 * (59 / LAMBDA) ** (M - 1)) < 4.1


def test_the_unremedied_chain_of_nine_to_twelve_leaves_the_second_operand_and_then_int32():
    """WITHOUT the rule (entries lazy for all k binds): the first k at which a running product leaves BOX_MUL_B, and at which a limb 8
    leaves int32 -- why k_tail_slices<12> makes its entries canonical (kernels.h: line_needs_canonical)"""
    first_b, first_i32 = {}, {}
    for M in range(9, 13):
        for k in range(K_TAIL_MAX + 1):
            left = _scan(M, k, k)[3]
            assert "mul_a" not in left
            if "mul_b" in left:
                first_b.setdefault(M, k)
            if "int32" in left:
                first_i32.setdefault(M, k)
    assert first_b == {9: 14, 10: 14, 11: 11, 12: 11}
    assert first_i32 == {11: 13, 12: 13}
    assert abs(_scan(12, 14, 14)[0] - 89) < 0.01 and _scan(12, 14, 14)[1] > 1000  # lines at -89 p, a running product beyond 1000 p


@pytest.mark.parametrize("M", range(9, 13))
def test_with_the_rule_products_of_nine_to_twelve_stay_inside_every_box(M):
    """the entries made canonical by the bind that would take n (lazy binds + 2) beyond 70: lazy <= 12 for M = 9, 10 and <= 9 for M = 11, 12"""
    n = fm.line_reach_n(M)
    depth = [fm.lazy_binds_under_the_rule(M, k) for k in range(17)]
    assert max(depth) == (12 if n == 5 else 9) and depth[:max(depth) + 2] == list(range(max(depth) + 1)) + [0]
    for k in range(17):
        line, peak, final, left = _scan(M, k, depth[k])
        assert not left, (k, sorted(left))
        assert line <= n * (depth[k] + 2) - 1 <= fm.LINE_REACH_MAX_P - 1 and peak < line + 1
        assert final <= _final_bounds(line, M)[1]
    if M == 12:  # the exponent loop of the same chain (tests/test_gpu_lazy_entries.py: the multiplicity shapes at sel = 14)
        for mult in ((12,), (4, 4, 4)):
            assert not _scan(M, 14, depth[14], mult)[3] and _scan(M, 14, 14, mult)[3] == {"mul_b", "int32"}


def test_the_lazy_sum_of_all_selector_products_stays_inside_the_top_limb():
    """worst_p + j counts a product at (k + 2) p; the all-selector products exceed that late in a tail (21.5 p against 16 for a product of 7
    after 14 binds).  One accumulator adds at most the round's pairs: 2^14 >> (k - 1) in a tail of 2^14 pairs that binds on the way in, 2^14 >> k
    in one that does not.  Where lazy_sum_needs_reduce(pairs, k + 2) does not fire, pairs x the largest product must fit kLazySumMaxP p.
    The model's worst ratio: 0.85 (M = 9 after 12 binds, the last before its entries are made canonical: 8 pairs x 29.9 p = 239 p of 282)"""
    worst = (0,)
    for M in range(2, 13):
        for k in range(K_TAIL_MAX + 1):
            final = _scan(M, k, k if M <= 8 else fm.lazy_binds_under_the_rule(M, k))[2]
            for first_bind in (0, 1):
                pairs = (1 << 14) >> (k - first_bind) if k >= first_bind else 0
                if pairs >= 1 and pairs * (k + 2) <= fm.LAZY_SUM_MAX_P:
                    assert pairs <= 16
                    worst = max(worst, (pairs * final / fm.LAZY_SUM_MAX_P, M, k, pairs))
    assert worst[0] < 1 and worst[1:] == (9, 12, 8) and 0.84 < worst[0] < 0.86, worst


# ---- the per-lane running sums of the big rounds: tree_pass's accumulator, and what it is handed ------------------------------
from tests import f29_pack_model as f29
from tests.test_lane_sum_host import lane_table

E255 = fm.F29_ENTRY_BOUND - 1  # the packed format's largest magnitude: 1.104 p


def _unsettled(j, c=23 << 200):
    """a sinking table's entry after j binds that are NOT settled (bind_f29: the table format before it was packed): c + j (delta - p)"""
    return fm.limbs_of(c + j * (fm.DELTA - P))


def test_the_running_sum_takes_31_unsettled_entries_at_minus_9_p_and_not_32():
    """the accumulator's own limit, whatever hands it its terms: between two reductions limb 8 holds 282 p.  Raw entries at -9 p (a sinking
    table after nine binds without f29_settle) leave int32 with the 32nd term, the one after which the sum would have been reduced; at
    -8 p they stay inside for any number of iterations; at the open end of the range those entries had, -(8 + 1) p, they do not"""
    s, r = fm.sinking_challenges(9, fm.SEED + 40)
    tab = [fm.limbs_of(v) for v in fm.sinking_table(9, s, 1, sum(s))]
    for rj in r:
        tab = [fm.bind_f29(tab[2 * i], tab[2 * i + 1], rj) for i in range(len(tab) // 2)]
    assert fm.value(tab[0]) == fm.value(_unsettled(9, sum(s))) and -9 * P <= fm.value(tab[0]) < -9 * P + (1 << 242)
    _, peak, left = fm.big_lane_sum([_unsettled(9)] * 32, strict=False)
    assert left == 31 and peak > fm.LAZY_SUM_MAX_P
    with pytest.raises(AssertionError):
        fm.big_lane_sum([_unsettled(9)] * 32)
    acc, peak, left = fm.big_lane_sum([_unsettled(9)] * 31)
    assert left is None and 278 < peak < 279.1 and fm.value(acc) == 31 * fm.value(_unsettled(9))
    acc, peak, left = fm.big_lane_sum([_unsettled(8)] * 200)  # every block of 32 starts from the reduced sum
    assert left is None and 255 < peak < 257 and fm.value(acc) % P == 200 * fm.value(_unsettled(8)) % P
    assert fm.big_lane_sum([fm.limbs_of(1 - 9 * P)] * 32, strict=False)[2] == 31
    print(f"\n31 terms at -9 p: {31 * 9} p of {fm.LAZY_SUM_MAX_P}; 32 terms at -8 p + the reduced sum: {peak:.1f} p")


def test_the_two_pair_form_is_the_same_accumulator_over_half_the_terms():
    """64 products in 32 terms: fe_mul2_sum's result is (a b + c d) / 2^261 in a window of p, so a term is two products wide"""
    rng = random.Random(fm.SEED + 41)
    ops = [[fm.limbs_of(rng.randrange(P)) for _ in range(4)] for _ in range(70)]
    acc, peak, left = fm.big_lane_sum_pairs(ops)
    inv = pow(1 << fm.K, -1, P)
    assert left is None and fm.value(acc) % P == sum(fm.value(a) * fm.value(b) + fm.value(c) * fm.value(d) for a, b, c, d in ops) * inv % P
    assert -6 * P < fm.value(acc) < 2 * P and peak < 33 * 2  # 70 = 2 x 32 + 6: the reduced sum and six terms, each in (-p, 2 p^2 / 2^261]
    corner = [[fm.limbs_of(v) for v in (E255, E255, E255, E255)]] * 64  # 2 E^2 / 2^261 = 0.035 p: the window decides, not the operands
    assert fm.big_lane_sum_pairs(corner)[1] < 33


def _term_bound_p(M, two):
    """|a term of tree_pass| in p for factors whose line ends lie within E = 2^255 / p = 1.104: fe_mul(a, b) is within |a| |b| / LAMBDA + 1,
    a slope within 2 E, a quadratic's extension 2 q(inf) + 2 q(0) - q(1) within the sum, f(-1) = 2 lo - hi within 3 E"""
    E = fm.F29_ENTRY_BOUND / P
    mul = lambda a, b: a * b / LAMBDA
    q0, qi = mul(E, E) + 1, mul(2 * E, 2 * E) + 1
    ext = 2 * qi + 3 * q0
    widest = {1: E, 2: mul(2 * E, 2 * E), 3: max(mul(2 * E, qi), mul(3 * E, ext)), 4: max(mul(qi, qi), mul(ext, ext))}[M]
    return widest if M == 1 else (2 if two else 1) * widest + 1


@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_a_term_from_packed_entries_is_below_two_p(M):
    """what the big rounds actually hand the accumulator since bound tables are packed: LoadFactor returns a canonical entry or one
    settled into [-2^255, 2^255), however many binds lie behind it.  Every factor's pair on the corners of that box, both pairs of the
    two-pair form alike: no term of any node reaches kBigTermWorstP p, and the model's widest stays within the bound worked out by hand"""
    import itertools
    ends = [fm.limbs_of(v) for v in (E255, -E255 - 1)]
    widest = {False: 0, True: 0}
    for combo in itertools.product(itertools.product(ends, ends), repeat=M):
        lo, hi = [c[0] for c in combo], [c[1] for c in combo]
        for two in ([False] if M == 1 else [False, True]):
            terms = fm.tree_terms(M, lo, hi, lo if two else None, hi if two else None)
            assert len(terms) == M + 1 and all(fm.fits_i32(t) for t in terms)
            widest[two] = max(widest[two], max(abs(fm.value(t)) for t in terms) / P)
    for two, w in widest.items():
        assert w <= _term_bound_p(M, two) < fm.BIG_TERM_WORST_P, (M, two, w)
    print(f"\nM = {M}: widest term {widest[False]:.3f} p (bound {_term_bound_p(M, False):.3f})" +
          (f", two pairs {widest[True]:.3f} p (bound {_term_bound_p(M, True):.3f})" if M > 1 else ""))
    # the accumulator over the longest stretch between two reductions, every term at the box's end: 33 x 1.104 p of the 282
    if M == 1:
        for e in ends:
            acc, peak, left = fm.big_lane_sum([e] * 64)
            assert left is None and peak < 33 * 1.105 + 0.01 < fm.LAZY_SUM_MAX_P / 7


def test_a_sinking_table_bound_into_the_packed_format_never_sinks():
    """the tables of tests/test_gpu_big_sum_bounds.py in the model: bound with f29_settle (load_factor.hpp), a sinking table's entries are
    back near zero after every bind -- from the low end and from just below p -- so round 10's 32 raw terms a lane sum to less than 33 p"""
    nv = 12
    s, r = fm.sinking_challenges(nv, fm.SEED + 42)
    for c in (sum(s), P - 1):
        tab = [fm.limbs_of(v) for v in fm.sinking_table(nv, s, 1, c)]
        for k, rj in enumerate(r[:10], start=1):
            tab = [f29.bind_packed(tab[2 * i], tab[2 * i + 1], rj)[0] for i in range(len(tab) // 2)]
            vals = [fm.value(e) for e in tab]
            assert all(-P // 2 - (1 << 233) < v < P + k * (1 << 230) for v in vals) and all(f29.packable(e) for e in tab)
            assert all(0 <= v <= k * fm.DELTA + (1 << 206) for v in vals) or c == P - 1
            lo = tab[0::2][:64]
            acc, peak, left = fm.big_lane_sum(lo)
            assert left is None and peak < 33 * 1.105 and fm.value(acc) % P == sum(fm.value(e) for e in lo) % P


def test_products_at_the_design_bound_fit_every_big_round_the_library_admits():
    """the enumeration of lane_sum.hpp (every nv <= 40, every big round, the merged launch of 1, 2, 3, 4 and 12 rows and one launch per
    product) against DESIGN 4.6's bound for a term of a product of two to four over entries left lazy for j = round - 1 binds,
    (1 + j^2 / 70) p, twice that where a term holds two pairs: min(terms, 32) of them and the reduced sum stay inside 282 p.  That bound
    predates the packed format, which keeps the factors within 1.104 p and a term below 2 p in EVERY round (the previous tests): 33 x 2 =
    66 p.  For a raw entry counted by the range it had before (-(j + 1) p; the sinking family reached -j p) the same enumeration gives the
    nv at which 32 terms no longer fit"""
    tight, single_doc, single_family = (0,), [], []
    for nv, rnd, rows, M, grid, terms, two in lane_table():
        j, held = rnd - 1, min(terms, fm.BIG_SUM_REDUCE_EVERY)
        assert held + 1 == min(terms, 32) + 1 and (held + 1) * fm.BIG_TERM_WORST_P <= fm.LAZY_SUM_MAX_P
        if M >= 2:
            tight = max(tight, (held * fm.product_term_bound_p(j, bool(two)) + 1, nv, rnd, rows, M, terms))
        else:
            if held * (j + 1) + 1 > fm.LAZY_SUM_MAX_P:
                single_doc.append(nv)
            if held * j + 1 > fm.LAZY_SUM_MAX_P:
                single_family.append(nv)
    assert tight[0] <= fm.LAZY_SUM_MAX_P and 270 < tight[0] < 271 and tight[2] == 16 and tight[5] >= 32, tight
    w = fm.product_term_bound_p(15, True)
    acc, peak, left = fm.big_lane_sum([fm.limbs_of(-int(w * P))] * 64)
    assert left is None and tight[0] - 1.01 < peak <= tight[0]  # (the reduced sum is in [0, p): it counts for the terms' sign or against it)
    assert min(single_doc) == 32 and min(single_family) == 33
    print(f"\nproducts at (1 + j^2 / 70) p a pair: {tight[0]:.1f} p of {fm.LAZY_SUM_MAX_P} at nv {tight[1]} round {tight[2]} ({tight[5]} terms a lane); "
          f"from packed entries: {33 * fm.BIG_TERM_WORST_P} p in every round")
