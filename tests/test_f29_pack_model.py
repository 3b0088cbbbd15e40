"""The packed internal table format on the CPU: the bit-exact model (tests/f29_pack_model.py) round-trips, is bit-contiguous, and keeps
every bound entry inside [-2^255, 2^255) while staying congruent to the oracle's fix_variables.  No GPU."""
import random

import numpy as np
import pytest

from oracle import cref
from tests import f29_pack_model as pk
from tests import fe_model as fm
from tests import helpers as H

P = fm.P
BINDS = 40  # validate_desc admits nv <= 40


def test_constants():
    assert pk.HALF_P_TOP == 3798739 and pk.HALF_P_TOP == P >> 233 and pk.RULE_TOP == 3798740
    assert fm.value(pk.p_limbs()) == P and pk.packable(pk.p_limbs())
    assert pk.LIMIT * 1000 // P == 1104  # +-1.104 p


def test_round_trip_random():
    rng = random.Random(fm.SEED + 40)
    for _ in range(20000):
        l = [rng.randint(0, fm.MASK) for _ in range(8)] + [rng.randint(pk.TOP_LO, pk.TOP_HI)]
        w = pk.pack(l)
        assert all(0 <= x <= 0xFFFFFFFF for x in w)
        assert pk.unpack(w) == l
        assert pk.packed_value(w) == fm.value(l)  # bit-contiguous: the words ARE the value


def test_round_trip_corners():
    rows = pk.corner_limbs()
    assert len(rows) == 5 + 12 + 4
    for l in rows:
        assert pk.packable(l), l
        w = pk.pack(l)
        assert pk.unpack(w) == l and pk.packed_value(w) == fm.value(l)
    # a canonical value is its own packed form
    rng = random.Random(fm.SEED + 41)
    for v in [0, 1, P - 1] + [rng.randrange(P) for _ in range(500)]:
        assert pk.pack(fm.limbs_of(v)) == fm.words_of(v)
    # one past either end does not fit
    assert not pk.packable(fm.limbs_of(pk.LIMIT)) and not pk.packable(fm.limbs_of(-pk.LIMIT - 1))


def test_settle_decides_on_the_top_limb_and_leaves_exact_digits():
    rng = random.Random(fm.SEED + 42)
    rows = []
    for top in (-pk.RULE_TOP - 2, -pk.RULE_TOP - 1, -pk.RULE_TOP, -pk.RULE_TOP + 1, 0, fm.PH, -fm.PH - 1, -2 * fm.PH):
        for low in (0, fm.MASK, 2 * fm.MASK):  # a lazy sum of two normalised elements
            rows.append([low] * 8 + [top])
        rows += [[rng.randint(0, 2 * fm.MASK) for _ in range(8)] + [top] for _ in range(200)]
    for l in rows:
        out, added = pk.settle(l)
        assert added == (l[8] < -pk.RULE_TOP)
        assert fm.value(out) == fm.value(l) + (P if added else 0)
        assert all(0 <= x <= fm.MASK for x in out[:8])
        v = fm.value(l)
        if added:
            assert v + P < P // 2 + (1 << 232)
        else:
            assert v > -(P // 2) - (1 << 232)


# ---- 40 consecutive binds ------------------------------------------------------------------------------------------------------------------
def oracle_bind(lo: int, hi: int, r_std: int) -> int:
    """the oracle's fix_variables on the two-entry table (lo, hi) mod p, as a stored integer"""
    tab = np.stack([H.raw_limbs(lo % P), H.raw_limbs(hi % P)])
    out = cref.fix_variables(tab, H.mont_challenges([r_std]))
    return sum(int(out[0, k]) << (64 * k) for k in range(4))


def chain(start: int, partner_of, r):
    """entry <- bind(entry, partner_of(k, entry)) for every challenge: the invariant and the congruence after every bind -> (values, branches)"""
    cur = fm.limbs_of(start)
    vals, branches = [], []
    for k, rk in enumerate(r):
        hi = fm.limbs_of(partner_of(k, fm.value(cur)))
        assert pk.packable(cur) and pk.packable(hi), f"bind {k + 1}: a source outside the format"
        new, added = pk.bind_packed(cur, hi, rk)
        v = fm.value(new)
        assert abs(v) < pk.LIMIT and pk.packable(new), f"bind {k + 1}: {v / P:.4f} p"
        assert -(P // 2) - (1 << 232) - k * (1 << 230) < v < P + (k + 1) * (1 << 230), f"bind {k + 1}: outside the derived range"
        assert v % P == oracle_bind(fm.value(cur), fm.value(hi), rk), f"bind {k + 1}: not the oracle's element"
        assert pk.unpack(pk.pack(new)) == new
        cur = new
        vals.append(v)
        branches.append(added)
    return vals, branches


@pytest.mark.parametrize("m", [1, 7])
@pytest.mark.parametrize("high_start", [False, True])
def test_forty_binds_of_a_sinking_entry(m, high_start):
    """every pair's slope is -m s_j and the bind's term m 2^232 - p: without the rule the entry would be at -40 p"""
    s, r = fm.sinking_challenges(BINDS, 72000 + m)
    start = P - 1 if high_start else m * sum(s)
    vals, branches = chain(start, lambda k, v: v - m * s[k], r)
    # from near zero every bind lands at about -p and is brought back; from just below p the first lands near zero and is kept
    assert all(branches[1:]) and branches[0] == (not high_start), "the branches of the range rule"
    assert max(abs(v) for v in vals) < (BINDS * m + 1) << 232, "a sinking entry now stays near zero: it rises by m 2^232 a bind"


@pytest.mark.parametrize("flip", [False, True])
def test_forty_binds_with_selector_pairs(flip):
    """every fourth bind pairs the lazy entry with the constant p - 1 (a selector table's round), either way round: slopes of about +-1.5 p"""
    m = 3
    s, r = fm.sinking_challenges(BINDS, 73000 + flip)
    rng = random.Random(73100)
    r = [rk if k % 4 != 3 else rng.randrange(P) for k, rk in enumerate(r)]
    cur = fm.limbs_of(m * sum(s))
    for k, rk in enumerate(r):
        v0 = fm.value(cur)
        other = fm.limbs_of(P - 1) if k % 4 == 3 else fm.limbs_of(v0 - m * s[k])
        lo, hi = (other, cur) if (flip and k % 4 == 3) else (cur, other)
        new, _ = pk.bind_packed(lo, hi, rk)
        v = fm.value(new)
        assert abs(v) < pk.LIMIT and pk.packable(new), f"bind {k + 1}: {v / P:.4f} p"
        assert v % P == oracle_bind(fm.value(lo), fm.value(hi), rk), f"bind {k + 1}"
        cur = new


def test_forty_binds_alternating_zero_and_p_minus_one():
    """the entry against 0 and p - 1 in turn, under random challenges and under 0, 1, p - 1"""
    rng = random.Random(74000)
    for r in ([rng.randrange(P) for _ in range(BINDS)], [0, 1, P - 1, (P - 1) // 2] * (BINDS // 4)):
        for start in (0, P - 1):
            chain(start, lambda k, v: 0 if k % 2 else P - 1, r)
            chain(start, lambda k, v: P - 1 if k % 2 else 0, r)


def test_whole_tables_against_the_oracle():
    """every entry of small sinking, selector and alternating tables through every bind: each bound table is the oracle's, entry by entry"""
    nv = 7
    s, r = fm.sinking_challenges(nv, 75000)
    point = H.mont_challenges(r)
    alt = np.stack([H.raw_limbs(0 if x % 2 == 0 else P - 1) for x in range(1 << nv)])
    tabs = [H.sinking_table_limbs(nv, s, 1, sum(s)), H.sinking_table_limbs(nv, s, 5, P - 3), H.selector_table_limbs(nv, s, 2, 2, 2 * sum(s), False),
            H.selector_table_limbs(nv, s, 3, 4, 4 * sum(s) + 9, True), alt]
    branches = set()
    for tab in tabs:
        cur = [fm.limbs_of(sum(int(tab[x, k]) << (64 * k) for k in range(4))) for x in range(1 << nv)]
        for k in range(nv):
            nxt = []
            for b in range(len(cur) // 2):
                new, added = pk.bind_packed(cur[2 * b], cur[2 * b + 1], r[k])
                assert abs(fm.value(new)) < pk.LIMIT and pk.packable(new)
                branches.add(added)
                nxt.append(new)
            cur = nxt
            want = cref.fix_variables(tab, point[:k + 1])
            for x, l in enumerate(cur):
                assert fm.value(l) % P == sum(int(want[x, j]) << (64 * j) for j in range(4)), f"bind {k + 1}, entry {x}"
    assert branches == {False, True}
