"""Bit-exact model of the packed internal table format (sumcheck_amd/csrc/f29_pack.hpp): pack, unpack and the range rule, word by word
and limb by limb as the device code runs them, on top of tests/fe_model.py (which stays as it is).

An entry is nine limbs, limbs 0..7 in [0, 2^29) and limb 8 signed in 24 bits; packed it is its VALUE as a 256-bit two's-complement
integer in eight 32-bit words.  A bind into the format is lo + fe_mul_bind(hi - lo), then `settle`: p is added once where limb 8 of the
un-normalised sum reads below -(floor(p / 2^233) + 1), inside the carry chain that makes limbs 0..7 exact digits.  The invariant the format
rests on: from canonical tables, after k binds every entry lies in (-p / 2 - 2^232 - (k - 1) 2^230, p + k 2^230), inside
[-2^255, 2^255)."""
from tests import fe_model as fm

P, W, MASK = fm.P, fm.W, fm.MASK
M32 = 0xFFFFFFFF
HALF_P_TOP = fm.PH >> 1        # H = floor(p / 2^233)
RULE_TOP = HALF_P_TOP + 1      # p is added where limb 8 reads below -RULE_TOP: the value within 2^232 of -p / 2 on either side
LIMIT = 1 << 255               # |stored value| < LIMIT
TOP_LO, TOP_HI = -(1 << 23), (1 << 23) - 1


def p_limbs():
    return fm.limbs_of(P)


def _i32(x: int) -> int:
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def packable(l) -> bool:
    return all(0 <= x <= MASK for x in l[:8]) and TOP_LO <= l[8] <= TOP_HI


def pack(l):
    """f29_pack: word k = (limb k >> 3k) | (limb k+1 << (29 - 3k)), in 32-bit arithmetic"""
    assert packable(l), l
    return [(((l[k] & M32) >> (3 * k)) | ((l[k + 1] << (29 - 3 * k)) & M32)) & M32 for k in range(8)]


def unpack(w):
    """f29_unpack: fe_from_fr's shifts, limb 8 with an arithmetic shift"""
    l = [w[0] & MASK]
    for i in range(1, 8):
        l.append(((w[i - 1] >> (32 - 3 * i)) | ((w[i] << (3 * i)) & M32)) & MASK)
    l.append(_i32(w[7]) >> 8)
    return l


def packed_value(w) -> int:
    """the eight words read as ONE 256-bit two's-complement integer"""
    v = sum(int(x) << (32 * i) for i, x in enumerate(w))
    return v - (1 << 256) if v >> 255 else v


def settle(l):
    """f29_settle -> (limbs, added): int32 arithmetic, step by step"""
    assert fm.fits_i32(l)
    add = l[8] < -RULE_TOP
    pl = p_limbs()
    out, c = [], 0
    for i in range(8):
        t = l[i] + (pl[i] if add else 0) + c
        assert -(1 << 31) <= t <= fm.I32_MAX
        out.append(t & MASK)
        c = t >> W
    top = l[8] + (pl[8] if add else 0) + c
    assert -(1 << 31) <= top <= fm.I32_MAX
    return out + [top], add


def bind_packed(lo, hi, r_std: int):
    """load_factor.hpp's bind into the packed format -> (limbs, added)"""
    return settle(fm.fe_add(lo, fm.fe_mul_bind(fm.fe_sub(hi, lo), r_std)))


def corner_limbs():
    """the corners the format is pinned at: the ends of the range, the values around zero, +-p and +-p / 2, and the limb-level ends"""
    vals = [-LIMIT, LIMIT - 1, 0, -1, 1]
    for base in (P, -P, P // 2, -(P // 2)):
        vals += [base - 1, base, base + 1]
    rows = [fm.limbs_of(v) for v in vals]
    for low in (0, MASK):
        for top in (TOP_LO, TOP_HI):
            rows.append([low] * 8 + [top])
    return rows
