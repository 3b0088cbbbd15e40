"""Exact integer model of the carry-free field arithmetic (sumcheck_amd/csrc/fe_device.hpp and what is built on it), and the operand
vectors that pin every primitive at the limb and value ranges its call sites can reach.

Plain Python integers.  Nothing here walks limbs the way the kernels do: a Montgomery product is DEFINED as the integer
(T - M p) / 2^k with M = T p^-1 mod 2^k, and its limb form (limbs 0..7 in [0, 2^29), limb 8 the signed rest) is unique, so the device's
limbs compare bit for bit.  The lazy primitives (carry pass, line, combinations) are checked by value and by the limb ranges their
comments promise.
"""
import functools
import random

P = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
W = 29                      # bits per limb
NL = 9                      # limbs
K = W * NL                  # 261: the carry-free Montgomery radix is 2^261
MASK = (1 << W) - 1
PH = P >> 232               # 7597479: what a value of p puts into the top limb
R256 = (1 << 256) % P       # the tables' Montgomery radix
SEED = 0x5C20241008
N_RANDOM = 2000
I32_MAX = (1 << 31) - 1

# sc_debug_fe_op's op numbers (kernels_selftest.hip: FeOp)
OP_NORMALIZE, OP_CARRY_PASS, OP_TO_FR, OP_ROUND_TRIP, OP_FROM_FR = 0, 1, 2, 3, 4
OP_MUL, OP_MUL_CHAIN, OP_MUL_U, OP_MUL_U_CHAIN, OP_MUL2, OP_MUL2_CHAIN, OP_BIND, OP_BIND_CHAIN = 5, 6, 7, 8, 9, 10, 11, 12
OP_SHL5_MUL_U, OP_LINE, OP_ACCUM, OP_FOLD_CELL, OP_WIDE_VALUE, OP_WIDE_EXT = 13, 14, 15, 16, 17, 18

NODE_INF = 0x7FFFFFFF
MAX_FUSED_M = 8
LAZY_SUM_MAX_P = 282        # lane_sum.hpp: kLazySumMaxP = floor(2^31 / 7597479)


def node_value(s: int) -> int:
    """kernels.h: the evaluation nodes in the kernels' order 0, 1, inf, -1, 2, -2, 3, ..."""
    if s < 3:
        return (0, 1, NODE_INF)[s]
    return -((s - 3) // 2 + 1) if (s - 3) % 2 == 0 else (s - 3) // 2 + 2


# ---- limbs <-> integers -------------------------------------------------------------------------------------------------------------------
def value(limbs) -> int:
    return sum(int(l) << (W * i) for i, l in enumerate(limbs))


def limbs_of(v: int):
    """the unique form with limbs 0..7 in [0, 2^29) and limb 8 the signed rest"""
    return [(v >> (W * i)) & MASK for i in range(8)] + [v >> (W * 8)]


def words_of(v: int):
    """8 x u32 of a value in [0, 2^256)"""
    assert 0 <= v < (1 << 256)
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def fits_i32(limbs) -> bool:
    return all(-(1 << 31) <= l <= I32_MAX for l in limbs)


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
def mont_exact(T: int, k: int = K) -> int:
    """(T - M p) / 2^k with M = T p^-1 mod 2^k, 0 <= M < 2^k: the subtractive Montgomery reduction as one exact division"""
    M = (T * pow(P, -1, 1 << k)) % (1 << k)
    q, r = divmod(T - M * P, 1 << k)
    assert r == 0
    return q


def fe_mul(a, b):
    return limbs_of(mont_exact(value(a) * value(b)))


def fe_mul2_sum(a, b, c, d):
    return limbs_of(mont_exact(value(a) * value(b) + value(c) * value(d)))


def bind_rows(r_std: int):
    """BindConst: row i = (r 2^(29 i + 58)) mod p as a plain integer, r the challenge's standard value"""
    return [(r_std << (W * i + 58)) % P for i in range(NL)]


def fe_mul_bind(d, r_std: int):
    S = sum(int(d[i]) * Ri for i, Ri in enumerate(bind_rows(r_std)))
    return limbs_of(mont_exact(S, 58))


def fe_shl5_mul_u(a, x: int):
    """fe_mul_u(a, feu_shl5(x)): the multiplier is the integer 32 x, not reduced"""
    return limbs_of(mont_exact(value(a) * (32 * x)))


def wide_fold(lanes) -> int:
    return sum(int(l) << (32 * j) for j, l in enumerate(lanes)) % P


@functools.lru_cache(maxsize=None)
def lagrange_weights(m: int, x: int):
    """a polynomial of degree m from its values at the consecutive integers -((m-1)//2) .. m//2 and its leading coefficient, at x:
    {node j: weight}, and the leading coefficient's weight (wide_tree.hpp: wide_lagrange, wide_lead) -- derived here from the definition"""
    from fractions import Fraction
    nodes = list(range(-((m - 1) // 2), m // 2 + 1))
    w = {}
    for j in nodes:
        f = Fraction(1)
        for n in nodes:
            if n != j:
                f *= Fraction(x - n, j - n)
        assert f.denominator == 1
        w[j] = int(f)
    lead = 1
    for n in nodes:
        lead *= x - n
    return w, lead


def wide_expected(m: int, t: int, vals) -> int:
    """the value at node index t of the degree-m polynomial held as vals[s] = value at node index s (s = 2: leading coefficient)"""
    x = node_value(t)
    w, lead = lagrange_weights(m, x)
    tot = lead * value(vals[2])
    for s in range(len(vals)):
        if s == 2:
            continue
        j = node_value(s)
        if j in w and s <= max(m, 2):
            tot += w[j] * value(vals[s])
    return tot


# ---- operand vectors ------------------------------------------------------------------------------------------------------------------------
def limb_corners(lo: int, hi: int, top_lo: int = None, top_hi: int = None):
    """the limb-level corners of the box [lo, hi]^8 x [top_lo, top_hi]"""
    top_lo = lo if top_lo is None else top_lo
    top_hi = hi if top_hi is None else top_hi
    out = [[hi] * 8 + [top_hi], [lo] * 8 + [top_lo]]
    out.append([(hi if i % 2 == 0 else lo) for i in range(8)] + [top_hi])
    out.append([(lo if i % 2 == 0 else hi) for i in range(8)] + [top_lo])
    for i in range(NL):
        for bound in ((lo, hi) if i < 8 else (top_lo, top_hi)):
            v = [0] * NL
            v[i] = bound
            out.append(v)
    return out


def value_corners(bound: int, max_p: int):
    """value-level extremes as canonical limbs: +-(bound - 1), 0, +-1, p, p - 1, and multiples of p up to max_p (both signs)"""
    vals = [bound - 1, -(bound - 1), 0, 1, -1, P, P - 1, 1 - P, -P]
    k = 2
    while k <= max_p:
        vals += [k * P, -k * P, k * P - 1, 1 - k * P]
        k *= 2
    if max_p >= 1:
        vals += [max_p * P, -max_p * P]
    return [limbs_of(v) for v in vals if abs(v) < bound]


def random_limbs(rng: random.Random, n: int, lo: int, hi: int, top_lo: int = None, top_hi: int = None):
    top_lo = lo if top_lo is None else top_lo
    top_hi = hi if top_hi is None else top_hi
    return [[rng.randint(lo, hi) for _ in range(8)] + [rng.randint(top_lo, top_hi)] for _ in range(n)]


def box(lo, hi, top_lo=None, top_hi=None, value_bound=None, max_p=0):
    """a description of an operand's audited range"""
    return dict(lo=lo, hi=hi, top_lo=lo if top_lo is None else top_lo, top_hi=hi if top_hi is None else top_hi, value_bound=value_bound, max_p=max_p)


def in_box(limbs, bx) -> bool:
    return all(bx["lo"] <= l <= bx["hi"] for l in limbs[:8]) and bx["top_lo"] <= limbs[8] <= bx["top_hi"]


def corners_of(bx):
    out = limb_corners(bx["lo"], bx["hi"], bx["top_lo"], bx["top_hi"])
    if bx["value_bound"] is not None:
        out += [v for v in value_corners(bx["value_bound"], bx["max_p"]) if in_box(v, bx)]
    return out


def operand_sets(boxes, rng: random.Random, n_random: int = N_RANDOM):
    """rows of operands (one list of 9 limbs per box): the corners of every operand against the corners of the others (cyclically
    shifted, so that every corner of every operand meets several corners of the rest), then uniform draws inside the boxes"""
    cs = [corners_of(b) for b in boxes]
    n = max(len(c) for c in cs)
    rows = []
    for shift in range(n if len(boxes) > 1 else 1):
        for i in range(n):
            rows.append([cs[k][(i + k * shift) % len(cs[k])] for k in range(len(boxes))])
    rnd = [random_limbs(rng, n_random, b["lo"], b["hi"], b["top_lo"], b["top_hi"]) for b in boxes]
    rows += [[rnd[k][i] for k in range(len(boxes))] for i in range(n_random)]
    return rows


# The audited ranges.  T29 = 2^29.
T29 = 1 << W
# fe_mul / fe_mul_u, first operand: a value plus one lazy add or sub of carry-passed values -- |limb| <= 2^30 on all nine limbs
BOX_MUL_A = box(-(1 << 30), 1 << 30)
# fe_mul, second operand: a carry-passed value or a difference of two (wide_quad: fe_sub(h, l) of entries in [-4, 2^29 + 4)) -- |limb| <= 2^29 + 16
BOX_MUL_B = box(-(T29 + 16), T29 + 16)
# fe_mul_u's uniform operand: normalised limbs (feu_shl5's result, a challenge)
BOX_FEU = box(0, MASK)
# fe_mul2_sum: four carry-passed operands
BOX_MUL2 = box(-(T29 + 4), T29 + 4)
# fe_mul_bind: the lazy difference of two table entries
BOX_BIND_D = box(-(T29 + 16), T29 + 16)
# fe_carry_pass: any int32 in limbs 0..7 (sums of four carry-passed values, wide_quad_m1); limb 8 must take a carry of [-4, 3]
BOX_CARRY = box(-(1 << 31), I32_MAX, -(1 << 31) + 8, I32_MAX - 8)
# fe_normalize: limbs that take a carry of [-4, 3] without leaving int32
BOX_NORM = box(-(1 << 31) + 8, I32_MAX - 8)
# fe_to_fr: carry-passed limbs, ANY top limb (a lazy sum of 282 products of magnitude p fills the int32: kLazySumMaxP)
BOX_TO_FR = box(-8, T29 + 8, -(1 << 31) + 8, I32_MAX - 8, value_bound=LAZY_SUM_MAX_P * P, max_p=LAZY_SUM_MAX_P - 1)
# fe_line: two table entries as the LDS-resident kernels hold them -- carry-passed, the value a lazy sum within (-16 p, 16 p)
BOX_LINE = box(-4, T29 + 3, -16 * PH - 16, 16 * PH + 16, value_bound=16 * P, max_p=15)
# fe_comb5: a half's values -- fe_mul results and carry-passed sums of five of them (wide_quad_m1 / _p2)
BOX_COMB5 = box(-8, T29 + 8, -8 * PH - 8, 8 * PH + 8, value_bound=8 * P, max_p=7)
# wide_ext: a product tree's values -- fe_mul results of operands within 2 p
BOX_WIDE_EXT = box(0, MASK, -2 * PH - 2, 2 * PH + 2, value_bound=2 * P, max_p=1)

LINE_NODES = [node_value(t) for t in range(MAX_FUSED_M + 1)]  # 0, 1, inf, -1, 2, -2, 3, -3, 4
# wide_value<m, t> as the trees of five to eight instantiate it (m = 1: the single factor's line through fe_comb5)
WIDE_VALUE_CASES = [(4, t) for t in range(5, 9)] + [(3, t) for t in range(4, 8)] + [(2, t) for t in range(3, 7)] + [(1, t) for t in range(3, 6)]
# wide_ext<m, t> as the trees of nine to twelve instantiate it
WIDE_EXT_CASES = [(8, t) for t in range(9, 13)] + [(mb, t) for mb in range(1, 5) for t in range(max(mb, 2) + 1, mb + 9)]


def to_fr_vectors(rng: random.Random):
    """fe_to_fr: the box's corners, and the top limb on both sides of every quotient step out to the int32's end"""
    rows = corners_of(BOX_TO_FR) + random_limbs(rng, N_RANDOM, BOX_TO_FR["lo"], BOX_TO_FR["hi"], BOX_TO_FR["top_lo"], BOX_TO_FR["top_hi"])
    lows = [[0] * 8, [MASK] * 8, [T29 + 8] * 8, [-8] * 8]
    for k in range(1, LAZY_SUM_MAX_P + 1):
        for top in (k * (PH + 1) - 1, k * (PH + 1), -k * PH, -k * PH - 1):
            if BOX_TO_FR["top_lo"] <= top <= BOX_TO_FR["top_hi"]:
                rows.append(lows[k % 4] + [top])
                rows.append([rng.randint(0, MASK) for _ in range(8)] + [top])
    return rows


def fold_cell_vectors(rng: random.Random):
    top = (1 << 63) - 1
    rows = [[top] * 8, [0] * 8, [1] + [0] * 7, [0] * 7 + [top], [top] + [0] * 7, [0xFFFFFFFF] * 8, [1 << 32] * 8]
    for j in range(8):
        v = [0] * 8
        v[j] = top
        rows.append(v)
    rows += [[rng.randint(0, top) for _ in range(8)] for _ in range(N_RANDOM)]
    # sums the GKR initialisations make: up to 2^31 canonical words per lane
    rows += [[rng.randint(0, (1 << 63) - 1) >> rng.randint(0, 40) for _ in range(8)] for _ in range(200)]
    return rows


def product_regimes():
    """the accumulate op's terms: the ends of fe_mul's window on canonical operands -- 1 - p (limb 8 = -7597480) and p - 1 (limb 8 = 7597479)"""
    return {"1-p": limbs_of(1 - P), "p-1": limbs_of(P - 1)}


# ---- lazy table entries: the binds as the kernels run them, and tables that reach the ends of the entries' range ------------------
def carry_pass(a):
    """fe_device.hpp: fe_carry_pass -- every limb sheds its bits above 2^29 into the next one at once; limb 8 takes limb 7's carry, unreduced"""
    assert fits_i32(a)
    r = [a[0] & MASK] + [(a[i] & MASK) + (a[i - 1] >> W) for i in range(1, 8)] + [a[8] + (a[7] >> W)]
    assert fits_i32(r)
    return r


def fe_add(a, b):
    return [x + y for x, y in zip(a, b)]


def fe_sub(a, b):
    return [x - y for x, y in zip(a, b)]


def bind_f29(lo, hi, r_std: int):
    """load_factor.hpp's bind into the internal table format: lo + fe_mul_bind(hi - lo), one carry pass, no reduction"""
    return carry_pass(fe_add(lo, fe_mul_bind(fe_sub(hi, lo), r_std)))


def bind_lds(lo, hi, r_mont: int):
    """bt_bind_pass (batch_round.hpp: bt_bind's and k_tail_slices' bind in LDS): lo + fe_mul_u(hi - lo, 32 r), r the challenge as stored (Montgomery form), one carry pass"""
    return carry_pass(fe_add(lo, fe_shl5_mul_u(fe_sub(hi, lo), r_mont)))


def fe_line(lo, hi, x: int):
    """kernel_common.hpp: fe_line, step by step (one carry pass per step) -> (result, every intermediate handed to fe_carry_pass)"""
    if x == 0:
        return lo, []
    if x == 1:
        return hi, []
    step = fe_sub(hi, lo)
    if x == NODE_INF:
        return step, []
    seen = []
    if x < 0:
        cur = fe_sub(lo, step)
        for _ in range(-1, x, -1):
            seen.append(cur)
            cur = fe_sub(carry_pass(cur), step)
    else:
        cur = fe_add(hi, step)
        for _ in range(2, x):
            seen.append(cur)
            cur = fe_add(carry_pass(cur), step)
    seen.append(cur)
    return carry_pass(cur), seen


# delta: above 2^230 (the upper end of a bind's term) so that the term HAS to be m delta - p, and small enough that k binds of m delta leave
# an entry within 2^242 of -k p for every k m < 2^9 (2^240 forces the same terms; its entries pass -k p + 2^242 from k m = 4 on)
DELTA = 1 << 232
DELTA_WIDE = 1 << 240


def sinking_challenges(nv: int, seed: int, delta: int = DELTA):
    """-> (s, r): s_j in [1, 2^200) and the challenge r_j = delta / (p - s_j) mod p in STANDARD form, round j = 1..nv at index j - 1.
    A slope of value -m s_j times r_j is m delta (mod p), and both bind forms return a term in (-p - 2^230, 2^230): so m delta - p, for
    every 2^230 < m delta < p - 2^230.  An entry sinks by p - m delta in every bind: the lower end of (-(k + 1) p, p) after k."""
    rng = random.Random(seed)
    s = [rng.randrange(1, 1 << 200) for _ in range(nv)]
    return s, [delta * pow(P - sj, -1, P) % P for sj in s]


def sinking_table(nv: int, s, m: int, c: int):
    """the STORED integers e(x) = c - m sum_j x_j s_j (x_j = bit j - 1 of the index: the variable round j binds), all in [0, p)"""
    assert len(s) == nv and m >= 1 and m * sum(s) <= c < P
    tab = [c]
    for sj in s:
        tab = tab + [v - m * sj for v in tab]
    return tab


def selector_table(nv: int, s, sel: int, m: int, c: int, flip: bool = False):
    """a sinking table (in the other variables) on the half x_sel = 0, the constant p - 1 on the half x_sel = 1 (sel counts from 0: the
    variable round sel + 1 binds): after sel binds every pair is (an entry at -sel p, p - 1).  flip: the halves the other way round"""
    assert 0 <= sel < nv
    half = sinking_table(nv - 1, list(s[:sel]) + list(s[sel + 1:]), m, c)
    lo_mask = (1 << sel) - 1
    const_bit = 0 if flip else 1
    return [P - 1 if (x >> sel) & 1 == const_bit else half[(x & lo_mask) | ((x >> (sel + 1)) << sel)] for x in range(1 << nv)]


# ---- every factor of a product at its range end at once: BtPairProduct, the product loop of k_tail_slices and bt_sum_message --
MAX_WIDE_M = 12             # kernels.h: kMaxWideM
LINE_REACH_MAX_P = 70       # kernels.h: kLineReachMaxP = floor(2^261 / p)


def product_chain(vals, strict: bool = True):
    """BtPairProduct (batch_round.hpp: the one product loop of k_tail_slices and bt_sum_message): the first factor is handed on as the running product, every further one is
    fe_mul(val, prod) -- val the FIRST operand (BOX_MUL_A), the running product the SECOND (BOX_MUL_B), every result an int32 vector.
    A multiplicity e is the same value e times in `vals` (the exponent loop).  -> (product, peak |fe_mul result|, what was left: a set of
    "mul_a", "mul_b", "int32"); strict: leaving anything is an AssertionError"""
    left = set()
    prod, peak = vals[0], 0
    for val in vals[1:]:
        if not in_box(val, BOX_MUL_A):
            left.add("mul_a")
        if not in_box(prod, BOX_MUL_B):
            left.add("mul_b")
        prod = fe_mul(val, prod)
        if not fits_i32(prod):
            left.add("int32")
        peak = max(peak, abs(value(prod)))
    assert not (strict and left), f"the product chain leaves {sorted(left)}"
    return prod, peak, left


def line_reach_n(M: int) -> int:
    """the n of a line's reach (n (k + 2) - 1) p for entries in (-(k + 1) p, p): node x > 0 is x - 1 slopes beyond hi, node -x is x slopes
    beyond lo, and a product of M takes the nodes node_value(0 .. M) -- kernels.h: line_reach_n(D) = (D + 1) / 2"""
    n = max(x if x > 0 else 1 - x for x in (node_value(t) for t in range(M + 1)) if x != NODE_INF)
    assert n == (M + 1) // 2 or M == 1
    return n


def line_needs_canonical(n: int, worst_p: int) -> bool:
    """kernels.h: line_needs_canonical -- entries in (-(worst_p - 1) p, p) put a line within (n worst_p - 1) p; beyond 69 p a chain of
    fe_muls no longer keeps its running product inside fe_mul's second operand (prod' < prod L / 70.66 + 1 in units of p)"""
    return n * worst_p > LINE_REACH_MAX_P


def lazy_binds_under_the_rule(M: int, k: int) -> int:
    """k_tail_slices<12>'s bookkeeping for a tail that starts from canonical tables (tail_worst_p(0) = 2): the binds behind an entry since it
    was last canonical, after k binds.  A bind whose result could put a line beyond the reach writes its entries canonical instead"""
    n, lazy = line_reach_n(M), 0
    for _ in range(k):
        lazy = 0 if line_needs_canonical(n, lazy + 1 + 2) else lazy + 1
    return lazy


def selector_pair(k: int, m: int, c: int, flip: bool, lazy: int = None, delta: int = DELTA):
    """a selector table's pair in round k + 1 = sel + 1, in closed form: the entry that started at the stored integer c has sunk k times,
    c + k (m delta - p), against the constant p - 1 -- (lo, hi), flip: the other way round.  lazy < k: the entry was made canonical
    k - lazy binds ago (c + (k - lazy) m delta, still below p) and has sunk `lazy` times since"""
    lazy = k if lazy is None else lazy
    assert 0 <= lazy <= k and 0 <= c and c + k * m * delta < P
    e, one = limbs_of(c + k * m * delta - lazy * P), limbs_of(P - 1)
    return (one, e) if flip else (e, one)


def all_selector_values(M: int, k: int, orient: str, t_node: int, lazy: int = None, low: bool = True, mult=None):
    """the factors of one pair's product at node index t_node, in the kernel's order, when EVERY table is a selector at sel = k
    (tests/test_gpu_lazy_entries.py: selector(): m = 1 + t % 7): orient "up" (entries on the lo side), "down" or "alt" (odd tables down);
    low: the pair whose entries started lowest (c = t) or highest (c = 7 * 2^203 + t: beyond any m sum s_j); mult: the multiplicity of every
    table (default: M distinct tables)"""
    mult = [1] * M if mult is None else mult
    vals = []
    for t, e in enumerate(mult):
        flip = orient == "down" or (orient == "alt" and t % 2 == 1)
        lo, hi = selector_pair(k, 1 + t % 7, t if low else (7 << 203) + t, flip, lazy)
        vals += [fe_line(lo, hi, node_value(t_node))[0]] * e
    return vals


# ---- the per-lane running sums of the big rounds: tree_pass of kernels_big.hip ----------------------------------------------
BIG_SUM_REDUCE_EVERY = 32   # lane_sum.hpp: kBigSumReduceEvery
BIG_TERM_WORST_P = 2        # lane_sum.hpp: kBigTermWorstP
F29_ENTRY_BOUND = 1 << 255  # f29_pack.hpp: a packed entry is a 256-bit two's-complement integer


def big_lane_sum(terms, strict: bool = True):
    """one running sum of a lane of tree_pass over its pass: sum += term, a carry pass on odd iterations, fe_from_fr(fe_to_fr(sum)) when
    (iter & 31) == 31; every limb checked against int32 after every step.  -> (the sum, peak |limb 8| in units of p >> 232, the
    iteration at which a limb left int32 or None); strict: leaving is an AssertionError"""
    acc, peak = [0] * NL, 0
    for it, term in enumerate(terms):
        acc = fe_add(acc, term)
        peak = max(peak, abs(acc[8]))
        if not fits_i32(acc):
            assert not strict, f"the running sum leaves int32 in iteration {it}: limb 8 = {acc[8]} ({acc[8] / PH:.1f} p)"
            return acc, peak / PH, it
        if it & 1:
            acc = carry_pass(acc)
        if (it & (BIG_SUM_REDUCE_EVERY - 1)) == BIG_SUM_REDUCE_EVERY - 1:
            acc = limbs_of(value(acc) % P)
    return acc, peak / PH, None


def big_lane_sum_pairs(operands, strict: bool = True):
    """the two-pair form: a term is fe_mul2_sum(a, b, c, d) -- the final products of pairs b and b + stride behind ONE Montgomery reduction,
    so 64 products make 32 terms; operands: (a, b, c, d) per iteration, each inside BOX_MUL2"""
    for ops in operands:
        assert all(in_box(x, BOX_MUL2) for x in ops)
    return big_lane_sum([fe_mul2_sum(*ops) for ops in operands], strict)


def product_term_bound_p(j: int, two_pairs: bool) -> float:
    """DESIGN 4.6's bound on one term of a product of two to four whose factors are lazy entries in (-j p, p), in units of p: a product
    of lines within j p is within (1 + j^2 / 70) p; the two-pair form puts two of them behind one reduction"""
    return (2 if two_pairs else 1) * (1 + j * j / 70)


def tree_terms(M: int, lo, hi, lo2=None, hi2=None):
    """the M + 1 terms tree_pass adds for one iteration from its factors' line ends (lists of M limb vectors; lo2 / hi2: the second pair of
    the two-pair form), in the kernel's order of operations.  Nodes 0, 1, inf, -1, 2"""
    def quad(l0, h0, l1, h1):
        return fe_mul(l0, l1), fe_mul(h0, h1), fe_mul(fe_sub(h0, l0), fe_sub(h1, l1))

    def qm1(q):  # q(-1) = 2 q(inf) + 2 q(0) - q(1)
        return carry_pass(fe_sub(fe_add(fe_add(q[2], q[2]), fe_add(q[0], q[0])), q[1]))

    def qp2(q):  # q(2) = 2 q(inf) + 2 q(1) - q(0)
        return carry_pass(fe_sub(fe_add(fe_add(q[2], q[2]), fe_add(q[1], q[1])), q[0]))

    two = lo2 is not None
    mul = (lambda a, b, c, d: fe_mul2_sum(a, b, c, d)) if two else (lambda a, b, c, d: fe_mul(a, b))
    L2, H2 = (lo2, hi2) if two else (lo, hi)
    if M == 1:
        assert not two
        return [lo[0], hi[0]]
    if M == 2:
        return [mul(lo[0], lo[1], L2[0], L2[1]), mul(hi[0], hi[1], H2[0], H2[1]),
                mul(fe_sub(hi[0], lo[0]), fe_sub(hi[1], lo[1]), fe_sub(H2[0], L2[0]), fe_sub(H2[1], L2[1]))]
    q, s = quad(lo[0], hi[0], lo[1], hi[1]), quad(L2[0], H2[0], L2[1], H2[1])
    if M == 3:
        f = lambda l, h: carry_pass(fe_sub(fe_add(l, l), h))  # f2(-1) = 2 lo - hi
        return [mul(lo[2], q[0], L2[2], s[0]), mul(hi[2], q[1], H2[2], s[1]), mul(fe_sub(hi[2], lo[2]), q[2], fe_sub(H2[2], L2[2]), s[2]),
                mul(f(lo[2], hi[2]), qm1(q), f(L2[2], H2[2]), qm1(s))]
    assert M == 4
    qb, sb = quad(lo[2], hi[2], lo[3], hi[3]), quad(L2[2], H2[2], L2[3], H2[3])
    return [mul(q[0], qb[0], s[0], sb[0]), mul(q[1], qb[1], s[1], sb[1]), mul(q[2], qb[2], s[2], sb[2]),
            mul(qm1(q), qm1(qb), qm1(s), qm1(sb)), mul(qp2(q), qp2(qb), qp2(s), qp2(sb))]


def to_mont(r_std: int) -> int:
    """a standard-form value as the API takes it and the tables store it"""
    return r_std * R256 % P
