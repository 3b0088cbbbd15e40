"""Inputs of tests/test_gpu_gkr_edges.py (and of tests/test_gkr_edges_host.py, which builds every one of them without a GPU): single-instance
GKR rounds at the sizes where sumcheck_amd/csrc/gkr.hip changes route, at its largest dims and at the ends of the field's range.

What decides a route (gkr.hip):
  bucketed_form_pays / sparse_fix   2^dim <= 8 n + 1024: the bucketed kernels (and, in the list form, the eq TABLE); else the list form with eq
                                    evaluated per entry (k_sparse_scale_direct, plan gkr.eq_direct).  n is the list's length: nnz for the fold over
                                    g, the merged count n1 for the fold over u
  bucket_plan                       c = max(dim - 11, 0) cell bits per bucket, nb = 2^(dim - c) buckets (2048 from dim 11 on), and a bucket takes at
                                    most max(8192, 64 (n / nb + 1)) entries; one entry more anywhere and the list form takes the whole table
  grouped / counted                 phase two of an index-ordered list reads its buckets in place (gkr.bucketed_grouped); phase one, and any
                                    unordered list, goes through the counting sort (gkr.bucketed_counted)

Every builder asserts in numpy the facts its expected route rests on -- the inequality above on nnz and on n1, the fullest x and y bucket against
the cap -- and states which gkr.* plan counters each of the three calls must move (`expect`); the GPU test asserts exactly those."""
from dataclasses import dataclass

import numpy as np

from oracle import cref
from tests import helpers as H
from tests.test_gpu_gkr_batch_rounds import EDGE, P, raw

GROUPED, COUNTED, LIST, EQ_DIRECT, COEFF = ("gkr.bucketed_grouped", "gkr.bucketed_counted", "gkr.list_form", "gkr.eq_direct",
                                            "gkr.coeff_from_bound_table")
ONE = EDGE[1]
SEED = 0x6ED6E


def table_pays(n, k):
    """sparse_fix's eq table over k variables for a list of n entries (else the direct evaluation); with k = dim also bucketed_form_pays"""
    return n > 0 and (1 << k) <= 8 * n + 1024


def geometry(dim):
    """-> (cell bits per bucket, buckets)"""
    c = max(dim - 11, 0)
    assert c <= 10, "bucket_plan refuses more than 1024 cells per bucket"
    return c, 1 << (dim - c)


def cap(n, dim):
    """the most entries one bucket may hold in a list of n"""
    return max(8192, 64 * (n // geometry(dim)[1] + 1))


def bucket_counts(idx, dim, cell_shift):
    """entries per bucket when the cell is the dim-bit field of the index at `cell_shift`"""
    c, nb = geometry(dim)
    cell = (np.asarray(idx, dtype=np.uint64) >> np.uint64(cell_shift)) & np.uint64((1 << dim) - 1)
    return np.bincount((cell >> np.uint64(c)).astype(np.int64), minlength=nb)


def boolean_point(b, dim):
    """the point of {0, 1}^dim whose eq is 1 at index b and 0 elsewhere"""
    return np.stack([EDGE[(b >> j) & 1] for j in range(dim)])


def is_sorted(idx):
    return bool(np.all(idx[:-1] <= idx[1:]))


@dataclass
class Facts:
    nnz: int
    x_max: int   # fullest x bucket of f1 (phase one's cells)
    y_max: int   # fullest y bucket of f1 (phase two's cells inside sc_gkr_prove)
    x_rest: int  # the fullest x bucket but one
    cap: int     # for a list of nnz entries
    f1g: np.ndarray  # the distinct (x, y): the indices of f1(g, ., .)
    n1: int
    y1_max: int  # fullest y bucket of f1(g, ., .) (initialize_phase_two's cells)
    cap1: int    # for a list of n1 entries


def facts(idx, dim):
    xs = np.sort(bucket_counts(idx, dim, dim))
    f1g = np.unique(np.asarray(idx, dtype=np.uint64) >> np.uint64(dim))
    return Facts(nnz=int(idx.shape[0]), x_max=int(xs[-1]), x_rest=int(xs[-2]) if xs.shape[0] > 1 else 0, y_max=int(bucket_counts(idx, dim, 2 * dim).max()),
                 cap=cap(idx.shape[0], dim), f1g=f1g, n1=int(f1g.shape[0]), y1_max=int(bucket_counts(f1g, dim, dim).max()), cap1=cap(f1g.shape[0], dim))


@dataclass
class Case:
    """one sc_gkr_prove input; `shuffled`: f1 arrives out of index order, and initialize_phase_two gets f1(g, ., .) in reverse order"""
    name: str
    dim: int
    idx: np.ndarray
    vals: np.ndarray
    f2: np.ndarray
    f3: np.ndarray
    g: np.ndarray
    u: np.ndarray        # initialize_phase_two's point
    shuffled: bool
    expect: dict         # call -> {gkr.* plan: launches}, complete: a gkr.* plan not named must not move
    n1: int
    gkr_direct: int = 1  # policy "gkr_direct": 0 forces the list form

    def oracle_f1(self):
        """f1 as the map the oracle takes: repeated indices summed"""
        return H.merge_repeated(self.idx, self.vals)


def _make(name, dim, idx, vals, f2, f3, g, u, shuffled, expect, n1, gkr_direct=1):
    idx = np.ascontiguousarray(idx, dtype=np.uint64)
    assert idx.shape[0] == vals.shape[0] and int(idx.max()) < (1 << (3 * dim)) and 1 <= dim <= 21
    assert f2.shape == f3.shape == (1 << dim, 4) and g.shape == u.shape == (dim, 4)
    assert shuffled == (not is_sorted(idx)), "`shuffled` says whether the index check finds the list out of order"
    assert set(expect) == {"phase_one", "phase_two", "prove"} and all(set(v) <= {GROUPED, COUNTED, LIST, EQ_DIRECT, COEFF} for v in expect.values())
    for a in (idx, vals, f2, f3, g, u):
        a.setflags(write=False)
    return Case(name, dim, idx, vals, f2, f3, g, u, shuffled, expect, n1, gkr_direct)


def _tables(dim, seed):
    """random f2, f3, g, u"""
    return cref.synth_table(seed, 2, 1 << dim), cref.synth_table(seed, 3, 1 << dim), cref.synth_table(seed, 4, dim), cref.synth_table(seed, 5, dim)


def unique_indices(rng, bits, n, must=()):
    """n distinct indices below 2^bits, uniform over the whole range, in index order; the ones in `must` among them"""
    must = np.array(sorted(set(must)), dtype=np.uint64)
    assert n >= must.shape[0] and n <= (1 << bits)
    pool = np.zeros(0, dtype=np.uint64)
    while pool.shape[0] < n - must.shape[0]:
        draw = rng.integers(0, 1 << bits, size=n + n // 4 + 64, dtype=np.uint64)
        pool = np.setdiff1d(np.union1d(pool, draw), must)
    pool = pool[rng.permutation(pool.shape[0])[:n - must.shape[0]]]
    return np.sort(np.concatenate([must, pool]))


def _ordered(rng, idx, shuffled):
    """the list in index order, or in an order that is not"""
    idx = np.sort(idx)
    if shuffled and idx.shape[0] > 1:
        idx = idx[rng.permutation(idx.shape[0])]
        if is_sorted(idx):
            idx = idx[::-1].copy()
    return idx


def _routes_bucketed(shuffled, n1):
    """every table through the bucketed kernels"""
    p2 = COUNTED if shuffled and n1 > 1 else GROUPED
    prove = {COUNTED: 2, COEFF: 1} if shuffled else {GROUPED: 1, COUNTED: 1, COEFF: 1}
    return {"phase_one": {COUNTED: 1}, "phase_two": {p2: 1}, "prove": prove}


def _routes_sparse():
    """too sparse for 2^dim cells or an eq table, before and after the merge: the list form with eq evaluated per entry, in both phases"""
    return {"phase_one": {LIST: 1, EQ_DIRECT: 1}, "phase_two": {LIST: 1, EQ_DIRECT: 1}, "prove": {LIST: 2, EQ_DIRECT: 2, COEFF: 1}}


# ---- a, b: the sparse switch ---------------------------------------------------------------------------------------------------------------
def sparse_case(dim, nnz, shuffled, top=False, ends=False):
    """nnz distinct random indices over all 3 dim bits.  top: the single index 2^(3 dim) - 1; ends: index 0 and 2^(3 dim) - 1 among them.
    Bucketed when 2^dim <= 8 nnz + 1024 (dim 11: from nnz = 128 on), else the list form with the direct eq evaluation in both phases."""
    rng = np.random.default_rng(SEED + 1000 * dim + nnz)
    last = (1 << (3 * dim)) - 1
    must = [last] if top else [0, last] if ends else []
    idx = _ordered(rng, unique_indices(rng, 3 * dim, nnz, must), shuffled)
    f = facts(idx, dim)
    assert f.n1 == nnz, "distinct (x, y) here: the merge must not change which side of the inequality phase two is on"
    if table_pays(nnz, dim):
        assert nnz == 128 and dim == 11 and (1 << dim) == 8 * nnz + 1024, "the first list length that pays at dim 11"
        assert max(f.x_max, f.y_max) <= f.cap and f.y1_max <= f.cap1
        expect = _routes_bucketed(shuffled, f.n1)
    else:
        assert (1 << dim) > 8 * nnz + 1024 and (1 << dim) > 8 * f.n1 + 1024
        assert dim != 11 or nnz in (1, 127), "dim 11: the last list length that does not pay, and a single entry"
        expect = _routes_sparse()
    f2, f3, g, u = _tables(dim, SEED + dim)
    name = f"sparse-dim{dim}-nnz{nnz}" + ("-top" if top else "") + ("-shuffled" if shuffled else "")
    return _make(name, dim, idx, cref.synth_table(SEED + dim, 1, nnz), f2, f3, g, u, shuffled, expect, f.n1)


# ---- c: the collapsing list ----------------------------------------------------------------------------------------------------------------
def collapsing_case(shuffled):
    """dim 12, 12000 non-zeros on 4 (x, y) pairs inside one x bucket: phase one's bucketed attempt finds 12000 > 8192 entries in it and the list
    form folds them with the eq TABLE (4096 <= 8 * 12000 + 1024); phase two then folds n1 = 4 entries, where 4096 > 8 * 4 + 1024: direct"""
    dim, per = 12, 3000
    rng = np.random.default_rng(SEED + 12000)
    x0 = 2 * 777
    pairs = [(x0, 5), (x0, 4000), (x0 + 1, 5), (x0 + 1, 2222)]
    assert geometry(dim)[0] == 1 and len({x >> 1 for x, _ in pairs}) == 1 and len(set(pairs)) == 4
    idx = np.concatenate([rng.permutation(1 << dim)[:per].astype(np.uint64) | np.uint64((x << dim) | (y << (2 * dim))) for x, y in pairs])
    idx = _ordered(rng, idx, shuffled)
    f = facts(idx, dim)
    assert f.nnz == 12000 == np.unique(idx).shape[0] and f.n1 == 4
    assert table_pays(f.nnz, dim) and f.x_max == 12000 > f.cap == 8192 and not table_pays(f.n1, dim)
    expect = {"phase_one": {COUNTED: 1, LIST: 1}, "phase_two": {LIST: 1, EQ_DIRECT: 1},
              "prove": {COUNTED: 2, LIST: 2, EQ_DIRECT: 1, COEFF: 1} if shuffled else {GROUPED: 1, COUNTED: 1, LIST: 2, EQ_DIRECT: 1, COEFF: 1}}
    f2, f3, g, u = _tables(dim, SEED + 12)
    return _make("collapsing" + ("-shuffled" if shuffled else ""), dim, idx, cref.synth_table(SEED + 12, 1, f.nnz), f2, f3, g, u, shuffled, expect, f.n1)


# ---- d: dense lists at the untested geometries ---------------------------------------------------------------------------------------------
def dense_case(dim, log_nnz, shuffled):
    """2^log_nnz distinct random indices: bucketed, c = kh = dim - 11.  dim 21 is check_gkr_args' last: 63-bit indices, 1024 cells = 64 KiB of LDS
    per workgroup, kMaxBuckets buckets; 2^18 is the shortest list that still pays there"""
    nnz = 1 << log_nnz
    rng = np.random.default_rng(SEED + 100 * dim + log_nnz)
    idx = _ordered(rng, unique_indices(rng, 3 * dim, nnz), shuffled)
    f = facts(idx, dim)
    assert geometry(dim) == (dim - 11, 2048)
    assert table_pays(nnz, dim) and table_pays(f.n1, dim), "before and after the merge"
    assert dim != 21 or not table_pays(nnz // 2, dim), "dim 21 at the shortest power of two that pays"
    assert max(f.x_max, f.y_max) <= f.cap and f.y1_max <= f.cap1
    f2, f3, g, u = _tables(dim, SEED + dim)
    return _make(f"dense-dim{dim}-nnz2^{log_nnz}" + ("-shuffled" if shuffled else ""), dim, idx, cref.synth_table(SEED + dim, 1, nnz), f2, f3, g, u, shuffled,
                 _routes_bucketed(shuffled, f.n1), f.n1)


# ---- e, f: exactly at the cap and one over; the fullest cell -------------------------------------------------------------------------------
def one_cell_case(count, shuffled, extreme):
    """dim 11 (one cell per bucket, cap 8192): ONE index `count` times, so that its x cell and its y cell hold `count` terms each.  8192 stays
    bucketed in both phases, 8193 is refused by both.  shuffled: two more entries in other cells, in front and behind, so that the list is out of order
    (the counting sort, and k_bucket_accumulate's (term, cell) pairs) while the full cell stays exactly as full.
    extreme: every phase-one term has the limbs of p - 1 -- g is the boolean point of z (eq = 1), f3 = 1, the values' stored limbs are p - 1 -- and so
    has every term of initialize_phase_two, whose u is the boolean point of x either way."""
    dim = 11
    z0, x0, y0 = 0x5A5, 0x2B3, 0x4C6
    at = lambda z, x, y: z | (x << dim) | (y << (2 * dim))
    idx = np.full(count, at(z0, x0, y0), dtype=np.uint64)
    vals = np.tile(raw(P - 1), (count, 1)) if extreme else cref.synth_table(SEED + count, 1, count)
    if shuffled:  # (same z: under the boolean g they count too)
        idx = np.concatenate([[at(z0, x0 + 1, y0 + 1)], idx, [at(z0, x0 - 1, y0 - 1)]]).astype(np.uint64)
        vals = np.concatenate([cref.synth_table(SEED, 6, 1), vals, cref.synth_table(SEED, 7, 1)])
    f2, f3, g, _ = _tables(dim, SEED + 11)
    if extreme:
        g, f3 = boolean_point(z0, dim), np.tile(ONE, (1 << dim, 1))
    u = boolean_point(x0, dim)
    f = facts(idx, dim)
    assert f.cap == 8192 and f.x_max == f.y_max == count and f.x_rest <= 1 and table_pays(f.nnz, dim)
    assert f.n1 == (3 if shuffled else 1) and not table_pays(f.n1, dim)
    sparse_two = {LIST: 1, EQ_DIRECT: 1}  # initialize_phase_two takes the MERGED list: one entry, or three
    if count <= f.cap:
        expect = _routes_bucketed(shuffled, f.n1)
        expect["phase_two"] = sparse_two
    else:  # phase one's attempt is refused: list form with the eq table (8 * 8193 + 1024 >= 2048); phase two's fold over u is sparse
        expect = {"phase_one": {COUNTED: 1, LIST: 1}, "phase_two": sparse_two,
                  "prove": {COUNTED: 2, LIST: 2, EQ_DIRECT: 1, COEFF: 1} if shuffled else {GROUPED: 1, COUNTED: 1, LIST: 2, EQ_DIRECT: 1, COEFF: 1}}
    name = f"one-cell-{count}" + ("-extreme" if extreme else "") + ("-shuffled" if shuffled else "")
    return _make(name, dim, idx, np.ascontiguousarray(vals), f2, f3, g, u, shuffled, expect, f.n1)


def crowded_y_case(shuffled):
    """dim 11: 8193 distinct non-zeros share y and spread over every x (at most 5 per x cell): phase one stays bucketed, phase two's plan finds cap + 1
    in one y cell -- sc_gkr_prove's "crowded y buckets although the x buckets were fine" branch builds the list then"""
    dim, n = 11, 8193
    i = np.arange(n, dtype=np.uint64)
    rng = np.random.default_rng(SEED + 8193)
    idx = _ordered(rng, (i >> np.uint64(dim)) | ((i & np.uint64(2047)) << np.uint64(dim)) | np.uint64(0x3E9 << (2 * dim)), shuffled)
    f = facts(idx, dim)
    assert np.unique(idx).shape[0] == n and f.cap == 8192 and f.x_max == 5 and f.y_max == 8193 == f.cap + 1
    assert f.n1 == 2048 and table_pays(f.n1, dim) and f.y1_max == 2048 <= f.cap1 and table_pays(n, dim)
    expect = _routes_bucketed(shuffled, f.n1)
    expect["prove"] = {COUNTED: 2, LIST: 1, COEFF: 1} if shuffled else {GROUPED: 1, COUNTED: 1, LIST: 1, COEFF: 1}
    f2, f3, g, u = _tables(dim, SEED + 13)
    return _make("crowded-y-8193" + ("-shuffled" if shuffled else ""), dim, idx, cref.synth_table(SEED + 13, 1, n), f2, f3, g, u, shuffled, expect, f.n1)


def long_list_cap_case(over):
    """dim 12, 300000 distinct non-zeros: n / nb = 146, so the cap is its other arm, 64 * 147 = 9408 > 8192.  One x bucket (two cells) holds exactly
    9408 entries, or 9409 (`over`: phase one refused); every other bucket, x or y, is far below"""
    dim, n, b0 = 12, 300000, 1234
    rng = np.random.default_rng(SEED + 300000)
    assert geometry(dim) == (1, 2048) and cap(n, dim) == 64 * (146 + 1) == 9408
    k = 9408 + (1 if over else 0)
    t = rng.permutation(1 << 25)[:k].astype(np.uint64)  # (z, low bit of x, y): distinct
    crowd = (t & np.uint64(4095)) | ((np.uint64(2 * b0) + ((t >> np.uint64(12)) & np.uint64(1))) << np.uint64(dim)) | ((t >> np.uint64(13)) << np.uint64(2 * dim))
    rest = unique_indices(rng, 3 * dim, n - k + 2000)
    rest = rest[((rest >> np.uint64(dim + 1)) & np.uint64(2047)) != np.uint64(b0)]
    rest = rest[rng.permutation(rest.shape[0])[:n - k]]
    idx = _ordered(rng, np.concatenate([crowd, rest]), True)
    f = facts(idx, dim)
    assert f.nnz == n == np.unique(idx).shape[0] and f.cap == 9408 and f.x_max == k == int(bucket_counts(idx, dim, dim)[b0])
    assert f.x_rest < 8192 and f.y_max < 8192 and table_pays(n, dim) and table_pays(f.n1, dim) and f.y1_max < f.cap1
    expect = _routes_bucketed(True, f.n1)
    if over:
        expect["phase_one"] = {COUNTED: 1, LIST: 1}
        expect["prove"] = {COUNTED: 2, LIST: 2, COEFF: 1}
    f2, f3, g, u = _tables(dim, SEED + 14)
    return _make(f"long-list-{k}-in-a-bucket", dim, idx, cref.synth_table(SEED + 14, 1, n), f2, f3, g, u, True, expect, f.n1)


@dataclass
class PhaseTwoCase:
    """one initialize_phase_two input: a list f1(g, ., .) that may repeat an index"""
    name: str
    dim: int
    idx: np.ndarray
    vals: np.ndarray
    u: np.ndarray
    expect: dict

    def oracle_f1g(self):
        return H.merge_repeated(self.idx, self.vals)


def full_cell_phase_two(count, shuffled):
    """dim 11: `count` entries on one (x, y), stored limbs p - 1, u the boolean point of x: every term has the limbs of p - 1, `count` of them in one cell.
    8192 stays bucketed (an ordered list: terms computed in k_bucket_accumulate; shuffled: through the counting sort), 8193 is summed by the list form's
    reduce_by_key.  shuffled: two more entries in other y cells, same x, in front and behind"""
    dim, x0, y0 = 11, 0x2B3, 0x4C6
    idx = np.full(count, x0 | (y0 << dim), dtype=np.uint64)
    vals = np.tile(raw(P - 1), (count, 1))
    if shuffled:
        idx = np.concatenate([[x0 | ((y0 + 1) << dim)], idx, [x0 | ((y0 - 1) << dim)]]).astype(np.uint64)
        vals = np.concatenate([cref.synth_table(SEED, 8, 1), vals, cref.synth_table(SEED, 9, 1)])
    n = idx.shape[0]
    counts = np.sort(bucket_counts(idx, dim, dim))
    assert shuffled == (not is_sorted(idx)) and table_pays(n, dim) and cap(n, dim) == 8192 and counts[-1] == count and counts[-2] <= 1
    expect = {COUNTED if shuffled else GROUPED: 1}
    if count > 8192:
        expect[LIST] = 1  # (with the eq table: 2048 <= 8 n + 1024)
    for a in (idx, vals):
        a.setflags(write=False)
    return PhaseTwoCase(f"phase-two-one-cell-{count}" + ("-shuffled" if shuffled else ""), dim, idx, np.ascontiguousarray(vals), boolean_point(x0, dim), expect)


# ---- g: points and tables from {0, 1, p - 1} -----------------------------------------------------------------------------------------------
def edge_values_case(dim, mixed, list_form, shuffled):
    """g and u from {0, 1} (mixed: from {0, 1, p - 1}, each at least once), f2 and f3 from {0, 1, p - 1}, values a quarter each 0, 1, p - 1 and random.
    Most of eq(g, .) is 0: half the non-zeros get a z at which it is not, so that f1(g, ., .) holds zero and non-zero entries, and y comes from 48 values,
    so that cells collect several of them.  list_form: policy gkr_direct = 0"""
    N = 1 << dim
    nnz = 3 * N
    rng = np.random.default_rng(SEED + 10 * dim + 2 * mixed + list_form)
    pick = lambda hi, n: rng.integers(0, hi, size=n)
    g, u = EDGE[pick(3 if mixed else 2, dim)].copy(), EDGE[pick(3 if mixed else 2, dim)].copy()
    if mixed:
        g[:3], u[:3] = EDGE[[2, 0, 1]], EDGE[[1, 2, 0]]
    is_one = lambda a: np.array([np.array_equal(r, EDGE[1]) for r in a])
    is_free = lambda a: np.array([np.array_equal(r, EDGE[2]) for r in a])
    bits = lambda m: np.uint64(sum(1 << j for j in range(dim) if m[j]))
    z = pick(N, 4 * nnz).astype(np.uint64)
    live = (z & bits(is_free(g))) | bits(is_one(g))  # eq(g, .) is not 0 exactly where the bits at the coordinates from {0, 1} are g's
    z = np.where(pick(2, 4 * nnz) == 1, live, z)
    ys = pick(N, 48).astype(np.uint64)
    idx = np.unique(z | (pick(N, 4 * nnz).astype(np.uint64) << np.uint64(dim)) | (ys[pick(48, 4 * nnz)] << np.uint64(2 * dim)))
    idx = _ordered(rng, idx[rng.permutation(idx.shape[0])[:nnz]], shuffled)
    vals = cref.synth_table(SEED + dim, 1, nnz)
    kind = pick(4, nnz)
    for k in range(3):
        vals[kind == k] = EDGE[k]
    f2, f3 = EDGE[pick(3, N)].copy(), EDGE[pick(3, N)].copy()
    f = facts(idx, dim)
    assert f.nnz == nnz and table_pays(nnz, dim) and table_pays(f.n1, dim) and max(f.x_max, f.y_max) <= f.cap and f.y1_max <= f.cap1
    gz = idx & np.uint64(N - 1)
    hit = (gz & ~bits(is_free(g))) == bits(is_one(g))
    live_pairs = np.unique(idx[hit] >> np.uint64(dim)).shape[0]
    assert 0.25 < hit.mean() < 0.9 and 0 < live_pairs < f.n1, "f1(g, ., .) has entries that are zero and entries that are not"
    if list_form:  # (with the eq table in both folds: the lists pay)
        expect = {"phase_one": {LIST: 1}, "phase_two": {LIST: 1}, "prove": {LIST: 2, COEFF: 1}}
    else:
        expect = _routes_bucketed(shuffled, f.n1)
    name = f"edge-values-dim{dim}-" + ("mixed" if mixed else "boolean") + ("-list-form" if list_form else "-bucketed") + ("-shuffled" if shuffled else "")
    return _make(name, dim, idx, vals, f2, f3, g, u, shuffled, expect, f.n1, gkr_direct=0 if list_form else 1)


# ---- the registry: name -> builder ---------------------------------------------------------------------------------------------------------
def _registry():
    cases = [
        lambda: sparse_case(11, 127, False), lambda: sparse_case(11, 127, True), lambda: sparse_case(11, 128, False), lambda: sparse_case(11, 128, True),
        lambda: sparse_case(11, 1, False), lambda: sparse_case(11, 1, False, top=True),
        lambda: sparse_case(13, 64, True, ends=True), lambda: sparse_case(17, 64, False, ends=True), lambda: sparse_case(21, 4096, True, ends=True),
        lambda: collapsing_case(False), lambda: collapsing_case(True),
        lambda: dense_case(17, 17, False), lambda: dense_case(17, 17, True), lambda: dense_case(19, 17, False), lambda: dense_case(19, 17, True),
        lambda: dense_case(21, 18, False), lambda: dense_case(21, 18, True),
        lambda: one_cell_case(8192, False, False), lambda: one_cell_case(8193, False, False),
        lambda: crowded_y_case(False), lambda: crowded_y_case(True), lambda: long_list_cap_case(False), lambda: long_list_cap_case(True),
        lambda: one_cell_case(8192, False, True), lambda: one_cell_case(8192, True, True), lambda: one_cell_case(8193, False, True),
        lambda: one_cell_case(8193, True, True),
    ]
    for dim in (4, 11, 12):
        for mixed in (False, True):
            for list_form in (False, True):
                cases.append(lambda dim=dim, mixed=mixed, list_form=list_form: edge_values_case(dim, mixed, list_form, shuffled=(dim + mixed + list_form) % 2 == 1))
    return cases


NAMES = [
    "sparse-dim11-nnz127", "sparse-dim11-nnz127-shuffled", "sparse-dim11-nnz128", "sparse-dim11-nnz128-shuffled", "sparse-dim11-nnz1", "sparse-dim11-nnz1-top",
    "sparse-dim13-nnz64-shuffled", "sparse-dim17-nnz64", "sparse-dim21-nnz4096-shuffled", "collapsing", "collapsing-shuffled",
    "dense-dim17-nnz2^17", "dense-dim17-nnz2^17-shuffled", "dense-dim19-nnz2^17", "dense-dim19-nnz2^17-shuffled", "dense-dim21-nnz2^18", "dense-dim21-nnz2^18-shuffled",
    "one-cell-8192", "one-cell-8193", "crowded-y-8193", "crowded-y-8193-shuffled", "long-list-9408-in-a-bucket", "long-list-9409-in-a-bucket",
    "one-cell-8192-extreme", "one-cell-8192-extreme-shuffled", "one-cell-8193-extreme", "one-cell-8193-extreme-shuffled",
    "edge-values-dim4-boolean-bucketed", "edge-values-dim4-boolean-list-form-shuffled", "edge-values-dim4-mixed-bucketed-shuffled", "edge-values-dim4-mixed-list-form",
    "edge-values-dim11-boolean-bucketed-shuffled", "edge-values-dim11-boolean-list-form", "edge-values-dim11-mixed-bucketed", "edge-values-dim11-mixed-list-form-shuffled",
    "edge-values-dim12-boolean-bucketed", "edge-values-dim12-boolean-list-form-shuffled", "edge-values-dim12-mixed-bucketed-shuffled", "edge-values-dim12-mixed-list-form",
]
CASES = dict(zip(NAMES, _registry()))
PHASE_TWO_CASES = {f"phase-two-one-cell-{count}" + ("-shuffled" if sh else ""): (lambda count=count, sh=sh: full_cell_phase_two(count, sh))
                   for count in (8192, 8193) for sh in (False, True)}


def build(name):
    case = (CASES.get(name) or PHASE_TWO_CASES[name])()
    assert case.name == name, (case.name, name)
    return case
