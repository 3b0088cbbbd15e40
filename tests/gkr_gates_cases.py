"""The oracle of the GKR batch handle's GATE form (sc_gkr_gates_init_batch / sc_gkr_gates_next_batch), composed from oracle/cref.py, and the
inputs the CPU and the GPU tests share.  A layer of multiplication and addition gates,
    W_out[z] = sum over MUL of v f2[x] f3[y] + sum over ADD of v (f2[x] + f3[y]),
is proved at E(z) = eq(g, z), or alpha eq(g, z) + beta eq(g2, z), by
    phase one over x:  f2(x) H1(x) + H2(x),   H1[x] = sum_MUL E[z] v f3[y] + sum_ADD E[z] v,   H2[x] = sum_ADD E[z] v f3[y]
    phase two over y:  f3(y) T1(y) + T2(y),   T1[y] = f2(u) sum_MUL E[z] eq(u,x) v + sum_ADD E[z] eq(u,x) v,   T2[y] = f2(u) sum_ADD E[z] eq(u,x) v.
Every table is linear in the list and in E, so each is built from cref.gkr_phase_one / cref.gkr_phase_two (ADD's "sum E v" is phase one with a
table of ones for f3) and combined with the oracle's own field operations; the messages are a cref.Prover's over the products
[(1, [0, 1]), (1, [2])].  Each case below states the inequality it rests on."""
import ctypes as C
import os
import re

import numpy as np

from oracle import cref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = cref.P
ONE = cref.ints_to_mont([1])[0]
ZERO = cref.ints_to_mont([0])[0]
MINUS_ONE = cref.ints_to_mont([P - 1])[0]
EDGE = np.stack([ZERO, ONE, MINUS_ONE])

INIT, NEXT = "sc_gkr_gates_init_batch", "sc_gkr_gates_next_batch"
EVAL = "sc_gkr_gates_layers_eval_batch"
ONE_BLOCK, COMPOSED = "batch.gkr_gates_one_block", "batch.gkr_gates_composed"
EVAL_ONE_BLOCK, EVAL_CELLS = "batch.gkr_gates_eval_one_block", "batch.gkr_gates_eval_cells"


def _int(pattern):
    found = re.findall(pattern, open(os.path.join(ROOT, "sumcheck_amd", "csrc", "batch_shape.hpp")).read())
    assert len(found) == 1, pattern
    return int(found[0])


MAX_DIM = _int(r"constexpr int kGkrBatchMaxDim = (\d+);")
MAX_NNZ_PER_CELL = _int(r"constexpr uint64_t kGkrBatchMaxNnzPerCell = (\d+);")


def one_block_fits(dim, mul_nnz, add_nnz):
    """the envelope of batch.gkr_gates_one_block: dim <= 9 and EACH list <= 64 x 2^dim"""
    return dim <= MAX_DIM and max(mul_nnz, add_nnz) <= MAX_NNZ_PER_CELL << dim


def _vec(op, a, b):
    """a (op) b over (k, 4) arrays of Montgomery limbs with the oracle's orc_fr_mul / orc_fr_add; b may be ONE element for all rows"""
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 4)
    out = np.empty_like(a)
    fn = getattr(cref.lib(), "orc_fr_" + op)
    V = C.c_void_p
    pa, pb, po, step = a.ctypes.data, b.ctypes.data, out.ctypes.data, 0 if b.shape[0] == 1 else 32
    for e in range(a.shape[0]):
        fn(V(pa + 32 * e), V(pb + step * e), V(po + 32 * e))
    return out


def mul(a, b):
    return _vec("mul", a, b)


def add(a, b):
    return _vec("add", a, b)


def ones(dim):
    return np.ascontiguousarray(np.repeat(ONE[None, :], 1 << dim, axis=0))


class Inst:
    """one instance of a gate layer: the two lists, the two tables, g and -- two-point form -- g2 and coef = (alpha, beta)"""

    def __init__(self, mul_list, add_list, f2, f3, g, g2=None, coef=None):
        (self.mul_idx, self.mul_vals), (self.add_idx, self.add_vals) = mul_list, add_list
        self.f2, self.f3, self.g, self.g2 = f2, f3, g, g2
        self.coef = None if coef is None else np.ascontiguousarray(coef, dtype=np.uint64).reshape(2, 4)
        self.dim = int(f2.shape[0]).bit_length() - 1

    def points(self):
        """[(weight or None, point)]: E = sum of weight x eq(point, .)"""
        return [(None, self.g)] if self.g2 is None else [(self.coef[0], self.g), (self.coef[1], self.g2)]

    def with_second(self, g2, coef):
        return Inst((self.mul_idx, self.mul_vals), (self.add_idx, self.add_vals), self.f2, self.f3, self.g, g2, coef)

    def three(self):
        """the three multiplication-only instances whose messages add up to this one's: (MUL, f2, f3), (ADD, f2, 1), (ADD, 1, f3) -- each as
        tests/gkr_two_point_cases.py's Walk2 takes it (g2 = g, (alpha, beta) = (1, 0) in one-point form)"""
        o = ones(self.dim)
        g2, coef = (self.g, np.stack([ONE, ZERO])) if self.g2 is None else (self.g2, self.coef)
        return [(self.mul_idx, self.mul_vals, self.f2, self.f3, self.g, g2, coef), (self.add_idx, self.add_vals, self.f2, o, self.g, g2, coef),
                (self.add_idx, self.add_vals, o, self.f3, self.g, g2, coef)]


def _weighted(parts):
    """sum of weight x table over [(weight or None, table)]"""
    acc = None
    for w, t in parts:
        t = t if w is None else mul(t, w)
        acc = t if acc is None else add(acc, t)
    return acc


def phase_one_tables(inst):
    """(H1, H2, the lists bound at every point of E: [(weight, mul (idx, vals), add (idx, vals))])"""
    dim, o = inst.dim, ones(inst.dim)
    h1, h2, bound = [], [], []
    for w, pt in inst.points():
        hm, mi, mv = cref.gkr_phase_one(inst.mul_idx, inst.mul_vals, dim, inst.f3, pt)
        ha, ai, av = cref.gkr_phase_one(inst.add_idx, inst.add_vals, dim, o, pt)
        ha3, _, _ = cref.gkr_phase_one(inst.add_idx, inst.add_vals, dim, inst.f3, pt)
        h1.append((w, add(hm, ha)))
        h2.append((w, ha3))
        bound.append((w, (mi, mv), (ai, av)))
    return _weighted(h1), _weighted(h2), bound


def phase_two_tables(inst, bound, u, f2u):
    """(T1, T2) from phase_one_tables' bound lists"""
    gm = _weighted([(w, cref.gkr_phase_two(m[0], m[1], inst.dim, u)) for w, m, _ in bound])
    ga = _weighted([(w, cref.gkr_phase_two(a[0], a[1], inst.dim, u)) for w, _, a in bound])
    return add(mul(gm, f2u), ga), mul(ga, f2u)


PRODUCTS = [(ONE, [0, 1]), (ONE, [2])]


class WalkG:
    """the oracle for ONE instance under the challenges chal (2 dim, 4): msgs (2 dim, 3, 4), final = (f2(u), f3(v), f3(v) T1(v) + T2(v)),
    and the tables H1, H2, T1, T2"""

    def __init__(self, inst, chal):
        dim = inst.dim
        chal = np.ascontiguousarray(chal, dtype=np.uint64).reshape(2 * dim, 4)
        self.H1, self.H2, bound = phase_one_tables(inst)
        msgs = []
        p = cref.Prover(cref.PolyDesc(dim, PRODUCTS, [inst.f2, self.H1, self.H2]))
        for t in range(dim):
            msgs.append(p.prove_round(None if t == 0 else chal[t - 1]))
        p.close()
        u = np.ascontiguousarray(chal[:dim])
        self.f2u = cref.fix_variables(inst.f2, u)[0]
        self.T1, self.T2 = phase_two_tables(inst, bound, u, self.f2u)
        p = cref.Prover(cref.PolyDesc(dim, PRODUCTS, [inst.f3, self.T1, self.T2]))
        for r in range(dim):
            msgs.append(p.prove_round(None if r == 0 else chal[dim + r - 1]))
        p.close()
        v = np.ascontiguousarray(chal[dim:])
        f3v, t1v, t2v = (cref.fix_variables(t, v)[0] for t in (inst.f3, self.T1, self.T2))
        self.msgs = np.stack(msgs)
        self.final = np.stack([self.f2u, f3v, cref.fr_binop("add", cref.fr_binop("mul", f3v, t1v), t2v)])


def walks(insts, chal):
    """chal: (2 dim, n, 4), or (2 dim, 4) shared by all"""
    chal = np.asarray(chal, dtype=np.uint64)
    return [WalkG(inst, chal if chal.ndim == 2 else chal[:, i]) for i, inst in enumerate(insts)]


# ---- the definition over python integers -------------------------------------------------------------------------------------------------
def eq_table(point_int, dim):
    """eq(point, b) for every b in the hypercube"""
    out = []
    for b in range(1 << dim):
        e = 1
        for j in range(dim):
            e = e * (point_int[j] if (b >> j) & 1 else (1 - point_int[j])) % P
        out.append(e)
    return out


def weights_int(inst):
    """E[z] over python integers"""
    dim = inst.dim
    E = [0] * (1 << dim)
    for w, pt in inst.points():
        wi = 1 if w is None else cref.mont_to_ints(w)[0]
        E = [(a + wi * b) % P for a, b in zip(E, eq_table(cref.mont_to_ints(pt), dim))]
    return E


def _terms(idx, vals, dim):
    N = 1 << dim
    vi = cref.mont_to_ints(vals) if len(idx) else []
    for i, v in zip(idx, vi):
        i = int(i)
        yield i & (N - 1), (i >> dim) & (N - 1), (i >> (2 * dim)) & (N - 1), v


def define_tables(inst, u_int=None):
    """H1, H2 (u_int None) or T1, T2 by the sums of the module's head, over python integers"""
    dim, N = inst.dim, 1 << inst.dim
    E, f2, f3 = weights_int(inst), cref.mont_to_ints(inst.f2), cref.mont_to_ints(inst.f3)
    a, b = [0] * N, [0] * N
    if u_int is None:
        for z, x, y, v in _terms(inst.mul_idx, inst.mul_vals, dim):
            a[x] = (a[x] + E[z] * v * f3[y]) % P
        for z, x, y, v in _terms(inst.add_idx, inst.add_vals, dim):
            a[x] = (a[x] + E[z] * v) % P
            b[x] = (b[x] + E[z] * v * f3[y]) % P
        return a, b
    equ = eq_table(u_int, dim)
    f2u = sum(e * t for e, t in zip(equ, f2)) % P
    for z, x, y, v in _terms(inst.mul_idx, inst.mul_vals, dim):
        a[y] = (a[y] + f2u * E[z] * equ[x] * v) % P
    for z, x, y, v in _terms(inst.add_idx, inst.add_vals, dim):
        a[y] = (a[y] + E[z] * equ[x] * v) % P
        b[y] = (b[y] + f2u * E[z] * equ[x] * v) % P
    return a, b


def define_layer(inst):
    """W_out over python integers"""
    dim = inst.dim
    f2, f3 = cref.mont_to_ints(inst.f2), cref.mont_to_ints(inst.f3)
    out = [0] * (1 << dim)
    for z, x, y, v in _terms(inst.mul_idx, inst.mul_vals, dim):
        out[z] = (out[z] + v * f2[x] * f3[y]) % P
    for z, x, y, v in _terms(inst.add_idx, inst.add_vals, dim):
        out[z] = (out[z] + v * (f2[x] + f3[y])) % P
    return out


def extension(table_int, point_int, dim):
    return sum(e * t for e, t in zip(eq_table(point_int, dim), table_int)) % P


def list_extension(idx, vals, dim, E, equ, eqv):
    """sum over the list of E[z] eq(u,x) eq(v,y) v"""
    return sum(E[z] * equ[x] * eqv[y] * v for z, x, y, v in _terms(idx, vals, dim)) % P


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def wiring(dim, seed, nnz, variant="repeated"):
    """(indices, values): repeated (every index about three times), random, edge (values from {0, 1, p - 1}).  nnz 0: empty arrays"""
    rng = np.random.default_rng(seed)
    if variant == "repeated" and nnz:
        pool = rng.integers(0, 1 << (3 * dim), size=max(nnz // 3, 1), dtype=np.uint64)
        idx = pool[rng.integers(0, pool.shape[0], size=nnz)]
    else:
        idx = rng.integers(0, 1 << (3 * dim), size=nnz, dtype=np.uint64)
    vals = cref.synth_table(seed, 1, nnz).copy() if nnz else np.zeros((0, 4), np.uint64)
    if variant == "edge" and nnz:
        vals[:] = EDGE[rng.integers(0, 3, size=nnz)]
    return np.ascontiguousarray(idx), np.ascontiguousarray(vals)


def instance(dim, seed, mul_nnz, add_nnz, two_point=False, variant="repeated"):
    N = 1 << dim
    inst = Inst(wiring(dim, seed, mul_nnz, variant), wiring(dim, seed + 1, add_nnz, variant), cref.synth_table(seed, 2, N), cref.synth_table(seed, 3, N),
                cref.synth_table(seed, 4, dim))
    return inst.with_second(cref.synth_table(seed, 5, dim), cref.synth_table(seed, 6, 2)) if two_point else inst


def instances(n, dim, seed, mul_nnz, add_nnz, two_point=False, variant="repeated"):
    return [instance(dim, seed + 7919 * i, mul_nnz, add_nnz, two_point, variant) for i in range(n)]


def challenges(n, dim, seed, shared=False):
    """(2 dim, n, 4), or (2 dim, 4) for a challenge all instances share"""
    c = cref.synth_table(seed, 9, 2 * dim * (1 if shared else n))
    return c.reshape(2 * dim, 4) if shared else c.reshape(2 * dim, n, 4)


def edge_instance(dim, seed, nnz, two_point):
    """every value, table entry, point and coefficient from {0, 1, p - 1}"""
    rng = np.random.default_rng(seed)
    N = 1 << dim
    pick = lambda k: np.ascontiguousarray(EDGE[rng.integers(0, 3, size=k)])
    inst = Inst(wiring(dim, seed, nnz, "edge"), wiring(dim, seed + 1, nnz, "edge"), pick(N), pick(N), pick(dim))
    return inst.with_second(pick(dim), pick(2)) if two_point else inst


def one_cell_instance(dim, nnz, seed):
    """both lists full of ONE index (z = x = y = cell) with values p - 1, tables of p - 1: every term of both phases lands in one cell of
    the kernel's accumulator -- 2 nnz terms in the pass that takes both lists.  With nnz = 64 x 2^dim at dim 9 that is 2^16 terms of
    32-bit limbs: a lane stays below 2^16 x 2^32 = 2^48 < 2^63, the bound wide_fold_cell states"""
    N = 1 << dim
    cell = np.uint64((seed * 2654435761) % N)
    idx = np.full(nnz, cell | (cell << np.uint64(dim)) | (cell << np.uint64(2 * dim)), dtype=np.uint64)
    vals = np.ascontiguousarray(np.repeat(MINUS_ONE[None, :], nnz, axis=0))
    table = np.ascontiguousarray(np.repeat(MINUS_ONE[None, :], N, axis=0))
    return Inst((idx, vals), (idx.copy(), vals.copy()), table, table.copy(), cref.synth_table(seed, 4, dim))


def define_layers(layers, f2, f3):
    """layers: per layer ((mul_idx, mul_vals), (add_idx, add_vals)); f2, f3: (2^dim, 4) Montgomery limbs -> per layer the (2^dim, 4) table,
    layer 0 over (f2, f3), every later layer over the layer before on both sides"""
    a, b, out = f2, f3, []
    for mul_list, add_list in layers:
        w = cref.ints_to_mont(define_layer(Inst(mul_list, add_list, a, b, None)))
        out.append(w)
        a = b = w
    return out


def one_cell_terms(dim, nnz, z, seed):
    """nnz terms that all land in cell z with value p - 1, and a table of p - 1: (indices, values, table)"""
    rng = np.random.default_rng(seed)
    N = 1 << dim
    x, y = rng.integers(0, N, size=nnz, dtype=np.uint64), rng.integers(0, N, size=nnz, dtype=np.uint64)
    idx = np.ascontiguousarray(np.uint64(z) | (x << np.uint64(dim)) | (y << np.uint64(2 * dim)))
    return idx, np.ascontiguousarray(np.repeat(MINUS_ONE[None, :], nnz, axis=0)), np.ascontiguousarray(np.repeat(MINUS_ONE[None, :], N, axis=0))
