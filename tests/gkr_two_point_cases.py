"""The oracle of the GKR batch handle's two-point form (sc_gkr_two_point_init_batch / _next_batch), composed from oracle/cref.py as the Walk of
tests/test_gpu_gkr_batch_rounds.py is, and the inputs the CPU and the GPU tests share.  Where the one-point handle uses eq(g, z) the
two-point form uses E(z) = alpha eq(g, z) + beta eq(g2, z); both initialisations are linear in that factor, so
  phase one's table  h = alpha h_g(g) + beta h_g(g2)               two cref.gkr_phase_one calls, combined with cref.fr_binop;
  phase two's table  f1_gu = alpha f1(g, u, .) + beta f1(g2, u, .)  likewise from the two lists through cref.gkr_phase_two;
everything else -- the provers, f2(u), f2(u) f3, the final triple -- is the Walk's."""
import ctypes as C

import numpy as np

from oracle import cref

P = cref.P
ONE = cref.ints_to_mont([1])[0]
ZERO = cref.ints_to_mont([0])[0]
MINUS_ONE = cref.ints_to_mont([P - 1])[0]
EDGE = {0: ZERO, 1: ONE, -1: MINUS_ONE}


def combine(alpha, a, beta, b):
    """alpha a + beta b, element by element over (k, 4) arrays of Montgomery limbs: cref.fr_binop's "mul" and "add" (the oracle's
    orc_fr_mul and orc_fr_add), called on the rows in place -- a table of 2^16 entries is 200 000 calls"""
    a, b = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4), np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 4)
    alpha, beta = np.ascontiguousarray(alpha, dtype=np.uint64), np.ascontiguousarray(beta, dtype=np.uint64)
    out, t = np.empty_like(a), np.empty((2, 4), dtype=np.uint64)
    mul, add = cref.lib().orc_fr_mul, cref.lib().orc_fr_add
    V = C.c_void_p
    pal, pbe, t0, t1 = V(alpha.ctypes.data), V(beta.ctypes.data), V(t.ctypes.data), V(t.ctypes.data + 32)
    pa, pb, po = a.ctypes.data, b.ctypes.data, out.ctypes.data
    for e in range(a.shape[0]):
        mul(pal, V(pa + 32 * e), t0)
        mul(pbe, V(pb + 32 * e), t1)
        add(t0, t1, V(po + 32 * e))
    return out


class Walk2:
    """the two-point oracle for ONE instance, with Walk's attributes: msgs (2 dim, 3, 4), the provers' tables after the round calls in
    `states`, final = (alpha f1(g,u,v) + beta f1(g2,u,v), f2(u), f2(u) f3(v)).  inst: (idx, vals, f2, f3, g, g2, (alpha, beta))"""

    def __init__(self, inst, dim, chal, states=()):
        idx, vals, f2, f3, g, g2, coef = inst
        alpha, beta = np.asarray(coef, dtype=np.uint64).reshape(2, 4)
        N = 1 << dim
        desc = lambda a, b: cref.PolyDesc(dim, [(ONE, [0, 1])], [a, b])
        h1, gi1, gv1 = cref.gkr_phase_one(idx, vals, dim, f3, g)
        h2, gi2, gv2 = cref.gkr_phase_one(idx, vals, dim, f3, g2)
        self.h = combine(alpha, h1, beta, h2)
        self.msgs, self.states = [], {}
        p = cref.Prover(desc(self.h, f2))
        for t in range(dim):
            self.msgs.append(p.prove_round(None if t == 0 else chal[t - 1]))
            if t + 1 in states:
                self.states[t + 1] = p.state()[1]
        p.close()
        u = np.ascontiguousarray(chal[:dim])
        f2u = cref.fix_variables(f2, u)[0]
        self.f1gu = combine(alpha, cref.gkr_phase_two(gi1, gv1, dim, u), beta, cref.gkr_phase_two(gi2, gv2, dim, u))
        t1 = np.stack([cref.fr_binop("mul", f3[e], f2u) for e in range(N)])  # mod.rs:71-75
        p = cref.Prover(desc(self.f1gu, t1))
        for r in range(dim):
            self.msgs.append(p.prove_round(None if r == 0 else chal[dim + r - 1]))
            if dim + r + 1 in states:
                self.states[dim + r + 1] = p.state()[1]
        p.close()
        v = np.ascontiguousarray(chal[dim:2 * dim])
        self.msgs = np.stack(self.msgs)
        self.final = np.stack([cref.fix_variables(self.f1gu, v)[0], f2u, cref.fix_variables(t1, v)[0]])


def walks2(insts, dim, chal, states=()):
    return [Walk2(inst, dim, np.ascontiguousarray(chal[:, i]), states) for i, inst in enumerate(insts)]


def second_points(n, dim, seed):
    """per instance a g2 and (alpha, beta), all distinct"""
    return [(cref.synth_table(seed + 7919 * i, 5, dim), cref.synth_table(seed + 7919 * i, 6, 2)) for i in range(n)]


def with_second(insts, seconds):
    """one-point instances (idx, vals, f2, f3, g) + second_points' pairs -> Walk2's instances"""
    return [tuple(a[:5]) + (s[0], s[1]) for a, s in zip(insts, seconds)]
