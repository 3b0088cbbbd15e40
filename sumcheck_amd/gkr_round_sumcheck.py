"""Host-side mirror of the reference's GKR round sumcheck API over the C ABI.

  initialize_phase_one / start_phase1_sumcheck / initialize_phase_two / start_phase2_sumcheck
                                   reference src/gkr_round_sumcheck/mod.rs:22-82
  GKRRoundSumcheck::{prove, verify} reference src/gkr_round_sumcheck/mod.rs:84-193
  GKRProof / GKRRoundSumcheckSubClaim reference src/gkr_round_sumcheck/data_structures.rs:9-57

The prover side (sparse fold, scatter, both sumcheck phases) runs on the GPU inside libsumcheck_hip.so.
The verifier side is O(dim) scalar work and stays on the host, like the reference's.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Sequence

import numpy as np

from . import field
from ._lib import SC_TABLES_ON_DEVICE, check, lib
from .ml_sumcheck import (Blake2b512Rng, DenseMultilinearExtension, IPForMLSumcheck, ListOfProductsOfPolynomials, ProverMsg,
                          ProverState, SumcheckError, _np64, _ptr, interpolate_uni_poly)


def _is_cuda(x) -> bool:
    return type(x).__module__.startswith("torch") and x.is_cuda


class SparseMultilinearExtension:
    """ark_poly::SparseMultilinearExtension: `indices` (nnz,) uint64 distinct, `values` (nnz, 4) Montgomery limbs -- numpy arrays
    (host) or torch int64 tensors on the GPU (HBM-resident; the library then reads them in place)."""

    def __init__(self, num_vars: int, indices, values):
        self.num_vars = num_vars
        self.on_device = _is_cuda(indices) and _is_cuda(values)
        if self.on_device:
            assert indices.is_contiguous() and values.is_contiguous() and values.numel() == 4 * indices.numel()
            self.indices, self.values = indices, values
        else:
            self.indices = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
            self.values = _np64(values).reshape(-1, 4)
            assert self.indices.shape[0] == self.values.shape[0]

    @property
    def nnz(self) -> int:
        return int(self.indices.shape[0])

    def _ptrs(self):
        if self.on_device:
            return C.c_void_p(self.indices.data_ptr()), C.c_void_p(self.values.data_ptr())
        return _ptr(self.indices), _ptr(self.values)

    def to_host(self) -> "SparseMultilinearExtension":
        if not self.on_device:
            return self
        return SparseMultilinearExtension(self.num_vars, self.indices.cpu().numpy().view(np.uint64), self.values.cpu().numpy().view(np.uint64))

    @classmethod
    def from_evaluations(cls, num_vars: int, evaluations):
        idx = [i for i, _ in evaluations]
        vals = [v for _, v in evaluations]
        return cls(num_vars, np.asarray(idx, dtype=np.uint64), np.stack(vals) if vals else np.zeros((0, 4), np.uint64))

    def evaluate(self, point) -> np.ndarray:
        """ark-poly SparseMultilinearExtension::evaluate on the GPU (sc_sparse_evaluate): the verifier's oracle query
        f1(g, u, v) of verify_subclaim (data_structures.rs:53)"""
        h = self.to_host()
        pt = np.ascontiguousarray(np.asarray(point, dtype=np.uint64).reshape(-1, 4))
        assert pt.shape[0] == self.num_vars
        out = np.zeros(4, dtype=np.uint64)
        check(lib().sc_sparse_evaluate(_ptr(h.indices), _ptr(h.values), h.indices.shape[0], self.num_vars,
                                       _ptr(pt) if pt.size else None, _ptr(out)))
        return out


def _dense_ptr(m: DenseMultilinearExtension):
    return C.c_void_p(m.data_ptr()) if m.on_device else _ptr(m.evaluations)


def initialize_phase_one(f1: SparseMultilinearExtension, f3: DenseMultilinearExtension, g):
    """mod.rs:22-42 -> (h_g dense, f1_at_g sparse).  Device-resident inputs (f1 and f3 both on the GPU) give device-resident
    outputs, produced in place by the library."""
    dim = f3.num_vars
    assert f1.num_vars == dim * 3
    g = _np64(g).reshape(-1, 4)
    assert g.shape[0] == dim
    nnz = f1.nnz
    dev = f1.on_device and f3.on_device
    assert dev or not (f1.on_device or f3.on_device), "mixing host and device inputs is not supported"
    n1 = C.c_uint64()
    i_ptr, v_ptr = f1._ptrs()
    if dev:
        import torch
        h_g = torch.empty((1 << dim, 4), dtype=torch.int64, device=f3.evaluations.device)
        oi = torch.empty(max(nnz, 1), dtype=torch.int64, device=h_g.device)
        ov = torch.empty((max(nnz, 1), 4), dtype=torch.int64, device=h_g.device)
        torch.cuda.current_stream(h_g.device).synchronize()  # the library works on its own stream
        check(lib().sc_gkr_phase_one(i_ptr, v_ptr, nnz, dim, _dense_ptr(f3), _ptr(g), SC_TABLES_ON_DEVICE, C.c_void_p(h_g.data_ptr()),
                                     C.c_void_p(oi.data_ptr()), C.c_void_p(ov.data_ptr()), C.byref(n1)))
        return DenseMultilinearExtension(dim, h_g), SparseMultilinearExtension(2 * dim, oi[: n1.value].contiguous(), ov[: n1.value].contiguous())
    h_g = np.empty((1 << dim, 4), dtype=np.uint64)
    oi = np.empty(max(nnz, 1), dtype=np.uint64)
    ov = np.empty((max(nnz, 1), 4), dtype=np.uint64)
    check(lib().sc_gkr_phase_one(i_ptr, v_ptr, nnz, dim, _dense_ptr(f3), _ptr(g), 0, _ptr(h_g), _ptr(oi), _ptr(ov), C.byref(n1)))
    return DenseMultilinearExtension(dim, h_g), SparseMultilinearExtension(2 * dim, oi[: n1.value].copy(), ov[: n1.value].copy())


def start_phase1_sumcheck(h_g: DenseMultilinearExtension, f2: DenseMultilinearExtension) -> ProverState:
    """mod.rs:45-54"""
    dim = h_g.num_vars
    assert f2.num_vars == dim
    poly = ListOfProductsOfPolynomials.new(dim)
    poly.add_product([h_g, f2], field.ONE)
    return IPForMLSumcheck.prover_init(poly)


def initialize_phase_two(f1_g: SparseMultilinearExtension, u) -> DenseMultilinearExtension:
    """mod.rs:57-63"""
    u = _np64(u).reshape(-1, 4)
    assert u.shape[0] * 2 == f1_g.num_vars
    dim = u.shape[0]
    i_ptr, v_ptr = f1_g._ptrs()
    if f1_g.on_device:
        import torch
        out = torch.empty((1 << dim, 4), dtype=torch.int64, device=f1_g.values.device)
        torch.cuda.current_stream(out.device).synchronize()
        check(lib().sc_gkr_phase_two(i_ptr, v_ptr, f1_g.nnz, dim, _ptr(u), SC_TABLES_ON_DEVICE, C.c_void_p(out.data_ptr())))
        return DenseMultilinearExtension(dim, out)
    out = np.empty((1 << dim, 4), dtype=np.uint64)
    check(lib().sc_gkr_phase_two(i_ptr, v_ptr, f1_g.nnz, dim, _ptr(u), 0, _ptr(out)))
    return DenseMultilinearExtension(dim, out)


def scale(m: DenseMultilinearExtension, scalar) -> DenseMultilinearExtension:
    """`DenseMultilinearExtension::zero() += (scalar, &m)` (mod.rs:71-75) on the GPU: every evaluation times one field element"""
    sv = _np64(scalar).reshape(4)
    n = 1 << m.num_vars
    if m.on_device:
        import torch
        out = torch.empty_like(m.evaluations)
        torch.cuda.current_stream(out.device).synchronize()
        check(lib().sc_dense_scale(_dense_ptr(m), n, _ptr(sv), C.c_void_p(out.data_ptr()), SC_TABLES_ON_DEVICE))
    else:
        out = np.empty((n, 4), dtype=np.uint64)
        check(lib().sc_dense_scale(_dense_ptr(m), n, _ptr(sv), _ptr(out), 0))
    return DenseMultilinearExtension(m.num_vars, out)


def start_phase2_sumcheck(f1_gu: DenseMultilinearExtension, f3: DenseMultilinearExtension, f2_u) -> ProverState:
    """mod.rs:66-82: f3 scaled by the scalar f2(u) (on the GPU), then one product of two tables"""
    dim = f1_gu.num_vars
    assert f3.num_vars == dim
    f3_f2u = scale(f3, f2_u)
    poly = ListOfProductsOfPolynomials.new(dim)
    poly.add_product([f1_gu, f3_f2u], field.ONE)
    return IPForMLSumcheck.prover_init(poly)


@dataclass
class GKRProof:  # data_structures.rs:9-19
    phase1_sumcheck_msgs: List[ProverMsg]
    phase2_sumcheck_msgs: List[ProverMsg]

    def extract_sum(self) -> np.ndarray:
        ev = self.phase1_sumcheck_msgs[0].evaluations
        return field.add(ev[0], ev[1])


@dataclass
class GKRRoundSumcheckSubClaim:  # data_structures.rs:22-31
    u: np.ndarray
    v: np.ndarray
    expected_evaluation: np.ndarray

    def verify_subclaim(self, f1: SparseMultilinearExtension, f2: DenseMultilinearExtension, f3: DenseMultilinearExtension, g) -> bool:
        """data_structures.rs:33-56"""
        dim = self.u.shape[0]
        assert self.v.shape[0] == dim and f1.num_vars == 3 * dim and f2.num_vars == dim and f3.num_vars == dim
        g = _np64(g).reshape(-1, 4)
        assert g.shape[0] == dim
        guv = np.concatenate([g, self.u, self.v])
        actual = field.to_int(f1.evaluate(guv)) * field.to_int(f2.evaluate(self.u)) % field.P * field.to_int(f3.evaluate(self.v)) % field.P
        return actual == field.to_int(self.expected_evaluation)

    @staticmethod
    def verify_subclaim_batch(subclaims: Sequence["GKRRoundSumcheckSubClaim"], f1s, f2s, f3s, gs) -> List[bool]:
        """verify_subclaim of n subclaims of one dim in one library call (GKRRoundSumcheck.evaluate_subclaims_batch): element i is
        subclaims[i].verify_subclaim(f1s[i], f2s[i], f3s[i], gs[i])"""
        n = len(subclaims)
        assert len(f1s) == n and len(f2s) == n and len(f3s) == n and len(gs) == n, "one f1, f2, f3 and g per subclaim"
        if n == 0:
            return []
        uv = np.stack([np.concatenate([_np64(c.u).reshape(-1, 4), _np64(c.v).reshape(-1, 4)]) for c in subclaims])
        ev = GKRRoundSumcheck.evaluate_subclaims_batch(f1s, f2s, f3s, gs, uv)
        return [bool(np.array_equal(ev[i, 3], _np64(c.expected_evaluation).reshape(4))) for i, c in enumerate(subclaims)]

    def verify_subclaim_two_point(self, f1: SparseMultilinearExtension, f2: DenseMultilinearExtension, f3: DenseMultilinearExtension, g, g2, alpha, beta) -> bool:
        """verify_subclaim for a round proved in two-point form: (alpha f1(g,u,v) + beta f1(g2,u,v)) f2(u) f3(v) against expected_evaluation"""
        return GKRRoundSumcheckSubClaim.verify_subclaim_two_point_batch([self], [f1], [f2], [f3], [g], [g2], [np.stack([_np64(alpha).reshape(4), _np64(beta).reshape(4)])])[0]

    @staticmethod
    def verify_subclaim_two_point_batch(subclaims: Sequence["GKRRoundSumcheckSubClaim"], f1s, f2s, f3s, gs, g2s, coeffs) -> List[bool]:
        """n subclaims of rounds proved in two-point form, from existing calls only: GKRRoundSumcheck.evaluate_subclaims_batch once over the
        gs and once over the g2s, then (alpha f1(g,u,v) + beta f1(g2,u,v)) f2(u) f3(v) in host field arithmetic.  coeffs: per instance
        (alpha, beta), (2, 4) limbs"""
        n = len(subclaims)
        assert len(f1s) == n and len(f2s) == n and len(f3s) == n and len(gs) == n and len(g2s) == n and len(coeffs) == n, "one f1, f2, f3, g, g2 and (alpha, beta) per subclaim"
        if n == 0:
            return []
        uv = np.stack([np.concatenate([_np64(c.u).reshape(-1, 4), _np64(c.v).reshape(-1, 4)]) for c in subclaims])
        e1 = GKRRoundSumcheck.evaluate_subclaims_batch(f1s, f2s, f3s, gs, uv)
        e2 = GKRRoundSumcheck.evaluate_subclaims_batch(f1s, f2s, f3s, g2s, uv)
        out = []
        for i, c in enumerate(subclaims):
            ab = _np64(coeffs[i]).reshape(2, 4)
            f1v = (field.to_int(ab[0]) * field.to_int(e1[i, 0]) + field.to_int(ab[1]) * field.to_int(e2[i, 0])) % field.P
            out.append(f1v * field.to_int(e1[i, 1]) % field.P * field.to_int(e1[i, 2]) % field.P == field.to_int(c.expected_evaluation))
        return out


    def verify_subclaim_gates(self, mul_f1: SparseMultilinearExtension, add_f1: SparseMultilinearExtension, f2: DenseMultilinearExtension, f3: DenseMultilinearExtension,
                              g, g2=None, alpha=None, beta=None) -> bool:
        """verify_subclaim for a round proved in gate form: M f2(u) f3(v) + A (f2(u) + f3(v)) against expected_evaluation, M and A the
        E-weighted extensions of the two lists at (u, v)"""
        coeffs = None if g2 is None else [np.stack([_np64(alpha).reshape(4), _np64(beta).reshape(4)])]
        return GKRRoundSumcheckSubClaim.verify_subclaim_gates_batch([self], [mul_f1], [add_f1], [f2], [f3], [g], None if g2 is None else [g2], coeffs)[0]

    @staticmethod
    def verify_subclaim_gates_batch(subclaims: Sequence["GKRRoundSumcheckSubClaim"], mul_f1s, add_f1s, f2s, f3s, gs, g2s=None, coeffs=None) -> List[bool]:
        """n subclaims of rounds proved in gate form (GKRRoundSumcheck.prover_init_batch_gates), from existing calls only:
        GKRRoundSumcheck.evaluate_subclaims_batch per list and per point, then M f2(u) f3(v) + A (f2(u) + f3(v)) in host field arithmetic,
        with M = alpha mul(g,u,v) + beta mul(g2,u,v) and A likewise (one point: M = mul(g,u,v))."""
        n = len(subclaims)
        assert len(mul_f1s) == n and len(add_f1s) == n and len(f2s) == n and len(f3s) == n and len(gs) == n, "one mul, add, f2, f3 and g per subclaim"
        assert (g2s is None) == (coeffs is None) and (g2s is None or (len(g2s) == n and len(coeffs) == n)), "g2s and coeffs come together, one per subclaim"
        if n == 0:
            return []
        uv = np.stack([np.concatenate([_np64(c.u).reshape(-1, 4), _np64(c.v).reshape(-1, 4)]) for c in subclaims])
        ev = {(k, pt): GKRRoundSumcheck.evaluate_subclaims_batch(f1s, f2s, f3s, pts, uv)
              for k, f1s in (("mul", mul_f1s), ("add", add_f1s)) for pt, pts in ((0, gs), (1, g2s)) if pts is not None}
        out = []
        for i, c in enumerate(subclaims):
            w = {}
            for k in ("mul", "add"):
                w[k] = field.to_int(ev[k, 0][i, 0])
                if g2s is not None:
                    ab = _np64(coeffs[i]).reshape(2, 4)
                    w[k] = (field.to_int(ab[0]) * w[k] + field.to_int(ab[1]) * field.to_int(ev[k, 1][i, 0])) % field.P
            f2u, f3v = field.to_int(ev["mul", 0][i, 1]), field.to_int(ev["mul", 0][i, 2])
            out.append((w["mul"] * f2u % field.P * f3v + w["add"] * (f2u + f3v)) % field.P == field.to_int(c.expected_evaluation))
        return out


def _second_point(g2s, coeffs, n: int, dim: int):
    """the two-point form's extra arguments -> None (one-point form), or (n arrays (dim, 4), one array (n, 2, 4))"""
    if (g2s is None) != (coeffs is None):
        raise ValueError("g2s and coeffs come together (the two-point form) or not at all")
    if g2s is None:
        return None
    if len(g2s) != n or len(coeffs) != n:
        raise ValueError("one g2 and one (alpha, beta) per instance")
    g2_arr = [np.ascontiguousarray(_np64(a).reshape(-1, 4)) for a in g2s]
    if any(a.shape[0] != dim for a in g2_arr):
        raise ValueError(f"a g2 has dim elements ({dim})")
    coef = np.ascontiguousarray(np.stack([_np64(c).reshape(2, 4) for c in coeffs])) if n else np.zeros((0, 2, 4), np.uint64)
    return g2_arr, coef


def _verify_phase(rng: Blake2b512Rng, msgs: Sequence[ProverMsg], dim: int, asserted_sum):
    """verifier_init{max_multiplicands: 2} + verify_round x dim + check_and_generate_subclaim (mod.rs:157-166)"""
    rs = []
    for i in range(dim):
        rng.feed(msgs[i])
        rs.append(rng.sample_fr())
    expected = field.to_int(asserted_sum)
    for i in range(dim):
        ev = msgs[i].evaluations
        if ev.shape[0] != 3:
            raise SumcheckError(5, "incorrect number of evaluations")
        try:  # field.to_int refuses limbs >= p: a proof element must be a canonical field element
            s01 = (field.to_int(ev[0]) + field.to_int(ev[1])) % field.P
        except ValueError:
            raise SumcheckError(5, "proof element is not a canonical field element")
        if s01 != expected:
            raise SumcheckError(8, "Prover message is not consistent with the claim.")
        expected = field.to_int(interpolate_uni_poly(ev, rs[i]))
    return np.stack(rs) if rs else np.zeros((0, 4), np.uint64), field.from_int(expected)


def _gates_args(n: int, dim: int, mul_f1s, add_f1s, f2s, f3s, gs, second):
    """the argument arrays sc_gkr_gates_init_batch and sc_gkr_gates_next_batch share, from mul_idx to coef (lists None: six NULLs) -> (args, on_device)"""
    lists = [] if mul_f1s is None else list(mul_f1s) + list(add_f1s)
    assert mul_f1s is None or (len(mul_f1s) == n and len(add_f1s) == n), "one mul and one add list per instance"
    ons = [m.on_device for m in lists + list(f2s) + list(f3s)]
    dev = bool(ons) and all(ons)
    assert dev or not any(ons), "mixing host and device inputs is not supported"
    g_arr = []
    for i in range(n):
        assert f2s[i].num_vars == dim and f3s[i].num_vars == dim and all(f.num_vars == 3 * dim for f in lists), f"instance {i}: a batch has one dim"
        g_arr.append(np.ascontiguousarray(_np64(gs[i]).reshape(-1, 4)))
        assert g_arr[i].shape[0] == dim
    if dev:
        import torch
        torch.cuda.current_stream(f2s[0].evaluations.device).synchronize()  # the library works on its own stream

    def ptrs(vals):
        return (C.c_void_p * max(n, 1))(*[C.cast(v, C.c_void_p) for v in vals])

    wiring = []
    for f1s in ((mul_f1s, add_f1s) if mul_f1s is not None else ()):
        p = [f._ptrs() for f in f1s]
        wiring += [ptrs([q[0] for q in p]), ptrs([q[1] for q in p]), (C.c_uint64 * max(n, 1))(*[f.nnz for f in f1s])]
    if mul_f1s is None:
        wiring = [None] * 6
    g2_arr, coef = second if second is not None else (None, None)
    args = (*wiring, ptrs([_dense_ptr(m) for m in f2s]), ptrs([_dense_ptr(m) for m in f3s]), ptrs([_ptr(a) for a in g_arr]),
            None if g2_arr is None else ptrs([_ptr(a) for a in g2_arr]), None if coef is None else _ptr(coef))
    return _Kept(args, (g_arr, g2_arr, coef, lists)), dev


class _Kept(tuple):
    """a tuple of ctypes arguments that also holds the numpy arrays their pointers were taken from"""

    def __new__(cls, args, keep):
        t = super().__new__(cls, args)
        t.keep = keep
        return t


class GKRRoundSumcheck:
    @staticmethod
    def prove(rng: Blake2b512Rng, f1: SparseMultilinearExtension, f2: DenseMultilinearExtension, f3: DenseMultilinearExtension,
              g) -> GKRProof:
        """mod.rs:93-139: everything from the sparse fold to the last round polynomial runs inside sc_gkr_prove"""
        assert f1.num_vars == 3 * f2.num_vars and f1.num_vars == 3 * f3.num_vars
        dim = f2.num_vars
        g = _np64(g).reshape(-1, 4)
        assert g.shape[0] == dim
        proof = np.empty((2, max(dim, 1), 3, 4), dtype=np.uint64)
        dev = f1.on_device and f2.on_device and f3.on_device
        assert dev or not (f1.on_device or f2.on_device or f3.on_device), "mixing host and device inputs is not supported"
        if dev:
            import torch
            torch.cuda.current_stream(f2.evaluations.device).synchronize()  # the library works on its own stream
        i_ptr, v_ptr = f1._ptrs()
        check(lib().sc_gkr_prove(rng._h, i_ptr, v_ptr, f1.nnz, dim, _dense_ptr(f2), _dense_ptr(f3), _ptr(g),
                                 SC_TABLES_ON_DEVICE if dev else 0, _ptr(proof), None))
        return GKRProof([ProverMsg(proof[0, i].copy()) for i in range(dim)], [ProverMsg(proof[1, i].copy()) for i in range(dim)])

    @staticmethod
    def prove_batch(rngs: Sequence[Blake2b512Rng], f1s: Sequence[SparseMultilinearExtension], f2s: Sequence[DenseMultilinearExtension],
                    f3s: Sequence[DenseMultilinearExtension], gs, return_uv: bool = False):
        """n independent GKRRoundSumcheck.prove of one dim in one library call (sc_gkr_prove_batch) -> a list of GKRProof, proof i bit for
        bit prove(rngs[i], f1s[i], f2s[i], f3s[i], gs[i]) with rngs[i] continued accordingly -- with return_uv also the (n, 2, dim, 4)
        array of the sampled (u, v).  The same object may stand for several instances (one wiring predicate f1 for many data instances).
        Small instances (dim <= 9) are proved concurrently, a workgroup each, inside one kernel."""
        n = len(rngs)
        assert len(f1s) == n and len(f2s) == n and len(f3s) == n and len(gs) == n, "one f1, f2, f3 and g per rng"
        if n == 0:
            check(lib().sc_gkr_prove_batch(0, 0, None, None, None, None, None, None, None, 0, None, None))
            return ([], np.zeros((0, 2, 0, 4), np.uint64)) if return_uv else []
        dim = f2s[0].num_vars
        ons = [m.on_device for m in list(f1s) + list(f2s) + list(f3s)]
        dev = all(ons)
        assert dev or not any(ons), "mixing host and device inputs is not supported"
        g_arr = []
        for i in range(n):
            assert f2s[i].num_vars == dim and f3s[i].num_vars == dim and f1s[i].num_vars == 3 * dim, f"instance {i}: a batch has one dim"
            g_arr.append(_np64(gs[i]).reshape(-1, 4))
            assert g_arr[i].shape[0] == dim
        if dev:
            import torch
            torch.cuda.current_stream(f2s[0].evaluations.device).synchronize()  # the library works on its own stream

        def ptrs(vals):
            return (C.c_void_p * n)(*[C.cast(v, C.c_void_p) for v in vals])

        f1p = [f._ptrs() for f in f1s]
        nnz = (C.c_uint64 * n)(*[f.nnz for f in f1s])
        rows = max(dim, 1)
        proofs = np.empty((n, 2, rows, 3, 4), dtype=np.uint64)
        uv = np.empty((n, 2, rows, 4), dtype=np.uint64)
        check(lib().sc_gkr_prove_batch(n, dim, ptrs([r._h for r in rngs]), ptrs([p[0] for p in f1p]), ptrs([p[1] for p in f1p]), nnz,
                                       ptrs([_dense_ptr(m) for m in f2s]), ptrs([_dense_ptr(m) for m in f3s]), ptrs([_ptr(a) for a in g_arr]),
                                       SC_TABLES_ON_DEVICE if dev else 0, _ptr(proofs), _ptr(uv)))
        out = [GKRProof([ProverMsg(proofs[i, 0, j].copy()) for j in range(dim)], [ProverMsg(proofs[i, 1, j].copy()) for j in range(dim)]) for i in range(n)]
        return (out, uv[:, :, :dim].copy()) if return_uv else out

    @staticmethod
    def evaluate_subclaims_batch(f1s: Sequence[SparseMultilinearExtension], f2s: Sequence[DenseMultilinearExtension],
                                 f3s: Sequence[DenseMultilinearExtension], gs, uv) -> np.ndarray:
        """The three oracle queries of verify_subclaim (data_structures.rs:33-56) for n instances of one dim in one library call
        (sc_gkr_subclaim_batch) -> (n, 4, 4): f1(g,u,v), f2(u), f3(v) and their product, the value a caller compares with
        expected_evaluation.  uv: (n, 2, dim, 4), what prove_batch(..., return_uv=True) returns.  Inputs all on the host or all on the GPU,
        as for prove_batch; the same object may stand for several instances.  After prove_batch a caller finishes with this one call,
        not 3 n."""
        n = len(f1s)
        assert len(f2s) == n and len(f3s) == n and len(gs) == n, "one f1, f2, f3 and g per instance"
        if n == 0:
            check(lib().sc_gkr_subclaim_batch(0, 0, None, None, None, None, None, None, None, 0, None))
            return np.zeros((0, 4, 4), np.uint64)
        dim = f2s[0].num_vars
        ons = [m.on_device for m in list(f1s) + list(f2s) + list(f3s)]
        dev = all(ons)
        assert dev or not any(ons), "mixing host and device inputs is not supported"
        g_arr = []
        for i in range(n):
            assert f2s[i].num_vars == dim and f3s[i].num_vars == dim and f1s[i].num_vars == 3 * dim, f"instance {i}: a batch has one dim"
            g_arr.append(_np64(gs[i]).reshape(-1, 4))
            assert g_arr[i].shape[0] == dim
        uv_arr = np.ascontiguousarray(_np64(uv).reshape(n, 2, dim, 4))
        if dev:
            import torch
            torch.cuda.current_stream(f2s[0].evaluations.device).synchronize()  # the library works on its own stream

        def ptrs(vals):
            return (C.c_void_p * n)(*[C.cast(v, C.c_void_p) for v in vals])

        f1p = [f._ptrs() for f in f1s]
        nnz = (C.c_uint64 * n)(*[f.nnz for f in f1s])
        out = np.zeros((n, 4, 4), dtype=np.uint64)
        check(lib().sc_gkr_subclaim_batch(n, dim, ptrs([p[0] for p in f1p]), ptrs([p[1] for p in f1p]), nnz, ptrs([_dense_ptr(m) for m in f2s]),
                                          ptrs([_dense_ptr(m) for m in f3s]), ptrs([_ptr(a) for a in g_arr]), _ptr(uv_arr) if uv_arr.size else None,
                                          SC_TABLES_ON_DEVICE if dev else 0, _ptr(out)))
        return out

    @staticmethod
    def prover_init_batch(f1s: Sequence[SparseMultilinearExtension], f2s: Sequence[DenseMultilinearExtension],
                          f3s: Sequence[DenseMultilinearExtension], gs, g2s=None, coeffs=None) -> "GKRBatchProverState":
        """n x the two prover states of GKRRoundSumcheck.prove of one dim behind one handle (sc_gkr_batch_prover_init): the interactive
        rounds under the CALLER's transcript -- 2 dim calls of prove_round, then finish.  Inputs as for prove_batch (all on the host or
        all on the GPU; the same object may stand for several instances); they are copied: nothing is read after this returns.
        Plans: dim <= 9 runs one block per instance; under _lib.policy(batch_slices=1), set when the handle is built, dim 10 .. 16
        (nnz <= 64 x 2^dim, at most 16 GiB) gives every instance to many blocks (plan batch.gkr_rounds_slices: same bits); other
        shapes take the serial plan.
        g2s and coeffs (both or neither) build the handle in TWO-POINT form (sc_gkr_two_point_init_batch): per instance a second point
        g2 and (alpha, beta); alpha eq(g, .) + beta eq(g2, .) stands where eq(g, .) stands, so the handle proves
        alpha W(g) + beta W(g2) = sum (alpha f1(g,x,y) + beta f1(g2,x,y)) f2(x) f3(y) -- a GKR layer below the output layer."""
        n = len(f1s)
        assert len(f2s) == n and len(f3s) == n and len(gs) == n, "one f1, f2, f3 and g per instance"
        second = _second_point(g2s, coeffs, n, f2s[0].num_vars if n else 0)
        dim = f2s[0].num_vars if n else 0
        ons = [m.on_device for m in list(f1s) + list(f2s) + list(f3s)]
        dev = bool(ons) and all(ons)
        assert dev or not any(ons), "mixing host and device inputs is not supported"
        g_arr = []
        for i in range(n):
            assert f2s[i].num_vars == dim and f3s[i].num_vars == dim and f1s[i].num_vars == 3 * dim, f"instance {i}: a batch has one dim"
            g_arr.append(_np64(gs[i]).reshape(-1, 4))
            assert g_arr[i].shape[0] == dim
        if dev:
            import torch
            torch.cuda.current_stream(f2s[0].evaluations.device).synchronize()  # the library works on its own stream

        def ptrs(vals):
            return (C.c_void_p * max(n, 1))(*[C.cast(v, C.c_void_p) for v in vals])

        f1p = [f._ptrs() for f in f1s]
        nnz = (C.c_uint64 * max(n, 1))(*[f.nnz for f in f1s])
        h = C.c_void_p()
        if second is None:
            check(lib().sc_gkr_batch_prover_init(n, dim, ptrs([p[0] for p in f1p]), ptrs([p[1] for p in f1p]), nnz, ptrs([_dense_ptr(m) for m in f2s]),
                                                 ptrs([_dense_ptr(m) for m in f3s]), ptrs([_ptr(a) for a in g_arr]), SC_TABLES_ON_DEVICE if dev else 0, C.byref(h)))
        else:
            g2_arr, coef = second
            check(lib().sc_gkr_two_point_init_batch(n, dim, ptrs([p[0] for p in f1p]), ptrs([p[1] for p in f1p]), nnz, ptrs([_dense_ptr(m) for m in f2s]),
                                                    ptrs([_dense_ptr(m) for m in f3s]), ptrs([_ptr(a) for a in g_arr]), ptrs([_ptr(a) for a in g2_arr]), _ptr(coef),
                                                    SC_TABLES_ON_DEVICE if dev else 0, C.byref(h)))
        return GKRBatchProverState(h, n, dim)

    @staticmethod
    def prover_init_batch_gates(mul_f1s: Sequence[SparseMultilinearExtension], add_f1s: Sequence[SparseMultilinearExtension], f2s: Sequence[DenseMultilinearExtension],
                                f3s: Sequence[DenseMultilinearExtension], gs, g2s=None, coeffs=None) -> "GKRBatchProverState":
        """prover_init_batch for layers of multiplication AND addition gates (sc_gkr_gates_init_batch):
            W_out[z] = sum over mul_f1 of v f2[x] f3[y] + sum over add_f1 of v (f2[x] + f3[y]),
        claimed at gs[i], or -- with g2s and coeffs -- as alpha W_out(g) + beta W_out(g2).  The handle is driven as any other (2 dim calls of
        prove_round, finish, reset, randomness); its finish returns f2(u), f3(v) and f3(v) T1(v) + T2(v), the value the verifier compares;
        tables() is refused; later layers come through next_layer_gates.  Plans: dim <= 9 with each list <= 64 x 2^dim runs one block per
        instance (batch.gkr_gates_one_block); every other shape, and every handle built under _lib.policy(gkr_gates_fused=0), is composed
        of three multiplication-only instances per instance (batch.gkr_gates_composed) -- same bits."""
        n = len(f2s)
        assert len(mul_f1s) == n and len(add_f1s) == n and len(f3s) == n and len(gs) == n, "one mul, add, f2, f3 and g per instance"
        dim = f2s[0].num_vars if n else 0
        second = _second_point(g2s, coeffs, n, dim)
        args, dev = _gates_args(n, dim, mul_f1s, add_f1s, f2s, f3s, gs, second)
        h = C.c_void_p()
        check(lib().sc_gkr_gates_init_batch(n, dim, *args, SC_TABLES_ON_DEVICE if dev else 0, C.byref(h)))
        st = GKRBatchProverState(h, n, dim)
        st._keep = args  # (nothing is read after init; kept only so that ctypes arrays outlive the call on every interpreter)
        return st

    @staticmethod
    def evaluate_layers_batch(f1_layers: Sequence[Sequence[SparseMultilinearExtension]], f2s: Sequence[DenseMultilinearExtension],
                              f3s: Sequence[DenseMultilinearExtension]) -> List[List[DenseMultilinearExtension]]:
        """The values of a circuit's layers for n instances of one dim, on the GPU (sc_gkr_layers_eval_batch): f1_layers[k][i] is the wiring
        of layer k of instance i, layer 0 next to the inputs f2s[i], f3s[i] -> out[k][i], with
            out[0][i][z] = sum over f1_layers[0][i]'s non-zeros (z | x << dim | y << 2 dim, v) of v f2s[i][x] f3s[i][y]
            out[k][i]    = the same over f1_layers[k][i] with out[k-1][i] on both sides.
        The same object may stand for several instances and layers (one wiring for all instances is the usual case).  Inputs all on the
        host or all on the GPU; device tensors in give device tensors out, allocated here and usable directly as the f2s / f3s of
        prover_init_batch and GKRBatchProverState.next_layer -- a layer's values never leave the device."""
        n_layers, n = len(f1_layers), len(f2s)
        assert len(f3s) == n and all(len(layer) == n for layer in f1_layers), "one f1 per layer and instance, one f2 and f3 per instance"
        if n == 0 or n_layers == 0:
            check(lib().sc_gkr_layers_eval_batch(n, 0, n_layers, None, None, None, None, None, 0, None))
            return [[] for _ in range(n_layers)]
        dim = f2s[0].num_vars
        flat = [f for layer in f1_layers for f in layer]
        ons = [m.on_device for m in flat + list(f2s) + list(f3s)]
        dev = all(ons)
        assert dev or not any(ons), "mixing host and device inputs is not supported"
        for i in range(n):
            assert f2s[i].num_vars == dim and f3s[i].num_vars == dim and all(layer[i].num_vars == 3 * dim for layer in f1_layers), f"instance {i}: a batch has one dim"
        total = n_layers * n
        if dev:
            import torch
            device = f2s[0].evaluations.device
            outs = [torch.empty((1 << dim, 4), dtype=torch.int64, device=device) for _ in range(total)]
            torch.cuda.current_stream(device).synchronize()  # the library works on its own stream
            out_ptrs = [C.c_void_p(t.data_ptr()) for t in outs]
        else:
            outs = [np.empty((1 << dim, 4), dtype=np.uint64) for _ in range(total)]
            out_ptrs = [_ptr(t) for t in outs]

        def ptrs(vals):
            return (C.c_void_p * len(vals))(*[C.cast(v, C.c_void_p) for v in vals])

        f1p = [f._ptrs() for f in flat]
        nnz = (C.c_uint64 * total)(*[f.nnz for f in flat])
        check(lib().sc_gkr_layers_eval_batch(n, dim, n_layers, ptrs([p[0] for p in f1p]), ptrs([p[1] for p in f1p]), nnz, ptrs([_dense_ptr(m) for m in f2s]),
                                             ptrs([_dense_ptr(m) for m in f3s]), SC_TABLES_ON_DEVICE if dev else 0, ptrs(out_ptrs)))
        return [[DenseMultilinearExtension(dim, outs[k * n + i]) for i in range(n)] for k in range(n_layers)]

    @staticmethod
    def evaluate_layers_batch_gates(mul_layers: Sequence[Sequence[SparseMultilinearExtension]], add_layers: Sequence[Sequence[SparseMultilinearExtension]],
                                    f2s: Sequence[DenseMultilinearExtension], f3s: Sequence[DenseMultilinearExtension]) -> List[List[DenseMultilinearExtension]]:
        """evaluate_layers_batch for layers of multiplication AND addition gates (sc_gkr_gates_layers_eval_batch): mul_layers[k][i] and
        add_layers[k][i] are the two wiring lists of layer k of instance i, and
            out[0][i][z] = sum over mul of v f2s[i][x] f3s[i][y] + sum over add of v (f2s[i][x] + f3s[i][y])
            out[k][i]    = the same over layer k's lists with out[k-1][i] on both sides.
        Device tensors in give device tensors out, usable directly as the f2s / f3s of prover_init_batch_gates and next_layer_gates."""
        n_layers, n = len(mul_layers), len(f2s)
        assert len(add_layers) == n_layers and len(f3s) == n and all(len(layer) == n for layer in list(mul_layers) + list(add_layers)), "one mul and one add list per layer and instance"
        if n == 0 or n_layers == 0:
            check(lib().sc_gkr_gates_layers_eval_batch(n, 0, n_layers, None, None, None, None, None, None, None, None, 0, None))
            return [[] for _ in range(n_layers)]
        dim = f2s[0].num_vars
        flat_m, flat_a = [f for layer in mul_layers for f in layer], [f for layer in add_layers for f in layer]
        ons = [m.on_device for m in flat_m + flat_a + list(f2s) + list(f3s)]
        dev = all(ons)
        assert dev or not any(ons), "mixing host and device inputs is not supported"
        for i in range(n):
            assert f2s[i].num_vars == dim and f3s[i].num_vars == dim, f"instance {i}: a batch has one dim"
        assert all(f.num_vars == 3 * dim for f in flat_m + flat_a), "a batch has one dim"
        total = n_layers * n
        if dev:
            import torch
            device = f2s[0].evaluations.device
            outs = [torch.empty((1 << dim, 4), dtype=torch.int64, device=device) for _ in range(total)]
            torch.cuda.current_stream(device).synchronize()  # the library works on its own stream
            out_ptrs = [C.c_void_p(t.data_ptr()) for t in outs]
        else:
            outs = [np.empty((1 << dim, 4), dtype=np.uint64) for _ in range(total)]
            out_ptrs = [_ptr(t) for t in outs]

        def ptrs(vals):
            return (C.c_void_p * len(vals))(*[C.cast(v, C.c_void_p) for v in vals])

        lists = []
        for flat in (flat_m, flat_a):
            f1p = [f._ptrs() for f in flat]
            lists += [ptrs([p[0] for p in f1p]), ptrs([p[1] for p in f1p]), (C.c_uint64 * total)(*[f.nnz for f in flat])]
        check(lib().sc_gkr_gates_layers_eval_batch(n, dim, n_layers, *lists, ptrs([_dense_ptr(m) for m in f2s]), ptrs([_dense_ptr(m) for m in f3s]),
                                                   SC_TABLES_ON_DEVICE if dev else 0, ptrs(out_ptrs)))
        return [[DenseMultilinearExtension(dim, outs[k * n + i]) for i in range(n)] for k in range(n_layers)]

    @staticmethod
    def verify(rng: Blake2b512Rng, f2_num_vars: int, proof: GKRProof, claimed_sum) -> GKRRoundSumcheckSubClaim:
        """mod.rs:147-192"""
        dim = f2_num_vars
        u, exp1 = _verify_phase(rng, proof.phase1_sumcheck_msgs, dim, claimed_sum)
        v, exp2 = _verify_phase(rng, proof.phase2_sumcheck_msgs, dim, exp1)
        return GKRRoundSumcheckSubClaim(u, v, exp2)


class GKRBatchProverState:
    """The handle of GKRRoundSumcheck.prover_init_batch (sc_gkr_batch_prover_*): n instances, 2 dim rounds, one call per round."""

    def __init__(self, h, n: int, dim: int):
        self._h, self.n, self.dim = h, n, dim

    def _chal(self, r, shared: bool):
        a = np.ascontiguousarray(_np64(r).reshape(-1, 4))
        assert a.shape[0] == (1 if shared else self.n), "one challenge per instance, or one for all with shared=True"
        return a

    def prove_round(self, r=None, shared: bool = False) -> np.ndarray:
        """-> (n, 3, 4): message t of phase one (calls 0 .. dim-1), then of phase two.  r: None exactly on the first call, afterwards the
        previous round's challenges, (n, 4) or -- shared -- (4,)"""
        out = np.empty((self.n, 3, 4), dtype=np.uint64)
        a = None if r is None else self._chal(r, shared)
        check(lib().sc_gkr_batch_prove_round(self._h, None if a is None else _ptr(a), 1 if shared else 0, _ptr(out)))
        return out

    def finish(self, r, shared: bool = False):
        """the last challenge v_{dim-1} -> (uv (n, 2, dim, 4), final (n, 3, 4): f1(g,u,v), f2(u), f2(u) f3(v))"""
        a = self._chal(r, shared)
        uv = np.empty((self.n, 2, self.dim, 4), dtype=np.uint64)
        fin = np.empty((self.n, 3, 4), dtype=np.uint64)
        check(lib().sc_gkr_batch_prover_finish(self._h, _ptr(a), 1 if shared else 0, _ptr(uv), _ptr(fin)))
        return uv, fin

    @property
    def round(self) -> int:
        rnd = C.c_uint32()
        check(lib().sc_gkr_batch_prover_state(self._h, 0, None, None, None, C.byref(rnd)))
        return int(rnd.value)

    def randomness(self, i: int) -> np.ndarray:
        """u followed by the v's instance i has received so far"""
        out = np.zeros((2 * self.dim, 4), dtype=np.uint64)
        k = C.c_uint32()
        check(lib().sc_gkr_batch_prover_state(self._h, i, _ptr(out), C.byref(k), None, None))
        return out[: k.value].copy()

    def tables(self, i: int) -> np.ndarray:
        """the current phase's two tables of instance i, canonical: (2, 2^(dim - bound), 4)"""
        t = self.round
        pr = t - self.dim if t > self.dim else t
        out = np.empty((2, 1 << (self.dim - max(pr - 1, 0)), 4), dtype=np.uint64)
        check(lib().sc_gkr_batch_prover_state(self._h, i, None, None, _ptr(out), None))
        return out

    def reset(self) -> None:
        check(lib().sc_gkr_batch_prover_reset(self._h))

    def next_layer(self, f2s, f3s, gs, f1s=None, g2s=None, coeffs=None) -> None:
        """The handle onto the next layer's inputs (sc_gkr_layer_next_batch): nothing is allocated, and afterwards the handle is at round 0
        exactly as prover_init_batch over these inputs would leave it -- same plan, same bits.  f1s=None keeps the wiring the handle
        holds.  Inputs are where prover_init_batch's were (all on the host, or all on the GPU) and are copied: nothing is read after this
        returns.  Callable in any state; an argument error leaves the handle where it was.  The copy fits whenever the objects repeat in
        the pattern prover_init_batch's did and f1 is kept or has no more non-zeros per instance than it had there.
        g2s and coeffs (both or neither) put the handle onto a layer in TWO-POINT form (sc_gkr_two_point_next_batch), whichever form it
        was built in; without them the layer is in one-point form."""
        n, dim = self.n, self.dim
        second = _second_point(g2s, coeffs, n, dim)
        assert len(f2s) == n and len(f3s) == n and len(gs) == n and (f1s is None or len(f1s) == n), "one f2, f3 and g (and f1) per instance"
        ons = [m.on_device for m in list(f1s or []) + list(f2s) + list(f3s)]
        dev = all(ons)
        assert dev or not any(ons), "mixing host and device inputs is not supported"
        g_arr = []
        for i in range(n):
            assert f2s[i].num_vars == dim and f3s[i].num_vars == dim and (f1s is None or f1s[i].num_vars == 3 * dim), f"instance {i}: the handle's dim is {dim}"
            g_arr.append(_np64(gs[i]).reshape(-1, 4))
            assert g_arr[i].shape[0] == dim
        if dev:
            import torch
            torch.cuda.current_stream(f2s[0].evaluations.device).synchronize()  # the library works on its own stream

        def ptrs(vals):
            return (C.c_void_p * n)(*[C.cast(v, C.c_void_p) for v in vals])

        f1p = [f._ptrs() for f in f1s] if f1s is not None else None
        head = (self._h, ptrs([p[0] for p in f1p]) if f1p else None, ptrs([p[1] for p in f1p]) if f1p else None, (C.c_uint64 * n)(*[f.nnz for f in f1s]) if f1p else None,
                ptrs([_dense_ptr(m) for m in f2s]), ptrs([_dense_ptr(m) for m in f3s]), ptrs([_ptr(a) for a in g_arr]))
        if second is None:
            check(lib().sc_gkr_layer_next_batch(*head, SC_TABLES_ON_DEVICE if dev else 0))
        else:
            g2_arr, coef = second
            check(lib().sc_gkr_two_point_next_batch(*head, ptrs([_ptr(a) for a in g2_arr]), _ptr(coef), SC_TABLES_ON_DEVICE if dev else 0))

    def next_layer_gates(self, f2s, f3s, gs, mul_f1s=None, add_f1s=None, g2s=None, coeffs=None) -> None:
        """next_layer for a handle of prover_init_batch_gates (sc_gkr_gates_next_batch): mul_f1s and add_f1s both None keeps both lists,
        both given is new wiring.  g2s and coeffs (both or neither) choose the layer's form.  An argument error leaves a proof in progress
        exactly where it was."""
        n, dim = self.n, self.dim
        if (mul_f1s is None) != (add_f1s is None):
            raise ValueError("mul_f1s and add_f1s come together (new wiring) or not at all (the handle's wiring is kept)")
        assert len(f2s) == n and len(f3s) == n and len(gs) == n, "one f2, f3 and g per instance"
        second = _second_point(g2s, coeffs, n, dim)
        args, dev = _gates_args(n, dim, mul_f1s, add_f1s, f2s, f3s, gs, second)
        check(lib().sc_gkr_gates_next_batch(self._h, *args, SC_TABLES_ON_DEVICE if dev else 0))

    def close(self) -> None:
        if self._h:
            lib().sc_gkr_batch_prover_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
