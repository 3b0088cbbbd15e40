"""The oracle queries behind a batch of proofs: sc_poly_evaluate_batch / sc_gkr_subclaim_batch against a loop of the single-instance calls
over the same inputs (sc_poly_evaluate; sc_sparse_evaluate + 2 x sc_poly_evaluate) -- what a caller of the batched provers writes without
them.   python tools/eval_batch_bench.py [--out FILE] [--quick]

ML: the c2 shape (one product of three tables) at nv 6 / 8 / 10 and config 3's shape (ten tables) at nv 6 / 8, host and device tables, plus
the c2 shape at nv 12 / 14 on the device (where the one-block plan's envelope ends).  GKR: dim 6 / 8 / 9 with nnz = 2 x 2^dim, device
inputs.  n = 1, 16, 256.  The batched call (policy "batch" = 2, so that small n show the kernel and not the call's own choice) and the loop
are ALTERNATED within one process, seven repetitions of at least 256 instances each; medians, with the min-max spread of each beside them.
The single-instance functions are the parent commit's, unchanged: the loop IS the parent's cost.  Both sides' outputs of the last repetition
are compared bit for bit, and a sample of instances with the oracle.  `wins`: the batched median beats the loop's by more than the two
spreads together -- the condition under which policy "batch" = 1 may choose the kernel for that (shape, n)."""
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib

C2 = [[0, 1, 2]]
C3 = [[0, 1, 2, 3], [4, 5, 6], [7, 8], [9]]
ML_ROWS = [("c2", C2, 6, True), ("c2", C2, 8, True), ("c2", C2, 10, True), ("c3", C3, 6, True), ("c3", C3, 8, True),
           ("c2", C2, 6, False), ("c2", C2, 8, False), ("c2", C2, 10, False), ("c3", C3, 6, False), ("c3", C3, 8, False),
           ("c2", C2, 12, True), ("c2", C2, 14, True)]
GKR_DIMS = [6, 8, 9]
NS = [1, 16, 256]
REPS, MIN_INSTANCES = 7, 256


def summary(ts):
    return {"median": round(statistics.median(ts), 2), "min": round(min(ts), 2), "max": round(max(ts), 2)}


def verdict(tb, tl):
    mb, ml = statistics.median(tb), statistics.median(tl)
    return {"batched_us_per_instance": summary(tb), "loop_us_per_instance": summary(tl), "speedup": round(ml / mb, 2),
            "wins": bool(ml - mb > (max(tb) - min(tb)) + (max(tl) - min(tl)))}


class MlBatch:
    def __init__(self, n, nv, shapes, seed, device):
        nt = max(max(s) for s in shapes) + 1
        self.n, self.nv, self.U = n, nv, nt
        self.tabs = np.stack([np.stack([cref.synth_table(seed + 7919 * i, s, 1 << nv) for s in range(nt)]) for i in range(min(n, 16))])
        self.tabs = np.ascontiguousarray(self.tabs[np.arange(n) % self.tabs.shape[0]])  # (n, nt, 2^nv, 4): tables of its own per instance
        self.coefs = np.stack([cref.synth_table(seed + 7919 * i, 1000, len(shapes)) for i in range(n)])
        self.points = cref.synth_table(seed, 5000, n * nv).reshape(n, nv, 4)
        self.shapes = shapes
        self.big = torch.from_numpy(self.tabs.view(np.int64)).to("cuda:0") if device else None
        torch.cuda.synchronize()
        offs, idx = [0], []
        for sh in shapes:
            idx.extend(sh)
            offs.append(len(idx))
        self.offs, self.idx = np.asarray(offs, np.uint32), np.asarray(idx, np.uint32)
        self.descs = (_lib.PolyDesc * n)()
        self.keep = []
        for i in range(n):
            ptrs = (C.c_void_p * nt)(*[(self.big[i, s].data_ptr() if device else self.tabs[i, s].ctypes.data) for s in range(nt)])
            d = self.descs[i]
            d.num_vars, d.max_multiplicands, d.n_products, d.n_tables = nv, max(len(s) for s in shapes), len(shapes), nt
            d.coeffs = self.coefs[i].ctypes.data_as(C.POINTER(C.c_uint64))
            d.prod_offsets = self.offs.ctypes.data_as(C.POINTER(C.c_uint32))
            d.prod_indices = self.idx.ctypes.data_as(C.POINTER(C.c_uint32))
            d.tables = C.cast(ptrs, C.POINTER(C.c_void_p))
            d.flags = _lib.SC_TABLES_ON_DEVICE if device else 0
            self.keep.append(ptrs)

    def oracle(self, i):
        prods = [(self.coefs[i][k], list(sh)) for k, sh in enumerate(self.shapes)]
        return cref.poly_evaluate(cref.PolyDesc(self.nv, prods, [self.tabs[i, s] for s in range(self.U)]), self.points[i])


def ml_batched(b, n, policy, out, tv):
    L = sc.lib()
    calls = max(1, -(-MIN_INSTANCES // n))
    with _lib.policy(batch=policy):
        t0 = time.perf_counter()
        for _ in range(calls):
            _lib.check(L.sc_poly_evaluate_batch(b.descs, n, C.c_void_p(b.points.ctypes.data), C.c_void_p(out.ctypes.data), C.c_void_p(tv.ctypes.data)))
        return (time.perf_counter() - t0) / (calls * n) * 1e6  # (the call returns after its synchronise: the values are on the host)


def ml_loop(b, n, out, tv):
    """the parent commit's way: one sc_poly_evaluate per instance"""
    L = sc.lib()
    calls = max(1, -(-MIN_INSTANCES // n))
    t0 = time.perf_counter()
    for _ in range(calls):
        for i in range(n):
            _lib.check(L.sc_poly_evaluate(C.byref(b.descs[i]), C.c_void_p(b.points[i].ctypes.data), C.c_void_p(out[i].ctypes.data), C.c_void_p(tv[i].ctypes.data)))
    return (time.perf_counter() - t0) / (calls * n) * 1e6


class GkrBatch:
    def __init__(self, n, dim, seed):
        N = 1 << dim
        rng = np.random.default_rng(seed)
        self.n, self.dim = n, dim
        self.idx = np.stack([np.unique(rng.integers(0, 1 << (3 * dim), size=4 * N, dtype=np.uint64))[: 2 * N] for _ in range(n)])  # distinct: sc_sparse_evaluate's contract
        self.vals = np.stack([cref.synth_table(seed + i, 1, 2 * N) for i in range(n)])
        self.f2 = np.stack([cref.synth_table(seed + i, 2, N) for i in range(n)])
        self.f3 = np.stack([cref.synth_table(seed + i, 3, N) for i in range(n)])
        self.g = np.stack([cref.synth_table(seed + i, 4, dim) for i in range(n)])
        self.uv = cref.synth_table(seed, 6000, n * 2 * dim).reshape(n, 2, dim, 4)
        self.guv = np.ascontiguousarray(np.concatenate([self.g, self.uv[:, 0], self.uv[:, 1]], axis=1))
        td = lambda a: torch.from_numpy(a.view(np.int64)).to("cuda:0")
        self.dev = [td(self.idx), td(self.vals), td(self.f2), td(self.f3)]
        torch.cuda.synchronize()
        arr = lambda vals: (C.c_void_p * n)(*vals)
        self.p_idx, self.p_vals, self.p_f2, self.p_f3 = (arr([t[i].data_ptr() for i in range(n)]) for t in self.dev)
        self.p_g = arr([self.g[i].ctypes.data for i in range(n)])
        self.nnz = (C.c_uint64 * n)(*([2 * N] * n))
        self.one = cref.ints_to_mont([1])
        self.offs, self.ix = np.asarray([0, 1], np.uint32), np.asarray([0], np.uint32)
        self.d1 = []  # per instance the one-table descriptors of f2 and f3 (device tables), built once: not part of the loop's time
        for i in range(n):
            pair = []
            for t in (self.dev[2], self.dev[3]):
                ptr = (C.c_void_p * 1)(t[i].data_ptr())
                d = _lib.PolyDesc()
                d.num_vars, d.max_multiplicands, d.n_products, d.n_tables = dim, 1, 1, 1
                d.coeffs = self.one.ctypes.data_as(C.POINTER(C.c_uint64))
                d.prod_offsets = self.offs.ctypes.data_as(C.POINTER(C.c_uint32))
                d.prod_indices = self.ix.ctypes.data_as(C.POINTER(C.c_uint32))
                d.tables = C.cast(ptr, C.POINTER(C.c_void_p))
                d.flags = _lib.SC_TABLES_ON_DEVICE
                pair.append((d, ptr))
            self.d1.append(pair)

    def oracle_f1(self, i):
        oi, ov = cref.sparse_fix_variables(self.idx[i], self.vals[i], self.guv[i])
        return ov[0] if len(oi) else np.zeros(4, np.uint64)


def gkr_batched(b, n, policy, out):
    L = sc.lib()
    calls = max(1, -(-MIN_INSTANCES // n))
    with _lib.policy(batch=policy):
        t0 = time.perf_counter()
        for _ in range(calls):
            _lib.check(L.sc_gkr_subclaim_batch(n, b.dim, b.p_idx, b.p_vals, b.nnz, b.p_f2, b.p_f3, b.p_g, C.c_void_p(b.uv.ctypes.data), _lib.SC_TABLES_ON_DEVICE,
                                               C.c_void_p(out.ctypes.data)))
        return (time.perf_counter() - t0) / (calls * n) * 1e6


def gkr_loop(b, n, out):
    """the parent commit's way: sc_sparse_evaluate (a host list) and two sc_poly_evaluate per instance; the product is three host multiplications"""
    L = sc.lib()
    calls = max(1, -(-MIN_INSTANCES // n))
    t0 = time.perf_counter()
    for _ in range(calls):
        for i in range(n):
            _lib.check(L.sc_sparse_evaluate(C.c_void_p(b.idx[i].ctypes.data), C.c_void_p(b.vals[i].ctypes.data), 2 << b.dim, 3 * b.dim, C.c_void_p(b.guv[i].ctypes.data),
                                            C.c_void_p(out[i, 0].ctypes.data)))
            _lib.check(L.sc_poly_evaluate(C.byref(b.d1[i][0][0]), C.c_void_p(b.uv[i, 0].ctypes.data), C.c_void_p(out[i, 1].ctypes.data), None))
            _lib.check(L.sc_poly_evaluate(C.byref(b.d1[i][1][0]), C.c_void_p(b.uv[i, 1].ctypes.data), C.c_void_p(out[i, 2].ctypes.data), None))
    return (time.perf_counter() - t0) / (calls * n) * 1e6


def main():
    args = sys.argv[1:]
    ns = [1, 256] if "--quick" in args else NS
    ml_rows = ML_ROWS[:2] + ML_ROWS[5:6] if "--quick" in args else ML_ROWS
    rows = []
    for name, shapes, nv, device in ml_rows:
        b = MlBatch(max(ns), nv, shapes, 9300 + nv, device)
        row = {"call": "sc_poly_evaluate_batch", "shape": name, "nv": nv, "tables": "device" if device else "host", "n": {}}
        for n in ns:
            got, ref = np.zeros((n, 4), np.uint64), np.zeros((n, 4), np.uint64)
            gtv, rtv = np.zeros((n, b.U, 4), np.uint64), np.zeros((n, b.U, 4), np.uint64)
            ml_batched(b, n, 2, got, gtv)  # (work areas, code objects)
            ml_loop(b, min(n, 8), ref, rtv)
            tb, tl = [], []
            for _ in range(REPS):  # alternated
                got[:] = 0
                tb.append(ml_batched(b, n, 2, got, gtv))
                tl.append(ml_loop(b, n, ref, rtv))
            assert np.array_equal(got, ref) and np.array_equal(gtv, rtv), f"{name} nv {nv}, n {n}: the batched call and the loop differ"
            for i in range(min(n, 16)):
                assert np.array_equal(got[i], b.oracle(i)), f"{name} nv {nv}, n {n}, instance {i}: differs from the oracle"
            row["n"][str(n)] = verdict(tb, tl)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del b
    for dim in ([6] if "--quick" in args else GKR_DIMS):
        b = GkrBatch(max(ns), dim, 9400 + dim)
        row = {"call": "sc_gkr_subclaim_batch", "dim": dim, "nnz": 2 << dim, "inputs": "device (the loop's sc_sparse_evaluate takes the list from the host)", "n": {}}
        for n in ns:
            got, ref = np.zeros((n, 4, 4), np.uint64), np.zeros((n, 4, 4), np.uint64)
            gkr_batched(b, n, 2, got)
            gkr_loop(b, min(n, 8), ref)
            tb, tl = [], []
            for _ in range(REPS):
                got[:] = 0
                tb.append(gkr_batched(b, n, 2, got))
                tl.append(gkr_loop(b, n, ref))
            assert np.array_equal(got[:, :3], ref[:, :3]), f"dim {dim}, n {n}: the batched call and the loop differ"
            for i in range(min(n, 16)):
                assert np.array_equal(got[i, 0], b.oracle_f1(i)), f"dim {dim}, n {n}, instance {i}: f1(g,u,v) differs from the oracle"
            row["n"][str(n)] = verdict(tb, tl)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del b
    out = {"tool": "tools/eval_batch_bench.py", "library": os.path.basename(_lib.SO_PATH), "reps": REPS, "min_instances_per_rep": MIN_INSTANCES,
           "baseline": "a loop of the single-instance calls over the same inputs (sc_poly_evaluate; sc_sparse_evaluate + 2 x sc_poly_evaluate)",
           "statistic": "median of the repetitions, microseconds per instance, with min and max", "wins": "batched median + both spreads < loop median", "rows": rows}
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
