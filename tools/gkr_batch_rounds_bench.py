"""The batched interactive GKR rounds: a sc_gkr_batch_prover handle built under policy "batch" = 2 (k_batch_gkr_phase<1|2> and k_batch_round:
one launch per round call for the whole batch) against what a caller with a transcript of its own had before -- a loop, written here, over
the single-instance entry points: per instance sc_gkr_phase_one, sc_prover_init, dim x sc_prove_round, sc_prover_bind_final (f2(u)),
sc_gkr_phase_two, sc_dense_scale, sc_prover_init, dim x sc_prove_round.
    python tools/gkr_batch_rounds_bench.py [--out FILE] [--quick]

Inputs are device-resident, nnz = 2 x 2^dim distinct indices, dim 6 / 8 / 9, n = 1 / 16 / 256; fixed, distinct challenges per instance (no
transcript: the caller's hashing is not the library's time).  The two are ALTERNATED within one process, seven repetitions of several
proofs each; medians, with the min-max spread beside them.  Two figures for the handle: `rewound` is reset + 2 dim round calls + finish
(phase one's tables are kept: the same inputs under other challenges), `with_init` is init + 2 dim round calls + finish + free (new
inputs, which is what the loop pays every time).  Both sides' messages of the last repetition are compared bit for bit.
`wins`: the handle's median WITH init beats the loop's by more than the two spreads together; `wins_rewound` the same without init.
For n <= 16 the handle's own serial plan (a handle built under policy "batch" = 0, with init) is timed as well: it is what a small-n
rule under policy "batch" = 1 would run instead of the kernel."""
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

DIMS = [6, 8, 9]
NS = [1, 16, 256]
REPS = 7
ONE = cref.ints_to_mont([1])[0]
DEV = _lib.SC_TABLES_ON_DEVICE
V = C.c_void_p


def summary(ts):
    return {"median": round(statistics.median(ts), 2), "min": round(min(ts), 2), "max": round(max(ts), 2)}


def td(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


class Batch:
    def __init__(self, n, dim, seed):
        self.n, self.dim = n, dim
        N, nnz = 1 << dim, 2 << dim
        self.N, self.nnz = N, nnz
        rng = np.random.default_rng(seed)
        k = min(n, 16)  # distinct inputs; further instances repeat them as objects of their own
        idx = []
        for i in range(k):
            u = np.unique(rng.integers(0, 1 << (3 * dim), size=2 * nnz, dtype=np.uint64))
            idx.append(rng.permutation(u)[:nnz])
            assert idx[-1].shape[0] == nnz
        self.idx = [td(idx[i % k]) for i in range(n)]
        self.vals = [td(cref.synth_table(seed + i % k, 1, nnz)) for i in range(n)]
        self.f2 = [td(cref.synth_table(seed + i % k, 2, N)) for i in range(n)]
        self.f3 = [td(cref.synth_table(seed + i % k, 3, N)) for i in range(n)]
        self.g = [cref.synth_table(seed + i % k, 4, dim) for i in range(n)]
        self.chal = np.ascontiguousarray(cref.synth_table(seed, 7000, 2 * dim * n).reshape(2 * dim, n, 4))  # [challenge j][instance]
        self.u = [np.ascontiguousarray(self.chal[:dim, i]) for i in range(n)]
        # the loop's work areas, allocated once
        self.h_g = torch.empty((N, 4), dtype=torch.int64, device="cuda:0")
        self.gi = torch.empty(nnz, dtype=torch.int64, device="cuda:0")
        self.gv = torch.empty((nnz, 4), dtype=torch.int64, device="cuda:0")
        self.f1gu = torch.empty((N, 4), dtype=torch.int64, device="cuda:0")
        self.t1 = torch.empty((N, 4), dtype=torch.int64, device="cuda:0")
        self.fin = torch.empty((2, 4), dtype=torch.int64, device="cuda:0")
        self.offs, self.ix = np.asarray([0, 2], np.uint32), np.asarray([0, 1], np.uint32)
        torch.cuda.synchronize()

        def ptrs(vals):
            return (V * n)(*vals)
        self.args = (ptrs([t.data_ptr() for t in self.idx]), ptrs([t.data_ptr() for t in self.vals]), (C.c_uint64 * n)(*[nnz] * n), ptrs([t.data_ptr() for t in self.f2]),
                     ptrs([t.data_ptr() for t in self.f3]), ptrs([a.ctypes.data for a in self.g]))

    def init(self, policy=2):
        h = V()
        with _lib.policy(batch=policy):
            _lib.check(sc.lib().sc_gkr_batch_prover_init(self.n, self.dim, *self.args, DEV, C.byref(h)))
        return h

    def desc(self, a, b):
        d = _lib.PolyDesc()
        tabs = (V * 2)(a, b)
        d.num_vars, d.max_multiplicands, d.n_products, d.n_tables = self.dim, 2, 1, 2
        d.coeffs = ONE.ctypes.data_as(C.POINTER(C.c_uint64))
        d.prod_offsets = self.offs.ctypes.data_as(C.POINTER(C.c_uint32))
        d.prod_indices = self.ix.ctypes.data_as(C.POINTER(C.c_uint32))
        d.tables = C.cast(tabs, C.POINTER(V))
        d.flags = DEV | _lib.SC_TABLES_BORROW
        return d, tabs


def handle_proof(b, h, out, rewind):
    """[reset +] 2 dim round calls + finish; out (2 dim, n, 3, 4)"""
    L = sc.lib()
    if rewind:
        _lib.check(L.sc_gkr_batch_prover_reset(h))
    for t in range(2 * b.dim):
        _lib.check(L.sc_gkr_batch_prove_round(h, V(b.chal[t - 1].ctypes.data) if t else None, 0, V(out[t].ctypes.data)))
    _lib.check(L.sc_gkr_batch_prover_finish(h, V(b.chal[2 * b.dim - 1].ctypes.data), 0, None, None))


def loop_proof(b, out):
    """the caller's loop over the single-instance entry points; out (2 dim, n, 3, 4)"""
    L, dim = sc.lib(), b.dim
    n1 = C.c_uint64()
    f2u = np.empty((2, 4), np.uint64)
    for i in range(b.n):
        g, u = V(b.g[i].ctypes.data), V(b.u[i].ctypes.data)
        _lib.check(L.sc_gkr_phase_one(V(b.idx[i].data_ptr()), V(b.vals[i].data_ptr()), b.nnz, dim, V(b.f3[i].data_ptr()), g, DEV, V(b.h_g.data_ptr()), V(b.gi.data_ptr()),
                                      V(b.gv.data_ptr()), C.byref(n1)))
        d, keep = b.desc(b.h_g.data_ptr(), b.f2[i].data_ptr())
        p = V()
        _lib.check(L.sc_prover_init(C.byref(d), C.byref(p)))
        for t in range(dim):
            _lib.check(L.sc_prove_round(p, V(b.chal[t - 1, i].ctypes.data) if t else None, V(out[t, i].ctypes.data)))
        _lib.check(L.sc_prover_bind_final(p, V(b.chal[dim - 1, i].ctypes.data), V(b.fin.data_ptr())))
        f2u[:] = b.fin.cpu().numpy().view(np.uint64)  # (h_g(u), f2(u)); the copy waits for the device
        L.sc_prover_free(p)
        _lib.check(L.sc_gkr_phase_two(V(b.gi.data_ptr()), V(b.gv.data_ptr()), n1.value, dim, u, DEV, V(b.f1gu.data_ptr())))
        _lib.check(L.sc_dense_scale(V(b.f3[i].data_ptr()), b.N, V(f2u[1].ctypes.data), V(b.t1.data_ptr()), DEV))
        d, keep = b.desc(b.f1gu.data_ptr(), b.t1.data_ptr())
        p = V()
        _lib.check(L.sc_prover_init(C.byref(d), C.byref(p)))
        for r in range(dim):
            _lib.check(L.sc_prove_round(p, V(b.chal[dim + r - 1, i].ctypes.data) if r else None, V(out[dim + r, i].ctypes.data)))
        L.sc_prover_free(p)


def timed(fn, count):
    t0 = time.perf_counter()
    for _ in range(count):
        fn()
    return (time.perf_counter() - t0) / count * 1e6


def main():
    args = sys.argv[1:]
    quick = "--quick" in args
    rows = []
    for dim in (DIMS[:1] if quick else DIMS):
        row = {"dim": dim, "nnz": 2 << dim, "inputs": "device", "n": {}}
        for n in ([1, 16] if quick else NS):
            b = Batch(n, dim, 9700 + dim)
            count = max(2, 32 // n)
            got, ref = np.zeros((2 * dim, n, 3, 4), np.uint64), np.zeros((2 * dim, n, 3, 4), np.uint64)
            h = b.init()
            before = _lib.plan_stats()
            handle_proof(b, h, got, True)  # (code objects, first-launch attributes)
            loop_proof(b, ref)

            def with_init():
                hh = b.init()
                handle_proof(b, hh, got, False)
                sc.lib().sc_gkr_batch_prover_free(hh)
            with_init()

            def serial_with_init():  # the handle's own serial plan: what a small-n rule under policy "batch" = 1 would choose instead
                hh = b.init(0)
                handle_proof(b, hh, ser, False)
                sc.lib().sc_gkr_batch_prover_free(hh)
            ser = np.zeros_like(got)
            serial_leg = n <= 16
            if serial_leg:
                serial_with_init()
                assert np.array_equal(ser, ref), f"dim {dim}, n {n}: the handle's serial plan and the loop differ"
            rw, wi, lp, sp = [], [], [], []
            for _ in range(REPS):  # alternated
                got[:] = 0
                rw.append(timed(lambda: handle_proof(b, h, got, True), count))
                wi.append(timed(with_init, count))
                lp.append(timed(lambda: loop_proof(b, ref), max(1, count // 2)))
                if serial_leg:
                    sp.append(timed(serial_with_init, max(1, count // 2)))
            after = _lib.plan_stats()
            assert after["batch.gkr_rounds_one_block"] > before["batch.gkr_rounds_one_block"] and (after["batch.gkr_rounds_serial"] > before["batch.gkr_rounds_serial"]) == serial_leg
            assert np.array_equal(got, ref), f"dim {dim}, n {n}: the handle and the loop differ"
            sc.lib().sc_gkr_batch_prover_free(h)
            spread = lambda ts: max(ts) - min(ts)
            mr, mw, ml = statistics.median(rw), statistics.median(wi), statistics.median(lp)
            row["n"][str(n)] = {"handle_rewound_us_per_proof": summary(rw), "handle_with_init_us_per_proof": summary(wi), "loop_us_per_proof": summary(lp),
                                "handle_rewound_us_per_round_call": summary([x / (2 * dim) for x in rw]), "loop_us_per_instance_round": round(ml / (2 * dim * n), 3),
                                "handle_rewound_us_per_instance_round": round(mr / (2 * dim * n), 3), "speedup_with_init": round(ml / mw, 2), "speedup_rewound": round(ml / mr, 2),
                                "wins": bool(ml - mw > spread(wi) + spread(lp)), "wins_rewound": bool(ml - mr > spread(rw) + spread(lp))}
            if serial_leg:  # (a gkr_rounds_batch_min_n rule would pay only where this is the faster of the handle's two plans)
                row["n"][str(n)]["serial_plan_with_init_us_per_proof"] = summary(sp)
                row["n"][str(n)]["kernel_ahead_of_serial_plan_with_init"] = bool(statistics.median(sp) - mw > spread(wi) + spread(sp))
            del b
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"tool": "tools/gkr_batch_rounds_bench.py", "library": os.path.basename(_lib.SO_PATH), "reps": REPS,
           "handle": "policy batch = 2; rewound: sc_gkr_batch_prover_reset + 2 dim calls of sc_gkr_batch_prove_round + finish; with_init: init + the same + free",
           "loop": "per instance sc_gkr_phase_one, sc_prover_init, dim x sc_prove_round, sc_prover_bind_final, sc_gkr_phase_two, sc_dense_scale, sc_prover_init, dim x sc_prove_round",
           "statistic": "median of the repetitions, microseconds per proof of the whole batch, with min and max; fixed challenges, no transcript",
           "wins": "the handle's median + both spreads < the loop's median", "rows": rows}
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
