"""The batched interactive rounds: sc_batch_prove_round on a handle built under policy "batch" = 2 (k_batch_round, one launch per round
for the whole batch) against the serial plan of the SAME library (a handle built under policy "batch" = 0: n ordinary provers inside
the handle, a round is a loop of sc_prove_round) -- what a caller with a transcript of its own pays per round and per proof.
    python tools/batch_rounds_bench.py [--out FILE] [--quick]

Shapes: c2 (one product of three tables) at nv 6 / 8 / 9 and the two-table shape (a GKR phase's) at nv 10, device tables; n = 1, 16, 256.
A proof is reset(NULL) + num_vars round calls with fixed, distinct challenges per instance (no transcript: the caller's hashing is not
the library's time).  The two handles are ALTERNATED within one process, seven repetitions of several proofs each; medians, with the
min-max spread beside them.  Both handles' messages of the last repetition are compared bit for bit, and a sample of instances with
the oracle.  `ahead`: the batched median beats the serial one by more than the two spreads together."""
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
TWO_TABLES = [[0, 1]]
ROWS = [("c2", C2, 6), ("c2", C2, 8), ("c2", C2, 9), ("two_tables", TWO_TABLES, 10)]
NS = [1, 16, 256]
REPS = 7


def summary(ts):
    return {"median": round(statistics.median(ts), 2), "min": round(min(ts), 2), "max": round(max(ts), 2)}


class Batch:
    def __init__(self, n, nv, shapes, seed):
        nt = max(max(s) for s in shapes) + 1
        self.n, self.nv, self.U, self.shapes, self.D = n, nv, nt, shapes, max(len(s) for s in shapes) + 1
        tabs = np.stack([np.stack([cref.synth_table(seed + 7919 * i, s, 1 << nv) for s in range(nt)]) for i in range(min(n, 16))])
        self.tabs = np.ascontiguousarray(tabs[np.arange(n) % tabs.shape[0]])  # (n, nt, 2^nv, 4)
        self.coefs = np.stack([cref.synth_table(seed + 7919 * i, 1000, len(shapes)) for i in range(n)])
        self.chal = np.ascontiguousarray(cref.synth_table(seed, 7000, n * nv).reshape(nv, n, 4))
        self.big = torch.from_numpy(self.tabs.view(np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        offs, idx = [0], []
        for sh in shapes:
            idx.extend(sh)
            offs.append(len(idx))
        self.offs, self.idx = np.asarray(offs, np.uint32), np.asarray(idx, np.uint32)
        self.descs = (_lib.PolyDesc * n)()
        self.keep = []
        for i in range(n):
            ptrs = (C.c_void_p * nt)(*[self.big[i, s].data_ptr() for s in range(nt)])
            d = self.descs[i]
            d.num_vars, d.max_multiplicands, d.n_products, d.n_tables = nv, self.D - 1, len(shapes), nt
            d.coeffs = self.coefs[i].ctypes.data_as(C.POINTER(C.c_uint64))
            d.prod_offsets = self.offs.ctypes.data_as(C.POINTER(C.c_uint32))
            d.prod_indices = self.idx.ctypes.data_as(C.POINTER(C.c_uint32))
            d.tables = C.cast(ptrs, C.POINTER(C.c_void_p))
            d.flags = _lib.SC_TABLES_ON_DEVICE
            self.keep.append(ptrs)

    def handle(self, policy):
        h = C.c_void_p()
        with _lib.policy(batch=policy):
            _lib.check(sc.lib().sc_batch_prover_init(self.descs, self.n, C.byref(h)))
        return h

    def oracle(self, i):
        prods = [(self.coefs[i][k], list(sh)) for k, sh in enumerate(self.shapes)]
        p = cref.Prover(cref.PolyDesc(self.nv, prods, [self.tabs[i, s] for s in range(self.U)]), threads=1)
        return np.stack([p.prove_round(None if j == 0 else self.chal[j - 1, i]) for j in range(self.nv)])


def proofs(b, h, count, out):
    """count x (reset + nv round calls) -> (us per round call, us per proof); out (nv, n, D, 4) holds the last proof's messages"""
    L = sc.lib()
    t_round = 0.0
    t0 = time.perf_counter()
    for _ in range(count):
        _lib.check(L.sc_batch_prover_reset(h, None))
        for j in range(b.nv):
            r = C.c_void_p(b.chal[j - 1].ctypes.data) if j else None
            o = C.c_void_p(out[j].ctypes.data)
            t1 = time.perf_counter()
            _lib.check(L.sc_batch_prove_round(h, r, 0, o))  # (returns after its synchronise: the messages are on the host)
            t_round += time.perf_counter() - t1
    total = time.perf_counter() - t0
    return t_round / (count * b.nv) * 1e6, total / count * 1e6


def main():
    args = sys.argv[1:]
    quick = "--quick" in args
    ns = [1, 256] if quick else NS
    rows = []
    for name, shapes, nv in (ROWS[:1] + ROWS[3:] if quick else ROWS):
        row = {"shape": name, "nv": nv, "tables": "device", "n": {}}
        for n in ns:
            b = Batch(n, nv, shapes, 9500 + nv)
            hb, hs = b.handle(2), b.handle(0)
            before = _lib.plan_stats()
            count = max(2, 64 // n)
            got, ref = np.zeros((nv, n, b.D, 4), np.uint64), np.zeros((nv, n, b.D, 4), np.uint64)
            proofs(b, hb, 2, got)  # (code objects, first-launch attributes)
            proofs(b, hs, 1, ref)
            rb, pb, rs, ps = [], [], [], []
            for _ in range(REPS):  # alternated
                got[:] = 0
                x, y = proofs(b, hb, count, got)
                rb.append(x)
                pb.append(y)
                x, y = proofs(b, hs, count, ref)
                rs.append(x)
                ps.append(y)
            after = _lib.plan_stats()
            assert after["batch.rounds_one_block"] > before["batch.rounds_one_block"] and after["batch.rounds_serial"] > before["batch.rounds_serial"]
            assert np.array_equal(got, ref), f"{name} nv {nv}, n {n}: the batched rounds and the serial plan differ"
            for i in range(min(n, 4)):
                assert np.array_equal(got[:, i], b.oracle(i)), f"{name} nv {nv}, n {n}, instance {i}: differs from the oracle"
            mb, ms = statistics.median(pb), statistics.median(ps)
            row["n"][str(n)] = {"batched_us_per_round_call": summary(rb), "serial_us_per_round_call": summary(rs),
                                "batched_us_per_proof": summary(pb), "serial_us_per_proof": summary(ps),
                                "batched_us_per_instance_round": round(statistics.median(rb) / n, 3), "serial_us_per_instance_round": round(statistics.median(rs) / n, 3),
                                "speedup_per_proof": round(ms / mb, 2), "ahead": bool(ms - mb > (max(pb) - min(pb)) + (max(ps) - min(ps)))}
            sc.lib().sc_batch_prover_free(hb)
            sc.lib().sc_batch_prover_free(hs)
            del b
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"tool": "tools/batch_rounds_bench.py", "library": os.path.basename(_lib.SO_PATH), "reps": REPS,
           "proof": "sc_batch_prover_reset(NULL) + num_vars calls of sc_batch_prove_round, fixed challenges, no transcript",
           "baseline": "the serial plan of the same library: a handle built under policy batch = 0 (n provers inside the handle, a loop of sc_prove_round)",
           "statistic": "median of the repetitions, microseconds, with min and max", "ahead": "batched median + both spreads < serial median (per proof)", "rows": rows}
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
