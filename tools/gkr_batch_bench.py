"""Many small GKR round proofs: sc_gkr_prove_batch against a loop of sc_gkr_prove calls over the same instances (what a caller writes
without the batch call).   python tools/gkr_batch_bench.py [--out FILE] [--quick] [--no-trace]

dim 6, 8, 9; n = 1, 4, 16, 64, 256, 1024 instances with device-resident inputs of their own, nnz = 2 x 2^dim.  The batched call (policy
"batch" = 2, so the small n show the kernel and not the call's own choice; `auto` is the call as shipped) and the loop are ALTERNATED within
one process, five repetitions of at least 128 proofs each, medians.  The proofs of the last repetition of both are compared with each
other bit for bit, and with the oracle.  From a child process run with SC_HOST_TRACE=1: the kernel's span (HIP events) and the host's
hashing time inside one batch of 256."""
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib

DIMS = [6, 8, 9]
NS = [1, 4, 16, 64, 256, 1024]
REPS, MIN_PROOFS = 5, 128


class Batch:
    def __init__(self, n, dim, seed):
        N = 1 << dim
        rng = np.random.default_rng(seed)
        self.n, self.dim = n, dim
        self.idx = rng.integers(0, 1 << (3 * dim), size=(n, 2 * N), dtype=np.uint64)
        self.vals = np.stack([cref.synth_table(seed + i, 1, 2 * N) for i in range(n)])
        self.f2 = np.stack([cref.synth_table(seed + i, 2, N) for i in range(n)])
        self.f3 = np.stack([cref.synth_table(seed + i, 3, N) for i in range(n)])
        self.g = np.stack([cref.synth_table(seed + i, 4, dim) for i in range(n)])
        td = lambda a: torch.from_numpy(a.view(np.int64)).to("cuda:0")
        self.dev = [td(self.idx), td(self.vals), td(self.f2), td(self.f3)]
        torch.cuda.synchronize()
        row = lambda t, i: t[i].data_ptr()
        arr = lambda vals: (C.c_void_p * n)(*vals)
        self.p_idx, self.p_vals, self.p_f2, self.p_f3 = (arr([row(t, i) for i in range(n)]) for t in self.dev)
        self.p_g = arr([self.g[i].ctypes.data for i in range(n)])
        self.nnz = (C.c_uint64 * n)(*([2 * N] * n))

    def oracle(self, i):
        return cref.gkr_prove(self.idx[i], self.vals[i], self.dim, self.f2[i], self.f3[i], self.g[i], threads=1)[0]


def _rngs(L, n):
    hs = [L.sc_rng_setup() for _ in range(n)]
    return hs, (C.c_void_p * n)(*hs)


def time_batched(b, n, policy, out):
    L = sc.lib()
    calls = max(1, -(-MIN_PROOFS // n))
    sets = [_rngs(L, n) for _ in range(calls)]
    with _lib.policy(batch=policy):
        t0 = time.perf_counter()
        for hs, arr in sets:
            _lib.check(L.sc_gkr_prove_batch(n, b.dim, arr, b.p_idx, b.p_vals, b.nnz, b.p_f2, b.p_f3, b.p_g, _lib.SC_TABLES_ON_DEVICE, C.c_void_p(out.ctypes.data), None))
        dt = (time.perf_counter() - t0) / (calls * n)
    for hs, _ in sets:
        for h in hs:
            L.sc_rng_free(h)
    return dt * 1e6


def time_loop(b, n, out):
    """the parent commit's way: one sc_gkr_prove per instance"""
    L = sc.lib()
    calls = max(1, -(-MIN_PROOFS // n))
    sets = [_rngs(L, n) for _ in range(calls)]
    t0 = time.perf_counter()
    for hs, _ in sets:
        for i in range(n):
            _lib.check(L.sc_gkr_prove(hs[i], b.p_idx[i], b.p_vals[i], b.nnz[i], b.dim, b.p_f2[i], b.p_f3[i], b.p_g[i], _lib.SC_TABLES_ON_DEVICE,
                                      C.c_void_p(out[i].ctypes.data), None))
    dt = (time.perf_counter() - t0) / (calls * n)
    for hs, _ in sets:
        for h in hs:
            L.sc_rng_free(h)
    return dt * 1e6


def trace_child():
    for dim in DIMS:
        b = Batch(256, dim, 9100 + dim)
        out = np.empty((256, 2, dim, 3, 4), dtype=np.uint64)
        for _ in range(3):
            sys.stderr.write(f"[row] {dim}\n")
            sys.stderr.flush()
            time_batched(b, 256, 2, out)


def main():
    args = sys.argv[1:]
    if "--trace-child" in args:
        return trace_child()
    ns = [1, 256] if "--quick" in args else NS
    rows = []
    for dim in DIMS:
        b = Batch(max(ns), dim, 9100 + dim)
        row = {"dim": dim, "nnz": 2 << dim, "batched_us_per_proof": {}, "auto_us_per_proof": {}, "loop_us_per_proof": {}, "speedup": {}}
        for n in ns:
            got = np.zeros((n, 2, dim, 3, 4), dtype=np.uint64)
            ref = np.zeros((n, 2, dim, 3, 4), dtype=np.uint64)
            time_batched(b, n, 2, got)  # (work areas, code objects, the kept prover)
            time_loop(b, min(n, 8), ref)
            tb, ta, tl = [], [], []
            for rep in range(REPS):  # alternated
                got[:] = 0
                tb.append(time_batched(b, n, 2, got))
                tl.append(time_loop(b, n, ref))
                ta.append(time_batched(b, n, 1, got))
            assert np.array_equal(got, ref), f"dim {dim}, n {n}: the batched call and the loop differ"
            for i in range(min(n, 64)):
                assert np.array_equal(got[i], b.oracle(i)), f"dim {dim}, n {n}, instance {i}: differs from the oracle"
            mb, ma, ml = statistics.median(tb), statistics.median(ta), statistics.median(tl)
            row["batched_us_per_proof"][str(n)] = round(mb, 2)
            row["auto_us_per_proof"][str(n)] = round(ma, 2)
            row["loop_us_per_proof"][str(n)] = round(ml, 2)
            row["speedup"][str(n)] = round(ml / mb, 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del b
    if "--no-trace" not in args:
        env = dict(os.environ, SC_HOST_TRACE="1")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-child"], capture_output=True, text=True, timeout=600, env=env)
        cur = None
        for line in r.stderr.splitlines():
            m = re.match(r"\[row\] (\d+)", line)
            if m:
                cur = next(x for x in rows if x["dim"] == int(m.group(1)))
            m = re.search(r"batch: n 256, dim (\d+), plan batch.gkr_one_block, grid (\d+) \((\d+) per CU\), mailbox (\w+), total ([\d.]+) us, kernel ([\d.]+) us, host hash ([\d.]+) us", line)
            if m and cur is not None:  # (the last of the three repetitions stays)
                cur["trace_n256"] = {"grid": int(m.group(2)), "blocks_per_cu": int(m.group(3)), "mailbox": m.group(4), "call_us": float(m.group(5)),
                                     "kernel_span_us": float(m.group(6)), "host_hash_us_in_loop": float(m.group(7)),
                                     "host_hash_us_per_instance_round_in_loop": round(float(m.group(7)) / (256 * 2 * int(m.group(1))), 3)}
    out = {"tool": "tools/gkr_batch_bench.py", "library": os.path.basename(_lib.SO_PATH), "reps": REPS, "min_proofs_per_rep": MIN_PROOFS,
           "baseline": "a loop of sc_gkr_prove calls over the same instances", "statistic": "median", "rows": rows}
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
