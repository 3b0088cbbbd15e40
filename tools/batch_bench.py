"""Many small proofs: sc_ml_prove_batch against the serial loop on a kept borrowing handle (reset(tables); prove() -- the fastest path
without the batch call).   python tools/batch_bench.py [--serial-only] [--out FILE] [--shapes c2,gkr,c3] [--quick]

Shapes c2 / gkr / c3, num_vars 6, 8 and the largest the batched kernel takes for the shape, n = 1, 4, 16, 64, 256, 1024 instances with
device-resident tables of their own (one set of coefficients: the serial loop's handle has one).  Minimum of five repetitions of at least
400 proofs each; every proof of the last repetition is compared with the oracle.  Per row: us per proof batched (policy "batch" = 2, so
the small n show the kernel and not the call's own choice; `auto` is the call as shipped), us per proof of the serial loop, the host's
hash time per instance and round (feed_prover_msg + sample_fr over the recorded messages, timed alone through the C ABI: two calls'
overhead included), and -- from a child process run with SC_HOST_TRACE=1 -- the kernel's span from HIP events and the hash time the
library measured inside its loop.  --serial-only uses no new symbol: the same file runs against a build of an older commit
(SC_LIB_PATH=... SC_AB_ALLOW_MISSING=1)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib
from tests import helpers as H

SHAPES = {"c2": ([[0, 1, 2]], 3, 9), "gkr": ([[0, 1]], 2, 10), "c3": ([[0, 1, 2, 3], [4, 5, 6], [7, 8], [9]], 10, 8)}  # shape, tables, largest batched nv
NS = [1, 4, 16, 64, 256, 1024]
REPS, MIN_PROOFS = 5, 400


def make(n, nv, shapes, nt, seed):
    tabs = np.stack([np.stack([cref.synth_table(seed + 7919 * i, s, 1 << nv) for s in range(nt)]) for i in range(n)])
    coefs = cref.synth_table(seed, 1000, len(shapes))
    big = torch.from_numpy(tabs.view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    polys = []
    for i in range(n):
        mles = [sc.DenseMultilinearExtension(nv, big[i, s]) for s in range(nt)]
        poly = sc.ListOfProductsOfPolynomials(nv)
        for k, sh in enumerate(shapes):
            poly.add_product([mles[t] for t in sh], coefs[k])
        polys.append(poly)
    want = [cref.ml_prove(H.desc_from(nv, shapes, list(tabs[i]), coefs), threads=1)[0] for i in range(n)]
    return polys, want, big


def serial_loop(polys, want):
    """reset(tables of instance i); prove() on one borrowing handle"""
    n, nv = len(polys), polys[0].num_variables
    st = sc.IPForMLSumcheck.prover_init(polys[0], borrow=True)
    ptrs = [(C.c_void_p * len(p.flattened_ml_extensions))(*[t.data_ptr() for t in p.flattened_ml_extensions]) for p in polys]
    L = sc.lib()
    proof = np.empty((nv, polys[0].max_multiplicands + 1, 4), dtype=np.uint64)
    pp = C.c_void_p(proof.ctypes.data)
    best = 1e9
    for rep in range(REPS):
        t0 = time.perf_counter()
        for i in range(MIN_PROOFS):
            _lib.check(L.sc_prover_reset(st._h, ptrs[i % n], _lib.SC_TABLES_ON_DEVICE))
            _lib.check(L.sc_ml_prove_handle(st._h, None, pp))
        best = min(best, (time.perf_counter() - t0) / MIN_PROOFS)
    for i in range(n):  # every instance once more, compared
        _lib.check(L.sc_prover_reset(st._h, ptrs[i], _lib.SC_TABLES_ON_DEVICE))
        _lib.check(L.sc_ml_prove_handle(st._h, None, pp))
        assert np.array_equal(proof, want[i]), f"serial loop, instance {i}"
    st.close()
    return best * 1e6


def batched(polys, want, policy):
    """the C ABI as a Rust or C caller uses it: the descriptor array is built once, the call is timed"""
    n, nv, D = len(polys), polys[0].num_variables, polys[0].max_multiplicands + 1
    descs, keep = (_lib.PolyDesc * n)(), []
    for i, poly in enumerate(polys):
        d, k = poly._desc(False)
        C.memmove(C.byref(descs, i * C.sizeof(_lib.PolyDesc)), C.byref(d), C.sizeof(_lib.PolyDesc))
        keep.append(k)
    proofs = np.empty((n, nv, D, 4), dtype=np.uint64)
    pp = C.c_void_p(proofs.ctypes.data)
    L = sc.lib()
    calls = max(1, -(-MIN_PROOFS // n))
    best = 1e9
    with _lib.policy(batch=policy):
        _lib.check(L.sc_ml_prove_batch(descs, n, None, pp, None))  # (work areas, code object)
        for rep in range(REPS):
            proofs[:] = 0
            t0 = time.perf_counter()
            for _ in range(calls):
                _lib.check(L.sc_ml_prove_batch(descs, n, None, pp, None))
            best = min(best, (time.perf_counter() - t0) / (calls * n))
    for i in range(n):
        assert np.array_equal(proofs[i], want[i]), f"batched, instance {i}"
    return best * 1e6


def hash_alone(want):
    """feed_prover_msg + sample_fr per recorded message, one transcript per instance, one thread"""
    L = sc.lib()
    n, nv, D = len(want), want[0].shape[0], want[0].shape[1]
    out = np.empty(4, dtype=np.uint64)
    po = C.c_void_p(out.ctypes.data)
    msgs = [[C.c_void_p(w[j].ctypes.data) for j in range(nv)] for w in want]
    best = 1e9
    for rep in range(REPS):
        rngs = [C.c_void_p(L.sc_rng_setup()) for _ in range(n)]
        t0 = time.perf_counter()
        for j in range(nv):
            for i in range(n):
                L.sc_rng_feed_prover_msg(rngs[i], msgs[i][j], D)
                L.sc_rng_sample_fr(rngs[i], po)
        best = min(best, (time.perf_counter() - t0) / (n * nv))
        for r in rngs:
            L.sc_rng_free(r)
    return best * 1e6


def trace_child(shape_names):
    """(run with SC_HOST_TRACE=1) three batches of 256 per shape and size; the library's trace lines go to stderr"""
    for name in shape_names:
        shapes, nt, nv_max = SHAPES[name]
        for nv in sorted({6, 8, nv_max}):
            polys, _, keep = make(256, nv, shapes, nt, 9000 + nv)
            with _lib.policy(batch=2):
                for _ in range(3):
                    sys.stderr.write(f"[row] {name} {nv}\n")
                    sys.stderr.flush()
                    sc.MLSumcheck.prove_batch(polys)
            del keep


def main():
    args = sys.argv[1:]
    serial_only = "--serial-only" in args
    names = args[args.index("--shapes") + 1].split(",") if "--shapes" in args else list(SHAPES)
    if "--trace-child" in args:
        return trace_child(names)
    ns = [1, 256] if "--quick" in args else NS
    rows = []
    for name in names:
        shapes, nt, nv_max = SHAPES[name]
        for nv in sorted({6, 8, nv_max}):
            polys, want, keep = make(max(ns), nv, shapes, nt, 9000 + nv)
            row = {"shape": name, "nv": nv, "serial_us_per_proof": round(serial_loop(polys[:256], want[:256]), 2)}
            if not serial_only:
                row["host_hash_us_per_instance_round_alone"] = round(hash_alone(want[:256]), 3)
                row["batched_us_per_proof"] = {str(n): round(batched(polys[:n], want[:n], 2), 2) for n in ns}
                row["auto_us_per_proof"] = {str(n): round(batched(polys[:n], want[:n], 1), 2) for n in ns}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del keep
    if not serial_only and "--no-trace" not in args:
        env = dict(os.environ, SC_HOST_TRACE="1")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-child", "--shapes", ",".join(names)], capture_output=True, text=True, timeout=600, env=env)
        cur = None
        for line in r.stderr.splitlines():
            m = re.match(r"\[row\] (\w+) (\d+)", line)
            if m:
                cur = next(x for x in rows if x["shape"] == m.group(1) and x["nv"] == int(m.group(2)))
            m = re.search(r"batch: n 256, nv (\d+), plan batch.one_block, grid (\d+) \((\d+) per CU\), mailbox (\w+), total ([\d.]+) us, kernel ([\d.]+) us, host hash ([\d.]+) us", line)
            if m and cur is not None:  # (the last of the three repetitions stays)
                cur["trace_n256"] = {"grid": int(m.group(2)), "blocks_per_cu": int(m.group(3)), "mailbox": m.group(4), "call_us": float(m.group(5)),
                                     "kernel_span_us": float(m.group(6)), "host_hash_us_in_loop": float(m.group(7)),
                                     "host_hash_us_per_instance_round_in_loop": round(float(m.group(7)) / (256 * int(m.group(1))), 3)}
    out = {"tool": "tools/batch_bench.py" + (" --serial-only" if serial_only else ""), "library": os.path.basename(_lib.SO_PATH), "reps": REPS,
           "min_proofs_per_rep": MIN_PROOFS, "rows": rows}
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
