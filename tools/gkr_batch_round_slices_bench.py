"""The sliced plan of the batched interactive GKR rounds: a sc_gkr_batch_prover handle built under policy "batch_slices" = 1 (plan
batch.gkr_rounds_slices: k_batch_gkr_terms + k_batch_gkr_fold for the two initialisations, k_batch_round_slices + k_batch_round_fin for the
rounds beyond one block's LDS, k_batch_round behind them) against a handle built under "batch_slices" = 0 over the SAME device arrays --
the serial plan of the same library (n pairs of ordinary provers inside the handle, a round is a loop of sc_prove_round).
tools/batch_round_slices_bench.py's and tools/gkr_batch_rounds_bench.py's method.
    python tools/gkr_batch_round_slices_bench.py [--out FILE] [--quick] [--kernels [--ab-lib FILE]]

Inputs are device-resident, nnz = 2 x 2^dim distinct indices; dim 10 / 12 / 14 / 16, n = 1 / 16 / 256 (a cell the 16 GiB rule sends to the
serial plan is left out); fixed, distinct challenges per instance (no transcript).  The two handles are ALTERNATED within one process, seven
repetitions of one or several proofs each; medians, with the min-max spread beside them.  Two figures per handle: `rewound` is reset +
2 dim round calls + finish, `with_init` is init + the same + free.  Both handles' messages of the last repetition are compared bit for bit,
and instance 0's with the oracle (the walk composed from oracle/cref.py).  `ahead`: the sliced median beats the serial one by more than
the two spreads together.

--kernels: per cell a child process under `rocprofv3 --kernel-trace --stats` runs three proofs with init on the sliced plan alone
(--kernel-leg DIM N); the averages of k_batch_gkr_terms<1|2> and k_batch_gkr_fold<1|2> and the atomics per second they imply (eight per
non-zero) are recorded.  --ab-lib FILE: the same legs on a second build of the library (the cells cell-major:
-DSC_GKR_CELLS_CELL_MAJOR), for the layout A/B."""
import csv
import ctypes as C
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib
from gkr_batch_rounds_bench import ONE, REPS, Batch, V, handle_proof, summary, timed

DIMS = [10, 12, 14, 16]
NS = [1, 16, 256]
KERNEL_CELLS = [(10, 256), (12, 16), (12, 256), (14, 256), (16, 16), (16, 256)]
NAME = "batch.gkr_rounds_slices"
MAX_BYTES = 16 << 30


def sliced_fits(n, dim):
    """batch_slices.hpp: gkr_bs_handle_bytes against kBsMaxWorkBytes"""
    return n * ((2 * 2 * 2 * 2 * 48 + 64) << dim) <= MAX_BYTES


def init(b, slices):
    h = V()
    with _lib.policy(batch_slices=slices):
        _lib.check(sc.lib().sc_gkr_batch_prover_init(b.n, b.dim, *b.args, _lib.SC_TABLES_ON_DEVICE, C.byref(h)))
    return h


def oracle(b, i):
    """instance i's 2 dim messages: tests/test_gpu_gkr_batch_rounds.py's Walk"""
    dim, N = b.dim, b.N
    host = lambda t: np.ascontiguousarray(t.cpu().numpy().view(np.uint64))
    idx, vals, f2, f3 = host(b.idx[i]).reshape(-1), host(b.vals[i]), host(b.f2[i]), host(b.f3[i])
    chal = np.ascontiguousarray(b.chal[:, i])
    desc = lambda x, y: cref.PolyDesc(dim, [(ONE, [0, 1])], [x, y])
    h_g, gi, gv = cref.gkr_phase_one(idx, vals, dim, f3, b.g[i])
    msgs = []
    p = cref.Prover(desc(h_g, f2))
    for t in range(dim):
        msgs.append(p.prove_round(None if t == 0 else chal[t - 1]))
    p.close()
    u = np.ascontiguousarray(chal[:dim])
    f2u = cref.fix_variables(f2, u)[0]
    t1 = np.stack([cref.fr_binop("mul", f3[e], f2u) for e in range(N)])
    p = cref.Prover(desc(cref.gkr_phase_two(gi, gv, dim, u), t1))
    for r in range(dim):
        msgs.append(p.prove_round(None if r == 0 else chal[dim + r - 1]))
    p.close()
    return np.stack(msgs)


def kernel_leg(dim, n):
    """three proofs with init on the sliced plan, nothing else: the body of a rocprofv3 child"""
    b = Batch(n, dim, 9800 + dim)
    got = np.zeros((2 * dim, n, 3, 4), np.uint64)
    before = _lib.plan_stats()[NAME]
    for _ in range(3):
        h = init(b, 1)
        handle_proof(b, h, got, False)
        sc.lib().sc_gkr_batch_prover_free(h)
    assert _lib.plan_stats()[NAME] == before + 6 * dim
    print("kernel leg ok", dim, n, flush=True)


def kernel_times(dim, n, lib_path=None):
    """-> {kernel: average microseconds} of the four initialisation kernels, from a rocprofv3 child"""
    out = tempfile.mkdtemp(prefix="gkr_slices_prof_")
    env = dict(os.environ)
    if lib_path:
        env["SC_LIB_PATH"] = lib_path
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "leg", "--", sys.executable, os.path.abspath(__file__), "--kernel-leg", str(dim), str(n)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "kernel leg ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        stats = [os.path.join(d, f) for d, _, fs in os.walk(out) for f in fs if f.endswith("kernel_stats.csv")]
        assert stats, "no kernel_stats.csv under " + out
        res = {}
        for row in csv.DictReader(open(stats[0])):
            for k in ("k_batch_gkr_terms<1>", "k_batch_gkr_terms<2>", "k_batch_gkr_fold<1>", "k_batch_gkr_fold<2>"):
                if k in row["Name"]:
                    res[k] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2)}
        assert len(res) == 4 and all(v["calls"] == 3 for v in res.values()), res
        return res
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    args = sys.argv[1:]
    if "--kernel-leg" in args:
        k = args.index("--kernel-leg")
        return kernel_leg(int(args[k + 1]), int(args[k + 2]))
    quick = "--quick" in args
    rows, kernels = [], []
    for dim in (DIMS[:2] if quick else DIMS):
        row = {"dim": dim, "nnz": 2 << dim, "inputs": "device", "n": {}}
        for n in ([1, 16] if quick else NS):
            if not sliced_fits(n, dim):
                row["n"][str(n)] = "left out: beyond 16 GiB, the serial plan"
                continue
            b = Batch(n, dim, 9800 + dim)
            count = max(1, (8 if dim <= 12 else 4) // n)
            got, ref = np.zeros((2 * dim, n, 3, 4), np.uint64), np.zeros((2 * dim, n, 3, 4), np.uint64)
            hb, hs = init(b, 1), init(b, 0)
            before = _lib.plan_stats()
            handle_proof(b, hb, got, True)  # (code objects, first-launch attributes)
            handle_proof(b, hs, ref, True)
            mid = _lib.plan_stats()
            assert mid[NAME] == before[NAME] + 2 * dim and mid["batch.gkr_rounds_serial"] == before["batch.gkr_rounds_serial"] + 2 * dim, "one handle sliced, the other serial"

            def with_init(slices, out):
                h = init(b, slices)
                handle_proof(b, h, out, False)
                sc.lib().sc_gkr_batch_prover_free(h)
            with_init(1, got)
            rb, wb, rs, ws = [], [], [], []
            for _ in range(REPS):  # alternated
                got[:] = 0
                ref[:] = 0
                rb.append(timed(lambda: handle_proof(b, hb, got, True), count))
                rs.append(timed(lambda: handle_proof(b, hs, ref, True), count))
                wb.append(timed(lambda: with_init(1, got), count))
                ws.append(timed(lambda: with_init(0, ref), count))
            assert np.array_equal(got, ref), f"dim {dim}, n {n}: the sliced plan and the serial plan differ"
            assert np.array_equal(got[:, 0], oracle(b, 0)), f"dim {dim}, n {n}, instance 0: differs from the oracle"
            sc.lib().sc_gkr_batch_prover_free(hb)
            sc.lib().sc_gkr_batch_prover_free(hs)
            spread = lambda ts: max(ts) - min(ts)
            m = statistics.median
            row["n"][str(n)] = {"sliced_rewound_us_per_proof": summary(rb), "serial_rewound_us_per_proof": summary(rs),
                                "sliced_with_init_us_per_proof": summary(wb), "serial_with_init_us_per_proof": summary(ws),
                                "sliced_rewound_us_per_instance_round": round(m(rb) / (2 * dim * n), 3), "serial_rewound_us_per_instance_round": round(m(rs) / (2 * dim * n), 3),
                                "speedup_rewound": round(m(rs) / m(rb), 2), "speedup_with_init": round(m(ws) / m(wb), 2),
                                "ahead_rewound": bool(m(rs) - m(rb) > spread(rb) + spread(rs)), "ahead_with_init": bool(m(ws) - m(wb) > spread(wb) + spread(ws))}
            del b
        rows.append(row)
        print(json.dumps(row), flush=True)
    if "--kernels" in args:
        ab = args[args.index("--ab-lib") + 1] if "--ab-lib" in args else None
        for dim, n in (KERNEL_CELLS[:1] if quick else KERNEL_CELLS):
            nnz = 2 << dim
            rec = {"dim": dim, "n": n, "nnz": nnz, "atomics_per_phase": 8 * nnz * n, "lane_major": kernel_times(dim, n)}
            for ph in (1, 2):
                rec["lane_major"][f"atomics_per_second_phase{ph}"] = round(8 * nnz * n / (rec["lane_major"][f"k_batch_gkr_terms<{ph}>"]["avg_us"] * 1e-6) / 1e9, 2)
            if ab:
                rec["cell_major"] = kernel_times(dim, n, ab)
            kernels.append(rec)
            print(json.dumps(rec), flush=True)
    out = {"tool": "tools/gkr_batch_round_slices_bench.py", "library": os.path.basename(_lib.SO_PATH), "reps": REPS,
           "proof": "rewound: sc_gkr_batch_prover_reset + 2 dim calls of sc_gkr_batch_prove_round + finish; with_init: init + the same + free; fixed challenges, no transcript",
           "sliced": "a handle built under policy batch_slices = 1: plan batch.gkr_rounds_slices",
           "baseline": "a handle built under policy batch_slices = 0 over the same device arrays: plan batch.gkr_rounds_serial",
           "statistic": "median of the repetitions, microseconds per proof of the whole batch, with min and max", "ahead": "sliced median + both spreads < serial median",
           "kernels": {"method": "rocprofv3 --kernel-trace --stats over three proofs with init per cell, averages in microseconds; atomics_per_second in G/s, eight 64-bit atomics per non-zero",
                       "reference": "profiles/r2d_gkr_init.txt: 8.4 M global 64-bit atomics in 0.4 ms, 21 G/s", "cells": kernels}, "rows": rows}
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
