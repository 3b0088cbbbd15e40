"""sc_gkr_layer_next_batch: what putting a GKR batch handle onto the next layer's inputs costs, against what a caller had before.
    python tools/gkr_next_layer_bench.py [--out FILE] [--quick]

tools/gkr_batch_rounds_bench.py's method: device-resident inputs, nnz = 2 x 2^dim distinct indices, fixed distinct challenges per instance (no
transcript), medians of seven repetitions with the min-max spread beside them, the variants ALTERNATED inside one process.  Handles are
built under policy "batch" = 2; dim 10 / 12 / 14 / 16 additionally under "batch_slices" = 1 (plan batch.gkr_rounds_slices).  Two input sets
per cell, both on the device; one proof of the whole batch over the SECOND set is
  (a) next_layer   sc_gkr_layer_next_batch onto the second set (new wiring, new tables, new g), 2 dim round calls, finish -- on a handle
                   that was on the first set (it is put back onto the first set outside the timed region);
  (b) rebuild      what a caller does today on the same library: sc_gkr_batch_prover_free, sc_gkr_batch_prover_init over the second set, the
                   same rounds and finish;
  (c) reset        sc_gkr_batch_prover_reset on a handle that already is on the second set, the same rounds and finish: the floor.
`next_layer_call_us` is the call of (a) alone.  `ahead`: (a)'s median beats (b)'s by more than the two min-max spreads together.  Every
variant's messages of the last repetition are compared with each other bit for bit, and instance 0's with the oracle (the walk composed from
oracle/cref.py)."""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

import sumcheck_amd as sc
from sumcheck_amd import _lib
from gkr_batch_round_slices_bench import oracle, sliced_fits
from gkr_batch_rounds_bench import REPS, Batch, V, handle_proof, summary

CELLS = [(dim, 0) for dim in (6, 8, 9)] + [(dim, 1) for dim in (10, 12, 14, 16)]  # (dim, policy "batch_slices")
NS = [1, 16, 256]
DEV = _lib.SC_TABLES_ON_DEVICE


def init(b, slices):
    h = V()
    with _lib.policy(batch=2, batch_slices=slices):
        _lib.check(sc.lib().sc_gkr_batch_prover_init(b.n, b.dim, *b.args, DEV, C.byref(h)))
    return h


def next_layer(h, b):
    _lib.check(sc.lib().sc_gkr_layer_next_batch(h, *b.args, DEV))


def main():
    args = sys.argv[1:]
    quick = "--quick" in args
    L = sc.lib()
    rows = []
    for dim, slices in (CELLS[:1] + CELLS[3:4] if quick else CELLS):
        row = {"dim": dim, "nnz": 2 << dim, "inputs": "device", "batch_slices": slices, "n": {}}
        for n in ([1, 16] if quick else NS):
            if slices and not sliced_fits(n, dim):
                row["n"][str(n)] = {"skipped": "beyond the sliced plan's 16 GiB"}
                continue
            b1, b2 = Batch(n, dim, 9900 + dim), Batch(n, dim, 9950 + dim)
            count = max(2, 32 // n) if dim <= 9 else (2 if (n << dim) <= (1 << 20) else 1)
            outs = {k: np.zeros((2 * dim, n, 3, 4), np.uint64) for k in "abc"}
            ha, hc = init(b1, slices), init(b2, slices)
            state = {"hb": init(b1, slices), "call": 0.0}
            plan = "batch.gkr_rounds_slices" if slices else "batch.gkr_rounds_one_block"
            before = _lib.plan_stats()

            def var_a():
                t0 = time.perf_counter()
                next_layer(ha, b2)
                state["call"] += time.perf_counter() - t0
                handle_proof(b2, ha, outs["a"], False)

            def var_b():
                L.sc_gkr_batch_prover_free(state["hb"])
                state["hb"] = init(b2, slices)
                handle_proof(b2, state["hb"], outs["b"], False)

            def var_c():
                handle_proof(b2, hc, outs["c"], True)

            def sample(fn, undo=None):
                total = 0.0
                for _ in range(count):
                    t0 = time.perf_counter()
                    fn()
                    total += time.perf_counter() - t0
                    if undo:
                        undo()
                return total / count * 1e6

            for fn in (var_a, var_b, var_c):  # (code objects, first-launch attributes)
                fn()
            next_layer(ha, b1)
            ta, tb, tc, tcall = [], [], [], []
            for _ in range(REPS):  # alternated
                for o in outs.values():
                    o[:] = 0
                state["call"] = 0.0
                ta.append(sample(var_a, undo=lambda: next_layer(ha, b1)))  # (back onto the first set, untimed: every timed call brings in a set the handle is not on)
                tcall.append(state["call"] / count * 1e6)
                tb.append(sample(var_b))
                tc.append(sample(var_c))
            after = _lib.plan_stats()
            assert after["batch.gkr_next_layer"] - before["batch.gkr_next_layer"] == 2 * count * REPS + 2, "every call of (a) and every call back is counted once"
            assert after[plan] > before[plan] and after["batch.gkr_rounds_serial"] == before["batch.gkr_rounds_serial"], plan
            assert np.array_equal(outs["a"], outs["b"]) and np.array_equal(outs["a"], outs["c"]), f"dim {dim}, n {n}: the three variants differ"
            assert np.array_equal(outs["a"][:, 0], oracle(b2, 0)), f"dim {dim}, n {n}, instance 0: differs from the oracle"
            for h in (ha, hc, state["hb"]):
                L.sc_gkr_batch_prover_free(h)
            spread = lambda ts: max(ts) - min(ts)
            ma, mb, mc = statistics.median(ta), statistics.median(tb), statistics.median(tc)
            row["n"][str(n)] = {"next_layer_us_per_proof": summary(ta), "rebuild_us_per_proof": summary(tb), "reset_us_per_proof": summary(tc), "next_layer_call_us": summary(tcall),
                                "round_call_us": round(mc / (2 * dim + 1), 2), "next_layer_over_reset_us": round(ma - mc, 2), "speedup_over_rebuild": round(mb / ma, 2),
                                "ahead": bool(mb - ma > spread(ta) + spread(tb)), "proofs_per_sample": count}
            del b1, b2
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"tool": "tools/gkr_next_layer_bench.py", "library": os.path.basename(_lib.SO_PATH), "reps": REPS,
           "next_layer": "sc_gkr_layer_next_batch onto the second input set (new f1, f2, f3, g) + 2 dim calls of sc_gkr_batch_prove_round + finish",
           "rebuild": "sc_gkr_batch_prover_free + sc_gkr_batch_prover_init over the second set + the same rounds + finish",
           "reset": "sc_gkr_batch_prover_reset on a handle over the second set + the same rounds + finish",
           "statistic": "median of the repetitions, microseconds per proof of the whole batch, with min and max; fixed challenges, no transcript",
           "round_call_us": "reset's median over its 2 dim + 1 calls", "ahead": "next_layer's median + both spreads < rebuild's median", "rows": rows}
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
