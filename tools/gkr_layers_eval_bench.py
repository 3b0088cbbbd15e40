"""sc_gkr_layers_eval_batch: what evaluating a circuit's layers on the device costs, and what share of proving a layer that is.
    python tools/gkr_layers_eval_bench.py [--out FILE] [--quick]

tools/gkr_next_layer_bench.py's method: device-resident arrays, nnz = 2 x 2^dim distinct indices per list, medians of seven repetitions with
the min-max spread beside them, everything of a cell inside one process.  A cell is (dim, n, n_layers); every layer of an instance uses the
instance's one wiring (pointers may repeat), layer 0 reads the instance's f2 and f3, outputs are allocated once.  Per cell:
  eval_us_per_call      one call of sc_gkr_layers_eval_batch (upload, the index check's round trip, the launches, one synchronisation);
  us_per_layer          that over n_layers;  nnz_per_s = n x n_layers x nnz over it;  atomics_per_s = 8 x nnz_per_s on plan
                        batch.gkr_eval_cells (eight 64-bit atomic adds per non-zero) -- beside the 23-27 G/s of k_batch_gkr_terms;
  cells_us_per_call     dim <= 9 only: the same call under policy "batch" = 0, i.e. per-layer launches instead of ONE launch for all layers;
  next_layer_proof_us   n_layers = 1 only: sc_gkr_layer_next_batch onto a second input set + 2 dim round calls + finish on a handle
                        (tools/gkr_next_layer_bench.py's variant (a)), and eval_share = us_per_layer / (us_per_layer + next_layer_proof_us).
Before a cell is timed, every layer of instance 0 is compared with the definition in big integers (tests/gkr_layers_eval_cases.py).
There is no parent-commit counterpart: the capability is new, no speed-up is claimed."""
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
import torch

import sumcheck_amd as sc
from sumcheck_amd import _lib
from gkr_batch_round_slices_bench import sliced_fits
from gkr_batch_rounds_bench import REPS, Batch, V, handle_proof, summary
from gkr_next_layer_bench import init, next_layer
from tests import gkr_layers_eval_cases as K

DIMS = [6, 8, 9, 10, 12, 14, 16]
NS = [1, 16, 256]
LAYERS = [1, 8]
DEV = _lib.SC_TABLES_ON_DEVICE


class Call:
    """the arguments of one call over a Batch: n_layers layers, every layer of an instance on the instance's wiring"""

    def __init__(self, b, n_layers):
        n, total = b.n, b.n * n_layers
        self.b, self.n_layers = b, n_layers
        self.out = [torch.empty((b.N, 4), dtype=torch.int64, device="cuda:0") for _ in range(total)]
        torch.cuda.synchronize()
        ptrs = lambda vals: (V * len(vals))(*vals)
        self.args = (n, b.dim, n_layers, ptrs([t.data_ptr() for t in b.idx] * n_layers), ptrs([t.data_ptr() for t in b.vals] * n_layers), (C.c_uint64 * total)(*[b.nnz] * total),
                     ptrs([t.data_ptr() for t in b.f2]), ptrs([t.data_ptr() for t in b.f3]), DEV, ptrs([t.data_ptr() for t in self.out]))

    def run(self):
        _lib.check(sc.lib().sc_gkr_layers_eval_batch(*self.args))

    def check_instance_0(self):
        host = lambda t: np.ascontiguousarray(t.cpu().numpy().view(np.uint64))
        b = self.b
        want = K.define_layers([(host(b.idx[0]).reshape(-1), host(b.vals[0]))] * self.n_layers, host(b.f2[0]), host(b.f3[0]), b.dim)
        for k, w in enumerate(want):
            assert np.array_equal(host(self.out[k * b.n]), w), f"dim {b.dim}, n {b.n}: layer {k} of instance 0 differs from the definition"


def timed(fn, count):
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(count):
            fn()
        ts.append((time.perf_counter() - t0) / count * 1e6)
    return ts


def main():
    args = sys.argv[1:]
    quick = "--quick" in args
    rows = []
    for dim in ([6, 10] if quick else DIMS):
        for n in ([1, 16] if quick else NS):
            b = Batch(n, dim, 9700 + dim)
            count = max(2, 32 // n) if dim <= 9 else (2 if (n << dim) <= (1 << 20) else 1)
            row = {"dim": dim, "n": n, "nnz": b.nnz, "inputs": "device", "plan": K.ONE_BLOCK if K.one_block_fits(dim, b.nnz) else K.CELLS, "calls_per_sample": count, "layers": {}}
            per_layer_1 = None
            for n_layers in LAYERS:
                c = Call(b, n_layers)
                before = _lib.plan_stats()
                with _lib.policy(batch=2):
                    c.run()
                    c.check_instance_0()
                    ts = timed(c.run, count)
                after = _lib.plan_stats()
                assert after[row["plan"]] - before[row["plan"]] == 1 + REPS * count, row["plan"]
                med = statistics.median(ts)
                cell = {"eval_us_per_call": summary(ts), "us_per_layer": round(med / n_layers, 2), "nnz_per_s": round(n * n_layers * b.nnz / med * 1e6, 0)}
                if row["plan"] == K.CELLS:
                    cell["atomics_per_s"] = 8 * cell["nnz_per_s"]
                else:
                    with _lib.policy(batch=0):
                        c.run()
                        c.check_instance_0()
                        cell["cells_us_per_call"] = summary(timed(c.run, count))
                if n_layers == 1:
                    per_layer_1 = med
                row["layers"][str(n_layers)] = cell
                del c
            slices = 0 if dim <= 9 else 1
            if slices and not sliced_fits(n, dim):
                row["next_layer_proof_us"] = {"skipped": "beyond the sliced plan's 16 GiB"}
            else:
                b2 = Batch(n, dim, 9750 + dim)
                h = init(b, slices)
                out = np.zeros((2 * dim, n, 3, 4), np.uint64)

                def proof():
                    next_layer(h, b2)
                    handle_proof(b2, h, out, False)
                    next_layer(h, b)  # (back onto the first set; timed with it and halved below: both calls bring in a set the handle is not on)
                    handle_proof(b, h, out, False)

                proof()
                tp = [t / 2 for t in timed(proof, 1 if dim > 9 else count)]
                sc.lib().sc_gkr_batch_prover_free(h)
                row["next_layer_proof_us"] = summary(tp)
                row["eval_share_of_proving_a_layer"] = round(per_layer_1 / (per_layer_1 + statistics.median(tp)), 4)
                del b2
            rows.append(row)
            print(json.dumps(row), flush=True)
            del b
            sc.lib().sc_release_caches()
    out = {"tool": "tools/gkr_layers_eval_bench.py", "library": os.path.basename(_lib.SO_PATH), "reps": REPS,
           "statistic": "median of the repetitions, microseconds per call of the whole batch, with min and max; device arrays, nnz = 2 x 2^dim per list",
           "eval": "sc_gkr_layers_eval_batch over n instances x n_layers layers, one wiring per instance for all its layers",
           "cells_us_per_call": "dim <= 9: the same call under policy batch = 0 (plan batch.gkr_eval_cells: per-layer launches)",
           "next_layer_proof_us": "sc_gkr_layer_next_batch onto another input set + 2 dim calls of sc_gkr_batch_prove_round + finish (dim >= 10: policy batch_slices = 1)",
           "eval_share_of_proving_a_layer": "us_per_layer at n_layers = 1 over (itself + next_layer_proof_us)", "rows": rows}
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
