"""The two-point form of the GKR batch handle (sc_gkr_two_point_init_batch / sc_gkr_two_point_next_batch): what the second point costs.
    python tools/gkr_two_point_bench.py [--out FILE] [--quick]

tools/gkr_next_layer_bench.py's method: device-resident inputs, nnz = 2 x 2^dim distinct indices, fixed distinct challenges per instance (no
transcript), medians of seven repetitions with the min-max spread beside them, the two forms ALTERNATED inside one process.  Handles are
built under policy "batch" = 2; dim 10 / 12 / 14 / 16 additionally under "batch_slices" = 1 (plan batch.gkr_rounds_slices).  Per cell a
one-point handle and a two-point handle (distinct g2 and (alpha, beta) per instance) stand over the SAME device arrays; reported per form:
  proof   sc_gkr_batch_prover_reset, 2 dim round calls, finish (phase one is not rebuilt; phase two is, at round call dim);
  init    sc_gkr_batch_prover_init / sc_gkr_two_point_init_batch alone (the handle is freed outside the timed region);
  next    sc_gkr_layer_next_batch / sc_gkr_two_point_next_batch alone, onto a second input set (the handle is put back outside it).
The baseline is the one-point handle: the ratios say what the second point costs; there is no pass bar.  `behind`: the two-point median is
above the one-point median by more than the two min-max spreads together.  Checked in every cell: under (alpha, beta) = (1, 0) the two-point
handle's messages equal the one-point handle's bit for bit, and instance 0's two-point messages equal the oracle's (tests/gkr_two_point_cases.py:
Walk2, composed from oracle/cref.py)."""
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
from oracle import cref
from sumcheck_amd import _lib
from gkr_batch_round_slices_bench import sliced_fits
from gkr_batch_rounds_bench import REPS, Batch, V, handle_proof, summary
from tests import gkr_two_point_cases as K

CELLS = [(dim, 0) for dim in (6, 8, 9)] + [(dim, 1) for dim in (10, 12, 14, 16)]  # (dim, policy "batch_slices")
NS = [1, 16, 256]
DEV = _lib.SC_TABLES_ON_DEVICE
TWO = "batch.gkr_two_point"


class Second:
    """per instance a second point and (alpha, beta), host memory; one_zero: (1, 0) for every instance"""

    def __init__(self, n, dim, seed, one_zero=False):
        self.g2 = [cref.synth_table(seed + i, 5, dim) for i in range(n)]
        self.coef = np.ascontiguousarray(np.stack([np.stack([K.ONE, K.ZERO]) if one_zero else cref.synth_table(seed + i, 6, 2) for i in range(n)]))
        self.args = ((V * n)(*[a.ctypes.data for a in self.g2]), V(self.coef.ctypes.data))


def init(b, slices, second=None):
    h = V()
    with _lib.policy(batch=2, batch_slices=slices):
        if second is None:
            _lib.check(sc.lib().sc_gkr_batch_prover_init(b.n, b.dim, *b.args, DEV, C.byref(h)))
        else:
            _lib.check(sc.lib().sc_gkr_two_point_init_batch(b.n, b.dim, *b.args, *second.args, DEV, C.byref(h)))
    return h


def next_layer(h, b, second=None):
    if second is None:
        _lib.check(sc.lib().sc_gkr_layer_next_batch(h, *b.args, DEV))
    else:
        _lib.check(sc.lib().sc_gkr_two_point_next_batch(h, *b.args, *second.args, DEV))


def oracle(b, s, i):
    host = lambda t: np.ascontiguousarray(t.cpu().numpy().view(np.uint64))
    inst = (host(b.idx[i]).reshape(-1), host(b.vals[i]), host(b.f2[i]), host(b.f3[i]), b.g[i], s.g2[i], s.coef[i])
    return K.Walk2(inst, b.dim, np.ascontiguousarray(b.chal[:, i])).msgs


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
            s1, s2, s10 = Second(n, dim, 9700 + dim), Second(n, dim, 9750 + dim), Second(n, dim, 9800 + dim, one_zero=True)
            count = max(2, 32 // n) if dim <= 9 else (2 if (n << dim) <= (1 << 20) else 1)
            out1, out2 = np.zeros((2 * dim, n, 3, 4), np.uint64), np.zeros((2 * dim, n, 3, 4), np.uint64)
            h1, h2 = init(b1, slices), init(b1, slices, s1)
            plan = "batch.gkr_rounds_slices" if slices else "batch.gkr_rounds_one_block"
            before = _lib.plan_stats()

            def sample(fn, undo=None):
                total = 0.0
                for _ in range(count):
                    t0 = time.perf_counter()
                    r = fn()
                    total += time.perf_counter() - t0
                    if undo:
                        undo(r)
                return total / count * 1e6

            forms = {"one_point": (h1, out1, None, None), "two_point": (h2, out2, s1, s2)}
            t = {k: {"proof": [], "init": [], "next": []} for k in forms}
            for k, (h, out, sa, sb) in forms.items():  # (code objects, first-launch attributes)
                handle_proof(b1, h, out, True)
                L.sc_gkr_batch_prover_free(init(b1, slices, sa))
                next_layer(h, b2, sb)
                next_layer(h, b1, sa)
            for _ in range(REPS):  # alternated
                for k, (h, out, sa, sb) in forms.items():
                    t[k]["proof"].append(sample(lambda: handle_proof(b1, h, out, True)))
                    t[k]["init"].append(sample(lambda: init(b1, slices, sa), undo=L.sc_gkr_batch_prover_free))
                    t[k]["next"].append(sample(lambda: next_layer(h, b2, sb), undo=lambda _r: next_layer(h, b1, sa)))  # (back onto the first set, untimed)
            after = _lib.plan_stats()
            assert after[TWO] - before[TWO] == 3 + 3 * count * REPS, "every two-point init, next call and call back is counted once"
            assert after[plan] > before[plan] and after["batch.gkr_rounds_serial"] == before["batch.gkr_rounds_serial"], plan
            assert np.array_equal(out2[:, 0], oracle(b1, s1, 0)), f"dim {dim}, n {n}, instance 0: the two-point messages differ from the oracle's"
            assert not np.array_equal(out1, out2)
            next_layer(h2, b1, s10)
            handle_proof(b1, h2, out2, False)
            assert np.array_equal(out1, out2), f"dim {dim}, n {n}: (1, 0) does not give the one-point handle's messages"
            for h in (h1, h2):
                L.sc_gkr_batch_prover_free(h)
            spread = lambda ts: max(ts) - min(ts)
            cell = {"proofs_per_sample": count}
            for what in ("proof", "init", "next"):
                a, b = t["one_point"][what], t["two_point"][what]
                ma, mb = statistics.median(a), statistics.median(b)
                cell[what] = {"one_point_us": summary(a), "two_point_us": summary(b), "two_over_one": round(mb / ma, 3), "behind": bool(mb - ma > spread(a) + spread(b))}
            row["n"][str(n)] = cell
            del b1, b2
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"tool": "tools/gkr_two_point_bench.py", "library": os.path.basename(_lib.SO_PATH), "reps": REPS,
           "proof": "sc_gkr_batch_prover_reset + 2 dim calls of sc_gkr_batch_prove_round + finish, the whole batch",
           "init": "sc_gkr_batch_prover_init | sc_gkr_two_point_init_batch alone", "next": "sc_gkr_layer_next_batch | sc_gkr_two_point_next_batch alone, onto a second input set",
           "statistic": "median of the repetitions, microseconds, with min and max; fixed challenges, no transcript; the two forms alternated in one job",
           "behind": "the two-point median is above the one-point median by more than the two min-max spreads together", "rows": rows}
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
