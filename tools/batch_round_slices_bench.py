"""The sliced rounds of the batched interactive provers: sc_batch_prove_round on a handle built under policy "batch_slices" = 1 (plan
batch.rounds_slices: k_batch_round_slices + k_batch_round_fin for the rounds beyond one block's LDS, k_batch_round behind them) against a
handle built under "batch_slices" = 0 over the SAME device tables -- the serial plan (n ordinary provers inside the handle, a round is a
loop of sc_prove_round), whose code the sliced plan does not touch.  tools/batch_rounds_bench.py's method.
    python tools/batch_round_slices_bench.py [--out FILE] [--quick]

Shapes: c2 (one product of three tables) at nv 10 / 12 / 14 / 16, the two-table shape (a GKR phase's) at nv 12 / 16, config 3's shape (ten
tables, four products) at nv 10 / 12; device tables; n = 1, 16, 256.  A proof is reset(NULL) + num_vars round calls with fixed, distinct
challenges per instance (no transcript).  The two handles are ALTERNATED within one process, seven repetitions of several proofs each;
medians, with the min-max spread beside them.  Both handles' messages of the last repetition are compared bit for bit, and a sample of
instances with the oracle.  `ahead`: the sliced median beats the serial one by more than the two spreads together."""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

import sumcheck_amd as sc
from sumcheck_amd import _lib
from batch_rounds_bench import C2, REPS, TWO_TABLES, Batch, proofs, summary

C3 = [[0, 1, 2, 3], [4, 5, 6], [7, 8], [9]]
ROWS = [("c2", C2, 10), ("c2", C2, 12), ("c2", C2, 14), ("c2", C2, 16), ("two_tables", TWO_TABLES, 12), ("two_tables", TWO_TABLES, 16), ("c3", C3, 10), ("c3", C3, 12)]
NS = [1, 16, 256]


def handle(b, slices):
    h = C.c_void_p()
    with _lib.policy(batch_slices=slices):
        _lib.check(sc.lib().sc_batch_prover_init(b.descs, b.n, C.byref(h)))
    return h


def main():
    args = sys.argv[1:]
    quick = "--quick" in args
    ns = [1, 16] if quick else NS
    rows = []
    for name, shapes, nv in ([ROWS[0], ROWS[4]] if quick else ROWS):
        row = {"shape": name, "nv": nv, "tables": "device", "n": {}}
        for n in ns:
            b = Batch(n, nv, shapes, 9700 + nv)
            hb, hs = handle(b, 1), handle(b, 0)
            before = _lib.plan_stats()
            count = max(2, 64 // n) if nv <= 12 else max(2, 16 // n)
            got, ref = np.zeros((nv, n, b.D, 4), np.uint64), np.zeros((nv, n, b.D, 4), np.uint64)
            proofs(b, hb, 2, got)  # (code objects, first-launch attributes)
            proofs(b, hs, 1, ref)
            mid = _lib.plan_stats()
            sliced_rounds = (mid["batch.rounds_slices"] - before["batch.rounds_slices"]) // 2
            assert sliced_rounds >= 1 and mid["batch.rounds_serial"] == before["batch.rounds_serial"] + nv, "one handle sliced, the other serial"
            rb, pb, rs, ps = [], [], [], []
            for _ in range(REPS):  # alternated
                got[:] = 0
                x, y = proofs(b, hb, count, got)
                rb.append(x)
                pb.append(y)
                x, y = proofs(b, hs, count, ref)
                rs.append(x)
                ps.append(y)
            assert np.array_equal(got, ref), f"{name} nv {nv}, n {n}: the sliced rounds and the serial plan differ"
            for i in range(min(n, 2)):
                assert np.array_equal(got[:, i], b.oracle(i)), f"{name} nv {nv}, n {n}, instance {i}: differs from the oracle"
            mb, ms = statistics.median(pb), statistics.median(ps)
            row["n"][str(n)] = {"sliced_rounds_of_a_proof": sliced_rounds,
                                "sliced_us_per_round_call": summary(rb), "serial_us_per_round_call": summary(rs),
                                "sliced_us_per_proof": summary(pb), "serial_us_per_proof": summary(ps),
                                "sliced_us_per_instance_round": round(statistics.median(rb) / n, 3), "serial_us_per_instance_round": round(statistics.median(rs) / n, 3),
                                "speedup_per_proof": round(ms / mb, 2), "ahead": bool(ms - mb > (max(pb) - min(pb)) + (max(ps) - min(ps)))}
            sc.lib().sc_batch_prover_free(hb)
            sc.lib().sc_batch_prover_free(hs)
            del b
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"tool": "tools/batch_round_slices_bench.py", "library": os.path.basename(_lib.SO_PATH), "reps": REPS,
           "proof": "sc_batch_prover_reset(NULL) + num_vars calls of sc_batch_prove_round, fixed challenges, no transcript",
           "sliced": "a handle built under policy batch_slices = 1: rounds 0 .. nv - nv_max as k_batch_round_slices + k_batch_round_fin, the rest as k_batch_round",
           "baseline": "a handle built under policy batch_slices = 0 over the same device tables: the serial plan (n provers inside the handle, a loop of sc_prove_round)",
           "statistic": "median of the repetitions, microseconds, with min and max", "ahead": "sliced median + both spreads < serial median (per proof)", "rows": rows}
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
