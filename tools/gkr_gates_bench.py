"""The gate form of the GKR batch handle (sc_gkr_gates_init_batch / sc_gkr_gates_next_batch): the kernel plan against the composed plan, and
what gates cost.
    python tools/gkr_gates_bench.py [--out FILE] [--quick]

tools/gkr_two_point_bench.py's method: device-resident inputs, fixed distinct challenges per instance (no transcript), medians of seven
repetitions with the min-max spread beside them, the variants ALTERNATED inside one process.  Handles are built under policy "batch" = 2.
Per cell (dim 6 / 8 / 9, n = 1 / 16 / 256) the lists are the two halves of one list of 2 x 2^dim distinct indices, |MUL| = |ADD| = 2^dim, in
one-point form; three handles stand over the SAME device arrays:
  fused     a gate handle built under policy "gkr_gates_fused" = 1 (plan batch.gkr_gates_one_block);
  composed  a gate handle built under "gkr_gates_fused" = 0 (plan batch.gkr_gates_composed: 3 n multiplication-only instances inside);
  mul_only  a sc_gkr_batch_prover_init handle over the whole list of 2 x 2^dim non-zeros as multiplication gates (ANOTHER statement: reported
            as a ratio with no bar -- it shows what gates cost).
Reported per variant:
  proof   sc_gkr_batch_prover_reset, 2 dim round calls, finish;
  init    the init call alone (the handle is freed outside the timed region);
  next    sc_gkr_gates_next_batch alone (fused and composed), onto a second input set (the handle is put back outside it).
  eval    (d) one layer's values on the device: sc_gkr_gates_layers_eval_batch over both lists against sc_gkr_layers_eval_batch over the MUL
          list alone, on the one-block plan (policy "batch" = 2) and on the cells plan (policy "batch" = 0); instance 0's gate layer equal
          to the big-integer definition before timing.
`ahead`: the fused median is below the composed median by more than the two min-max spreads together.  Checked in every cell: the fused and
the composed messages are equal bit for bit, and instance 0's equal the oracle's (tests/gkr_gates_cases.py: WalkG, from oracle/cref.py)."""
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
from gkr_batch_rounds_bench import REPS, Batch, V, handle_proof, summary
from tests import gkr_gates_cases as K

DIMS = [6, 8, 9]
NS = [1, 16, 256]
DEV = _lib.SC_TABLES_ON_DEVICE


def gate_args(b):
    """the Batch's list split in two: MUL its first 2^dim entries, ADD the rest; then f2, f3, g, no second point"""
    n, N = b.n, b.N
    ptrs = lambda vals: (V * n)(*vals)
    half = (C.c_uint64 * n)(*[N] * n)
    return (ptrs([t.data_ptr() for t in b.idx]), ptrs([t.data_ptr() for t in b.vals]), half, ptrs([t.data_ptr() + 8 * N for t in b.idx]),
            ptrs([t.data_ptr() + 32 * N for t in b.vals]), half, b.args[3], b.args[4], b.args[5], None, None)


def init(b, fused):
    h = V()
    with _lib.policy(batch=2, gkr_gates_fused=fused):
        _lib.check(sc.lib().sc_gkr_gates_init_batch(b.n, b.dim, *gate_args(b), DEV, C.byref(h)))
    return h


def init_mul_only(b):
    h = V()
    with _lib.policy(batch=2):
        _lib.check(sc.lib().sc_gkr_batch_prover_init(b.n, b.dim, *b.args, DEV, C.byref(h)))
    return h


def next_layer(h, b):
    _lib.check(sc.lib().sc_gkr_gates_next_batch(h, *gate_args(b), DEV))


def oracle(b, i):
    host = lambda t: np.ascontiguousarray(t.cpu().numpy().view(np.uint64))
    idx, vals, N = host(b.idx[i]).reshape(-1), host(b.vals[i]), b.N
    inst = K.Inst((idx[:N], vals[:N]), (idx[N:], vals[N:]), host(b.f2[i]), host(b.f3[i]), b.g[i])
    return K.WalkG(inst, np.ascontiguousarray(b.chal[:, i])).msgs


def eval_cell(b, count):
    """(d): {plan: {with_add_us, mul_only_us, with_over_without}}"""
    import torch
    L, n, dim, N = sc.lib(), b.n, b.dim, b.N
    ga = gate_args(b)
    outs = [torch.empty((N, 4), dtype=torch.int64, device="cuda:0") for _ in range(n)]
    torch.cuda.synchronize()
    po = (V * n)(*[t.data_ptr() for t in outs])
    gates = lambda: _lib.check(L.sc_gkr_gates_layers_eval_batch(n, dim, 1, *ga[:8], DEV, po))
    mul_only = lambda: _lib.check(L.sc_gkr_layers_eval_batch(n, dim, 1, ga[0], ga[1], ga[2], ga[6], ga[7], DEV, po))
    host = lambda t: np.ascontiguousarray(t.cpu().numpy().view(np.uint64))
    idx, vals = host(b.idx[0]).reshape(-1), host(b.vals[0])
    want = K.define_layers([((idx[:N], vals[:N]), (idx[N:], vals[N:]))], host(b.f2[0]), host(b.f3[0]))[0]
    res = {}
    for plan, pol in (("one_block", 2), ("cells", 0)):
        with _lib.policy(batch=pol):
            before = _lib.plan_stats()
            gates()
            assert np.array_equal(host(outs[0]), want), f"dim {dim}, n {n}, {plan}: the gate layer differs from the definition"
            mul_only()
            t = {"with_add": [], "mul_only": []}
            for _ in range(REPS):  # alternated
                for k, fn in (("with_add", gates), ("mul_only", mul_only)):
                    t0 = time.perf_counter()
                    for _c in range(count):
                        fn()
                    t[k].append((time.perf_counter() - t0) / count * 1e6)
            after = _lib.plan_stats()
            name = K.EVAL_ONE_BLOCK if plan == "one_block" else K.EVAL_CELLS
            assert after[name] - before[name] == 1 + count * REPS, name
        res[plan] = {"with_add_us": summary(t["with_add"]), "mul_only_us": summary(t["mul_only"]),
                     "with_over_without": round(statistics.median(t["with_add"]) / statistics.median(t["mul_only"]), 3)}
    return res


def main():
    args = sys.argv[1:]
    quick = "--quick" in args
    L = sc.lib()
    rows = []
    for dim in (DIMS[:1] if quick else DIMS):
        row = {"dim": dim, "mul_nnz": 1 << dim, "add_nnz": 1 << dim, "inputs": "device", "n": {}}
        for n in ([1, 16] if quick else NS):
            b1, b2 = Batch(n, dim, 9100 + dim), Batch(n, dim, 9150 + dim)
            count = max(2, 32 // n)
            outs = {k: np.zeros((2 * dim, n, 3, 4), np.uint64) for k in ("fused", "composed", "mul_only")}
            hs = {"fused": init(b1, 1), "composed": init(b1, 0), "mul_only": init_mul_only(b1)}
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

            makers = {"fused": lambda: init(b1, 1), "composed": lambda: init(b1, 0), "mul_only": lambda: init_mul_only(b1)}
            t = {k: {"proof": [], "init": [], "next": []} for k in hs}
            for k, h in hs.items():  # (code objects, first-launch attributes)
                handle_proof(b1, h, outs[k], True)
                L.sc_gkr_batch_prover_free(makers[k]())
                if k != "mul_only":
                    next_layer(h, b2)
                    next_layer(h, b1)
            for _ in range(REPS):  # alternated
                for k, h in hs.items():
                    t[k]["proof"].append(sample(lambda: handle_proof(b1, h, outs[k], True)))
                    t[k]["init"].append(sample(makers[k], undo=L.sc_gkr_batch_prover_free))
                    if k != "mul_only":
                        t[k]["next"].append(sample(lambda: next_layer(h, b2), undo=lambda _r: next_layer(h, b1)))  # (back onto the first set, untimed)
            after = _lib.plan_stats()
            assert after[K.ONE_BLOCK] > before[K.ONE_BLOCK] and after[K.COMPOSED] > before[K.COMPOSED]
            assert after["batch.gkr_rounds_serial"] == before["batch.gkr_rounds_serial"], "the inner handle runs one block per instance at these dims"
            assert np.array_equal(outs["fused"], outs["composed"]), f"dim {dim}, n {n}: the fused and the composed messages differ"
            assert np.array_equal(outs["fused"][:, 0], oracle(b1, 0)), f"dim {dim}, n {n}, instance 0: the messages differ from the oracle's"
            for h in hs.values():
                L.sc_gkr_batch_prover_free(h)
            spread = lambda ts: max(ts) - min(ts)
            cell = {"proofs_per_sample": count}
            for what in ("proof", "init", "next"):
                f, c = t["fused"][what], t["composed"][what]
                mf, mc = statistics.median(f), statistics.median(c)
                cell[what] = {"fused_us": summary(f), "composed_us": summary(c), "composed_over_fused": round(mc / mf, 3), "ahead": bool(mc - mf > spread(f) + spread(c))}
                if what != "next":
                    m = t["mul_only"][what]
                    cell[what]["mul_only_us"] = summary(m)
                    cell[what]["fused_over_mul_only"] = round(mf / statistics.median(m), 3)
            cell["eval"] = eval_cell(b1, count)
            row["n"][str(n)] = cell
            del b1, b2
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"tool": "tools/gkr_gates_bench.py", "library": os.path.basename(_lib.SO_PATH), "reps": REPS,
           "proof": "sc_gkr_batch_prover_reset + 2 dim calls of sc_gkr_batch_prove_round + finish, the whole batch",
           "init": "sc_gkr_gates_init_batch alone (mul_only: sc_gkr_batch_prover_init)", "next": "sc_gkr_gates_next_batch alone, new wiring, onto a second input set",
           "variants": {"fused": "policy gkr_gates_fused = 1: plan batch.gkr_gates_one_block", "composed": "policy gkr_gates_fused = 0: plan batch.gkr_gates_composed",
                        "mul_only": "sc_gkr_batch_prover_init over the 2 x 2^dim non-zeros as multiplication gates: another statement, a ratio with no bar"},
           "statistic": "median of the repetitions, microseconds, with min and max; fixed challenges, no transcript; the variants alternated in one job",
           "ahead": "the fused median is below the composed median by more than the two min-max spreads together",
           "eval": "one layer: sc_gkr_gates_layers_eval_batch over both lists (with_add) against sc_gkr_layers_eval_batch over the MUL list (mul_only), per plan", "rows": rows}
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
