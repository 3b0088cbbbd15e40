"""The per-lane running sums of the big rounds (tree_pass in kernels_big.hip) at the pass length at which they are
reduced.  A lane adds one term per iteration of its grid-stride loop and makes its sums canonical after every 32nd; for a product of ONE
table the term is the raw entry.  In the shipped library a lane makes 32 iterations of round 10 only from 33 variables on (a table of
256 GiB), but the condition is about iterations, not about size: the experiments build caps the grid (SC_GRID) and moves the big / small
boundary (SC_SMALL_LOG2), so with ONE block and the boundary at 2^12 pairs, round 10 of a proof in 23 variables is a big round of 2^13
pairs -- 256 lanes x exactly 32 iterations.  Rounds 1 to 9 of the same proof run on that one block too: 2^14 down to 64 iterations a lane,
every 32nd reducing.

The tables are the sinking tables of tests/fe_model.py under their own challenges.  Before bound tables were packed they left every
entry at -9 p in round 10, and 32 of those (288 p) do not fit the top limb's 282 p; since then f29_settle brings every bound entry back
inside +-2^255 (tests/test_fe_model_host.py has both in the exact model), so every case here is expected to pass -- this file pins that.

Each case is a child process on libsumcheck_hip_exp.so (the knobs are read once per process).  Every message of all 23 rounds is
compared bit for bit with cref.Prover.prove_round, and the bound tables with its .state() after round 10."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

WORKER = r'''
import ctypes as C, json, sys, time
import numpy as np
import torch
import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib
from tests import fe_model as fm
from tests import helpers as H
assert _lib.SO_PATH.endswith("libsumcheck_hip_exp.so")
case = json.loads(sys.argv[1])
NV, ROUND = 23, 10
shapes, cap = case["shapes"], case["grid"]
pairs = 1 << (NV - ROUND)
grid_for_pairs = sc.lib().sc_debug_grid_for_pairs  # (a debug entry: exported, not declared in _lib.SIGNATURES)
grid_for_pairs.restype, grid_for_pairs.argtypes = C.c_int, [C.c_uint64]
assert grid_for_pairs(pairs) == cap == grid_for_pairs(1 << (NV - 1)), "every big round's grid is capped: min(grid_for_pairs, .) in launch_round"
assert pairs // (cap * 256) == case["iterations"]
s, r = fm.sinking_challenges(NV, 69000)
c = fm.P - 1 if case["high"] else sum(s)
sink = H.sinking_table_limbs(NV, s, 1, c)
H.assert_entries_match(sink, H.sinking_entry(s, 1, c))
nt = max(max(sh) for sh in shapes) + 1
tabs = [sink if t == case["sinking"] else cref.synth_table(69001, t, 1 << NV) for t in range(nt)]
coefs = cref.synth_table(69002, 1000, len(shapes))
chal = H.mont_challenges(r)
t0 = time.perf_counter()
op = cref.Prover(H.desc_from(NV, shapes, tabs, coefs), threads=cref.max_threads())
want = [op.prove_round(None if j == 0 else chal[j - 1]) for j in range(ROUND)]
_, otabs, _ = op.state()
want += [op.prove_round(chal[j - 1]) for j in range(ROUND, NV)]
op.close()
t1 = time.perf_counter()
pol = {"resident": 0}
if case["lag"] is not None:
    pol["lag_single"] = case["lag"]
with _lib.policy(**pol):
    poly, _ = H.hip_poly_from(NV, shapes, tabs, coefs, device="cuda:0")
    torch.cuda.synchronize()
    st = sc.IPForMLSumcheck.prover_init(poly)
    bad, bad_tabs, moved = [], [], {}
    for j in range(NV):
        before = _lib.plan_stats()
        got = sc.IPForMLSumcheck.prove_round(st, None if j == 0 else sc.VerifierMsg(chal[j - 1])).evaluations
        if not np.array_equal(got, want[j]):
            bad.append(j + 1)
        if j + 1 == ROUND:
            after = _lib.plan_stats()
            moved = {k: after[k] - before[k] for k in after if after[k] != before[k]}
            for u, t in enumerate(st.flattened_ml_extensions):
                if not np.array_equal(t.evaluations, otabs[u]):
                    bad_tabs.append(u)
    st.close()
t2 = time.perf_counter()
print("RESULT " + json.dumps({"bad_rounds": bad, "bad_tables": bad_tabs, "round10_plans": moved,
                              "oracle_s": round(t1 - t0, 2), "device_s": round(t2 - t1, 2)}))
'''

SINGLE, BESIDE = [[0]], [[0, 1], [2]]
BOUND = {"SC_GRID": "1", "SC_SMALL_LOG2": "12"}
CASES = {
    # round 10: 32 iterations a lane, the 32nd term added before the sum is reduced
    "at-the-bound": dict(env=BOUND, shapes=SINGLE, sinking=0, high=False, lag=None, grid=1, iterations=32, plan="big.merged.bind"),
    # ... with the table bound by every round instead of caught up by k_fix_deep in round 6
    "at-the-bound-no-lag": dict(env=BOUND, shapes=SINGLE, sinking=0, high=False, lag=0, grid=1, iterations=32, plan="big.merged.bind"),
    # the same tables on two blocks: 16 iterations
    "control-two-blocks": dict(env={"SC_GRID": "2", "SC_SMALL_LOG2": "12"}, shapes=SINGLE, sinking=0, high=False, lag=None, grid=2, iterations=16,
                               plan="big.merged.bind"),
    # the merged kernel's M = 1 row (32 terms) next to an M = 2 row (two pairs a term: 16).  (Node 1 is computed, not taken from the claim
    # identity: finalize_keeps_sums wants more than 8 blocks a row, i.e. SC_GRID >= 16 and a proof in 27 variables for the same 32 iterations)
    "beside-a-product-of-two": dict(env=BOUND, shapes=BESIDE, sinking=2, high=False, lag=None, grid=1, iterations=32, plan="big.merged.bind"),
    # k_prod_tree<1>: the same tree_pass<1>, one launch per product
    "one-launch-per-product": dict(env=dict(BOUND, SC_MERGE="0"), shapes=SINGLE, sinking=0, high=False, lag=None, grid=1, iterations=32,
                                   plan="big.per_product_tree"),
    # c just below p: round 1 adds 2^14 entries near p a lane on the one block, 512 reductions apart
    "from-the-upper-end": dict(env=BOUND, shapes=SINGLE, sinking=0, high=True, lag=None, grid=1, iterations=32, plan="big.merged.bind"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_big_round_lane_sums_at_the_reduction_interval(name):
    case = dict(CASES[name])
    env, plan = case.pop("env"), case.pop("plan")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = {k: v for k, v in os.environ.items() if not k.startswith("SC_")}
    e.update(env, SC_LIB_VARIANT="exp")
    r = subprocess.run([sys.executable, "-c", WORKER, json.dumps(case)], capture_output=True, text=True, timeout=300, cwd=root, env=e)
    lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert r.returncode == 0 and len(lines) == 1, r.stdout[-1000:] + r.stderr[-3000:]
    res = json.loads(lines[0][7:])
    print(f"\n{name} {env}: {res}")
    assert res["round10_plans"].get("big.store_f29", 0) >= 1 and res["round10_plans"].get(plan, 0) >= 1, "round 10 must run as a big round of the expected kind"
    assert res["round10_plans"].get("big.claim_identity", 0) == 0 and ("big.merged.bind" in res["round10_plans"]) != ("big.per_product_tree" in res["round10_plans"])
    assert res["bad_rounds"] == [] and res["bad_tables"] == [], f"rounds {res['bad_rounds']} and bound tables {res['bad_tables']} differ from the oracle's"
