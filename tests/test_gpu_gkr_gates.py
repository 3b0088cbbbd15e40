"""GPU tests of the GKR batch handle's gate form (sc_gkr_gates_init_batch / sc_gkr_gates_next_batch: GKRRoundSumcheck.prover_init_batch_gates
and GKRBatchProverState.next_layer_gates): layers of multiplication and addition gates.  The oracle is the WalkG of tests/gkr_gates_cases.py
(composed from oracle/cref.py) under the same challenges: every message of every round of every instance, (u, v) and finish's three values
are compared bit for bit, on both plans -- batch.gkr_gates_one_block (k_batch_gkr_gates_phase) and batch.gkr_gates_composed (an inner handle
of three multiplication-only instances per instance, on each of ITS plans) -- and the plan counters each call moves are asserted.  Handles
are built under policy "batch" = 2 unless a case says otherwise."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib
from tests import gkr_gates_cases as K
from tests import test_gpu_gkr_batch_rounds as R
from tests import test_gpu_gkr_next_layer as NL

pytestmark = pytest.mark.gpu
INNER = ("batch.gkr_rounds_one_block", "batch.gkr_rounds_slices", "batch.gkr_rounds_serial")


def counters():
    p = _lib.plan_stats()
    return (p[K.ONE_BLOCK], p[K.COMPOSED]) + tuple(p[k] for k in INNER)


def moved(before, fused=0, composed=0, one_block=0, slices=0, serial=0):
    want = (before[0] + fused, before[1] + composed, before[2] + one_block, before[3] + slices, before[4] + serial)
    assert counters() == want, "gates_one_block / gates_composed / inner one_block / slices / serial"


def objects(insts, device="cuda:0"):
    """K.Inst's -> the library's objects, on the host (device=None) or on the GPU"""
    put = NL.td if device is not None else (lambda a: a)
    dim = insts[0].dim
    b = {"raw": insts, "gs": [a.g for a in insts], "dim": dim}
    b["muls"] = [sc.SparseMultilinearExtension(3 * dim, put(a.mul_idx), put(a.mul_vals)) for a in insts]
    b["adds"] = [sc.SparseMultilinearExtension(3 * dim, put(a.add_idx), put(a.add_vals)) for a in insts]
    b["f2s"] = [sc.DenseMultilinearExtension(dim, put(a.f2)) for a in insts]
    b["f3s"] = [sc.DenseMultilinearExtension(dim, put(a.f3)) for a in insts]
    two = insts[0].g2 is not None
    b["g2s"], b["coeffs"] = ([a.g2 for a in insts], [a.coef for a in insts]) if two else (None, None)
    if device is not None:
        torch.cuda.synchronize()
    return b


def init(b, **pol):
    with _lib.policy(**({"batch": 2} if not pol else pol)):
        return sc.GKRRoundSumcheck.prover_init_batch_gates(b["muls"], b["adds"], b["f2s"], b["f3s"], b["gs"], g2s=b["g2s"], coeffs=b["coeffs"])


def onto(st, b, keep=False):
    st.next_layer_gates(b["f2s"], b["f3s"], b["gs"], None if keep else b["muls"], None if keep else b["adds"], g2s=b["g2s"], coeffs=b["coeffs"])
    assert st.round == 0 and st.randomness(0).shape[0] == 0


def ragged(n, dim, k):
    """per instance: none at all, one, more than a stride per lane -- and for a lone instance three per cell; k shifts the pattern so that
    an instance's two lists differ in length"""
    N = 1 << dim
    return [3 * N - k] if n == 1 else [[0, 1, 3 * N, N // 2 + 1][(i + k) % 4] for i in range(n)]


def layer(n, dim, seed, two_point, mul_nnzs=None, add_nnzs=None, variant="repeated"):
    mul_nnzs, add_nnzs = mul_nnzs or ragged(n, dim, 0), add_nnzs or ragged(n, dim, 1)
    return [K.instance(dim, seed + 7919 * i, mul_nnzs[i], add_nnzs[i], two_point, variant) for i in range(n)]


# ---- 1. parity with the oracle on the kernel plan ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _parity_case(dim, n, two_point):
    """shared by the device and the host case of a shape: the walks depend on the seeds only"""
    insts = layer(n, dim, 61000 + 97 * dim + n, two_point)
    chal = R.challenges(n, dim, 61500 + dim + n, edge_instance=n // 2 if n > 1 else None)  # (one instance's challenges run through 0, 1, p - 1)
    chal.setflags(write=False)
    return insts, chal, K.walks(insts, chal)


@pytest.mark.parametrize("device", ["cuda:0", None], ids=["device", "host"])
@pytest.mark.parametrize("two_point", [False, True], ids=["one-point", "two-point"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("dim", [1, 2, 5, 9])
def test_one_block_every_round_equals_the_walk(dim, n, two_point, device):
    """dim 1: one pair; 2: fewer cells than a wavefront; 5: eq's halves differ in size; 9: two strides per lane and the LDS full.  Ragged
    lists with repeated indices: an instance with no MUL gates, one with no ADD gates"""
    insts, chal, want = _parity_case(dim, n, two_point)
    before = counters()
    st = init(objects(insts, device))
    moved(before)
    R.drive(st, chal, want)
    st.close()
    moved(before, fused=2 * dim)


@pytest.mark.parametrize("fused", [1, 0], ids=["one-block", "composed"])
def test_one_wiring_for_all_instances_under_a_shared_challenge(fused):
    """the composed plan hands a shared challenge to its inner handle as it is, per-instance ones replicated three times"""
    dim, n = 5, 4
    N = 1 << dim
    base = K.instance(dim, 62000, 3 * N, 2 * N, True)
    insts = [K.Inst((base.mul_idx, base.mul_vals), (base.add_idx, base.add_vals), cref.synth_table(62100 + i, 2, N), cref.synth_table(62100 + i, 3, N),
                    cref.synth_table(62100 + i, 4, dim), cref.synth_table(62100 + i, 5, dim), cref.synth_table(62100 + i, 6, 2)) for i in range(n)]
    b = objects(insts)
    b["muls"], b["adds"] = [b["muls"][0]] * n, [b["adds"][0]] * n  # ONE object for all: copied once
    chal = R.challenges(n, dim, 62002, edge_instance=None)
    same = np.repeat(chal[:, :1], n, axis=1)
    want = K.walks(insts, same)
    st = init(b, batch=2, gkr_gates_fused=fused)
    shared = R.drive(st, chal, want, shared=True, label="shared: ")
    st.reset()
    each = R.drive(st, same, want, label="n times, after a reset: ")
    st.close()
    for x, y in zip(shared, each):
        assert np.array_equal(x, y)


# ---- 2. the ends of the envelope -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over", [None, "mul", "add"], ids=["exactly", "mul-one-over", "add-one-over"])
def test_both_lists_at_the_limit_and_one_entry_over_on_either(over):
    """dim 9, both lists at exactly 64 x 2^9: the kernel plan; one entry more on either list: the composed plan, the same oracle"""
    dim, full = 9, 64 << 9
    inst = K.instance(dim, 63000, full + (over == "mul"), full + (over == "add"), True, "random")
    assert K.one_block_fits(dim, len(inst.mul_idx), len(inst.add_idx)) == (over is None)
    chal = R.challenges(1, dim, 63001, edge_instance=None)
    want = K.walks([inst], chal)
    before = counters()
    st = init(objects([inst]))
    R.drive(st, chal, want)
    st.close()
    if over is None:
        moved(before, fused=2 * dim)
    else:
        moved(before, composed=2 * dim, serial=2 * dim)  # (the inner handle: one list beyond ITS envelope puts all three instances on the serial plan)


# ---- 3. values at the ends of the field, degenerate lists ------------------------------------------------------------------------------
def test_both_full_lists_in_one_cell_with_values_p_minus_one():
    """2 x 64 x 2^9 terms of p - 1 times tables of p - 1 into ONE cell of the pass that takes both lists: the lanes at their bound.  In phase
    one that cell's field sum is zero -- MUL's terms are E (p - 1)(p - 1) = E, ADD's E (p - 1) = -E, as many of each -- and so it is in phase
    two, where f2(u) = -1 turns MUL's terms into ADD's negatives; the cell's integer lanes hold all 2^16 terms either way.  H2 and T2 have
    their one cell"""
    dim = 9
    inst = K.one_cell_instance(dim, 64 << dim, 64001)
    chal = R.challenges(1, dim, 64002, edge_instance=None)
    want = K.walks([inst], chal)
    assert not want[0].H1.any() and not want[0].T1.any() and all(np.count_nonzero(t.any(axis=1)) == 1 for t in (want[0].H2, want[0].T2))
    before = counters()
    st = init(objects([inst]))
    R.drive(st, chal, want)
    st.close()
    moved(before, fused=2 * dim)


@pytest.mark.parametrize("two_point", [False, True], ids=["one-point", "two-point"])
@pytest.mark.parametrize("fused", [1, 0], ids=["one-block", "composed"])
def test_everything_from_zero_one_and_p_minus_one(fused, two_point):
    """g, g2, f2, f3, the lists' values, alpha, beta and every challenge from {0, 1, p - 1}"""
    dim, n = 3, 6
    insts = [K.edge_instance(dim, 65000 + i, 20, two_point) for i in range(n)]
    chal = np.ascontiguousarray(np.stack([[K.EDGE[(j + i) % 3] for i in range(n)] for j in range(2 * dim)]))
    want = K.walks(insts, chal)
    assert any(w.msgs.any() for w in want)
    st = init(objects(insts), batch=2, gkr_gates_fused=fused)
    R.drive(st, chal, want)
    st.close()


@pytest.mark.parametrize("fused", [1, 0], ids=["one-block", "composed"])
def test_one_and_zero_give_the_one_point_bits(fused):
    dim, n = 4, 2
    one = layer(n, dim, 66000, False)
    two = [a.with_second(cref.synth_table(66100 + i, 5, dim), np.stack([K.ONE, K.ZERO])) for i, a in enumerate(one)]
    chal = R.challenges(n, dim, 66001)
    want = K.walks(one, chal)
    st = init(objects(two), batch=2, gkr_gates_fused=fused)
    R.drive(st, chal, want, label="(1, 0): ")
    st.close()


def test_with_no_addition_gates_the_messages_are_the_multiplication_handles():
    """an empty ADD list: bit for bit the messages of a sc_gkr_batch_prover_init handle over the MUL list; its finals relate as stated"""
    dim, n = 5, 3
    N = 1 << dim
    insts = layer(n, dim, 67000, False, [3 * N, 1, N], [0] * n)
    chal = R.challenges(n, dim, 67001)
    b = objects(insts)
    want = K.walks(insts, chal)
    st = init(b)
    got, _, fin = R.drive(st, chal, want)
    st.close()
    with _lib.policy(batch=2):
        old = sc.GKRRoundSumcheck.prover_init_batch(b["muls"], b["f2s"], b["f3s"], b["gs"])
    msgs = []
    for t in range(2 * dim):
        msgs.append(old.prove_round(None if t == 0 else chal[t - 1]))
    _, fin_old = old.finish(chal[2 * dim - 1])
    old.close()
    assert np.array_equal(got, np.stack(msgs, axis=1))
    for i in range(n):
        assert np.array_equal(fin[i, 0], fin_old[i, 1]) and np.array_equal(fin[i, 2], cref.fr_binop("mul", fin_old[i, 0], fin_old[i, 2]))


@pytest.mark.parametrize("fused", [1, 0], ids=["one-block", "composed"])
@pytest.mark.parametrize("mul_nnz,add_nnz", [(0, 40), (0, 0)], ids=["no-mul", "neither"])
def test_an_empty_multiplication_list_and_both_empty(mul_nnz, add_nnz, fused):
    dim, n = 4, 2
    insts = layer(n, dim, 68000 + add_nnz, True, [mul_nnz] * n, [add_nnz] * n)
    chal = R.challenges(n, dim, 68001)
    want = K.walks(insts, chal)
    assert want[0].msgs.any() == bool(add_nnz)
    st = init(objects(insts), batch=2, gkr_gates_fused=fused)
    R.drive(st, chal, want)
    st.close()


# ---- 4. the composed plan ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 9])
def test_fused_and_composed_agree_bit_for_bit_and_with_the_oracle(dim):
    n = 3
    insts = layer(n, dim, 69000 + dim, True)
    chal = R.challenges(n, dim, 69001 + dim)
    want = K.walks(insts, chal)
    b = objects(insts)
    before = counters()
    st = init(b, batch=2, gkr_gates_fused=0)
    composed = R.drive(st, chal, want, label="composed: ")
    st.close()
    moved(before, composed=2 * dim, one_block=2 * dim)
    st = init(b)
    fused = R.drive(st, chal, want, label="fused: ")
    st.close()
    moved(before, composed=2 * dim, one_block=2 * dim, fused=2 * dim)
    for x, y in zip(composed, fused):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("dim,slices", [(10, 0), (10, 1), (11, 1)], ids=["dim10-inner-serial", "dim10-inner-slices", "dim11-inner-sliced-rounds"])
def test_beyond_one_block_the_inner_handle_chooses_its_plan(dim, slices):
    n = 2
    N = 1 << dim
    insts = layer(n, dim, 70000 + dim, True, [2 * N, N // 2 + 1], [N + 1, 3 * N])
    chal = R.challenges(n, dim, 70001 + dim, edge_instance=None)
    want = K.walks(insts, chal)
    before = counters()
    st = init(objects(insts), batch=2, batch_slices=slices)
    R.drive(st, chal, want)
    st.close()
    moved(before, composed=2 * dim, slices=2 * dim if slices else 0, serial=0 if slices else 2 * dim)


# ---- 5. the handle's state -----------------------------------------------------------------------------------------------------------
def _status(fn):
    with pytest.raises(_lib.SumcheckError) as e:
        fn()
    return e.value.code


@pytest.mark.parametrize("fused", [1, 0], ids=["one-block", "composed"])
def test_reset_in_the_middle_of_phase_two_state_and_the_status_codes_of_misuse(fused):
    dim, n = 3, 2
    insts = layer(n, dim, 71000, True)
    chal = R.challenges(n, dim, 71001)
    want = K.walks(insts, chal)
    b = objects(insts)
    st = init(b, batch=2, gkr_gates_fused=fused)
    assert _status(lambda: st.prove_round(chal[0])) == _lib.SC_ERR_FIRST_ROUND_HAS_MSG
    assert _status(lambda: st.finish(chal[0])) == _lib.SC_ERR_NOT_ACTIVE
    for t in range(dim + 2):
        got = st.prove_round(None if t == 0 else chal[t - 1])
        assert np.array_equal(got, np.stack([w.msgs[t] for w in want]))
    assert st.round == dim + 2 and np.array_equal(st.randomness(1), chal[:dim + 1, 1])
    assert _status(lambda: st.prove_round()) == _lib.SC_ERR_MISSING_MSG
    assert _status(lambda: st.tables(0)) == _lib.SC_ERR_BAD_ARG, "a gate handle exports no tables"
    bad = chal[dim + 1].copy()
    bad[1] = R.P_LIMBS
    assert _status(lambda: st.prove_round(bad)) == _lib.SC_ERR_BAD_ARG
    assert st.round == dim + 2, "an argument error leaves the handle where it was"
    # the older next calls refuse a gate handle; the proof in progress goes on
    assert _status(lambda: st.next_layer(b["f2s"], b["f3s"], b["gs"])) == _lib.SC_ERR_BAD_ARG
    assert _status(lambda: st.next_layer(b["f2s"], b["f3s"], b["gs"], g2s=b["g2s"], coeffs=b["coeffs"])) == _lib.SC_ERR_BAD_ARG
    got = st.prove_round(chal[dim + 1])
    assert np.array_equal(got, np.stack([w.msgs[dim + 2] for w in want]))
    st.reset()
    assert st.round == 0 and st.randomness(0).shape[0] == 0
    R.drive(st, chal, want, label="after a reset in phase two: ")
    assert _status(lambda: st.prove_round(chal[0])) == _lib.SC_ERR_NOT_ACTIVE
    assert _status(lambda: st.finish(chal[0])) == _lib.SC_ERR_NOT_ACTIVE
    st.reset()
    R.drive(st, chal, want, label="after a reset behind finish: ")
    st.close()


def test_a_handle_of_the_older_inits_is_refused_by_the_gate_call():
    dim, n = 3, 2
    insts = layer(n, dim, 72000, False)
    b = objects(insts)
    with _lib.policy(batch=2):
        old = sc.GKRRoundSumcheck.prover_init_batch(b["muls"], b["f2s"], b["f3s"], b["gs"])
    assert _status(lambda: old.next_layer_gates(b["f2s"], b["f3s"], b["gs"])) == _lib.SC_ERR_BAD_ARG
    old.close()


# ---- 6. the next layer, and its errors in the middle of a proof ------------------------------------------------------------------------
@pytest.mark.parametrize("device", ["cuda:0", None], ids=["device", "host"])
@pytest.mark.parametrize("fused", [1, 0], ids=["one-block", "composed"])
def test_next_with_kept_and_with_new_wiring_and_errors_that_leave_the_proof_where_it_was(fused, device):
    dim, n = 4, 3
    N = 1 << dim
    a = layer(n, dim, 73000, True, [3 * N] * n, [2 * N] * n)
    kept = [K.Inst((x.mul_idx, x.mul_vals), (x.add_idx, x.add_vals), cref.synth_table(73100 + i, 2, N), cref.synth_table(73100 + i, 3, N), cref.synth_table(73100 + i, 4, dim))
            for i, x in enumerate(a)]  # the same wiring, new tables, ONE point
    new = layer(n, dim, 73200, True, [2 * N, 0, 3 * N], [2 * N, N, 1])  # new wiring, no longer than init's
    chal = R.challenges(n, dim, 73001)
    wa, wk, wn = K.walks(a, chal), K.walks(kept, chal), K.walks(new, chal)
    ba, bk, bn = objects(a, device), objects(kept, device), objects(new, device)
    st = init(ba, batch=2, gkr_gates_fused=fused)
    half = dim + 1
    for t in range(half):
        assert np.array_equal(st.prove_round(None if t == 0 else chal[t - 1]), np.stack([w.msgs[t] for w in wa]))
    # ---- errors, each in the middle of the proof ----
    L = sc.lib()
    ptrs = lambda objs, k: (C.c_void_p * n)(*[C.cast(o._ptrs()[k], C.c_void_p) for o in objs])
    dense = lambda ms: (C.c_void_p * n)(*[C.cast(sc.gkr_round_sumcheck._dense_ptr(m), C.c_void_p) for m in ms])
    gp = (C.c_void_p * n)(*[x.g.ctypes.data for x in new])
    g2p = (C.c_void_p * n)(*[x.g2.ctypes.data for x in new])
    coef = np.ascontiguousarray(np.stack([x.coef for x in new]))
    nnz = lambda objs: (C.c_uint64 * n)(*[o.nnz for o in objs])
    flags = _lib.SC_TABLES_ON_DEVICE if device is not None else 0
    full = [ptrs(bn["muls"], 0), ptrs(bn["muls"], 1), nnz(bn["muls"]), ptrs(bn["adds"], 0), ptrs(bn["adds"], 1), nnz(bn["adds"])]
    for hole in (0, 2, 4):  # a mixed NULL pattern
        mixed = list(full)
        mixed[hole] = None
        assert L.sc_gkr_gates_next_batch(st._h, *mixed, dense(bn["f2s"]), dense(bn["f3s"]), gp, g2p, coef.ctypes.data, flags) == _lib.SC_ERR_BAD_ARG
        assert "come together" in L.sc_last_error().decode()
    assert L.sc_gkr_gates_next_batch(st._h, *full, dense(bn["f2s"]), dense(bn["f3s"]), gp, g2p, None, flags) == _lib.SC_ERR_BAD_ARG, "g2 without coef"
    assert L.sc_gkr_gates_next_batch(st._h, *full, dense(bn["f2s"]), dense(bn["f3s"]), gp, g2p, coef.ctypes.data, flags ^ _lib.SC_TABLES_ON_DEVICE) == _lib.SC_ERR_BAD_ARG
    bad = [K.Inst((x.mul_idx, x.mul_vals), (x.add_idx.copy(), x.add_vals), x.f2, x.f3, x.g, x.g2, x.coef) for x in new]
    bad[1].add_idx[N // 2] |= np.uint64(1) << np.uint64(3 * dim)  # an out-of-range index in an ADD list (device lists: found on the device)
    bb = objects(bad, device)
    with pytest.raises(_lib.SumcheckError) as e:
        st.next_layer_gates(bb["f2s"], bb["f3s"], bb["gs"], bb["muls"], bb["adds"], g2s=bb["g2s"], coeffs=bb["coeffs"])
    assert e.value.code == _lib.SC_ERR_BAD_ARG and e.value.msg == ("instance 1: add has an index out of range" if device is not None else f"instance 1: add index {N // 2} out of range")
    longer = layer(n, dim, 73300, True, [3 * N + 1] * n, [2 * N] * n)  # one entry more than init reserved
    bl = objects(longer, device)
    if fused:
        with pytest.raises(_lib.SumcheckError) as e:
            st.next_layer_gates(bl["f2s"], bl["f3s"], bl["gs"], bl["muls"], bl["adds"], g2s=bl["g2s"], coeffs=bl["coeffs"])
        assert e.value.code == _lib.SC_ERR_BAD_ARG and "build a new handle" in e.value.msg
    # ---- the proof continues with the oracle's bits ----
    assert st.round == half
    for t in range(half, 2 * dim):
        assert np.array_equal(st.prove_round(chal[t - 1]), np.stack([w.msgs[t] for w in wa])), t
    _, fin = st.finish(chal[2 * dim - 1])
    assert np.array_equal(fin, np.stack([w.final for w in wa]))
    # ---- kept wiring in one-point form, then new wiring in two-point form, then back ----
    before = counters()
    onto(st, bk, keep=True)
    R.drive(st, chal, wk, label="kept wiring: ")
    onto(st, bn)
    st.prove_round()
    onto(st, bn)  # callable in the middle of a proof
    R.drive(st, chal, wn, label="new wiring: ")
    onto(st, ba)
    R.drive(st, chal, wa, label="back onto init's layer: ")
    st.close()
    moved(before, fused=(6 * dim + 1) * fused, composed=(6 * dim + 1) * (1 - fused), one_block=(6 * dim + 1) * (1 - fused))


# ---- 7. the layers' values ------------------------------------------------------------------------------------------------------------
def eval_counters():
    p = _lib.plan_stats()
    return p[K.EVAL_ONE_BLOCK], p[K.EVAL_CELLS], p["batch.gkr_eval_layers_one_block"], p["batch.gkr_eval_cells"]


def eval_moved(before, one_block=0, cells=0, old_one_block=0, old_cells=0):
    assert eval_counters() == (before[0] + one_block, before[1] + cells, before[2] + old_one_block, before[3] + old_cells), "gates eval one_block / cells / mul-only one_block / cells"


def host(m):
    return np.ascontiguousarray(m.evaluations.cpu().numpy().view(np.uint64)) if m.on_device else m.evaluations


def evaluate(layers, f2s, f3s, dim, device="cuda:0", **pol):
    """layers[k][i] = ((mul_idx, mul_vals), (add_idx, add_vals)) -> the library's tables as host arrays, [k][i]"""
    put = NL.td if device is not None else (lambda a: a)
    sp = lambda lst: sc.SparseMultilinearExtension(3 * dim, put(lst[0]), put(lst[1]))
    muls, adds = [[sp(w[0]) for w in layer] for layer in layers], [[sp(w[1]) for w in layer] for layer in layers]
    d2, d3 = [sc.DenseMultilinearExtension(dim, put(a)) for a in f2s], [sc.DenseMultilinearExtension(dim, put(a)) for a in f3s]
    if device is not None:
        torch.cuda.synchronize()
    with _lib.policy(**({"batch": 2} if not pol else pol)):
        out = sc.GKRRoundSumcheck.evaluate_layers_batch_gates(muls, adds, d2, d3)
    return [[host(m) for m in layer] for layer in out]


@pytest.mark.parametrize("device", ["cuda:0", None], ids=["device", "host"])
@pytest.mark.parametrize("dim", [1, 4, 9, 10, 12])
def test_the_layers_equal_the_definition_in_big_integers(dim, device):
    """dims 1, 4, 9: one block for all layers; 10, 12: the cells.  Two layers, two instances, lists of different lengths with repeated indices"""
    n, N = 2, 1 << dim
    nn = [(2 * N + 1, N), (N // 2 + 1, 3 * N)]
    layers = [[(K.wiring(dim, 75000 + 100 * k + i, nn[k][0]), K.wiring(dim, 75050 + 100 * k + i, nn[k][1])) for i in range(n)] for k in range(2)]
    f2s, f3s = [cref.synth_table(75500 + i, 2, N) for i in range(n)], [cref.synth_table(75500 + i, 3, N) for i in range(n)]
    want = [K.define_layers([layers[0][i], layers[1][i]], f2s[i], f3s[i]) for i in range(n)]
    cref.fix_variables(want[0][1], cref.synth_table(75600, 4, dim))  # (the oracle's own reading of an expected layer)
    before = eval_counters()
    got = evaluate(layers, f2s, f3s, dim, device)
    eval_moved(before, one_block=int(dim <= K.MAX_DIM), cells=int(dim > K.MAX_DIM))
    for i in range(n):
        for k in range(2):
            assert np.array_equal(got[k][i], want[i][k]) and want[i][k].any(), (k, i)


@pytest.mark.parametrize("dim", [4, 10])
def test_mul_only_equals_the_multiplication_call_and_add_only_equals_the_definition(dim):
    n, N = 2, 1 << dim
    empty = (np.zeros(0, np.uint64), np.zeros((0, 4), np.uint64))
    lists = [K.wiring(dim, 76000 + dim + i, 2 * N + i) for i in range(n)]
    f2s, f3s = [cref.synth_table(76100 + i, 2, N) for i in range(n)], [cref.synth_table(76100 + i, 3, N) for i in range(n)]
    got = evaluate([[(l, empty) for l in lists]], f2s, f3s, dim)
    sp = lambda lst: sc.SparseMultilinearExtension(3 * dim, NL.td(lst[0]), NL.td(lst[1]))
    before = eval_counters()
    with _lib.policy(batch=2):
        old = sc.GKRRoundSumcheck.evaluate_layers_batch([[sp(l) for l in lists]], [sc.DenseMultilinearExtension(dim, NL.td(a)) for a in f2s],
                                                        [sc.DenseMultilinearExtension(dim, NL.td(a)) for a in f3s])
    eval_moved(before, old_one_block=int(dim <= K.MAX_DIM), old_cells=int(dim > K.MAX_DIM))
    add_only = evaluate([[(empty, l) for l in lists]], f2s, f3s, dim)
    for i in range(n):
        assert np.array_equal(got[0][i], host(old[0][i])), "MUL only: sc_gkr_layers_eval_batch's bits"
        want = K.define_layers([(empty, lists[i])], f2s[i], f3s[i])[0]
        cref.fix_variables(want, cref.synth_table(76200, 4, dim))
        assert np.array_equal(add_only[0][i], want) and want.any(), "ADD only"


@pytest.mark.parametrize("dim,batch", [(9, 0), (10, 2)], ids=["dim9-cells", "dim10-cells"])
def test_seventy_thousand_addition_terms_of_p_minus_one_in_one_cell(dim, batch):
    """70000 > 64 x 2^9 ADD terms v (A[x] + B[y]) with v = A[x] = B[y] = p - 1, all in ONE cell z: every term is (p - 1)(p - 2) = 2, so the
    cell is 140000 and every other cell zero; 70000 x 2^32 < 2^63 is the lane's bound"""
    N, nnz = 1 << dim, 70000
    idx, vals, table = K.one_cell_terms(dim, nnz, 5, 77000 + dim)
    empty = (np.zeros(0, np.uint64), np.zeros((0, 4), np.uint64))
    before = eval_counters()
    got = evaluate([[(empty, (idx, vals))]], [table], [table], dim, batch=batch)[0][0]
    eval_moved(before, cells=1)
    want = np.zeros((N, 4), np.uint64)
    want[5] = cref.ints_to_mont([2 * nnz])[0]
    assert np.array_equal(got, want)
    assert np.array_equal(cref.fix_variables(got, cref.ints_to_mont([1, 0, 1] + [0] * (dim - 3)))[0], want[5]), "the oracle reads cell 5"


@pytest.mark.parametrize("dim", [4, 10])
def test_an_out_of_range_device_index_is_found_before_any_output_is_written(dim):
    n, N = 2, 1 << dim
    lists = [[(K.wiring(dim, 78000 + i + 10 * k, N), K.wiring(dim, 78050 + i + 10 * k, N + 1)) for i in range(n)] for k in range(2)]
    bad_idx = lists[1][1][1][0].copy()
    bad_idx[N // 2] |= np.uint64(1) << np.uint64(3 * dim)
    lists[1][1] = (lists[1][1][0], (bad_idx, lists[1][1][1][1]))
    sp = lambda lst: sc.SparseMultilinearExtension(3 * dim, NL.td(lst[0]), NL.td(lst[1]))
    muls, adds = [[sp(w[0]) for w in layer] for layer in lists], [[sp(w[1]) for w in layer] for layer in lists]
    f2s = [sc.DenseMultilinearExtension(dim, NL.td(cref.synth_table(78100 + i, 2, N))) for i in range(n)]
    outs = [torch.full((N, 4), 7, dtype=torch.int64, device="cuda:0") for _ in range(2 * n)]
    torch.cuda.synchronize()
    ptrs = lambda vals: (C.c_void_p * len(vals))(*[C.cast(v, C.c_void_p) for v in vals])
    args = []
    for flat in ([f for layer in muls for f in layer], [f for layer in adds for f in layer]):
        args += [ptrs([f._ptrs()[0] for f in flat]), ptrs([f._ptrs()[1] for f in flat]), (C.c_uint64 * (2 * n))(*[f.nnz for f in flat])]
    dp = ptrs([C.c_void_p(m.data_ptr()) for m in f2s])
    before = eval_counters()
    with _lib.policy(batch=2):
        rc = sc.lib().sc_gkr_gates_layers_eval_batch(n, dim, 2, *args, dp, dp, _lib.SC_TABLES_ON_DEVICE, ptrs([C.c_void_p(t.data_ptr()) for t in outs]))
    assert rc == _lib.SC_ERR_BAD_ARG and sc.lib().sc_last_error().decode() == "layer 1 instance 1: add has an index out of range"
    eval_moved(before)
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in outs), "no output was written"
    muls[0][0].evaluate(cref.synth_table(78200, 4, 3 * dim))  # (the library is usable afterwards)


# ---- 8. a circuit end to end ---------------------------------------------------------------------------------------------------------
def _transcript_challenge(rng, msgs):
    for m in msgs:
        rng.feed_prover_msg(m)
    return rng.sample_fr()


def _prove_layer(st, rng):
    """2 dim round calls and finish under the test's transcript, one challenge shared by all instances -> (first message, u, v, final)"""
    first, r = None, None
    for t in range(2 * st.dim):
        msgs = st.prove_round(r, shared=r is not None)
        first = msgs if t == 0 else first
        r = _transcript_challenge(rng, msgs)
    uv, fin = st.finish(r, shared=True)
    return first, uv[0, 0], uv[0, 1], fin


@pytest.mark.parametrize("dim", [3, 9])
def test_a_circuit_of_three_gate_layers_is_proved_back_to_its_inputs(dim):
    """three layers of both kinds of gate, each reading the layer below on both sides, evaluated on the device
    (sc_gkr_gates_layers_eval_batch) and compared with the definition; the handle reads the layers' values where the evaluation left them.
    The output layer is claimed at one point, every layer below at the two points the layer above
    ended on; at each layer the claim is alpha W(u) + beta W(v), the subclaim verifies, and a flipped limb is rejected"""
    n, n_layers = 2, 3
    N = 1 << dim
    nnzs = [(N + 1, N), (2 * N, N + 3), (3 * N, 2 * N)]  # (mul, add) per layer; the output layer, which the handle is built over, has the longest lists
    inputs = [(cref.synth_table(74000 + dim + i, 2, N), cref.synth_table(74000 + dim + i, 3, N)) for i in range(n)]
    wires = [[(K.wiring(dim, 74100 + 10 * k + i, nnzs[k][0], "random"), K.wiring(dim, 74200 + 10 * k + i, nnzs[k][1], "random")) for i in range(n)] for k in range(n_layers)]
    W = []  # W[k][i]: layer k's values
    for k in range(n_layers):
        below = inputs if k == 0 else [(w, w) for w in W[k - 1]]
        W.append([cref.ints_to_mont(K.define_layer(K.Inst(wires[k][i][0], wires[k][i][1], below[i][0], below[i][1], None))) for i in range(n)])
    sp = lambda lst: sc.SparseMultilinearExtension(3 * dim, NL.td(lst[0]), NL.td(lst[1]))
    muls = [[sp(wires[k][i][0]) for i in range(n)] for k in range(n_layers)]
    adds = [[sp(wires[k][i][1]) for i in range(n)] for k in range(n_layers)]
    in2, in3 = [sc.DenseMultilinearExtension(dim, NL.td(a)) for a, _ in inputs], [sc.DenseMultilinearExtension(dim, NL.td(b)) for _, b in inputs]
    torch.cuda.synchronize()
    before = eval_counters()
    with _lib.policy(batch=2):
        dW = sc.GKRRoundSumcheck.evaluate_layers_batch_gates(muls, adds, in2, in3)  # dW[k][i] stay on the device: the handle reads them there
    eval_moved(before, one_block=1)
    for k in range(n_layers):
        for i in range(n):
            assert np.array_equal(host(dW[k][i]), W[k][i]), f"layer {k}, instance {i}: the evaluated layer differs from the definition"
    rng = cref.Rng()
    rng.feed_bytes(b"gkr gate layers end to end")
    at = lambda table, point: cref.fix_variables(table, point)[0]
    mul, add = (lambda a, b: cref.fr_binop("mul", a, b)), (lambda a, b: cref.fr_binop("add", a, b))
    g = np.stack([rng.sample_fr() for _ in range(dim)])
    with _lib.policy(batch=2):
        st = sc.GKRRoundSumcheck.prover_init_batch_gates(muls[2], adds[2], dW[1], dW[1], [g] * n)
    first, u, v, fin = _prove_layer(st, rng)
    for i in range(n):
        assert np.array_equal(add(first[i, 0], first[i, 1]), at(W[2][i], g)), f"output layer, instance {i}: the claim is W(g)"
    claims = [sc.GKRRoundSumcheckSubClaim(u, v, fin[i, 2]) for i in range(n)]
    assert sc.GKRRoundSumcheckSubClaim.verify_subclaim_gates_batch(claims, muls[2], adds[2], dW[1], dW[1], [g] * n) == [True] * n
    below = {1: (dW[0], dW[0], W[1]), 0: (in2, in3, W[0])}
    for k in (1, 0):
        alpha, beta = rng.sample_fr(), rng.sample_fr()
        coeffs = [np.stack([alpha, beta])] * n
        st.next_layer_gates(below[k][0], below[k][1], [u] * n, muls[k], adds[k], g2s=[v] * n, coeffs=coeffs)
        gu, gv = u, v
        first, u, v, fin = _prove_layer(st, rng)
        for i in range(n):
            want = add(mul(alpha, at(below[k][2][i], gu)), mul(beta, at(below[k][2][i], gv)))
            assert np.array_equal(add(first[i, 0], first[i, 1]), want), f"layer {k}, instance {i}: the claim is alpha W(u) + beta W(v)"
        claims = [sc.GKRRoundSumcheckSubClaim(u, v, fin[i, 2]) for i in range(n)]
        assert sc.GKRRoundSumcheckSubClaim.verify_subclaim_gates_batch(claims, muls[k], adds[k], below[k][0], below[k][1], [gu] * n, [gv] * n, coeffs) == [True] * n
        if k == 1:
            flipped = fin[0, 2].copy()
            flipped[1] ^= np.uint64(1)
            wrong = [sc.GKRRoundSumcheckSubClaim(u, v, flipped)] + claims[1:]
            assert sc.GKRRoundSumcheckSubClaim.verify_subclaim_gates_batch(wrong, muls[k], adds[k], below[k][0], below[k][1], [gu] * n, [gv] * n, coeffs) == [False] + [True] * (n - 1)
    st.close()
    for i in range(n):  # the last layer ends on the INPUT tables
        assert np.array_equal(fin[i, 0], at(inputs[i][0], u)) and np.array_equal(fin[i, 1], at(inputs[i][1], v)), f"instance {i}: f2(u), f3(v) of the inputs"


# ---- 9. the C++ mirror ---------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_gates():
    """include/sumcheck_amd.hpp: a program proves layer A in two-point form, layer B (new wiring) in one-point form, layer A's tables over
    B's kept wiring, and layer A again on one handle at dim 4, checks the verifier's helper, and prints its inputs, its challenges and every
    message; the messages are compared with the walks over what it printed"""
    import subprocess
    from tests import test_gkr_gates_host as GH
    r = subprocess.run([GH.build_gates_mirror()], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-2000:] + r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        key, colon, words = line.partition(":")
        if colon:  # (an empty list prints no word)
            rows[key.strip()] = np.array([int(w, 16) for w in words.split()], dtype=np.uint64)
    dim, n = int(rows["dim"][0]), int(rows["n"][0])
    assert dim == 4 and n >= 3
    lst = lambda name, kind, i: (rows[f"{name} {kind} idx {i}"], rows[f"{name} {kind} vals {i}"].reshape(-1, 4))
    tab = lambda name, what, i, k: rows[f"{name} {what} {i}"].reshape(k, 4)
    def inst(wires, tabs, i, two):
        return K.Inst(lst(wires, "mul", i), lst(wires, "add", i), tab(tabs, "f2", i, 1 << dim), tab(tabs, "f3", i, 1 << dim), tab(tabs, "g", i, dim),
                      tab(tabs, "g2", i, dim) if two else None, tab(tabs, "coef", i, 2) if two else None)
    for p, (wires, tabs, two) in enumerate([("A", "A", True), ("B", "B", False), ("B", "A", True), ("A", "A", True)]):
        chal = rows[f"pass {p} challenges"].reshape(2 * dim, n, 4)
        want = K.walks([inst(wires, tabs, i, two) for i in range(n)], chal)
        got = rows[f"pass {p} messages"].reshape(2 * dim, n, 3, 4)
        for i in range(n):
            assert np.array_equal(got[:, i], want[i].msgs), f"pass {p}, instance {i}: the messages differ from the walk's"
            assert np.array_equal(rows[f"pass {p} final"].reshape(n, 3, 4)[i], want[i].final), f"pass {p}, instance {i}: finish's three values"
    assert np.array_equal(rows["pass 0 challenges"], rows["pass 3 challenges"]) and np.array_equal(rows["pass 0 messages"], rows["pass 3 messages"])
