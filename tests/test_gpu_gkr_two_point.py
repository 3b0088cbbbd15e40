"""GPU tests of the GKR batch handle's two-point form (sc_gkr_two_point_init_batch / sc_gkr_two_point_next_batch:
GKRRoundSumcheck.prover_init_batch(..., g2s, coeffs) and GKRBatchProverState.next_layer(..., g2s, coeffs)): alpha eq(g, .) + beta eq(g2, .)
stands where the one-point handle uses eq(g, .).  The oracle is the Walk2 of tests/gkr_two_point_cases.py (composed from oracle/cref.py)
under the same challenges: every message of every round of every instance, the tables after round calls {1, dim, dim + 1, 2 dim - 1},
(u, v) and finish's triple are compared bit for bit, on all three plans, and the plan counters are asserted.  Handles are built under
policy "batch" = 2 unless a case says otherwise."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib
from tests import gkr_two_point_cases as K
from tests import test_gpu_gkr_batch as T
from tests import test_gpu_gkr_batch_rounds as R
from tests import test_gpu_gkr_next_layer as NL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO = "batch.gkr_two_point"


def counters():
    p = _lib.plan_stats()
    return p[TWO], p[NL.NEXT], p["batch.gkr_rounds_one_block"], p["batch.gkr_rounds_slices"], p["batch.gkr_rounds_serial"]


def moved(before, two_point=0, next_layer=0, one_block=0, slices=0, serial=0):
    want = (before[0] + two_point, before[1] + next_layer, before[2] + one_block, before[3] + slices, before[4] + serial)
    assert counters() == want, "two_point / next_layer / one_block / slices / serial"


def objects(insts, dim, device="cuda:0"):
    """Walk2's instances -> NL.objects' dict, with the second points"""
    b = NL.objects([a[:5] for a in insts], dim, device)
    b["raw"], b["g2s"], b["coeffs"] = insts, [a[5] for a in insts], [a[6] for a in insts]
    return b


def init2(b, **pol):
    with _lib.policy(**({"batch": 2} if not pol else pol)):
        return sc.GKRRoundSumcheck.prover_init_batch(b["f1s"], b["f2s"], b["f3s"], b["gs"], g2s=b["g2s"], coeffs=b["coeffs"])


def onto2(st, b, keep_f1=False):
    st.next_layer(b["f2s"], b["f3s"], b["gs"], None if keep_f1 else b["f1s"], g2s=b["g2s"], coeffs=b["coeffs"])
    assert st.round == 0 and st.randomness(0).shape[0] == 0


def layer2(n, dim, seed, nnzs, variant="repeated"):
    return K.with_second(NL.raw_layer(n, dim, seed, nnzs, variant), K.second_points(n, dim, seed + 5))


def ragged(n, dim):
    """none at all, one, more than a stride per lane -- and for a lone instance three per cell"""
    N = 1 << dim
    return [3 * N] if n == 1 else [[0, 1, 3 * N, N // 2 + 1][i % 4] for i in range(n)]


# ---- 1. one block per instance -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _one_block_case(dim, n):
    """shared by the device and the host case of a shape: the walks depend on the seeds only"""
    insts = layer2(n, dim, 71000 + 97 * dim + n, ragged(n, dim))
    chal = R.challenges(n, dim, 71500 + dim + n, edge_instance=n // 2 if n > 1 else None)  # (a lone instance keeps random challenges: under 0 / 1 / p - 1 most of eq(u, .) is zero)
    chal.setflags(write=False)
    return insts, chal, K.walks2(insts, dim, chal, R.state_rounds(dim))


@pytest.mark.parametrize("device", ["cuda:0", None], ids=["device", "host"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("dim", [1, 2, 5, 9])
def test_one_block_every_round_equals_the_walk(dim, n, device):
    """dim 1: no high half (kh = 0); 2; 5: halves of different sizes; 9: eq(g2, .) fills the region of eq(u, .) and the LDS is full.
    Ragged lists with repeated indices, one of them empty"""
    insts, chal, want = _one_block_case(dim, n)
    b = objects(insts, dim, device)
    before = counters()
    st = init2(b)
    moved(before, two_point=1)
    R.drive(st, chal, want, R.state_rounds(dim))
    st.close()
    moved(before, two_point=1, one_block=2 * dim)


def test_one_wiring_for_all_instances_and_a_second_point_each_under_a_shared_challenge():
    dim, n = 5, 4
    N = 1 << dim
    idx, vals = T.make_f1(dim, 72000, "random", 3 * N)
    sec = K.second_points(n, dim, 72001)
    insts = [(idx, vals, cref.synth_table(72100 + i, 2, N), cref.synth_table(72100 + i, 3, N), cref.synth_table(72100 + i, 4, dim), sec[i][0], sec[i][1]) for i in range(n)]
    f1 = sc.SparseMultilinearExtension(3 * dim, NL.td(idx), NL.td(vals))
    b = {"f1s": [f1] * n, "f2s": [sc.DenseMultilinearExtension(dim, NL.td(a[2])) for a in insts], "f3s": [sc.DenseMultilinearExtension(dim, NL.td(a[3])) for a in insts],
         "gs": [a[4] for a in insts], "g2s": [a[5] for a in insts], "coeffs": [a[6] for a in insts]}
    torch.cuda.synchronize()
    chal = R.challenges(n, dim, 72002, edge_instance=None)
    same = np.repeat(chal[:, :1], n, axis=1)
    want = K.walks2(insts, dim, same, R.state_rounds(dim))
    assert any(not np.array_equal(want[0].msgs, w.msgs) for w in want[1:]), "the second points differ, so do the proofs"
    st = init2(b)
    shared = R.drive(st, chal, want, R.state_rounds(dim), shared=True, label="shared: ")
    st.reset()
    each = R.drive(st, same, want, label="n times, after a reset: ")
    st.close()
    for x, y in zip(shared, each):
        assert np.array_equal(x, y)


# ---- 2. the sliced plan --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n", [(10, 2), (11, 2), (13, 2), (16, 1)])
def test_the_sliced_plan_equals_the_walk(dim, n):
    """dim 10: only the initialisations are sliced; 11: the first sliced rounds; 13: kl = 7, kh = 6; 16: both halves full"""
    N = 1 << dim
    insts = layer2(n, dim, 73000 + dim, [N // 8] if n == 1 else [2 * N, N // 2 + 1])
    chal = R.challenges(n, dim, 73500 + dim, edge_instance=None)  # (random: under u from {0, 1, p - 1} phase two's table would be all but empty at these dims)
    want = K.walks2(insts, dim, chal, R.state_rounds(dim))
    assert all(w.f1gu.any() for w in want), "phase two has something to prove"
    b = objects(insts, dim)
    before = counters()
    st = init2(b, batch=2, batch_slices=1)
    R.drive(st, chal, want, R.state_rounds(dim))
    st.close()
    moved(before, two_point=1, slices=2 * dim)


def test_the_sliced_plan_with_every_term_of_an_instance_in_one_cell():
    """64 x 2^10 terms at dim 10, all with one x and one y: every term of either phase lands in ONE cell, the lanes' bound at its end"""
    dim, n = 10, 1
    N = 1 << dim
    nnz = 64 * N
    rng = np.random.default_rng(74000)
    z = rng.integers(0, N, size=nnz, dtype=np.uint64)
    idx = np.ascontiguousarray(z | np.uint64(777 << dim) | np.uint64(1001 << (2 * dim)))
    vals = cref.synth_table(74001, 1, nnz).copy()
    vals[::3] = K.MINUS_ONE  # the largest canonical pattern in a third of the terms
    sec = K.second_points(n, dim, 74002)
    insts = [(idx, vals, cref.synth_table(74003, 2, N), cref.synth_table(74003, 3, N), cref.synth_table(74003, 4, dim), sec[0][0], sec[0][1])]
    chal = R.challenges(n, dim, 74004, edge_instance=None)
    want = K.walks2(insts, dim, chal, R.state_rounds(dim))
    assert want[0].f1gu[1001].any() and not np.delete(want[0].f1gu, 1001, axis=0).any(), "phase two's one cell"
    before = counters()
    st = init2(objects(insts, dim), batch=2, batch_slices=1)
    R.drive(st, chal, want, R.state_rounds(dim))
    st.close()
    moved(before, two_point=1, slices=2 * dim)


# ---- 3. the serial plan --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n,pol,over", [(10, 2, {"batch": 2}, False), (4, 3, {"batch": 0}, False), (17, 1, {"batch": 2, "batch_slices": 1}, False),
                                            (10, 1, {"batch": 2, "batch_slices": 1}, True)], ids=["dim10-no-key", "dim4-batch0", "dim17", "dim10-nnz-over"])
def test_the_serial_plan_gives_the_same_bits(dim, n, pol, over):
    N = 1 << dim
    nnzs = [64 * N + 1] if over else ([N // 16] if dim == 17 else [2 * N, 0, N // 2 + 1][:n])
    insts = layer2(n, dim, 75000 + dim + int(over), nnzs)
    chal = R.challenges(n, dim, 75500 + dim, edge_instance=0 if dim == 4 else None)
    want = K.walks2(insts, dim, chal, R.state_rounds(dim))
    assert all(w.f1gu.any() for w in want if w.h.any()), "phase two has something to prove"
    before = counters()
    st = init2(objects(insts, dim), **pol)
    R.drive(st, chal, want, R.state_rounds(dim))
    st.reset()
    R.drive(st, chal, want, label="after a reset: ")
    st.close()
    moved(before, two_point=1, serial=2 * 2 * dim)


# ---- 4. values -----------------------------------------------------------------------------------------------------------------------
def _edge_point(dim, k):
    return np.stack([K.EDGE[(-1, 0, 1)[(j + k) % 3]] for j in range(dim)])


def test_coefficients_and_points_at_the_ends_of_the_field():
    """alpha, beta, g and g2 from {0, 1, p - 1}: alpha = 0, beta = 0, both zero (every message zero), all at the edge"""
    dim = 3
    N = 1 << dim
    base = NL.raw_layer(6, dim, 76000, [3 * N] * 6, "repeated")
    Z, ONE, M = K.ZERO, K.ONE, K.MINUS_ONE
    seconds = [(cref.synth_table(76001, 5, dim), np.stack([Z, ONE])), (cref.synth_table(76002, 5, dim), np.stack([M, Z])), (cref.synth_table(76003, 5, dim), np.stack([Z, Z])),
               (_edge_point(dim, 0), np.stack([M, M])), (_edge_point(dim, 1), np.stack([ONE, M])), (_edge_point(dim, 2), np.stack([ONE, ONE]))]
    insts = K.with_second(base, seconds)
    for i in (3, 4):
        insts[i] = insts[i][:4] + (_edge_point(dim, i),) + insts[i][5:]  # g at the edge as well
    n = len(insts)
    chal = R.challenges(n, dim, 76004)
    want = K.walks2(insts, dim, chal, R.state_rounds(dim))
    assert not want[2].msgs.any() and not want[2].final[0].any(), "alpha = beta = 0: a proof of zero"
    one_point_at_g2 = R.Walk(insts[0][:4] + (insts[0][5],), dim, np.ascontiguousarray(chal[:, 0]))
    assert np.array_equal(want[0].msgs, one_point_at_g2.msgs), "(0, 1): the one-point proof at g2"
    st = init2(objects(insts, dim))
    R.drive(st, chal, want, R.state_rounds(dim))
    st.close()


def test_g2_equal_to_g_is_alpha_plus_beta_times_the_one_point_proof():
    dim, n = 4, 3
    N = 1 << dim
    base = NL.raw_layer(n, dim, 77000, [2 * N, 0, N + 1], "repeated")
    coefs = cref.synth_table(77001, 6, 2 * n).reshape(n, 2, 4)
    insts = [a + (a[4], coefs[i]) for i, a in enumerate(base)]
    chal = R.challenges(n, dim, 77002)
    st = init2(objects(insts, dim))
    msgs, _, fin = R.drive(st, chal, K.walks2(insts, dim, chal))
    st.close()
    for i, w in enumerate(R.walks(base, dim, chal)):
        s = cref.fr_binop("add", coefs[i, 0], coefs[i, 1])
        assert np.array_equal(msgs[i].reshape(-1, 4), K.combine(s, w.msgs.reshape(-1, 4), K.ZERO, w.msgs.reshape(-1, 4))), f"instance {i}: (alpha + beta) x the one-point messages"
        assert np.array_equal(fin[i, 0], cref.fr_binop("mul", s, w.final[0])) and np.array_equal(fin[i, 1:], w.final[1:]), f"instance {i}: finish's triple"


@pytest.mark.parametrize("dim,pol", [(4, {"batch": 2}), (10, {"batch": 2, "batch_slices": 1}), (4, {"batch": 0})], ids=["one_block", "slices", "serial"])
def test_one_and_zero_give_the_one_point_handles_bits_on_every_plan(dim, pol):
    """(alpha, beta) = (1, 0) with an arbitrary g2: messages, tables and triple of the one-point handle, bit for bit"""
    n = 2
    N = 1 << dim
    base = NL.raw_layer(n, dim, 78000 + dim, [2 * N, N // 2 + 1], "repeated")
    insts = K.with_second(base, [(cref.synth_table(78001 + i, 5, dim), np.stack([K.ONE, K.ZERO])) for i in range(n)])
    chal = R.challenges(n, dim, 78002 + dim)
    want = R.walks(base, dim, chal, R.state_rounds(dim))  # the ONE-point oracle
    one = NL.init(NL.objects(base, dim), **pol)
    a = R.drive(one, chal, want, R.state_rounds(dim), label="one-point handle: ")
    one.close()
    two = init2(objects(insts, dim), **pol)
    b = R.drive(two, chal, want, R.state_rounds(dim), label="two-point handle under (1, 0): ")
    two.close()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ---- 5. forms on one handle ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _forms_case():
    dim, n = 4, 3
    N = 1 << dim
    A, B = layer2(n, dim, 79000, [2 * N, 3 * N, N]), layer2(n, dim, 79500, [0, N, N // 2])
    same_wiring = [A[i][:2] + B[i][2:] for i in range(n)]  # B's values, points and coefficients under A's wiring
    ca, cb = R.challenges(n, dim, 79001, edge_instance=1), R.challenges(n, dim, 79002)
    for c in (ca, cb):
        c.setflags(write=False)
    return dim, n, A, B, same_wiring, ca, cb


@pytest.mark.parametrize("pol", [{"batch": 2}, {"batch": 0}], ids=["one_block", "serial"])
def test_a_handle_built_in_one_point_form_changes_form_layer_by_layer(pol):
    dim, n, A, B, same_wiring, ca, cb = _forms_case()
    states = R.state_rounds(dim)
    one_a = [a[:5] for a in A]
    a, b, kept = objects(A, dim), objects(B, dim), objects(same_wiring, dim)
    st = NL.init(a, **pol)
    before = counters()
    R.drive(st, ca, R.walks(one_a, dim, ca, states), states, label="built one-point: ")
    onto2(st, b)
    R.drive(st, cb, K.walks2(B, dim, cb, states), states, label="a two-point layer: ")
    NL.onto(st, a)
    R.drive(st, ca, R.walks(one_a, dim, ca, states), states, label="a one-point layer: ")
    onto2(st, kept, keep_f1=True)
    R.drive(st, cb, K.walks2(same_wiring, dim, cb, states), states, label="a two-point layer, wiring kept: ")
    st.close()
    areas = pol["batch"] != 0
    moved(before, two_point=2, next_layer=3 if areas else 0, one_block=4 * 2 * dim if areas else 0, serial=0 if areas else 4 * 2 * dim)


def test_a_handle_built_in_two_point_form_gives_the_same_bits_after_a_reset_and_returns_to_one_point_form():
    dim, n, A, B, same_wiring, ca, cb = _forms_case()
    states = R.state_rounds(dim)
    a = objects(A, dim)
    want = K.walks2(A, dim, ca, states)
    st = init2(a)
    first = R.drive(st, ca, want, states)
    st.reset()
    again = R.drive(st, ca, want, states, label="after a reset: ")
    for x, y in zip(first, again):
        assert np.array_equal(x, y)
    before = counters()
    NL.onto(st, a)  # sc_gkr_layer_next_batch on a handle in two-point form: the one-point form over the same arrays
    R.drive(st, ca, R.walks([x[:5] for x in A], dim, ca, states), states, label="back in one-point form: ")
    st.close()
    moved(before, next_layer=1, one_block=2 * dim)


def test_refused_calls_in_the_middle_of_phase_two_leave_the_proof_where_it_was():
    dim, n, A, B, same_wiring, ca, cb = _forms_case()
    a, b = objects(A, dim), objects(B, dim)
    want = K.walks2(A, dim, ca, R.state_rounds(dim))
    st = init2(a)
    upto = dim + 2
    for t in range(upto):
        assert np.array_equal(st.prove_round(None if t == 0 else ca[t - 1]), np.stack([w.msgs[t] for w in want]))
    before = counters()
    coeffs = [c.copy() for c in b["coeffs"]]
    coeffs[1][1] = R.P_LIMBS  # beta of instance 1 is p itself
    assert R._raises(_lib.SC_ERR_BAD_ARG, st.next_layer, b["f2s"], b["f3s"], b["gs"], b["f1s"], g2s=b["g2s"], coeffs=coeffs) == "instance 1: coefficient is not canonical"
    g2s = [g.copy() for g in b["g2s"]]
    g2s[2][dim - 1] = R.P_LIMBS
    g2s[1][0] = R.P_LIMBS  # the lowest failing instance decides
    assert R._raises(_lib.SC_ERR_BAD_ARG, st.next_layer, b["f2s"], b["f3s"], b["gs"], b["f1s"], g2s=g2s, coeffs=b["coeffs"]) == "instance 1: g2 is not canonical"
    ptrs = lambda vals: (C.c_void_p * n)(*[C.cast(v, C.c_void_p) for v in vals])
    keep = [np.ascontiguousarray(g) for g in b["gs"]] + [np.ascontiguousarray(g) for g in b["g2s"]]
    args = [ptrs([C.c_void_p(m.data_ptr()) for m in b["f2s"]]), ptrs([C.c_void_p(m.data_ptr()) for m in b["f3s"]]), ptrs([g.ctypes.data for g in keep[:n]]),
            ptrs([g.ctypes.data for g in keep[n:]])]
    assert sc.lib().sc_gkr_two_point_next_batch(st._h, None, None, None, *args, None, _lib.SC_TABLES_ON_DEVICE) == _lib.SC_ERR_BAD_ARG  # a null coef
    assert "null" in sc.lib().sc_last_error().decode()
    with pytest.raises(ValueError):
        st.next_layer(b["f2s"], b["f3s"], b["gs"], b["f1s"], g2s=b["g2s"])
    moved(before)
    assert st.round == upto
    for t in range(upto, 2 * dim):
        assert np.array_equal(st.prove_round(ca[t - 1]), np.stack([w.msgs[t] for w in want])), f"round call {t} after the refused calls"
        if t + 1 in R.state_rounds(dim):
            for i in range(n):
                assert np.array_equal(st.tables(i), want[i].states[t + 1]), (t, i)
    uv, fin = st.finish(ca[2 * dim - 1])
    for i in range(n):
        assert np.array_equal(uv[i].reshape(2 * dim, 4), ca[:, i]) and np.array_equal(fin[i], want[i].final), i
    onto2(st, b)  # and the handle still takes a good layer
    R.drive(st, cb, K.walks2(B, dim, cb), label="layer B after the refused calls: ")
    st.close()
    moved(before, two_point=1, next_layer=1, one_block=(2 * dim - upto) + 2 * dim)


# ---- 6. the verifier's helper --------------------------------------------------------------------------------------------------------
def test_the_verifiers_helper_accepts_the_provers_triple_and_rejects_one_flipped_bit():
    dim, n, A, B, same_wiring, ca, cb = _forms_case()
    a = objects(A, dim)
    st = init2(a)
    _, uv, fin = R.drive(st, ca, K.walks2(A, dim, ca))
    st.close()
    claims = [sc.GKRRoundSumcheckSubClaim(uv[i, 0], uv[i, 1], cref.fr_binop("mul", fin[i, 0], fin[i, 2])) for i in range(n)]
    args = (a["f1s"], a["f2s"], a["f3s"], a["gs"], a["g2s"], a["coeffs"])
    assert sc.GKRRoundSumcheckSubClaim.verify_subclaim_two_point_batch(claims, *args) == [True] * n
    assert claims[0].verify_subclaim_two_point(a["f1s"][0], a["f2s"][0], a["f3s"][0], a["gs"][0], a["g2s"][0], a["coeffs"][0][0], a["coeffs"][0][1])
    claims[1].expected_evaluation = claims[1].expected_evaluation ^ np.array([0, 0, 1, 0], dtype=np.uint64)
    assert sc.GKRRoundSumcheckSubClaim.verify_subclaim_two_point_batch(claims, *args) == [True, False, True]
    assert sc.GKRRoundSumcheckSubClaim.verify_subclaim_batch(claims[:1], a["f1s"][:1], a["f2s"][:1], a["f3s"][:1], a["gs"][:1]) == [False], "not a one-point claim"


# ---- 7. the C++ mirror ---------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_two_point():
    """the overloads of include/sumcheck_amd.hpp: a program proves layer A in two-point form, layer B in two-point form, layer A in
    one-point form and layer A in two-point form again on one handle at dim 4, checks the verifier's helper, and prints its inputs, its
    challenges and every message; the messages are compared with the walks over what it printed"""
    from tests import test_cpp_mirror as M
    src = os.path.join(ROOT, "tests", "cpp", "test_gkr_two_point_mirror.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "test_gkr_two_point_mirror.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, "-o", out, "-L", M.LIBDIR, "-lsumcheck_hip", f"-Wl,-rpath,{M.LIBDIR}",
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-2000:] + r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        key, colon, words = line.partition(":")
        if colon:  # (an empty list prints no word)
            rows[key.strip()] = np.array([int(w, 16) for w in words.split()], dtype=np.uint64)
    dim, n = int(rows["dim"][0]), int(rows["n"][0])
    assert dim == 4 and n >= 2
    layers = {}
    for name in "AB":
        layers[name] = [(rows[f"{name} idx {i}"], rows[f"{name} vals {i}"].reshape(-1, 4), rows[f"{name} f2 {i}"].reshape(-1, 4), rows[f"{name} f3 {i}"].reshape(-1, 4),
                         rows[f"{name} g {i}"].reshape(dim, 4), rows[f"{name} g2 {i}"].reshape(dim, 4), rows[f"{name} coef {i}"].reshape(2, 4)) for i in range(n)]
    for p, (name, two) in enumerate([("A", True), ("B", True), ("A", False), ("A", True)]):
        chal = rows[f"pass {p} challenges"].reshape(2 * dim, n, 4)
        want = K.walks2(layers[name], dim, chal) if two else R.walks([a[:5] for a in layers[name]], dim, chal)
        got = rows[f"pass {p} messages"].reshape(2 * dim, n, 3, 4)
        for i in range(n):
            assert np.array_equal(got[:, i], want[i].msgs), f"pass {p} (layer {name}), instance {i}: the messages differ from the walk's"
            assert np.array_equal(rows[f"pass {p} final"].reshape(n, 3, 4)[i], want[i].final), f"pass {p} (layer {name}), instance {i}: finish's triple"
    assert np.array_equal(rows["pass 0 challenges"], rows["pass 3 challenges"]) and np.array_equal(rows["pass 0 messages"], rows["pass 3 messages"])
