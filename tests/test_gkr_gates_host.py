"""CPU tests of the GKR batch handle's gate form (sc_gkr_gates_init_batch / sc_gkr_gates_next_batch): the oracle of tests/gkr_gates_cases.py
against the definition in big integers (the sums over the hypercube) and against the sum of the three multiplication-only instances' walks;
the identities the protocol rests on; the two prototypes under their own marker SC_API_GKRG against the shim's declarations and the ctypes
table; the older scanners, none of which may see the names; the wrappers of every mirror; the policy key and the plans' names; the argument
errors that need no device.  The values the library computes are tests/test_gpu_gkr_gates.py's."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib
from tests import gkr_gates_cases as K
from tests import gkr_two_point_cases as K2
from tests import test_gkr_batch_rounds_host as GR
from tests import test_gkr_next_layer_host as NH
from tests import test_gkr_two_point_host as TP
from tests import test_rust_shim as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = cref.P
HDR = open(os.path.join(ROOT, "include", "sumcheck_hip.h")).read()
PP = "*const *const u64"
PARAMS = {K.INIT: ["u32", "u32", PP, PP, "*const u64", PP, PP, "*const u64", PP, PP, PP, PP, "*const u64", "u32", "*mut *mut sc_gkr_batch_prover"],
          K.NEXT: ["*mut sc_gkr_batch_prover", PP, PP, "*const u64", PP, PP, "*const u64", PP, PP, PP, PP, "*const u64", "u32"],
          K.EVAL: ["u32", "u32", "u32", PP, PP, "*const u64", PP, PP, "*const u64", PP, PP, "u32", "*const *mut u64"]}
NAMES = (K.INIT, K.NEXT, K.EVAL)
P_LIMBS = np.array([(P >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], dtype=np.uint64)
ints = lambda a: cref.mont_to_ints(np.asarray(a))


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_point", [False, True], ids=["one-point", "two-point"])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_the_builders_equal_the_definition_in_big_integers(dim, two_point):
    """H1, H2, T1, T2 as sums over the lists' entries with E, eq(u, .) and f2(u) computed from their definitions (repeated indices add up)"""
    N = 1 << dim
    inst = K.instance(dim, 71000 + dim, 3 * N, 2 * N + 1, two_point)
    assert len(set(int(i) for i in inst.mul_idx)) < len(inst.mul_idx), "a repeated index"
    chal = K.challenges(1, dim, 71100 + dim)[:, 0]
    w = K.WalkG(inst, chal)
    h1, h2 = K.define_tables(inst)
    t1, t2 = K.define_tables(inst, ints(chal[:dim]))
    assert ints(w.H1) == h1 and ints(w.H2) == h2 and ints(w.T1) == t1 and ints(w.T2) == t2
    assert any(h1) and any(h2) and any(t1) and any(t2)


@pytest.mark.parametrize("two_point", [False, True], ids=["one-point", "two-point"])
@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_the_identities_the_protocol_rests_on(dim, two_point):
    N = 1 << dim
    inst = K.instance(dim, 72000 + dim, 2 * N, 3 * N, two_point)
    chal = K.challenges(1, dim, 72100 + dim)[:, 0]
    w = K.WalkG(inst, chal)
    m = [[ints(e)[0] for e in msg] for msg in w.msgs]
    # P_0(0) + P_0(1) = alpha W_out(g) + beta W_out(g2)
    w_out = K.define_layer(inst)
    claim = sum((1 if wt is None else ints(wt)[0]) * K.extension(w_out, ints(pt), dim) for wt, pt in inst.points()) % P
    assert (m[0][0] + m[0][1]) % P == claim
    # phase one's last message at u_last is phase two's claim
    at = lambda msg, r: ints(cref.interpolate_uni_poly(msg, r))[0]
    assert at(w.msgs[dim - 1], chal[dim - 1]) == (m[dim][0] + m[dim][1]) % P
    # phase two's last message at v_last is M f2(u) f3(v) + A (f2(u) + f3(v)), and it is the third final value
    E, equ, eqv = K.weights_int(inst), K.eq_table(ints(chal[:dim]), dim), K.eq_table(ints(chal[dim:]), dim)
    M = K.list_extension(inst.mul_idx, inst.mul_vals, dim, E, equ, eqv)
    A = K.list_extension(inst.add_idx, inst.add_vals, dim, E, equ, eqv)
    f2u, f3v = K.extension(ints(inst.f2), ints(chal[:dim]), dim), K.extension(ints(inst.f3), ints(chal[dim:]), dim)
    last = at(w.msgs[2 * dim - 1], chal[2 * dim - 1])
    assert last == (M * f2u * f3v + A * (f2u + f3v)) % P
    assert ints(w.final) == [f2u, f3v, last]
    # every round is consistent with the one before it
    for t in range(1, 2 * dim):
        assert (m[t][0] + m[t][1]) % P == at(w.msgs[t - 1], chal[t - 1]), t


@pytest.mark.parametrize("two_point", [False, True], ids=["one-point", "two-point"])
@pytest.mark.parametrize("dim", [1, 2, 4])
def test_every_message_is_the_sum_of_the_three_multiplication_only_instances(dim, two_point):
    """(MUL, f2, f3), (ADD, f2, 1), (ADD, 1, f3) under the same challenges -- what the composed plan computes; and the final values it forms:
    f2(u) = a1, f3(v) = c2, a0 a2 + b0 b2 + c0 c2"""
    N = 1 << dim
    inst = K.instance(dim, 73000 + dim, 3 * N, 2 * N, two_point)
    chal = K.challenges(1, dim, 73100 + dim)[:, 0]
    w = K.WalkG(inst, chal)
    a, b, c = (K2.Walk2(t, dim, chal) for t in inst.three())
    assert np.array_equal(w.msgs.reshape(-1, 4), K.add(K.add(a.msgs.reshape(-1, 4), b.msgs.reshape(-1, 4)), c.msgs.reshape(-1, 4)))
    third = K.add(K.add(K.mul(a.final[0], a.final[2]), K.mul(b.final[0], b.final[2])), K.mul(c.final[0], c.final[2]))[0]
    assert np.array_equal(w.final, np.stack([a.final[1], c.final[2], third]))
    assert np.array_equal(c.final[1], K.ONE), "the table of ones at u"


@pytest.mark.parametrize("mul_nnz,add_nnz", [(9, 0), (0, 9), (0, 0)], ids=["no-add", "no-mul", "neither"])
def test_an_empty_list_on_either_side(mul_nnz, add_nnz):
    """no ADD list: H2 = T2 = 0 and the messages are the multiplication-only walk's; no MUL list: H1 = sum_ADD E v; neither: all zero"""
    dim = 2
    inst = K.instance(dim, 74000 + mul_nnz, mul_nnz, add_nnz, True)
    chal = K.challenges(1, dim, 74100)[:, 0]
    w = K.WalkG(inst, chal)
    h1, h2 = K.define_tables(inst)
    assert ints(w.H1) == h1 and ints(w.H2) == h2
    if add_nnz == 0:
        assert not w.H2.any() and not w.T2.any()
        a = K2.Walk2(inst.three()[0], dim, chal)
        assert np.array_equal(w.msgs, a.msgs)
        assert np.array_equal(w.final[0], a.final[1]) and np.array_equal(w.final[2], K.mul(a.final[0], a.final[2])[0])
    if mul_nnz == 0 and add_nnz:
        assert w.H1.any() and w.H2.any()
    if mul_nnz == 0 and add_nnz == 0:
        assert not w.msgs.any() and not w.final[2].any()


def test_the_one_cell_case_is_as_full_as_its_docstring_says():
    inst = K.one_cell_instance(3, 64 << 3, 5)
    assert len(set(int(i) for i in inst.mul_idx)) == 1 and len(inst.mul_idx) == len(inst.add_idx) == 64 << 3
    i, N = int(inst.mul_idx[0]), 8
    assert i & (N - 1) == (i >> 3) & (N - 1) == (i >> 6) & (N - 1)
    assert K.one_block_fits(9, 64 << 9, 64 << 9) and not K.one_block_fits(9, (64 << 9) + 1, 0) and not K.one_block_fits(9, 0, (64 << 9) + 1) and not K.one_block_fits(10, 1, 1)
    assert 2 * (64 << 9) * (1 << 32) < 1 << 63


# ---- the prototypes ------------------------------------------------------------------------------------------------------------------
def _header_prototypes():
    """the SC_API_GKRG prototypes, parameter types in the shim's spelling (tests/test_gkr_two_point_host.py's reading)"""
    old = dict(RS.C_BASE)
    RS.C_BASE["sc_gkr_batch_prover"] = "sc_gkr_batch_prover"
    try:
        protos = {}
        for m in re.finditer(r"SC_API_GKRG\s+([^;(]+?)\b(sc_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", HDR, re.S):
            ret, name, params = m.group(1).strip(), m.group(2), " ".join(m.group(3).split())
            plist = [RS.c_type_to_rust(re.match(r"(.*?)([A-Za-z_][A-Za-z_0-9]*)$", prm.strip()).group(1)) for prm in params.split(",")]
            protos[name] = (plist, None if ret == "void" else RS.c_type_to_rust(ret))
        return protos
    finally:
        RS.C_BASE.clear()
        RS.C_BASE.update(old)


def test_the_symbols_are_declared_exported_and_in_their_own_signature_table():
    protos = _header_prototypes()
    assert set(protos) == set(NAMES) == set(_lib.SIGNATURES_GKRG)
    assert re.search(r"#define SC_API_GKRG SC_API /\*[^\n]*\*/\n", HDR), "SC_API with only a comment behind it on the line"
    version_line = HDR.split("#define SC_ABI_VERSION 5", 1)[1].split("\n", 1)[0]
    so = C.CDLL(_lib.SO_PATH)
    for name in NAMES:
        assert protos[name] == (PARAMS[name], "c_int")
        assert name in version_line and hasattr(so, name)
        res, args = _lib.SIGNATURES_GKRG[name]
        assert res is C.c_int and len(args) == len(PARAMS[name])
        assert all(name not in table for table in (_lib.SIGNATURES, _lib.SIGNATURES_EXT, _lib.SIGNATURES_GKRB, _lib.SIGNATURES_GKRL, _lib.SIGNATURES_GKR2, _lib.SIGNATURES_GKRE))
    assert sc.lib().sc_abi_version() == 5


def test_none_of_the_older_scanners_sees_the_names_and_their_closed_sets_hold():
    for marker in ("SC_API", "SC_API_EXT", "SC_API_GKRB", "SC_API_GKRL", "SC_API_GKR2", "SC_API_GKRE"):
        names = [m.group(2) for m in re.finditer(marker + r"\s+([^;(]+?)\b(sc_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", HDR, re.S)]
        assert names and not set(names) & set(NAMES), marker
    assert set(GR._header_prototypes()) == set(GR.NAMES)
    assert set(NH._header_prototypes()) == {NH.NAME} == set(_lib.SIGNATURES_GKRL)
    assert set(TP._header_prototypes()) == {TP.INIT, TP.NEXT} == set(_lib.SIGNATURES_GKR2)
    rs = open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()
    for name in NAMES:
        assert not re.search(r"pub\s+fn\s+" + name + r"\b", rs), "a private declaration: the shim's pub externs are SC_API prototypes"


def test_the_shim_declares_them_as_the_header_does_and_wraps_them():
    rs = open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()
    protos = _header_prototypes()
    for name in NAMES:
        found = []
        for block in re.findall(r'extern "C" \{(.*?)\n\}', rs, re.S):
            for m in re.finditer(r"\bfn (" + name + r")\s*\((.*?)\)\s*(?:->\s*([^;]+?))?\s*;", block, re.S):
                assert len(re.findall(r"\bfn\s+sc_", block)) == 1, "a block of its own"
                params = " ".join(m.group(2).split())
                found.append(([p.split(":", 1)[1].strip() for p in params.split(",") if p.strip()], m.group(3).strip() if m.group(3) else None))
        assert found == [protos[name]], (name, found)
    assert re.search(r"pub fn gkr_prover_init_batch_gates<F: Limbs4>\(", rs) and re.search(r"pub fn gkr_next_layer_batch_gates<F: Limbs4>\(", rs) and re.search(r"pub fn gkr_evaluate_layers_batch_gates<F: Limbs4>\(", rs)


def test_every_mirror_wraps_them_and_the_documents_name_them():
    hpp = open(os.path.join(ROOT, "include", "sumcheck_amd.hpp")).read()
    assert K.INIT in hpp and K.NEXT in hpp and "prover_init_batch_gates(" in hpp and "next_layer_gates(" in hpp and "verify_subclaim_gates_batch(" in hpp
    assert K.EVAL in hpp and "evaluate_layers_batch_gates(" in hpp
    assert list(inspect.signature(sc.GKRRoundSumcheck.evaluate_layers_batch_gates).parameters) == ["mul_layers", "add_layers", "f2s", "f3s"]
    assert list(inspect.signature(sc.GKRRoundSumcheck.prover_init_batch_gates).parameters) == ["mul_f1s", "add_f1s", "f2s", "f3s", "gs", "g2s", "coeffs"]
    assert {"mul_f1s", "add_f1s", "g2s", "coeffs"} <= set(inspect.signature(sc.GKRBatchProverState.next_layer_gates).parameters)
    assert callable(sc.GKRRoundSumcheckSubClaim.verify_subclaim_gates) and callable(sc.GKRRoundSumcheckSubClaim.verify_subclaim_gates_batch)
    for doc in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert K.INIT in text and K.EVAL in text and all(p in text for p in (K.ONE_BLOCK, K.COMPOSED, K.EVAL_ONE_BLOCK, K.EVAL_CELLS)), doc
    from sumcheck_amd import build
    assert "kernels_batch_gkr_gates.hip" in build.SOURCES and "gkr_gates.hip" in build.SOURCES


# ---- the policy key and the plans -------------------------------------------------------------------------------------------------------
def test_the_policy_key_defaults_to_one_and_takes_zero_and_one():
    assert _lib.get_policy("gkr_gates_fused") == 1
    try:
        _lib.set_policy("gkr_gates_fused", 0)
        assert _lib.get_policy("gkr_gates_fused") == 0
        with pytest.raises(_lib.SumcheckError) as e:
            _lib.set_policy("gkr_gates_fused", 2)
        assert e.value.code == _lib.SC_ERR_BAD_ARG and e.value.msg == "policy gkr_gates_fused takes 0..1"
    finally:
        _lib.set_policy("gkr_gates_fused", 1)
    assert '"gkr_gates_fused" (1)' in HDR


def test_the_plans_are_named_side_by_side_and_every_position_test_still_holds():
    names = list(_lib.plan_stats())
    assert len(names) == sc.lib().sc_plan_count() and K.ONE_BLOCK in HDR and K.COMPOSED in HDR
    assert [names.index(p) - names.index(K.ONE_BLOCK) for p in (K.COMPOSED, K.EVAL_ONE_BLOCK, K.EVAL_CELLS)] == [1, 2, 3]
    assert K.EVAL_ONE_BLOCK in HDR and K.EVAL_CELLS in HDR
    TP.test_the_plan_is_named_and_every_position_test_still_holds()


# ---- argument errors that need no device -----------------------------------------------------------------------------------------------
def _ptrs(arrs):
    return (C.c_void_p * len(arrs))(*[None if a is None else a.ctypes.data for a in arrs])


def _init_status(insts, dim, drop=None, mixture=None):
    """sc_gkr_gates_init_batch over host arrays -> (status, message); drop: an argument position to pass as NULL"""
    n = len(insts)
    keep = [np.ascontiguousarray(np.stack([i.coef for i in insts]))] if insts and insts[0].coef is not None else [None]
    args = [n, dim, _ptrs([i.mul_idx if len(i.mul_idx) else None for i in insts]), _ptrs([i.mul_vals if len(i.mul_idx) else None for i in insts]),
            (C.c_uint64 * max(n, 1))(*[len(i.mul_idx) for i in insts]), _ptrs([i.add_idx if len(i.add_idx) else None for i in insts]),
            _ptrs([i.add_vals if len(i.add_idx) else None for i in insts]), (C.c_uint64 * max(n, 1))(*[len(i.add_idx) for i in insts]), _ptrs([i.f2 for i in insts]),
            _ptrs([i.f3 for i in insts]), _ptrs([i.g for i in insts]), None if keep[0] is None else _ptrs([i.g2 for i in insts]), None if keep[0] is None else keep[0].ctypes.data]
    if drop is not None:
        args[drop] = None
    if mixture == "g2":
        args[12] = None
    if mixture == "coef":
        args[11] = None
    h = C.c_void_p()
    rc = sc.lib().sc_gkr_gates_init_batch(*args, 0, C.byref(h))
    msg = sc.lib().sc_last_error().decode()
    assert bool(h.value) == (rc == _lib.SC_OK), "a handle exactly on success"
    if h.value:
        sc.lib().sc_gkr_batch_prover_free(h)
    return rc, msg


def test_the_checks_run_before_any_device_call_and_name_the_list():
    n, dim = 3, 2
    good = K.instances(n, dim, 75000, 5, 4, True)
    for pos in (2, 3, 4, 5, 6, 7, 8, 9, 10):
        assert _init_status(good, dim, drop=pos) == (_lib.SC_ERR_BAD_ARG, "null argument"), pos
    for which in ("g2", "coef"):
        rc, msg = _init_status(good, dim, mixture=which)
        assert rc == _lib.SC_ERR_BAD_ARG and "come together" in msg
    assert _init_status([], dim)[0] == _lib.SC_ERR_BAD_ARG and "n == 0" in sc.lib().sc_last_error().decode()
    assert _init_status(good, 0)[0] == _lib.SC_ERR_CONSTANT_POLY
    assert _init_status(good, 22)[0] == _lib.SC_ERR_BAD_ARG
    bad = K.instances(n, dim, 75000, 5, 4, True)
    bad[2].add_idx[3] = np.uint64(1) << np.uint64(3 * dim)
    assert _init_status(bad, dim) == (_lib.SC_ERR_BAD_ARG, "instance 2: add index 3 out of range")
    bad[1].mul_idx[4] = np.uint64(1) << np.uint64(63)
    assert _init_status(bad, dim) == (_lib.SC_ERR_BAD_ARG, "instance 1: mul index 4 out of range"), "the lowest failing instance decides"
    bad[1].add_idx[0] = np.uint64(1) << np.uint64(3 * dim)
    assert _init_status(bad, dim) == (_lib.SC_ERR_BAD_ARG, "instance 1: mul index 4 out of range"), "mul is checked before add"
    bad = K.instances(n, dim, 75000, 5, 4, True)
    bad[1].g2[1] = P_LIMBS
    assert _init_status(bad, dim) == (_lib.SC_ERR_BAD_ARG, "instance 1: g2 is not canonical")
    bad[0].coef[1] = P_LIMBS
    assert _init_status(bad, dim) == (_lib.SC_ERR_BAD_ARG, "instance 0: coefficient is not canonical")
    bad[0].g[0] = P_LIMBS
    rc, msg = _init_status(bad, dim)
    assert rc == _lib.SC_ERR_BAD_ARG and msg.startswith("instance 0: g[0]")
    empty = K.instances(n, dim, 75100, 0, 0, False)  # (lists with nnz == 0 have null pointers)
    for insts in (good, empty):
        rc, msg = _init_status(insts, dim)  # good arguments get as far as the device: no CPU fallback
        assert rc == _lib.SC_OK or (rc == _lib.SC_ERR_HIP and "no HIP device" in msg)


def test_the_layer_evaluations_checks_run_before_any_device_call_and_name_the_list():
    """host arrays: the definition's layers as outputs would need a device; the refusals do not"""
    dim, n, n_layers = 2, 2, 2
    N = 1 << dim
    total = n * n_layers
    lists = [[K.wiring(dim, 77000 + 10 * q + r, 5 + r) for r in range(total)] for q in range(2)]
    f2, f3 = [cref.synth_table(77100 + i, 2, N) for i in range(n)], [cref.synth_table(77100 + i, 3, N) for i in range(n)]
    outs = [np.zeros((N, 4), np.uint64) for _ in range(total)]

    def status(lists, outs=outs, drop=None, n_=n):
        args = [n_, dim, n_layers]
        for q in range(2):
            args += [_ptrs([l[0] for l in lists[q]]), _ptrs([l[1] for l in lists[q]]), (C.c_uint64 * total)(*[len(l[0]) for l in lists[q]])]
        args += [_ptrs(f2), _ptrs(f3), 0, _ptrs(outs)]
        if drop is not None:
            args[drop] = None
        rc = sc.lib().sc_gkr_gates_layers_eval_batch(*args)
        return rc, sc.lib().sc_last_error().decode()

    assert status(lists, n_=0)[0] == _lib.SC_OK
    for pos in (3, 4, 5, 6, 7, 8, 9, 10, 12):
        assert status(lists, drop=pos) == (_lib.SC_ERR_BAD_ARG, "layer 0 instance 0: null argument"), pos
    bad = [[(l[0].copy(), l[1]) for l in lists[q]] for q in range(2)]
    bad[1][3][0][2] = np.uint64(1) << np.uint64(3 * dim)
    assert status(bad) == (_lib.SC_ERR_BAD_ARG, "layer 1 instance 1: add has an index out of range")
    bad[0][3][0][0] = np.uint64(1) << np.uint64(40)
    assert status(bad) == (_lib.SC_ERR_BAD_ARG, "layer 1 instance 1: mul has an index out of range"), "mul is checked before add"
    assert status(lists, outs=outs[:3] + [lists[1][0][1]]) == (_lib.SC_ERR_BAD_ARG, "layer 1 instance 1: the output overlaps an input"), "an ADD list is an input"
    rc, msg = status(lists)
    assert rc == _lib.SC_OK or (rc == _lib.SC_ERR_HIP and "no HIP device" in msg)


def test_a_null_handle_is_a_bad_argument_and_the_python_arguments_come_together():
    assert sc.lib().sc_gkr_gates_next_batch(None, None, None, None, None, None, None, None, None, None, None, None, 0) == _lib.SC_ERR_BAD_ARG
    assert "null" in sc.lib().sc_last_error().decode()
    st = sc.GKRBatchProverState(C.c_void_p(), 1, 2)
    g = cref.synth_table(76000, 4, 2)
    with pytest.raises(ValueError):
        st.next_layer_gates([None], [None], [g], mul_f1s=[None])
    with pytest.raises(ValueError):
        st.next_layer_gates([None], [None], [g], g2s=[g])
    with pytest.raises(ValueError):
        sc.GKRRoundSumcheck.prover_init_batch_gates([], [], [], [], [], coeffs=[])


# ---- the C++ mirror ------------------------------------------------------------------------------------------------------------------
def build_gates_mirror():
    from tests import test_cpp_mirror as M
    src = os.path.join(ROOT, "tests", "cpp", "test_gkr_gates_mirror.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "test_gkr_gates_mirror.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", out, "-L", M.LIBDIR, "-lsumcheck_hip", f"-Wl,-rpath,{M.LIBDIR}",
                           "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_the_cpp_mirror_compiles_and_gets_as_far_as_the_device():
    """the program prints its inputs and then either proves (a GPU is present) or reports the library's "no CPU fallback" """
    r = subprocess.run([build_gates_mirror()], capture_output=True, text=True, timeout=600)
    assert r.returncode in (0, 3), r.stdout[-2000:] + r.stderr
    assert "A mul idx 0:" in r.stdout and "B add vals 2:" in r.stdout and ("DONE" in r.stdout or "no CPU fallback" in r.stdout)


# ---- the kernels' resources ------------------------------------------------------------------------------------------------------------
def test_the_new_kernel_uses_no_scratch_and_the_existing_kernels_have_the_parents_figures():
    """profiles/gkr_gates_kernel_resources.txt (a cross-compile's remarks): the four instantiations of k_batch_gkr_gates_phase without
    scratch and with k_batch_gkr_phase's static LDS; every existing GKR batch kernel and k_batch_round equal to the parent commit's line"""
    prof = open(os.path.join(ROOT, "profiles", "gkr_gates_kernel_resources.txt")).read()
    rows = {}
    for m in re.finditer(r"^(parent )?(k_\S+) VGPR (\d+) AGPR 0 scratch (\d+) occ (\d+) LDS (\d+)$", prof, re.M):
        rows[(bool(m.group(1)), m.group(2))] = tuple(int(m.group(k)) for k in (3, 4, 5, 6))  # VGPR, scratch, occupancy, LDS
    new = {k[1]: v for k, v in rows.items() if "gates" in k[1]}
    assert len(new) == 8 and all(v[1] == 0 for v in new.values()), "no scratch in the new kernels"
    assert sum("gates_eval" in k for k in new) == 4 and all(v[3] == 0 for k, v in new.items() if "gates_eval" in k), "the evaluation kernels: no static LDS"
    mine = {k[1]: v for k, v in rows.items() if not k[0] and "gates" not in k[1]}
    parent = {k[1]: v for k, v in rows.items() if k[0]}
    assert len(mine) == 16 and mine == parent, "the existing kernels are the parent's in every column"
    assert all(v[1] == 0 for v in rows.values())
    for phase in (1, 2):
        old = [v for k, v in mine.items() if k.startswith(f"k_batch_gkr_phaseILi{phase}ELi1E")]
        got = [v for k, v in new.items() if k.startswith(f"k_batch_gkr_gates_phaseILi{phase}ELi1E")]
        assert len(old) == len(got) == 1 and got[0][3] == old[0][3] and got[0][2] == old[0][2], "k_batch_gkr_phase's static LDS and occupancy"
