"""CPU tests of the GKR batch handle's two-point form (sc_gkr_two_point_init_batch / sc_gkr_two_point_next_batch): the oracle of
tests/gkr_two_point_cases.py against big integers computed from the definition, and against the one-point Walk by linearity; the two
prototypes under their own marker SC_API_GKR2 against the shim's declarations and the ctypes table, by the rules of
tests/test_gkr_next_layer_host.py; the older scanners, none of which may see the names; the wrappers of every mirror; the argument errors
that need no device; the plan's name; the resource figures of the new kernel instantiations.  The values themselves are
tests/test_gpu_gkr_two_point.py's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sumcheck_amd as sc
from oracle import cref, pyoracle
from sumcheck_amd import _lib
from tests import gkr_two_point_cases as K
from tests import test_gkr_batch_rounds_host as GR
from tests import test_gkr_next_layer_host as NH
from tests import test_gpu_gkr_batch as T
from tests import test_gpu_gkr_batch_rounds as R
from tests import test_rust_shim as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = cref.P
INIT, NEXT = "sc_gkr_two_point_init_batch", "sc_gkr_two_point_next_batch"
HDR = open(os.path.join(ROOT, "include", "sumcheck_hip.h")).read()
PP = "*const *const u64"
PARAMS = {INIT: ["u32", "u32", PP, PP, "*const u64", PP, PP, PP, PP, "*const u64", "u32", "*mut *mut sc_gkr_batch_prover"],
          NEXT: ["*mut sc_gkr_batch_prover", PP, PP, "*const u64", PP, PP, PP, PP, "*const u64", "u32"]}


def instance(dim, seed, nnz):
    N = 1 << dim
    idx, vals = T.make_f1(dim, seed, "repeated", nnz)
    sec = K.second_points(1, dim, seed + 3)[0]
    return (idx, vals, cref.synth_table(seed, 2, N), cref.synth_table(seed, 3, N), cref.synth_table(seed, 4, dim), sec[0], sec[1])


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_walk2_equals_the_definition_in_big_integers(dim):
    """h[x] = sum (alpha eq(g,z) + beta eq(g2,z)) v f3[y] and f1_gu[y] = sum (alpha eq(g,z) + beta eq(g2,z)) eq(u,x) v over the list's
    entries (repeated indices add up); finish's first value is f1_gu at v"""
    N = 1 << dim
    inst = instance(dim, 91000 + dim, 3 * N)
    chal = np.ascontiguousarray(R.challenges(1, dim, 91100 + dim, edge_instance=None)[:, 0])
    w = K.Walk2(inst, dim, chal)
    ints = lambda a: cref.mont_to_ints(np.asarray(a))
    idx, vals, f3 = [int(i) for i in inst[0]], ints(inst[1]), ints(inst[3])
    alpha, beta = ints(inst[6])
    eg, eg2, eu = pyoracle.precompute_eq(ints(inst[4])), pyoracle.precompute_eq(ints(inst[5])), pyoracle.precompute_eq(ints(chal[:dim]))
    E = [(alpha * eg[z] + beta * eg2[z]) % P for z in range(N)]
    h, f1gu = [0] * N, [0] * N
    for i, v in zip(idx, vals):
        z, x, y = i & (N - 1), (i >> dim) & (N - 1), i >> (2 * dim)
        h[x] = (h[x] + E[z] * v * f3[y]) % P
        f1gu[y] = (f1gu[y] + E[z] * eu[x] * v) % P
    assert ints(w.h) == h and ints(w.f1gu) == f1gu
    assert ints(w.final[:1]) == [pyoracle.dense_evaluate(f1gu, ints(chal[dim:]))]
    assert (ints(w.msgs[0, 0])[0] + ints(w.msgs[0, 1])[0]) % P == sum(hx * f2x for hx, f2x in zip(h, ints(inst[2]))) % P, "the claim: alpha W(g) + beta W(g2)"


@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_walk2_is_linear_in_the_two_one_point_walks(dim):
    """under the same challenges: msgs = alpha Walk(g).msgs + beta Walk(g2).msgs element by element, final[0] likewise; final[1] and
    final[2] do not depend on the point"""
    N = 1 << dim
    inst = instance(dim, 92000 + dim, 2 * N + 1)
    chal = np.ascontiguousarray(R.challenges(1, dim, 92100 + dim)[:, 0])
    w = K.Walk2(inst, dim, chal, R.state_rounds(dim))
    a, b = R.Walk(inst[:5], dim, chal), R.Walk(inst[:4] + (inst[5],), dim, chal)
    alpha, beta = inst[6]
    assert np.array_equal(w.msgs.reshape(-1, 4), K.combine(alpha, a.msgs.reshape(-1, 4), beta, b.msgs.reshape(-1, 4)))
    assert np.array_equal(w.final[:1], K.combine(alpha, a.final[:1], beta, b.final[:1]))
    assert np.array_equal(w.final[1:], a.final[1:]) and np.array_equal(w.final[1:], b.final[1:])
    assert sorted(w.states) == R.state_rounds(dim)


def test_one_and_zero_reproduce_the_one_point_walk():
    dim = 3
    inst = instance(dim, 93000, 20)
    chal = np.ascontiguousarray(R.challenges(1, dim, 93001)[:, 0])
    w = K.Walk2(inst[:6] + (np.stack([K.ONE, K.ZERO]),), dim, chal, R.state_rounds(dim))
    a = R.Walk(inst[:5], dim, chal, R.state_rounds(dim))
    assert np.array_equal(w.msgs, a.msgs) and np.array_equal(w.final, a.final)
    assert all(np.array_equal(w.states[t], a.states[t]) for t in a.states)


# ---- the prototypes ------------------------------------------------------------------------------------------------------------------
def _header_prototypes():
    """the SC_API_GKR2 prototypes, parameter types in the shim's spelling (tests/test_gkr_next_layer_host.py's reading)"""
    old = dict(RS.C_BASE)
    RS.C_BASE["sc_gkr_batch_prover"] = "sc_gkr_batch_prover"
    try:
        protos = {}
        for m in re.finditer(r"SC_API_GKR2\s+([^;(]+?)\b(sc_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", HDR, re.S):
            ret, name, params = m.group(1).strip(), m.group(2), " ".join(m.group(3).split())
            plist = [RS.c_type_to_rust(re.match(r"(.*?)([A-Za-z_][A-Za-z_0-9]*)$", prm.strip()).group(1)) for prm in params.split(",")]
            protos[name] = (plist, None if ret == "void" else RS.c_type_to_rust(ret))
        return protos
    finally:
        RS.C_BASE.clear()
        RS.C_BASE.update(old)


def test_the_symbols_are_declared_exported_and_in_their_own_signature_table():
    protos = _header_prototypes()
    assert set(protos) == {INIT, NEXT} == set(_lib.SIGNATURES_GKR2)
    assert re.search(r"#define SC_API_GKR2 SC_API /\*[^\n]*\*/\n", HDR), "SC_API with only a comment behind it on the line"
    version_line = HDR.split("#define SC_ABI_VERSION 5", 1)[1].split("\n", 1)[0]
    so = C.CDLL(_lib.SO_PATH)
    for name in (INIT, NEXT):
        assert protos[name] == (PARAMS[name], "c_int")
        assert not name.startswith("sc_gkr_batch_") and name in version_line and hasattr(so, name)
        res, args = _lib.SIGNATURES_GKR2[name]
        assert res is C.c_int and len(args) == len(PARAMS[name])
        assert all(name not in table for table in (_lib.SIGNATURES, _lib.SIGNATURES_EXT, _lib.SIGNATURES_GKRB, _lib.SIGNATURES_GKRL))
    assert sc.lib().sc_abi_version() == 5


def test_none_of_the_older_scanners_sees_the_names_and_their_closed_sets_hold():
    for marker in ("SC_API", "SC_API_EXT", "SC_API_GKRB", "SC_API_GKRL"):
        names = [m.group(2) for m in re.finditer(marker + r"\s+([^;(]+?)\b(sc_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", HDR, re.S)]
        assert names and INIT not in names and NEXT not in names, marker
    assert set(GR._header_prototypes()) == set(GR.NAMES)
    assert set(NH._header_prototypes()) == {NH.NAME} == set(_lib.SIGNATURES_GKRL)
    rs = open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()
    for name in (INIT, NEXT):
        assert not re.search(r"pub\s+fn\s+" + name + r"\b", rs), "a private declaration: the shim's pub externs are SC_API prototypes"


def test_the_shim_declares_them_as_the_header_does_and_wraps_them():
    rs = open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()
    protos = _header_prototypes()
    for name in (INIT, NEXT):
        found = []
        for block in re.findall(r'extern "C" \{(.*?)\n\}', rs, re.S):
            for m in re.finditer(r"\bfn (" + name + r")\s*\((.*?)\)\s*(?:->\s*([^;]+?))?\s*;", block, re.S):
                assert len(re.findall(r"\bfn\s+sc_", block)) == 1, "a block of its own"
                params = " ".join(m.group(2).split())
                found.append(([p.split(":", 1)[1].strip() for p in params.split(",") if p.strip()], m.group(3).strip() if m.group(3) else None))
        assert found == [protos[name]], (name, found)
    assert re.search(r"pub fn gkr_prover_init_batch_two_point<F: Limbs4>\(", rs) and re.search(r"pub fn gkr_next_layer_batch_two_point<F: Limbs4>\(", rs)


def test_every_mirror_wraps_them_and_the_documents_name_them():
    import inspect
    hpp = open(os.path.join(ROOT, "include", "sumcheck_amd.hpp")).read()
    assert INIT in hpp and NEXT in hpp and "verify_subclaim_two_point_batch(" in hpp and "verify_subclaim_two_point(" in hpp
    for fn in (sc.GKRRoundSumcheck.prover_init_batch, sc.GKRBatchProverState.next_layer):
        assert {"g2s", "coeffs"} <= set(inspect.signature(fn).parameters)
    assert callable(sc.GKRRoundSumcheckSubClaim.verify_subclaim_two_point) and callable(sc.GKRRoundSumcheckSubClaim.verify_subclaim_two_point_batch)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in (INIT, NEXT, "g2s", "coeffs", "gkr_prover_init_batch_two_point", "gkr_next_layer_batch_two_point", "verify_subclaim_two_point"):
        assert name in doc, name
    assert "batch.gkr_two_point" in open(os.path.join(ROOT, "README.md")).read() and "batch.gkr_two_point" in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---- argument errors that need no device -----------------------------------------------------------------------------------------------
def _init_args(n, dim, g2s, coef):
    N = 1 << dim
    keep = {"f2": [cref.synth_table(94000 + i, 2, N) for i in range(n)], "g": [cref.synth_table(94000 + i, 4, dim) for i in range(n)], "g2": g2s}
    ptrs = lambda arrs: (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in arrs])
    nnz = (C.c_uint64 * n)(*([0] * n))
    none = (C.c_void_p * n)()
    return keep, [n, dim, none, none, nnz, ptrs(keep["f2"]), ptrs(keep["f2"]), ptrs(keep["g"]), None if g2s is None else ptrs(g2s), None if coef is None else coef.ctypes.data]


def _init_status(n, dim, g2s, coef):
    keep, args = _init_args(n, dim, g2s, coef)
    h = C.c_void_p()
    rc = sc.lib().sc_gkr_two_point_init_batch(*args, 0, C.byref(h))
    msg = sc.lib().sc_last_error().decode()
    assert bool(h.value) == (rc == _lib.SC_OK), "a handle exactly on success"
    if h.value:
        sc.lib().sc_gkr_batch_prover_free(h)
    return rc, msg


def test_the_two_point_checks_run_before_any_device_call():
    n, dim = 3, 2
    g2s = [cref.synth_table(94100 + i, 5, dim) for i in range(n)]
    coef = np.ascontiguousarray(cref.synth_table(94200, 6, 2 * n).reshape(n, 2, 4))
    assert _init_status(n, dim, None, coef) == (_lib.SC_ERR_BAD_ARG, "null argument")
    assert _init_status(n, dim, g2s, None) == (_lib.SC_ERR_BAD_ARG, "null argument")
    assert _init_status(n, dim, [g2s[0], None, g2s[2]], coef) == (_lib.SC_ERR_BAD_ARG, "instance 1: null argument")
    bad = [g.copy() for g in g2s]
    bad[2][1] = R.P_LIMBS
    assert _init_status(n, dim, bad, coef) == (_lib.SC_ERR_BAD_ARG, "instance 2: g2 is not canonical")
    bad_coef = coef.copy()
    bad_coef[2, 0] = R.P_LIMBS
    bad_coef[1, 1] = R.P_LIMBS
    assert _init_status(n, dim, g2s, bad_coef) == (_lib.SC_ERR_BAD_ARG, "instance 1: coefficient is not canonical"), "the lowest failing instance decides"
    assert _init_status(n, dim, bad, bad_coef) == (_lib.SC_ERR_BAD_ARG, "instance 1: coefficient is not canonical")
    bad[0][0] = R.P_LIMBS
    assert _init_status(n, dim, bad, bad_coef) == (_lib.SC_ERR_BAD_ARG, "instance 0: g2 is not canonical")
    assert _init_status(n, 0, g2s, coef)[0] == _lib.SC_ERR_CONSTANT_POLY, "sc_gkr_batch_prover_init's checks come first"
    rc, msg = _init_status(n, dim, g2s, coef)  # good arguments get as far as the device: no CPU fallback
    assert rc == _lib.SC_OK or (rc == _lib.SC_ERR_HIP and "no HIP device" in msg)


def test_a_null_handle_is_a_bad_argument_and_the_python_arguments_come_together():
    assert sc.lib().sc_gkr_two_point_next_batch(None, None, None, None, None, None, None, None, None, 0) == _lib.SC_ERR_BAD_ARG
    assert "null" in sc.lib().sc_last_error().decode()
    st = sc.GKRBatchProverState(C.c_void_p(), 1, 2)
    g = cref.synth_table(95000, 4, 2)
    with pytest.raises(ValueError):
        st.next_layer([None], [None], [g], g2s=[g])
    with pytest.raises(ValueError):
        st.next_layer([None], [None], [g], coeffs=[np.stack([K.ONE, K.ZERO])])
    with pytest.raises(ValueError):
        sc.GKRRoundSumcheck.prover_init_batch([], [], [], [], coeffs=[])


# ---- the plan and the kernels ----------------------------------------------------------------------------------------------------------
def test_the_plan_is_named_and_every_position_test_still_holds():
    names = list(_lib.plan_stats())
    assert "batch.gkr_two_point" in names and len(names) == sc.lib().sc_plan_count() and "batch.gkr_two_point" in HDR
    i = names.index("batch.gkr_two_point")
    assert names[i - 1] == "sharded.p2p" and names[i + 1] == "sharded.gather_tail"
    NH.test_the_plan_sits_between_the_two_bucketed_gkr_plans()


def test_the_new_instantiations_use_no_scratch_and_the_lds_they_state():
    from sumcheck_amd import build
    assert "kernels_batch_gkr_rounds.hip" in build.SOURCES and "kernels_batch_gkr_round_slices.hip" in build.SOURCES
    for f, text in (("kernels_batch_gkr_rounds.hip", "template <int kPhase, int kPoints>"), ("kernels_batch_gkr_round_slices.hip", "template <int kPhase, int kPoints>"),
                    ("kernels_batch_gkr_rounds.hip", "void k_gkr_two_point_combine(")):
        assert text in open(os.path.join(ROOT, "sumcheck_amd", "csrc", f)).read(), (f, text)
    prof = open(os.path.join(ROOT, "profiles", "gkr_two_point_kernel_resources.txt")).read()
    rows = {}
    for m in re.finditer(r"^(parent )?(k_[a-z_0-9]+?)(ILi(\d)(?:ELi(\d))?E\S*|E\S*) VGPR (\d+) AGPR 0 scratch (\d+) occ (\d+) LDS (\d+)$", prof, re.M):
        key = (bool(m.group(1)), m.group(2), int(m.group(4) or 0), int(m.group(5) or 0))
        rows[key] = tuple(int(m.group(k)) for k in (6, 7, 8, 9))  # VGPR, scratch, occupancy, LDS
    assert len(rows) == 11 + 6 and all(r[1] == 0 for r in rows.values()), "no scratch anywhere"
    for kernel in ("k_batch_gkr_phase", "k_batch_gkr_terms"):
        for phase in (1, 2):
            assert rows[(False, kernel, phase, 1)] == rows[(True, kernel, phase, 0)], "the one-point instantiations are the parent's"
    for phase in (1, 2):
        assert rows[(False, "k_batch_gkr_fold", phase, 0)] == rows[(True, "k_batch_gkr_fold", phase, 0)]
        assert rows[(False, "k_batch_gkr_phase", phase, 2)][3] == rows[(False, "k_batch_gkr_phase", phase, 1)][3], "no static LDS beyond the one-point kernel's; the dynamic 128 B x 2^dim is the launch's"
    half_pair, point = 2 * 256 * 32, 2 * 16 * 16  # lo | hi of at most 2^8 elements; a point of at most 16 elements
    assert rows[(False, "k_batch_gkr_terms", 1, 2)][3] == 2 * half_pair + point, "two pairs of half tables and g"
    assert rows[(False, "k_batch_gkr_terms", 2, 2)][3] == 3 * half_pair + 2 * point < 64 * 1024, "three pairs of half tables, 48 KB, and the points g and u"
    assert rows[(False, "k_gkr_two_point_combine", 0, 0)][3] == 0
