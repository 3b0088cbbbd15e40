"""CPU tests of the host side of sc_poly_evaluate_batch and sc_gkr_subclaim_batch: the symbols through every mirror (header, library,
ctypes table, Rust shim, C++ header), the four launch plans, and the argument checks, which run before any HIP call and before the device
count is asked -- so they behave the same with and without a device.  The values themselves are tests/test_gpu_eval_batch.py's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sumcheck_amd as sc
from oracle import cref
from oracle import pyoracle as po
from sumcheck_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_CANONICAL = np.array([0xffffffffffffffff] * 4, dtype=np.uint64)
P_LIMBS = np.array([(po.P >> (64 * i)) & 0xffffffffffffffff for i in range(4)], dtype=np.uint64)  # p itself is not canonical


def _poly(nv, shapes, seed):
    nt = max(max(s) for s in shapes) + 1
    mles = [sc.DenseMultilinearExtension(nv, cref.synth_table(seed, s, 1 << nv)) for s in range(nt)]
    coefs = cref.synth_table(seed, 1000, len(shapes))
    poly = sc.ListOfProductsOfPolynomials(nv)
    for k, sh in enumerate(shapes):
        poly.add_product([mles[i] for i in sh], coefs[k])
    return poly


def _points(n, nv, seed):
    return cref.synth_table(seed, 5, n * nv).reshape(n, nv, 4)


def _gkr(n, dim, seed, nnz=None):
    """n host instances -> (f1s, f2s, f3s, gs, uv)"""
    N = 1 << dim
    rng = np.random.default_rng(seed)
    k = N if nnz is None else nnz
    f1s = [sc.SparseMultilinearExtension(3 * dim, rng.integers(0, 1 << (3 * dim), size=k, dtype=np.uint64), cref.synth_table(seed + i, 1, k)) for i in range(n)]
    f2s = [sc.DenseMultilinearExtension(dim, cref.synth_table(seed + i, 2, N)) for i in range(n)]
    f3s = [sc.DenseMultilinearExtension(dim, cref.synth_table(seed + i, 3, N)) for i in range(n)]
    gs = [cref.synth_table(seed + i, 4, dim) for i in range(n)]
    uv = cref.synth_table(seed, 6, n * 2 * dim).reshape(n, 2, dim, 4)
    return f1s, f2s, f3s, gs, uv


def _raw_gkr(n, dim, f1s, f2s, f3s, gs, uv, flags=0, override=None):
    """the C entry point with explicit arrays; override: {argument name: replacement}"""
    def arr(vals):
        return (C.c_void_p * len(vals))(*[C.cast(v, C.c_void_p) for v in vals])
    uv = np.ascontiguousarray(uv)
    out = np.zeros((max(n, 1), 4, 4), np.uint64)
    a = {
        "f1_idx": arr([f._ptrs()[0] for f in f1s]),
        "f1_vals": arr([f._ptrs()[1] for f in f1s]),
        "nnz": (C.c_uint64 * len(f1s))(*[f.nnz for f in f1s]),
        "f2": arr([f.evaluations.ctypes.data for f in f2s]),
        "f3": arr([f.evaluations.ctypes.data for f in f3s]),
        "g": arr([g.ctypes.data for g in gs]),
        "uv": uv.ctypes.data_as(C.c_void_p),
        "out": out.ctypes.data_as(C.c_void_p),
    }
    a.update(override or {})
    rc = sc.lib().sc_gkr_subclaim_batch(n, dim, a["f1_idx"], a["f1_vals"], a["nnz"], a["f2"], a["f3"], a["g"], a["uv"], flags, a["out"])
    return rc, sc.lib().sc_last_error().decode()


def test_both_symbols_are_declared_exported_and_in_the_signature_table():
    hdr = open(os.path.join(ROOT, "include", "sumcheck_hip.h")).read()
    assert re.search(r"SC_API\s+int\s+sc_poly_evaluate_batch\s*\(\s*const sc_poly_desc \*descs,\s*uint32_t n,\s*const uint64_t \*points,\s*"
                     r"uint64_t \*out_values,\s*uint64_t \*out_table_values_or_null\s*\)", hdr)
    assert re.search(r"SC_API\s+int\s+sc_gkr_subclaim_batch\s*\(\s*uint32_t n,\s*uint32_t dim,\s*const uint64_t \*const \*f1_idx,\s*const uint64_t \*const \*f1_vals,\s*"
                     r"const uint64_t \*nnz,\s*const uint64_t \*const \*f2,\s*const uint64_t \*const \*f3,\s*const uint64_t \*const \*g,\s*"
                     r"const uint64_t \*uv,\s*uint32_t flags,\s*uint64_t \*out_evals\s*\)", hdr)
    version_line = hdr.split("#define SC_ABI_VERSION 5", 1)[1].split("\n", 1)[0]
    so = C.CDLL(_lib.SO_PATH)
    for name, n_args in (("sc_poly_evaluate_batch", 5), ("sc_gkr_subclaim_batch", 11)):
        assert name in version_line, f"{name} is an addition within ABI version 5: the version line names it"
        assert hasattr(so, name)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
    assert sc.lib().sc_abi_version() == 5


def test_the_mirrors_declare_and_wrap_them():
    rs = open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()
    block = re.search(r'extern "C" \{(.*?)\n\}', rs, re.S).group(1)
    assert re.search(r"pub fn sc_poly_evaluate_batch\s*\(descs: \*const sc_poly_desc, n: u32, points: \*const u64,", block)
    assert re.search(r"pub fn sc_gkr_subclaim_batch\s*\(n: u32, dim: u32, f1_idx: \*const \*const u64,", block)
    assert re.search(r"pub fn evaluate_batch<F: Limbs4>\(", rs) and re.search(r"pub fn gkr_verify_subclaim_batch<F: Limbs4>\(", rs)
    hpp = open(os.path.join(ROOT, "include", "sumcheck_amd.hpp")).read()
    for name in ("evaluate_batch(", "evaluate_subclaims_batch(", "verify_subclaim_batch(", "sc_poly_evaluate_batch(", "sc_gkr_subclaim_batch("):
        assert name in hpp, name
    assert callable(sc.ListOfProductsOfPolynomials.evaluate_batch)
    assert callable(sc.GKRRoundSumcheck.evaluate_subclaims_batch) and callable(sc.GKRRoundSumcheckSubClaim.verify_subclaim_batch)


def test_the_four_plans_are_listed_in_front_of_the_batched_provers():
    names = list(_lib.plan_stats())
    assert names[-4:] == ["batch.one_block", "batch.serial", "batch.gkr_one_block", "batch.gkr_serial"]
    assert names[-8:-4] == ["batch.eval_one_block", "batch.eval_serial", "batch.gkr_eval_one_block", "batch.gkr_eval_serial"]
    assert names[-9] == "fold_multi"


def test_an_empty_batch_is_ok_and_touches_nothing():
    assert sc.lib().sc_poly_evaluate_batch(None, 0, None, None, None) == _lib.SC_OK
    assert sc.lib().sc_gkr_subclaim_batch(0, 0, None, None, None, None, None, None, None, 0, None) == _lib.SC_OK
    assert sc.lib().sc_gkr_subclaim_batch(0, 7, None, None, None, None, None, None, None, _lib.SC_TABLES_ON_DEVICE, None) == _lib.SC_OK
    assert sc.ListOfProductsOfPolynomials.evaluate_batch([], np.zeros((0, 3, 4), np.uint64)).shape == (0, 4)
    assert sc.GKRRoundSumcheck.evaluate_subclaims_batch([], [], [], [], np.zeros((0, 2, 3, 4), np.uint64)).shape == (0, 4, 4)
    assert sc.GKRRoundSumcheckSubClaim.verify_subclaim_batch([], [], [], [], []) == []


# ---- sc_poly_evaluate_batch ---------------------------------------------------------------------------------------------------------
def _raw_ml(polys, points, descs=True, pts=True, out=True):
    n = len(polys)
    arr = (_lib.PolyDesc * n)()
    keep = []
    for i, p in enumerate(polys):
        d, k = p._desc(False)
        C.memmove(C.byref(arr, i * C.sizeof(_lib.PolyDesc)), C.byref(d), C.sizeof(_lib.PolyDesc))
        keep.append(k)
    points = np.ascontiguousarray(points)
    o = np.zeros((n, 4), np.uint64)
    rc = sc.lib().sc_poly_evaluate_batch(arr if descs else None, n, points.ctypes.data_as(C.c_void_p) if pts else None, o.ctypes.data_as(C.c_void_p) if out else None, None)
    return rc, sc.lib().sc_last_error().decode(), arr, keep


def test_ml_null_arrays_are_bad_arguments():
    polys = [_poly(3, [[0, 1, 2]], 200 + i) for i in range(3)]
    for kw in ({"descs": False}, {"pts": False}, {"out": False}):
        rc, msg, _, _ = _raw_ml(polys, _points(3, 3, 201), **kw)
        assert rc == _lib.SC_ERR_BAD_ARG and msg.startswith("instance 0: ") and "null" in msg, (kw, rc, msg)


def test_ml_a_null_table_names_the_lowest_failing_instance():
    n = 5
    polys = [_poly(3, [[0, 1, 2], [1, 2]], 210 + i) for i in range(n)]
    arr = (_lib.PolyDesc * n)()
    keep, tabs = [], []
    for i, p in enumerate(polys):
        d, k = p._desc(False)
        t = (C.c_void_p * 3)(*[d.tables[u] for u in range(3)])
        if i in (2, 4):
            t[1] = None
        d.tables = C.cast(t, C.POINTER(C.c_void_p))
        C.memmove(C.byref(arr, i * C.sizeof(_lib.PolyDesc)), C.byref(d), C.sizeof(_lib.PolyDesc))
        keep.append(k)
        tabs.append(t)
    pts, out = _points(n, 3, 211), np.zeros((n, 4), np.uint64)
    rc = sc.lib().sc_poly_evaluate_batch(arr, n, pts.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), None)
    msg = sc.lib().sc_last_error().decode()
    assert rc == _lib.SC_ERR_BAD_ARG and msg.startswith("instance 2: ") and "null" in msg, msg


def test_ml_a_descriptor_of_another_structure_is_named_as_by_the_batched_prover():
    polys = [_poly(3, [[0, 1, 2], [1, 2]], 220 + i) for i in range(4)]
    polys[2] = _poly(3, [[0, 1, 2], [0, 2]], 99)  # the same counts, other prod_indices
    with pytest.raises(sc.SumcheckError) as e:
        sc.ListOfProductsOfPolynomials.evaluate_batch(polys, _points(4, 3, 221))
    assert e.value.code == _lib.SC_ERR_BAD_ARG
    assert e.value.msg == "instance 2 differs from instance 0 in prod_indices: a batch has one structure"
    with pytest.raises(sc.SumcheckError) as e2:  # the same rule, the same text: sc_ml_prove_batch's
        sc.MLSumcheck.prove_batch(polys)
    assert e2.value.msg == e.value.msg
    polys[2], polys[3] = polys[0], _poly(3, [[0, 1, 2]], 98)
    with pytest.raises(sc.SumcheckError) as e:
        sc.ListOfProductsOfPolynomials.evaluate_batch(polys, _points(4, 3, 222))
    assert e.value.code == _lib.SC_ERR_BAD_ARG and e.value.msg.startswith("instance 3 differs from instance 0 in ")


def test_ml_a_non_canonical_point_or_coefficient_names_instance_and_element():
    polys = [_poly(4, [[0, 1, 2]], 230 + i) for i in range(4)]
    pts = _points(4, 4, 231).copy()
    pts[3, 0], pts[1, 2] = NOT_CANONICAL, P_LIMBS
    with pytest.raises(sc.SumcheckError) as e:
        sc.ListOfProductsOfPolynomials.evaluate_batch(polys, pts)
    assert e.value.code == _lib.SC_ERR_BAD_ARG and e.value.msg.startswith("instance 1: point[2]") and "canonical" in e.value.msg
    polys[2].products[0] = (NOT_CANONICAL.copy(), polys[2].products[0][1])
    with pytest.raises(sc.SumcheckError) as e:
        sc.ListOfProductsOfPolynomials.evaluate_batch(polys, _points(4, 4, 232))
    assert e.value.code == _lib.SC_ERR_BAD_ARG and e.value.msg.startswith("instance 2: coefficient 0") and "canonical" in e.value.msg


def test_ml_a_product_index_out_of_range_names_its_instance():
    polys = [_poly(2, [[0, 1], [1]], 240 + i) for i in range(3)]
    rc, msg, arr, keep = _raw_ml(polys, _points(3, 2, 241))
    bad = np.array([0, 1, 7], dtype=np.uint32)  # instance 1: table 7 of 2 (the structure check compares with instance 0 afterwards)
    arr[1].prod_indices = bad.ctypes.data_as(C.POINTER(C.c_uint32))
    pts, out = _points(3, 2, 241), np.zeros((3, 4), np.uint64)
    rc = sc.lib().sc_poly_evaluate_batch(arr, 3, pts.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), None)
    msg = sc.lib().sc_last_error().decode()
    assert rc == _lib.SC_ERR_BAD_ARG and msg.startswith("instance 1: ") and "table 7" in msg, msg


def test_ml_a_valid_batch_needs_a_device():
    polys = [_poly(5, [[0, 1, 2]], 250 + i) for i in range(3)] + [None]
    polys[3] = polys[0]  # a polynomial may stand for several instances
    pts = _points(4, 5, 251)
    if sc.lib().sc_device_count() > 0:
        got = sc.ListOfProductsOfPolynomials.evaluate_batch(polys, pts)
        assert got.shape == (4, 4)
        return
    with pytest.raises(sc.SumcheckError) as e:
        sc.ListOfProductsOfPolynomials.evaluate_batch(polys, pts)
    assert e.value.code == _lib.SC_ERR_HIP and "no HIP device visible" in e.value.msg and "no CPU fallback" in e.value.msg


# ---- sc_gkr_subclaim_batch ----------------------------------------------------------------------------------------------------------
def test_gkr_null_arrays_are_bad_arguments():
    inst = _gkr(3, 3, 300)
    for name in ("f1_idx", "f1_vals", "nnz", "f2", "f3", "g", "uv", "out"):
        rc, msg = _raw_gkr(3, 3, *inst, override={name: None})
        assert rc == _lib.SC_ERR_BAD_ARG and msg.startswith("instance 0: ") and "null" in msg, (name, rc, msg)


def test_gkr_a_null_entry_names_its_instance():
    inst = _gkr(4, 3, 310)
    for name, src in (("f2", inst[1]), ("f3", inst[2])):
        vals = [f.evaluations.ctypes.data for f in src]
        vals[2] = None
        rc, msg = _raw_gkr(4, 3, *inst, override={name: (C.c_void_p * 4)(*vals)})
        assert rc == _lib.SC_ERR_BAD_ARG and msg.startswith("instance 2: ") and "null" in msg, (name, rc, msg)
    gv = [g.ctypes.data for g in inst[3]]
    gv[1] = None
    rc, msg = _raw_gkr(4, 3, *inst, override={"g": (C.c_void_p * 4)(*gv)})
    assert rc == _lib.SC_ERR_BAD_ARG and msg.startswith("instance 1: "), msg
    iv = [C.cast(f._ptrs()[0], C.c_void_p) for f in inst[0]]
    iv[3] = None
    rc, msg = _raw_gkr(4, 3, *inst, override={"f1_idx": (C.c_void_p * 4)(*iv)})
    assert rc == _lib.SC_ERR_BAD_ARG and msg.startswith("instance 3: "), msg


def test_gkr_a_non_canonical_g_or_uv_names_instance_and_element():
    f1s, f2s, f3s, gs, uv = _gkr(4, 3, 320)
    gs[2][1] = NOT_CANONICAL
    with pytest.raises(sc.SumcheckError) as e:
        sc.GKRRoundSumcheck.evaluate_subclaims_batch(f1s, f2s, f3s, gs, uv)
    assert e.value.code == _lib.SC_ERR_BAD_ARG and e.value.msg.startswith("instance 2: g[1]") and "canonical" in e.value.msg
    f1s, f2s, f3s, gs, uv = _gkr(4, 3, 321)
    uv = uv.copy()
    uv[3, 0, 0], uv[1, 1, 2] = NOT_CANONICAL, P_LIMBS  # instance 1: v[2] = element 3 + 2 of its (u, v)
    with pytest.raises(sc.SumcheckError) as e:
        sc.GKRRoundSumcheck.evaluate_subclaims_batch(f1s, f2s, f3s, gs, uv)
    assert e.value.code == _lib.SC_ERR_BAD_ARG and e.value.msg.startswith("instance 1: uv[5]") and "canonical" in e.value.msg


def test_gkr_a_host_index_out_of_range_names_the_lowest_instance():
    dim = 3
    f1s, f2s, f3s, gs, uv = _gkr(6, dim, 330)
    f1s[4].indices[5] = np.uint64(1) << np.uint64(3 * dim)
    f1s[2].indices[0] = np.uint64(1) << np.uint64(63)
    with pytest.raises(sc.SumcheckError) as e:
        sc.GKRRoundSumcheck.evaluate_subclaims_batch(f1s, f2s, f3s, gs, uv)
    assert e.value.code == _lib.SC_ERR_BAD_ARG and e.value.msg.startswith("instance 2: ") and "out of range" in e.value.msg


def test_gkr_dim_out_of_range():
    inst = _gkr(2, 1, 340)
    for dim in (0, 22):
        rc, msg = _raw_gkr(2, dim, *inst)
        assert rc == _lib.SC_ERR_BAD_ARG and msg.startswith("instance 0: ") and f"dim {dim}" in msg, (dim, rc, msg)


def test_gkr_a_valid_batch_needs_a_device():
    f1s, f2s, f3s, gs, uv = _gkr(3, 4, 350)
    f1s = [f1s[0]] * 3  # one wiring predicate for every instance
    if sc.lib().sc_device_count() > 0:
        assert sc.GKRRoundSumcheck.evaluate_subclaims_batch(f1s, f2s, f3s, gs, uv).shape == (3, 4, 4)
        return
    with pytest.raises(sc.SumcheckError) as e:
        sc.GKRRoundSumcheck.evaluate_subclaims_batch(f1s, f2s, f3s, gs, uv)
    assert e.value.code == _lib.SC_ERR_HIP and "no HIP device visible" in e.value.msg and "no CPU fallback" in e.value.msg


# ---- the C++ mirror -----------------------------------------------------------------------------------------------------------------
def _build_cpp():
    from tests import test_cpp_mirror as M
    src = os.path.join(ROOT, "tests", "cpp", "test_eval_batch_mirror.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "test_eval_batch_mirror.bin")
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, "-o", out, "-L", M.LIBDIR, "-lsumcheck_hip", f"-Wl,-rpath,{M.LIBDIR}",
           "-Wl,-rpath,/opt/rocm/lib"]  # tests/test_cpp_mirror.py::build_cpp's command line, for this source
    subprocess.check_call(cmd)
    return out


def test_cpp_mirror_compiles_links_and_reports():
    """the C++ mirror's evaluate_batch / evaluate_subclaims_batch / verify_subclaim_batch against the C ABI: with a device they equal the
    single-instance calls instance by instance, without one the mirror's Panic carries the library's "no CPU fallback" """
    out = subprocess.run([_build_cpp()], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    if sc.lib().sc_device_count() > 0:
        assert out.returncode == 0 and "ALL TESTS PASSED" in out.stdout, out.stdout + out.stderr
    else:
        assert out.returncode == 3 and "no CPU fallback" in out.stdout, out.stdout + out.stderr
