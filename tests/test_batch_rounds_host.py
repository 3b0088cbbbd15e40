"""CPU tests of the host side of the batched interactive rounds (sc_batch_prover_*): the symbols through every mirror (header, library,
ctypes table, C++ header, Rust shim -- its declarations checked against the header's prototypes with tests/test_rust_shim.py's rules), the
two launch plans, and the argument checks of sc_batch_prover_init, which run before any HIP call and before the device count is asked --
so they behave the same with and without a device.  The values themselves are tests/test_gpu_batch_rounds.py's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib
from tests import test_rust_shim as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"sc_batch_prover_init": 3, "sc_batch_prove_round": 4, "sc_batch_prover_push_randomness": 3, "sc_batch_prover_state": 6,
         "sc_batch_prover_bind_final": 4, "sc_batch_prover_reset": 2, "sc_batch_prover_free": 1}
HDR = open(os.path.join(ROOT, "include", "sumcheck_hip.h")).read()


def _poly(nv, shapes, seed):
    nt = max(max(s) for s in shapes) + 1
    mles = [sc.DenseMultilinearExtension(nv, cref.synth_table(seed, s, 1 << nv)) for s in range(nt)]
    coefs = cref.synth_table(seed, 1000, len(shapes))
    poly = sc.ListOfProductsOfPolynomials(nv)
    for k, sh in enumerate(shapes):
        poly.add_product([mles[i] for i in sh], coefs[k])
    return poly


def _descs(polys):
    arr = (_lib.PolyDesc * max(len(polys), 1))()
    keep = []
    for i, p in enumerate(polys):
        d, k = p._desc(False)
        C.memmove(C.byref(arr, i * C.sizeof(_lib.PolyDesc)), C.byref(d), C.sizeof(_lib.PolyDesc))
        keep.append(k)
    return arr, keep


def _init(arr, n, out=True):
    h = C.c_void_p()
    rc = sc.lib().sc_batch_prover_init(arr, n, C.byref(h) if out else None)
    msg = sc.lib().sc_last_error().decode()
    if rc == _lib.SC_OK:
        sc.lib().sc_batch_prover_free(h)
    else:
        assert not h.value, "a failed init leaves no handle behind"
    return rc, msg


def _header_prototypes():
    """the SC_API_EXT prototypes, parameter types in the shim's spelling (tests/test_rust_shim.py's mapping plus the new opaque type)"""
    old = dict(RS.C_BASE)
    RS.C_BASE["sc_batch_prover"] = "sc_batch_prover"
    try:
        protos = {}
        for m in re.finditer(r"SC_API_EXT\s+([^;(]+?)\b(sc_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", HDR, re.S):
            ret, name, params = m.group(1).strip(), m.group(2), " ".join(m.group(3).split())
            plist = [RS.c_type_to_rust(re.match(r"(.*?)([A-Za-z_][A-Za-z_0-9]*)$", prm.strip()).group(1)) for prm in params.split(",")]
            protos[name] = (plist, None if ret == "void" else RS.c_type_to_rust(ret))
        return protos
    finally:
        RS.C_BASE.clear()
        RS.C_BASE.update(old)


def test_the_symbols_are_declared_exported_and_in_the_signature_table():
    protos = _header_prototypes()
    assert set(protos) == set(NAMES) == set(_lib.SIGNATURES_EXT)
    assert re.search(r"#define SC_API_EXT SC_API\b", HDR) and "typedef struct sc_batch_prover sc_batch_prover;" in HDR
    version_line = HDR.split("#define SC_ABI_VERSION 5", 1)[1].split("\n", 1)[0]
    assert "sc_batch_prover_" in version_line, "additions within ABI version 5: the version line names the family"
    so = C.CDLL(_lib.SO_PATH)
    for name, n_args in NAMES.items():
        assert hasattr(so, name), name
        assert len(protos[name][0]) == n_args and len(_lib.SIGNATURES_EXT[name][1]) == n_args, name
        assert (_lib.SIGNATURES_EXT[name][0] is None) == (protos[name][1] is None), name
        assert name not in _lib.SIGNATURES
    assert protos["sc_batch_prove_round"] == (["*mut sc_batch_prover", "*const u64", "u32", "*mut u64"], "c_int")
    assert sc.lib().sc_abi_version() == 5


def test_the_shim_declares_them_as_the_header_does_and_wraps_them():
    rs = open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()
    protos, ext = _header_prototypes(), {}
    for block in re.findall(r'extern "C" \{(.*?)\n\}', rs, re.S):
        for m in re.finditer(r"\bfn (sc_batch_[a-z0-9_]+)\s*\((.*?)\)\s*(?:->\s*([^;]+?))?\s*;", block, re.S):
            params = " ".join(m.group(2).split())
            ext[m.group(1)] = ([p.split(":", 1)[1].strip() for p in params.split(",") if p.strip()], m.group(3).strip() if m.group(3) else None)
    assert set(ext) == set(NAMES)
    for name, (rp, rr) in ext.items():
        assert (rp, rr) == protos[name], f"{name}: shim {rp} -> {rr}, header {protos[name]}"
    assert re.search(r"pub struct sc_batch_prover \{\s*_private: \[u8; 0\],\s*\}", rs)
    assert re.search(r"pub fn prover_init_batch<F: Limbs4>\(", rs) and re.search(r"pub fn prove_round_batch<F: Limbs4>\(", rs)


def test_the_python_and_cpp_mirrors_wrap_them():
    hpp = open(os.path.join(ROOT, "include", "sumcheck_amd.hpp")).read()
    for name in list(NAMES) + ["class BatchProverState", "prover_init_batch(", "prove_round_batch(", "bind_final(", "push_randomness("]:
        assert name in hpp, name
    assert callable(sc.IPForMLSumcheck.prover_init_batch) and callable(sc.IPForMLSumcheck.prove_round_batch)
    for attr in ("round", "randomness", "flattened_ml_extensions", "bind_final", "push_randomness", "reset", "close"):
        assert hasattr(sc.BatchProverState, attr), attr


def test_the_two_plans_sit_immediately_in_front_of_fold_multi():
    names = list(_lib.plan_stats())
    i = names.index("fold_multi")
    assert names[i - 2:i] == ["batch.rounds_one_block", "batch.rounds_serial"]
    assert names[i - 3] == "gkr.sharded" and len(names) == sc.lib().sc_plan_count()
    assert names[-9] == "fold_multi"


def test_the_kernel_source_is_built_and_uses_no_scratch():
    from sumcheck_amd import build
    assert "kernels_batch_rounds.hip" in build.SOURCES
    prof = open(os.path.join(ROOT, "profiles", "batch_rounds_kernel_resources.txt")).read()
    m = re.search(r"^k_batch_roundILi8\S* VGPR (\d+) AGPR 0 scratch (\d+) ", prof, re.M)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) <= 128


def test_null_arguments_and_an_empty_batch_are_bad_arguments():
    arr, keep = _descs([_poly(3, [[0, 1, 2]], 400 + i) for i in range(2)])
    rc, msg = _init(None, 2)
    assert rc == _lib.SC_ERR_BAD_ARG and "null" in msg
    rc, msg = _init(arr, 2, out=False)
    assert rc == _lib.SC_ERR_BAD_ARG and "null" in msg
    rc, msg = _init(arr, 0)
    assert rc == _lib.SC_ERR_BAD_ARG and "n == 0" in msg, msg
    L = sc.lib()
    out = np.zeros((8, 4), np.uint64)
    p = out.ctypes.data_as(C.c_void_p)
    assert L.sc_batch_prove_round(None, None, 0, p) == _lib.SC_ERR_BAD_ARG
    assert L.sc_batch_prover_push_randomness(None, p, 0) == _lib.SC_ERR_BAD_ARG
    assert L.sc_batch_prover_state(None, 0, None, None, None, None) == _lib.SC_ERR_BAD_ARG
    assert L.sc_batch_prover_bind_final(None, p, 0, p) == _lib.SC_ERR_BAD_ARG
    assert L.sc_batch_prover_reset(None, None) == _lib.SC_ERR_BAD_ARG
    L.sc_batch_prover_free(None)  # like free(NULL)


def test_a_descriptor_of_another_structure_is_named_as_by_the_batched_prover():
    polys = [_poly(3, [[0, 1, 2], [1, 2]], 410 + i) for i in range(4)]
    polys[2] = _poly(3, [[0, 1, 2], [0, 2]], 99)  # the same counts, other prod_indices
    with pytest.raises(sc.SumcheckError) as e:
        sc.IPForMLSumcheck.prover_init_batch(polys)
    assert e.value.code == _lib.SC_ERR_BAD_ARG
    assert e.value.msg == "instance 2 differs from instance 0 in prod_indices: a batch has one structure"
    with pytest.raises(sc.SumcheckError) as e2:  # the same rule, the same text: sc_ml_prove_batch's
        sc.MLSumcheck.prove_batch(polys)
    assert e2.value.msg == e.value.msg
    polys[2], polys[3] = polys[0], _poly(4, [[0, 1, 2], [1, 2]], 98)
    with pytest.raises(sc.SumcheckError) as e:
        sc.IPForMLSumcheck.prover_init_batch(polys)
    assert e.value.code == _lib.SC_ERR_BAD_ARG and e.value.msg == "instance 3 differs from instance 0 in num_vars: a batch has one structure"


def test_a_constant_is_the_reference_panic_with_its_instance():
    arr, keep = _descs([_poly(2, [[0, 1]], 420 + i) for i in range(3)])
    for i in range(3):
        arr[i].num_vars = 0
    rc, msg = _init(arr, 3)
    assert rc == _lib.SC_ERR_CONSTANT_POLY and msg == "instance 0: Attempt to prove a constant.", msg
    arr[0].num_vars = 2
    rc, msg = _init(arr, 3)
    assert rc == _lib.SC_ERR_CONSTANT_POLY and msg.startswith("instance 1: "), msg


def test_inconsistent_max_multiplicands_and_a_bad_coefficient_name_their_instance():
    polys = [_poly(3, [[0, 1, 2], [1]], 430 + i) for i in range(3)]
    arr, keep = _descs(polys)
    arr[1].max_multiplicands = 2
    rc, msg = _init(arr, 3)
    assert rc == _lib.SC_ERR_BAD_ARG and msg.startswith("instance 1: max_multiplicands 2 != max product length 3"), msg
    polys[2].products[1] = (np.array([0xffffffffffffffff] * 4, dtype=np.uint64), polys[2].products[1][1])
    arr, keep = _descs(polys)
    rc, msg = _init(arr, 3)
    assert rc == _lib.SC_ERR_BAD_ARG and msg.startswith("instance 2: coefficient 1") and "canonical" in msg, msg


def test_a_valid_batch_needs_a_device():
    polys = [_poly(5, [[0, 1, 2]], 440 + i) for i in range(3)] + [_poly(5, [[0, 1, 2]], 440)]
    if sc.lib().sc_device_count() > 0:
        st = sc.IPForMLSumcheck.prover_init_batch(polys)
        assert st.round == 0 and len(sc.IPForMLSumcheck.prove_round_batch(st, None)) == 4
        st.close()
        return
    with pytest.raises(sc.SumcheckError) as e:
        sc.IPForMLSumcheck.prover_init_batch(polys)
    assert e.value.code == _lib.SC_ERR_HIP and "no HIP device visible" in e.value.msg and "no CPU fallback" in e.value.msg


# ---- the C++ mirror -----------------------------------------------------------------------------------------------------------------
def _build_cpp():
    from tests import test_cpp_mirror as M
    src = os.path.join(ROOT, "tests", "cpp", "test_batch_rounds_mirror.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "test_batch_rounds_mirror.bin")
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, "-o", out, "-L", M.LIBDIR, "-lsumcheck_hip", f"-Wl,-rpath,{M.LIBDIR}",
           "-Wl,-rpath,/opt/rocm/lib"]  # tests/test_cpp_mirror.py::build_cpp's command line, for this source
    subprocess.check_call(cmd)
    return out


def test_cpp_mirror_compiles_links_and_reports():
    """the C++ mirror's prover_init_batch / prove_round_batch / BatchProverState against the C ABI: with a device they equal the
    single-instance prover round by round, without one the mirror's Panic carries the library's "no CPU fallback" """
    out = subprocess.run([_build_cpp()], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    if sc.lib().sc_device_count() > 0:
        assert out.returncode == 0 and "ALL TESTS PASSED" in out.stdout, out.stdout + out.stderr
    else:
        assert out.returncode == 3 and "no CPU fallback" in out.stdout, out.stdout + out.stderr
