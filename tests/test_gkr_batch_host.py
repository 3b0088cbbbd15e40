"""CPU tests of sc_gkr_prove_batch's host side: the symbol through every mirror (header, library, ctypes table, Rust shim, C++ header), the
two launch plans, and the argument checks, which run before any HIP call and before the device count is asked -- so they behave the same
with and without a device.  The proofs themselves are tests/test_gpu_gkr_batch.py's."""
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
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _instances(n, dim, seed, nnz=None):
    """n host instances -> (rngs, f1s, f2s, f3s, gs)"""
    N = 1 << dim
    rng = np.random.default_rng(seed)
    out = ([], [], [], [], [])
    for i in range(n):
        k = N if nnz is None else nnz
        idx = rng.integers(0, 1 << (3 * dim), size=k, dtype=np.uint64)
        out[0].append(_fed(i))
        out[1].append(sc.SparseMultilinearExtension(3 * dim, idx, cref.synth_table(seed + i, 1, k)))
        out[2].append(sc.DenseMultilinearExtension(dim, cref.synth_table(seed + i, 2, N)))
        out[3].append(sc.DenseMultilinearExtension(dim, cref.synth_table(seed + i, 3, N)))
        out[4].append(cref.synth_table(seed + i, 4, dim))
    return out


def _fed(i):
    r = sc.Blake2b512Rng.setup()
    r.feed(b"the caller's transcript before instance %d" % i)
    return r


def _untouched(rngs):
    """every transcript still yields what a twin with the same history yields: the failed call advanced none of them"""
    return all(np.array_equal(r.sample_fr(), _fed(i).sample_fr()) for i, r in enumerate(rngs))


def _raw_call(n, dim, rngs, f1s, f2s, f3s, gs, flags=0, override=None):
    """the C entry point with explicit arrays; override: {argument name: replacement}"""
    def arr(vals):
        return (C.c_void_p * len(vals))(*[C.cast(v, C.c_void_p) for v in vals])
    a = {
        "rngs": arr([r._h for r in rngs]),
        "f1_idx": arr([f._ptrs()[0] for f in f1s]),
        "f1_vals": arr([f._ptrs()[1] for f in f1s]),
        "nnz": (C.c_uint64 * len(f1s))(*[f.nnz for f in f1s]),
        "f2": arr([f.evaluations.ctypes.data for f in f2s]),
        "f3": arr([f.evaluations.ctypes.data for f in f3s]),
        "g": arr([g.ctypes.data for g in gs]),
    }
    proofs = np.zeros((max(n, 1), 2, max(dim, 1), 3, 4), np.uint64)
    a["out"] = proofs.ctypes.data_as(C.c_void_p)
    a.update(override or {})
    rc = sc.lib().sc_gkr_prove_batch(n, dim, a["rngs"], a["f1_idx"], a["f1_vals"], a["nnz"], a["f2"], a["f3"], a["g"], flags, a["out"], None)
    return rc, sc.lib().sc_last_error().decode()


def test_the_symbol_is_declared_exported_and_in_the_signature_table():
    hdr = open(os.path.join(ROOT, "include", "sumcheck_hip.h")).read()
    assert re.search(r"SC_API\s+int\s+sc_gkr_prove_batch\s*\(\s*uint32_t n,\s*uint32_t dim,\s*sc_rng \*const \*rngs,\s*const uint64_t \*const \*f1_idx,", hdr)
    assert "#define SC_ABI_VERSION 5" in hdr and "sc_gkr_prove_batch" in hdr.split("#define SC_ABI_VERSION 5", 1)[1].split("\n", 1)[0]
    assert hasattr(C.CDLL(_lib.SO_PATH), "sc_gkr_prove_batch")
    assert "sc_gkr_prove_batch" in _lib.SIGNATURES and len(_lib.SIGNATURES["sc_gkr_prove_batch"][1]) == 12
    assert sc.lib().sc_abi_version() == 5


def test_the_mirrors_declare_it_and_wrap_it():
    rs = open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()
    block = re.search(r'extern "C" \{(.*?)\n\}', rs, re.S).group(1)
    assert re.search(r"pub fn sc_gkr_prove_batch\s*\(n: u32, dim: u32, rngs: \*const \*mut sc_rng, f1_idx: \*const \*const u64,", block)
    assert re.search(r"pub fn gkr_prove_batch<F: Limbs4>\(instances: &mut \[GkrInstance<F>\]\) -> Vec<HipGKRProof<F>>", rs)
    hpp = open(os.path.join(ROOT, "include", "sumcheck_amd.hpp")).read()
    assert re.search(r"static std::vector<GKRProof> prove_batch\(", hpp) and "sc_gkr_prove_batch(" in hpp
    assert callable(sc.GKRRoundSumcheck.prove_batch)


def test_both_plans_are_listed_behind_the_existing_ones():
    names = list(_lib.plan_stats())
    assert names[-2:] == ["batch.gkr_one_block", "batch.gkr_serial"] and names[-4:-2] == ["batch.one_block", "batch.serial"]


def test_an_empty_batch_is_ok_and_touches_nothing():
    assert sc.lib().sc_gkr_prove_batch(0, 0, None, None, None, None, None, None, None, 0, None, None) == _lib.SC_OK
    assert sc.lib().sc_gkr_prove_batch(0, 7, None, None, None, None, None, None, None, _lib.SC_TABLES_ON_DEVICE, None, None) == _lib.SC_OK
    assert sc.GKRRoundSumcheck.prove_batch([], [], [], [], []) == []


def test_null_arrays_are_bad_arguments():
    inst = _instances(3, 3, 100)
    for name in ("rngs", "f1_idx", "f1_vals", "nnz", "f2", "f3", "g", "out"):
        rc, msg = _raw_call(3, 3, *inst, override={name: None})
        assert rc == _lib.SC_ERR_BAD_ARG and msg.startswith("instance 0: ") and "null" in msg, (name, rc, msg)


def test_a_null_entry_names_its_instance():
    inst = _instances(4, 3, 110)
    for name, src in (("f2", inst[2]), ("f3", inst[3])):
        vals = [f.evaluations.ctypes.data for f in src]
        vals[2] = None
        rc, msg = _raw_call(4, 3, *inst, override={name: (C.c_void_p * 4)(*vals)})
        assert rc == _lib.SC_ERR_BAD_ARG and msg.startswith("instance 2: ") and "null" in msg, (name, rc, msg)
    gv = [g.ctypes.data for g in inst[4]]
    gv[1] = None
    rc, msg = _raw_call(4, 3, *inst, override={"g": (C.c_void_p * 4)(*gv)})
    assert rc == _lib.SC_ERR_BAD_ARG and msg.startswith("instance 1: "), msg
    iv = [f._ptrs()[0] for f in inst[1]]
    iv = [C.cast(v, C.c_void_p) for v in iv]
    iv[3] = None
    rc, msg = _raw_call(4, 3, *inst, override={"f1_idx": (C.c_void_p * 4)(*iv)})
    assert rc == _lib.SC_ERR_BAD_ARG and msg.startswith("instance 3: "), msg


def test_a_null_or_repeated_rng_is_a_bad_argument_and_the_lowest_instance_decides():
    inst = _instances(5, 2, 120)
    hs = [r._h for r in inst[0]]
    rc, msg = _raw_call(5, 2, *inst, override={"rngs": (C.c_void_p * 5)(hs[0], hs[1], None, hs[3], hs[1])})
    assert rc == _lib.SC_ERR_BAD_ARG and msg.startswith("instance 2: ") and "null rng" in msg, msg
    rc, msg = _raw_call(5, 2, *inst, override={"rngs": (C.c_void_p * 5)(hs[0], hs[1], hs[2], hs[1], None)})
    assert rc == _lib.SC_ERR_BAD_ARG and msg.startswith("instance 3: ") and "rng" in msg, msg
    assert _untouched(inst[0]), "an argument error leaves every transcript where it was"


def test_a_non_canonical_g_names_its_instance_and_element():
    inst = _instances(4, 3, 130)
    inst[4][2][1] = np.array([0xffffffffffffffff] * 4, dtype=np.uint64)
    with pytest.raises(sc.SumcheckError) as e:
        sc.GKRRoundSumcheck.prove_batch(*inst)
    assert e.value.code == _lib.SC_ERR_BAD_ARG and e.value.msg.startswith("instance 2: g[1]") and "canonical" in e.value.msg
    p_limbs = np.array([(po.P >> (64 * i)) & 0xffffffffffffffff for i in range(4)], dtype=np.uint64)
    inst = _instances(2, 3, 131)
    inst[4][0][0] = p_limbs  # p itself is not canonical
    with pytest.raises(sc.SumcheckError) as e:
        sc.GKRRoundSumcheck.prove_batch(*inst)
    assert e.value.code == _lib.SC_ERR_BAD_ARG and e.value.msg.startswith("instance 0: g[0]")


def test_a_host_index_out_of_range_names_the_lowest_instance_and_advances_no_transcript():
    dim = 3
    inst = _instances(6, dim, 140)
    inst[1][4].indices[5] = np.uint64(1) << np.uint64(3 * dim)
    inst[1][2].indices[0] = np.uint64(1) << np.uint64(63)
    with pytest.raises(sc.SumcheckError) as e:
        sc.GKRRoundSumcheck.prove_batch(*inst)
    assert e.value.code == _lib.SC_ERR_BAD_ARG and e.value.msg.startswith("instance 2: ") and "out of range" in e.value.msg
    assert _untouched(inst[0])


def test_dim_zero_is_a_constant_and_dim_22_does_not_fit():
    inst = _instances(2, 1, 150)
    rc, msg = _raw_call(2, 0, *inst)
    assert rc == _lib.SC_ERR_CONSTANT_POLY and msg.startswith("instance 0: ") and "Attempt to prove a constant." in msg
    rc, msg = _raw_call(2, 22, *inst)
    assert rc == _lib.SC_ERR_BAD_ARG and msg.startswith("instance 0: ") and "dim 22" in msg


def test_a_valid_batch_fails_loudly_without_a_device():
    if sc.lib().sc_device_count() > 0:
        pytest.skip("a HIP device is visible")
    inst = _instances(3, 4, 160)
    with pytest.raises(sc.SumcheckError) as e:
        sc.GKRRoundSumcheck.prove_batch(*inst)
    assert e.value.code == _lib.SC_ERR_HIP and "no CPU fallback" in e.value.msg
    assert _untouched(inst[0])


def _build_cpp():
    from tests import test_cpp_mirror as M
    src = os.path.join(ROOT, "tests", "cpp", "test_gkr_batch_mirror.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "test_gkr_batch_mirror.bin")
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, "-o", out, "-L", M.LIBDIR, "-lsumcheck_hip", f"-Wl,-rpath,{M.LIBDIR}",
           "-Wl,-rpath,/opt/rocm/lib"]  # tests/test_cpp_mirror.py::build_cpp's command line, for this source
    subprocess.check_call(cmd)
    return out


def test_cpp_mirror_prove_batch_compiles_links_and_reports():
    """the C++ mirror's GKRRoundSumcheck::prove_batch against the C ABI: with a device its proofs and transcripts equal prove's instance by
    instance, without one the mirror's Panic carries the library's "no CPU fallback" """
    out = subprocess.run([_build_cpp()], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    if sc.lib().sc_device_count() > 0:
        assert out.returncode == 0 and "ALL TESTS PASSED" in out.stdout, out.stdout + out.stderr
    else:
        assert out.returncode == 3 and "no CPU fallback" in out.stdout, out.stdout + out.stderr
