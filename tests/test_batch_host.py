"""CPU tests of sc_ml_prove_batch's host side: the symbol through every mirror (header, library, ctypes table, Rust shim, C++ header), the
policy key and the two launch plans, and the argument checks, which run before any HIP call and so behave the same with and without a
device.  The proofs themselves are tests/test_gpu_batch.py's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _poly(nv, shapes, seed, n_tables=None):
    nt = n_tables or (max(max(s) for s in shapes) + 1)
    tabs = [cref.synth_table(seed, s, 1 << nv) for s in range(nt)]
    coefs = cref.synth_table(seed, 1000, len(shapes))
    mles = [sc.DenseMultilinearExtension(nv, t) for t in tabs]
    poly = sc.ListOfProductsOfPolynomials(nv)
    for k, sh in enumerate(shapes):
        poly.add_product([mles[i] for i in sh], coefs[k])
    return poly


def test_the_symbol_is_declared_exported_and_in_the_signature_table():
    hdr = open(os.path.join(ROOT, "include", "sumcheck_hip.h")).read()
    assert re.search(r"SC_API\s+int\s+sc_ml_prove_batch\s*\(\s*const sc_poly_desc \*descs,\s*uint32_t n,\s*sc_rng \*const \*rngs_or_null", hdr)
    assert "#define SC_ABI_VERSION 5" in hdr and "sc_ml_prove_batch" in hdr.split("#define SC_ABI_VERSION 5", 1)[1].split("\n", 1)[0]
    assert hasattr(C.CDLL(_lib.SO_PATH), "sc_ml_prove_batch")
    assert "sc_ml_prove_batch" in _lib.SIGNATURES
    assert sc.lib().sc_abi_version() == 5


def test_the_rust_shim_declares_it_and_wraps_it():
    rs = open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()
    block = re.search(r'extern "C" \{(.*?)\n\}', rs, re.S).group(1)
    assert re.search(r"pub fn sc_ml_prove_batch\s*\(descs: \*const sc_poly_desc, n: u32, rngs_or_null: \*const \*mut sc_rng,", block)
    assert re.search(r"pub fn prove_batch<F: Limbs4>\(polynomials: &\[ListOfProductsOfPolynomials<F>\]\) -> Vec<Proof<F>>", rs)


def test_policy_batch_round_trips_and_rejects_three():
    old = _lib.get_policy("batch")
    assert old == 1
    try:
        for v in (0, 2, 1):
            _lib.set_policy("batch", v)
            assert _lib.get_policy("batch") == v
        with pytest.raises(sc.SumcheckError) as e:
            _lib.set_policy("batch", 3)
        assert e.value.code == _lib.SC_ERR_BAD_ARG
        assert _lib.get_policy("batch") == 1
    finally:
        _lib.set_policy("batch", old)


def test_both_plans_are_listed():
    names = list(_lib.plan_stats())
    assert "batch.one_block" in names and "batch.serial" in names


def test_an_empty_batch_is_ok_and_touches_nothing():
    assert sc.lib().sc_ml_prove_batch(None, 0, None, None, None) == _lib.SC_OK
    assert sc.MLSumcheck.prove_batch([]) == []


def test_a_constant_instance_decides_the_status():
    polys = [_poly(3, [[0, 1, 2]], 7 + i) for i in range(5)]
    polys[3] = sc.ListOfProductsOfPolynomials(0)
    t = sc.DenseMultilinearExtension(0, cref.synth_table(3, 0, 1))
    polys[3].add_product([t, t, t], cref.synth_table(3, 1000, 1)[0])
    with pytest.raises(sc.SumcheckError) as e:
        sc.MLSumcheck.prove_batch(polys)
    assert e.value.code == _lib.SC_ERR_CONSTANT_POLY
    assert "Attempt to prove a constant" in e.value.msg and "instance 3" in e.value.msg


def test_a_descriptor_of_another_structure_is_named():
    polys = [_poly(3, [[0, 1, 2], [1, 2]], 11 + i) for i in range(4)]
    polys[2] = _poly(3, [[0, 1, 2], [0, 2]], 99)  # the same counts, other prod_indices
    with pytest.raises(sc.SumcheckError) as e:
        sc.MLSumcheck.prove_batch(polys)
    assert e.value.code == _lib.SC_ERR_BAD_ARG
    assert "instance 2" in e.value.msg and "prod_indices" in e.value.msg
    polys[2] = _poly(4, [[0, 1, 2], [1, 2]], 99)
    with pytest.raises(sc.SumcheckError) as e:
        sc.MLSumcheck.prove_batch(polys)
    assert e.value.code == _lib.SC_ERR_BAD_ARG and "instance 2" in e.value.msg and "num_vars" in e.value.msg


def test_one_rng_per_polynomial():
    polys = [_poly(2, [[0, 1]], 5 + i) for i in range(3)]
    with pytest.raises(ValueError):
        sc.MLSumcheck.prove_batch(polys, rngs=[sc.Blake2b512Rng.setup()])


def test_a_valid_batch_fails_loudly_without_a_device():
    if sc.lib().sc_device_count() > 0:
        pytest.skip("a HIP device is visible")
    polys = [_poly(4, [[0, 1, 2]], 21 + i) for i in range(3)]
    with pytest.raises(sc.SumcheckError) as e:
        sc.MLSumcheck.prove_batch(polys)
    assert e.value.code == _lib.SC_ERR_HIP and "no CPU fallback" in e.value.msg


def _build_batch_cpp():
    from tests import test_cpp_mirror as M
    src = os.path.join(ROOT, "tests", "cpp", "test_batch_mirror.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "test_batch_mirror.bin")
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, "-o", out, "-L", M.LIBDIR, "-lsumcheck_hip", f"-Wl,-rpath,{M.LIBDIR}",
           "-Wl,-rpath,/opt/rocm/lib"]  # tests/test_cpp_mirror.py::build_cpp's command line, for this source
    subprocess.check_call(cmd)
    return out


def test_cpp_mirror_prove_batch_compiles_links_and_reports():
    """the C++ mirror's prove_batch against the C ABI: with a device its proofs equal MLSumcheck::prove's, without one the mirror's Panic
    carries the library's "no CPU fallback" """
    out = subprocess.run([_build_batch_cpp()], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    if sc.lib().sc_device_count() > 0:
        assert out.returncode == 0 and "ALL TESTS PASSED" in out.stdout, out.stdout + out.stderr
    else:
        assert out.returncode == 3 and "no CPU fallback" in out.stdout, out.stdout + out.stderr
