"""CPU tests of the sliced rounds of the batched interactive provers: the policy key "batch_slices" and the plan batch.rounds_slices through
the library and the header, the rule of sumcheck_amd/csrc/batch_slices.hpp walked over every shape by a stand-alone C++ program (compiled
for the HOST under AddressSanitizer and UndefinedBehaviorSanitizer, as tests/test_lag_index_host.py compiles its own), the recorded kernel
resources, and the argument checks of sc_batch_prover_init, which do not depend on the key.  The values: tests/test_gpu_batch_round_slices.py."""
import os
import re
import subprocess

import pytest

import sumcheck_amd as sc
from sumcheck_amd import _lib
from tests import test_batch_rounds_host as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_batch_slices.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "test_batch_slices.bin")
HDR = open(os.path.join(ROOT, "include", "sumcheck_hip.h")).read()


def test_the_key_defaults_to_zero_and_takes_zero_and_one():
    assert _lib.get_policy("batch_slices") == 0
    try:
        _lib.set_policy("batch_slices", 1)
        assert _lib.get_policy("batch_slices") == 1
        with pytest.raises(sc.SumcheckError) as e:
            _lib.set_policy("batch_slices", 2)
        assert e.value.code == _lib.SC_ERR_BAD_ARG and e.value.msg == "policy batch_slices takes 0..1"
        assert _lib.get_policy("batch_slices") == 1, "a refused value changes nothing"
        with pytest.raises(sc.SumcheckError):
            _lib.set_policy("batch_slices", -1)
    finally:
        _lib.set_policy("batch_slices", 0)
    with _lib.policy(batch_slices=1):
        assert _lib.get_policy("batch_slices") == 1
    assert _lib.get_policy("batch_slices") == 0


def test_the_plan_is_named_in_front_of_the_gkr_plans():
    names = list(_lib.plan_stats())
    assert len(names) == sc.lib().sc_plan_count()
    i = names.index("batch.rounds_slices")
    assert names[i + 1] == "gkr.bucketed_grouped" and names[i - 1] == "sharded.gather_tail"
    assert names.count("batch.rounds_slices") == 1 and len(set(names)) == len(names)


def test_the_header_names_the_key_and_the_plan():
    assert '"batch_slices"' in HDR and "batch.rounds_slices" in HDR
    assert re.search(r'^ \*   "batch_slices" \(0\) ', HDR, re.M), "the policy list names the key with its default"
    assert "#define SC_ABI_VERSION 5" in HDR and set(BR.NAMES) == set(_lib.SIGNATURES_EXT), "no new entry point, no ABI version change"


def test_the_kernel_source_is_built_and_the_new_kernels_use_no_scratch():
    from sumcheck_amd import build
    assert "kernels_batch_round_slices.hip" in build.SOURCES and "batch_slices.hpp" in build.HEADERS
    prof = open(os.path.join(ROOT, "profiles", "batch_round_slices_kernel_resources.txt")).read()
    for kernel in (r"k_batch_round_slicesILi8\S*", r"k_batch_round_fin\S*"):
        m = re.search(rf"^{kernel} VGPR (\d+) AGPR 0 scratch (\d+) occ (\d+) ", prof, re.M)
        assert m and int(m.group(2)) == 0 and int(m.group(1)) <= 128, kernel
    m = re.search(r"^k_batch_round_slicesILi8\S* VGPR \d+ AGPR 0 scratch 0 occ (\d+) LDS (\d+)", prof, re.M)
    assert int(m.group(1)) >= 3 and 3 * (48 * 1024 + int(m.group(2))) <= 160 * 1024, "three blocks of a sliced launch share a CU: registers and LDS"


def test_batch_slices_header_on_the_host_under_sanitizers():
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "sumcheck_amd", "csrc"), SRC, "-o", BIN]
    subprocess.check_call(cmd)
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL TESTS PASSED" in out.stdout


def _argument_errors():
    """(status, text) of every argument check of sc_batch_prover_init that tests/test_batch_rounds_host.py walks"""
    got = []
    arr, keep = BR._descs([BR._poly(3, [[0, 1, 2]], 400 + i) for i in range(2)])
    got += [BR._init(None, 2), BR._init(arr, 2, out=False), BR._init(arr, 0)]
    polys = [BR._poly(3, [[0, 1, 2], [1, 2]], 410 + i) for i in range(4)]
    polys[2] = BR._poly(3, [[0, 1, 2], [0, 2]], 99)
    arr, keep = BR._descs(polys)
    got.append(BR._init(arr, 4))
    polys[2], polys[3] = polys[0], BR._poly(4, [[0, 1, 2], [1, 2]], 98)
    arr, keep = BR._descs(polys)
    got.append(BR._init(arr, 4))
    arr, keep = BR._descs([BR._poly(2, [[0, 1]], 420 + i) for i in range(3)])
    for i in range(3):
        arr[i].num_vars = 0
    got.append(BR._init(arr, 3))
    polys = [BR._poly(12, [[0, 1, 2], [1]], 430 + i) for i in range(3)]  # (a shape of the sliced plan)
    arr, keep = BR._descs(polys)
    arr[1].max_multiplicands = 2
    got.append(BR._init(arr, 3))
    return got


def test_the_argument_checks_do_not_depend_on_the_key():
    base = _argument_errors()
    assert [rc for rc, _ in base] == [_lib.SC_ERR_BAD_ARG] * 5 + [_lib.SC_ERR_CONSTANT_POLY, _lib.SC_ERR_BAD_ARG]
    assert base[3][1] == "instance 2 differs from instance 0 in prod_indices: a batch has one structure"
    assert base[6][1].startswith("instance 1: max_multiplicands 2 != max product length 3")
    with _lib.policy(batch_slices=1):
        assert _argument_errors() == base
