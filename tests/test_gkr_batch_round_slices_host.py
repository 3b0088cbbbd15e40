"""CPU tests of the sliced plan of the batched interactive GKR rounds (sc_gkr_batch_prover_* at dim 10 .. 16 under policy "batch_slices" = 1,
plan batch.gkr_rounds_slices): the plan's name through the library and the header, the rule of sumcheck_amd/csrc/batch_slices.hpp
(gkr_bs_plan) walked by a stand-alone C++ program (compiled for the HOST under AddressSanitizer and UndefinedBehaviorSanitizer, as
tests/test_batch_round_slices_host.py compiles its own), the recorded kernel resources, and the argument checks of
sc_gkr_batch_prover_init, which do not depend on the key.  The values: tests/test_gpu_gkr_batch_round_slices.py."""
import os
import re
import subprocess

import numpy as np

import sumcheck_amd as sc
from sumcheck_amd import _lib
from tests import test_gkr_batch_rounds_host as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_gkr_batch_slices.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "test_gkr_batch_slices.bin")
HDR = open(os.path.join(ROOT, "include", "sumcheck_hip.h")).read()
NAME = "batch.gkr_rounds_slices"


def test_the_plan_is_named_directly_behind_gkr_bucketed_counted():
    names = list(_lib.plan_stats())
    assert len(names) == sc.lib().sc_plan_count()
    i = names.index(NAME)
    assert names[i - 1] == "gkr.bucketed_counted" and names[i + 1] == "gkr.list_form"
    assert names.count(NAME) == 1 and len(set(names)) == len(names)
    assert [sc.lib().sc_plan_name(k).decode() for k in range(len(names))] == names and sc.lib().sc_plan_name(len(names)) is None


def test_the_neighbours_other_tests_pin_are_where_they_were():
    names = list(_lib.plan_stats())
    i = names.index("batch.rounds_slices")
    assert names[i - 1] == "sharded.gather_tail" and names[i + 1] == "gkr.bucketed_grouped"
    i = names.index("gkr.sharded")
    assert names[i - 3:i] == ["gkr.coeff_from_bound_table", "batch.gkr_rounds_one_block", "batch.gkr_rounds_serial"]
    assert names[-9:] == ["fold_multi", "batch.eval_one_block", "batch.eval_serial", "batch.gkr_eval_one_block", "batch.gkr_eval_serial", "batch.one_block",
                          "batch.serial", "batch.gkr_one_block", "batch.gkr_serial"]


def test_the_header_names_the_plan_and_keeps_the_key_line_and_the_abi():
    assert NAME in HDR
    assert re.search(r'^ \*   "batch_slices" \(0\) ', HDR, re.M), "the policy list names the key with its default, in its format"
    key_line = [l for l in HDR.splitlines() if l.startswith(' *   "batch_slices" (0) ')][0]
    assert "sc_gkr_batch_prover_init" in key_line
    assert "#define SC_ABI_VERSION 5" in HDR and set(GR.NAMES) == set(_lib.SIGNATURES_GKRB), "no new entry point, no ABI version change"
    assert _lib.get_policy("batch_slices") == 0, "the default stays"


def test_the_kernel_source_is_built_and_the_new_kernels_use_no_scratch():
    from sumcheck_amd import build
    assert "kernels_batch_gkr_round_slices.hip" in build.SOURCES and "batch_slices.hpp" in build.HEADERS
    prof = open(os.path.join(ROOT, "profiles", "gkr_batch_round_slices_kernel_resources.txt")).read()
    for kernel in ("k_batch_gkr_terms", "k_batch_gkr_fold"):
        for phase in (1, 2):
            m = re.search(rf"^{kernel}ILi{phase}\S* VGPR (\d+) AGPR 0 scratch (\d+) occ (\d+) LDS (\d+)", prof, re.M)
            assert m and int(m.group(2)) == 0 and int(m.group(1)) <= 128, (kernel, phase)
            if kernel == "k_batch_gkr_terms":  # two half tables of at most 2^8 elements per point, and the points
                assert int(m.group(4)) <= phase * (2 * 256 * 32 + 16 * 32) + 64, (kernel, phase, m.group(4))
    # the kernels that share bg_build_eq's header keep their committed register counts
    old = open(os.path.join(ROOT, "profiles", "gkr_batch_rounds_kernel_resources.txt")).read()
    for kernel in (r"k_batch_gkrENS\S*", r"k_batch_gkr_phaseILi1\S*", r"k_batch_gkr_phaseILi2\S*"):
        a, b = (re.search(rf"^{kernel} VGPR (\d+) AGPR 0 scratch 0 ", t, re.M) for t in (old, prof))
        assert a and b and a.group(1) == b.group(1), kernel
    old = open(os.path.join(ROOT, "profiles", "batch_round_slices_kernel_resources.txt")).read()
    a, b = (re.search(r"^k_batch_proofsILi8\S* VGPR (\d+) AGPR 0 scratch 0 ", t, re.M) for t in (old, prof))
    assert a and b and a.group(1) == b.group(1), "k_batch_proofs"


def test_the_plan_rule_on_the_host_under_sanitizers():
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "sumcheck_amd", "csrc"), SRC, "-o", BIN]
    subprocess.check_call(cmd)
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL TESTS PASSED" in out.stdout


def _argument_errors():
    """(status, text) of every argument check of sc_gkr_batch_prover_init that tests/test_gkr_batch_rounds_host.py walks, at a dim of the
    sliced plan where the check reads the arrays"""
    got = []
    keep = GR._args(2, 3)
    got += [GR._init(keep, 2, 3, null=k) for k in range(6)] + [GR._init(keep, 2, 3, out=False), GR._init(keep, 0, 3)]
    got += [GR._init(GR._args(2, 0), 2, 0), GR._init(GR._args(1, 2), 1, 22)]
    keep = GR._args(3, 10)
    keep[1][4] = keep[1][4].copy()
    keep[1][4][9] = GR.P_LIMBS
    got.append(GR._init(keep, 3, 10))
    keep = GR._args(3, 10)
    keep[2][0] = keep[2][0].copy()
    keep[2][0][7] |= np.uint64(1) << np.uint64(30)  # a bit at 3 dim
    got.append(GR._init(keep, 3, 10))
    return got


def test_the_argument_checks_do_not_depend_on_the_key():
    base = _argument_errors()
    assert [rc for rc, _ in base] == [_lib.SC_ERR_BAD_ARG] * 8 + [_lib.SC_ERR_CONSTANT_POLY] + [_lib.SC_ERR_BAD_ARG] * 3
    assert base[10][1] == "instance 1: g[9] is not a canonical field element" and base[11][1] == "instance 2: f1 index 7 out of range"
    with _lib.policy(batch_slices=1):
        assert _argument_errors() == base
    with _lib.policy(batch_slices=1, batch=0):
        assert _argument_errors() == base
