"""CPU tests of sc_gkr_layers_eval_batch (GKRRoundSumcheck.evaluate_layers_batch): the big-integer definition of
tests/gkr_layers_eval_cases.py against oracle/pyoracle.py; the prototype under its own marker SC_API_GKRE against the shim's declaration
and the ctypes table, by the rules of tests/test_gkr_two_point_host.py; the older scanners, none of which may see the name; the wrappers
of every mirror; the argument errors that need no device; the plans' names.  The values themselves are tests/test_gpu_gkr_layers_eval.py's."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import sumcheck_amd as sc
from oracle import cref, pyoracle
from sumcheck_amd import _lib
from tests import gkr_layers_eval_cases as K
from tests import test_gkr_batch_rounds_host as GR
from tests import test_gkr_next_layer_host as NH
from tests import test_rust_shim as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = cref.P
NAME = K.NAME
HDR = open(os.path.join(ROOT, "include", "sumcheck_hip.h")).read()
PP = "*const *const u64"
PARAMS = ["u32", "u32", "u32", PP, PP, "*const u64", PP, PP, "u32", "*const *mut u64"]


# ---- the definition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_the_definition_equals_pyoracles_phase_one_and_the_extension_of_the_layer(dim):
    """for a boolean point g = bits(z), sum_x initialize_phase_one(f1, f3, g)[x] f2[x] is cell z; for a random g it is the multilinear
    extension of the layer at g -- the claim a layer's sumcheck starts from"""
    N = 1 << dim
    idx, vals = K.wiring(dim, 81000 + dim, 3 * N, "repeated")
    f2, f3 = cref.mont_to_ints(cref.synth_table(81100 + dim, 2, N)), cref.mont_to_ints(cref.synth_table(81100 + dim, 3, N))
    w = K.define_layer(idx, cref.mont_to_ints(vals), dim, f2, f3)
    assert any(w) and len(set(int(i) for i in idx)) < len(idx), "repeated indices, something to compare"
    f1 = {}
    for i, v in zip(idx, cref.mont_to_ints(vals)):
        f1[int(i)] = (f1.get(int(i), 0) + v) % P  # (repeated indices add up: the dictionary form of the same list)
    for z in range(N):
        g = [(z >> j) & 1 for j in range(dim)]
        h, _ = pyoracle.initialize_phase_one(f1, 3 * dim, f3, g)
        assert sum(hx * ax for hx, ax in zip(h, f2)) % P == w[z], z
    g = cref.mont_to_ints(cref.synth_table(81200 + dim, 4, dim))
    h, _ = pyoracle.initialize_phase_one(f1, 3 * dim, f3, g)
    assert sum(hx * ax for hx, ax in zip(h, f2)) % P == pyoracle.dense_evaluate(w, g)


def test_the_chained_definition_feeds_a_layer_to_both_sides_of_the_next():
    dim = 2
    N = 1 << dim
    layers = [K.wiring(dim, 82000 + k, [5, 0, 7][k], "random") for k in range(3)]
    f2, f3 = cref.synth_table(82100, 2, N), cref.synth_table(82100, 3, N)
    out = K.define_layers(layers, f2, f3, dim)
    w0 = K.define_layer(layers[0][0], cref.mont_to_ints(layers[0][1]), dim, cref.mont_to_ints(f2), cref.mont_to_ints(f3))
    assert cref.mont_to_ints(out[0]) == w0 and not out[1].any() and not out[2].any(), "an empty layer is zero, and so is everything above it"
    sq = K.define_layers([layers[0], layers[2]], f2, f3, dim)
    assert cref.mont_to_ints(sq[1]) == K.define_layer(layers[2][0], cref.mont_to_ints(layers[2][1]), dim, w0, w0) and sq[1].any()


# ---- the prototype -------------------------------------------------------------------------------------------------------------------
def _header_prototypes():
    """the SC_API_GKRE prototypes, parameter types in the shim's spelling (tests/test_gkr_next_layer_host.py's reading)"""
    protos = {}
    for m in re.finditer(r"SC_API_GKRE\s+([^;(]+?)\b(sc_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", HDR, re.S):
        ret, name, params = m.group(1).strip(), m.group(2), " ".join(m.group(3).split())
        plist = [RS.c_type_to_rust(re.match(r"(.*?)([A-Za-z_][A-Za-z_0-9]*)$", prm.strip()).group(1)) for prm in params.split(",")]
        protos[name] = (plist, None if ret == "void" else RS.c_type_to_rust(ret))
    return protos


def test_the_symbol_is_declared_exported_and_in_its_own_signature_table():
    protos = _header_prototypes()
    assert set(protos) == {NAME} == set(_lib.SIGNATURES_GKRE)
    assert protos[NAME] == (PARAMS, "c_int")
    assert re.search(r"#define SC_API_GKRE SC_API /\*[^\n]*\*/\n", HDR), "SC_API with only a comment behind it on the line"
    version_line = HDR.split("#define SC_ABI_VERSION 5", 1)[1].split("\n", 1)[0]
    assert not NAME.startswith("sc_gkr_batch_") and NAME in version_line and hasattr(C.CDLL(_lib.SO_PATH), NAME)
    res, args = _lib.SIGNATURES_GKRE[NAME]
    assert res is C.c_int and len(args) == len(PARAMS)
    assert all(NAME not in table for table in (_lib.SIGNATURES, _lib.SIGNATURES_EXT, _lib.SIGNATURES_GKRB, _lib.SIGNATURES_GKRL, _lib.SIGNATURES_GKR2))
    assert sc.lib().sc_abi_version() == 5 and sc.lib().sc_gkr_layers_eval_batch.argtypes == args


def test_none_of_the_older_scanners_sees_the_name_and_their_closed_sets_hold():
    from tests import test_gkr_two_point_host as TP
    for marker in ("SC_API", "SC_API_EXT", "SC_API_GKRB", "SC_API_GKRL", "SC_API_GKR2"):
        names = [m.group(2) for m in re.finditer(marker + r"\s+([^;(]+?)\b(sc_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", HDR, re.S)]
        assert names and NAME not in names, marker
    assert NAME not in RS.header_prototypes()
    assert set(GR._header_prototypes()) == set(GR.NAMES)
    assert set(NH._header_prototypes()) == {NH.NAME} == set(_lib.SIGNATURES_GKRL)
    assert set(TP._header_prototypes()) == {TP.INIT, TP.NEXT} == set(_lib.SIGNATURES_GKR2)
    rs = open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()
    assert not re.search(r"pub\s+fn\s+" + NAME + r"\b", rs), "a private declaration: the shim's pub externs are SC_API prototypes"


def test_the_shim_declares_it_as_the_header_does_and_wraps_it():
    rs = open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()
    found = []
    for block in re.findall(r'extern "C" \{(.*?)\n\}', rs, re.S):
        for m in re.finditer(r"\bfn (" + NAME + r")\s*\((.*?)\)\s*(?:->\s*([^;]+?))?\s*;", block, re.S):
            assert len(re.findall(r"\bfn\s+sc_", block)) == 1, "a block of its own"
            params = " ".join(m.group(2).split())
            found.append(([p.split(":", 1)[1].strip() for p in params.split(",") if p.strip()], m.group(3).strip() if m.group(3) else None))
    assert found == [_header_prototypes()[NAME]], found
    assert re.search(r"pub fn gkr_evaluate_layers_batch<F: Limbs4>\(", rs)


def test_every_mirror_wraps_it_and_the_documents_name_it():
    hpp = open(os.path.join(ROOT, "include", "sumcheck_amd.hpp")).read()
    assert NAME in hpp and "evaluate_layers_batch(" in hpp
    assert list(inspect.signature(sc.GKRRoundSumcheck.evaluate_layers_batch).parameters) == ["f1_layers", "f2s", "f3s"]
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert NAME in text and K.ONE_BLOCK in text and K.CELLS in text, doc
    assert "gkr_evaluate_layers_batch" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    from sumcheck_amd import build
    assert "kernels_batch_gkr_eval_layers.hip" in build.SOURCES


# ---- argument errors that need no device -----------------------------------------------------------------------------------------------
class Args:
    """n instances x n_layers layers of host arrays at dim, every array its own; fields may be replaced before call()"""

    def __init__(self, n, dim, n_layers, nnz=3):
        N = 1 << dim
        self.n, self.dim, self.n_layers = n, dim, n_layers
        total = n * n_layers
        self.idx = [np.arange(nnz, dtype=np.uint64) % np.uint64(1 << (3 * dim)) for _ in range(total)]
        self.vals = [cref.synth_table(83000 + r, 1, nnz) for r in range(total)]
        self.nnz = [nnz] * total
        self.f2 = [cref.synth_table(83100 + i, 2, N) for i in range(n)]
        self.f3 = [cref.synth_table(83100 + i, 3, N) for i in range(n)]
        self.out = [np.full((N, 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64) for _ in range(total)]

    def call(self, flags=0, **null):
        ptrs = lambda arrs: (C.c_void_p * max(len(arrs), 1))(*[None if a is None else (a if isinstance(a, int) else a.ctypes.data) for a in arrs])
        nnz = (C.c_uint64 * max(len(self.nnz), 1))(*self.nnz)
        a = {"f1_idx": ptrs(self.idx), "f1_vals": ptrs(self.vals), "nnz": nnz, "f2": ptrs(self.f2), "f3": ptrs(self.f3), "out": ptrs(self.out)}
        for k in null:
            a[k] = None
        rc = sc.lib().sc_gkr_layers_eval_batch(self.n, self.dim, self.n_layers, a["f1_idx"], a["f1_vals"], a["nnz"], a["f2"], a["f3"], flags, a["out"])
        return rc, sc.lib().sc_last_error().decode()


def _reaches_the_device(rc, msg):
    return rc == _lib.SC_OK or (rc == _lib.SC_ERR_HIP and "no HIP device" in msg)


def test_null_arguments_and_null_entries_name_the_lowest_layer_and_instance():
    for name in ("f1_idx", "f1_vals", "nnz", "f2", "f3", "out"):
        rc, msg = Args(2, 2, 2).call(**{name: True})
        assert rc == _lib.SC_ERR_BAD_ARG and "null argument" in msg, name
    a = Args(3, 2, 2)
    a.out[1 * 3 + 2] = None
    a.vals[1 * 3 + 0] = None
    assert a.call() == (_lib.SC_ERR_BAD_ARG, "layer 1 instance 0: null argument"), "the lowest failing (layer, instance) decides"
    a.idx[0 * 3 + 2] = None
    assert a.call() == (_lib.SC_ERR_BAD_ARG, "layer 0 instance 2: null argument")
    a.f3[1] = None
    assert a.call() == (_lib.SC_ERR_BAD_ARG, "layer 0 instance 1: null argument")
    b = Args(2, 2, 2)
    b.idx[1], b.vals[1], b.nnz[1] = None, None, 0  # an empty list needs no arrays
    assert _reaches_the_device(*b.call())


def test_dim_and_nnz_out_of_range():
    rc, msg = Args(2, 1, 1).call()
    assert _reaches_the_device(rc, msg)
    a = Args(2, 1, 1)
    a.dim = 0
    assert a.call()[0] == _lib.SC_ERR_CONSTANT_POLY
    a.dim = 22
    rc, msg = a.call()
    assert rc == _lib.SC_ERR_BAD_ARG and "dim 22" in msg
    b = Args(2, 2, 2)
    b.nnz[1 * 2 + 1] = 1 << 31  # (refused before anything is read)
    rc, msg = b.call()
    assert rc == _lib.SC_ERR_BAD_ARG and msg.startswith("layer 1 instance 1: nnz too large")
    b.nnz[1 * 2 + 1] = 3
    assert _reaches_the_device(*b.call())


def test_a_host_index_with_a_bit_at_3_dim_is_refused_and_nothing_is_written():
    a = Args(2, 2, 3)
    a.idx[2 * 2 + 1] = a.idx[2 * 2 + 1].copy()
    a.idx[2 * 2 + 1][2] = np.uint64(1) << np.uint64(3 * 2)
    a.idx[1 * 2 + 0] = a.idx[1 * 2 + 0].copy()
    a.idx[1 * 2 + 0][0] = np.uint64(1) << np.uint64(63)
    assert a.call() == (_lib.SC_ERR_BAD_ARG, "layer 1 instance 0: f1 has an index out of range")
    a.idx[1 * 2 + 0][0] = 5
    assert a.call() == (_lib.SC_ERR_BAD_ARG, "layer 2 instance 1: f1 has an index out of range")
    assert all((o == np.uint64(0x5A5A5A5A5A5A5A5A)).all() for o in a.out)
    a.idx[2 * 2 + 1][2] = (1 << 6) - 1  # the largest index in range
    assert _reaches_the_device(*a.call())


def test_an_output_may_not_overlap_an_input_or_another_output():
    a = Args(2, 2, 2)
    a.out[1 * 2 + 1] = a.f2[0]
    rc, msg = a.call()
    assert (rc, msg) == (_lib.SC_ERR_BAD_ARG, "layer 1 instance 1: the output overlaps an input")
    a = Args(2, 2, 2)
    a.out[3] = a.out[0]
    assert a.call() == (_lib.SC_ERR_BAD_ARG, "layer 0 instance 0: the output overlaps another output")
    a = Args(2, 2, 2)
    big = np.zeros((6, 4), dtype=np.uint64)  # two tables of four entries that share two
    a.out[1], a.out[2] = big[:4], big[2:].ctypes.data
    assert a.call() == (_lib.SC_ERR_BAD_ARG, "layer 0 instance 1: the output overlaps another output")
    a = Args(2, 2, 2, nnz=8)
    a.out[2] = a.vals[1].ctypes.data + 32 * 7  # the last value of a list
    assert a.call() == (_lib.SC_ERR_BAD_ARG, "layer 1 instance 0: the output overlaps an input")
    a = Args(2, 2, 2)
    a.idx, a.vals, a.f3 = [a.idx[0]] * 4, [a.vals[0]] * 4, [a.f2[0], a.f2[0]]  # inputs may repeat, across instances and layers
    assert _reaches_the_device(*a.call())


def test_nothing_to_do_is_ok_and_touches_nothing():
    assert sc.lib().sc_gkr_layers_eval_batch(0, 0, 3, None, None, None, None, None, 0, None) == _lib.SC_OK
    assert sc.lib().sc_gkr_layers_eval_batch(3, 0, 0, None, None, None, None, None, 0, None) == _lib.SC_OK
    assert sc.GKRRoundSumcheck.evaluate_layers_batch([], [], []) == [] and sc.GKRRoundSumcheck.evaluate_layers_batch([[], []], [], []) == [[], []]


# ---- the plans -----------------------------------------------------------------------------------------------------------------------
def test_the_plans_are_named_and_every_position_test_still_holds():
    names = list(_lib.plan_stats())
    assert K.ONE_BLOCK in names and K.CELLS in names and len(names) == sc.lib().sc_plan_count()
    assert K.ONE_BLOCK in HDR and K.CELLS in HDR
    assert names.index(K.CELLS) == names.index(K.ONE_BLOCK) + 1
    NH.test_the_plan_sits_between_the_two_bucketed_gkr_plans()
    assert K.one_block_fits(9, 64 << 9) and not K.one_block_fits(9, (64 << 9) + 1) and not K.one_block_fits(10, 1)


def test_the_new_kernels_use_no_scratch_and_the_older_ones_keep_their_registers():
    """the committed figures are those of THIS build (tools/kernel_resources.py reads the remarks the build left behind), the new kernels use
    no scratch, and the existing GKR kernels have the parent's figures"""
    import subprocess
    import sys
    prof = open(os.path.join(ROOT, "profiles", "gkr_layers_eval_kernel_resources.txt")).read()
    live = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "k_batch_gkr"], capture_output=True, text=True, timeout=120, check=True).stdout.splitlines()
    mine = prof.split("the parent commit", 1)[0].splitlines()
    recorded = [line for line in mine if line.startswith("k_batch_gkr")]
    assert len(recorded) == 3 + 1 + 4 + 4 + 2 and all(line.rstrip() in [l.rstrip() for l in live] for line in recorded), "the file's rows of this commit are what the build reports"
    rows = {}
    for m in re.finditer(r"^(parent )?(k_[a-z_0-9]+?)(ILi(\d)(?:ELi(\d))?E\S*|E\S*|) VGPR (\d+) AGPR 0 scratch (\d+) occ (\d+) LDS (\d+)$", prof, re.M):
        rows[(bool(m.group(1)), m.group(2), int(m.group(4) or 0), int(m.group(5) or 0))] = tuple(int(m.group(k)) for k in (6, 7, 8, 9))
    for kernel in ("k_batch_gkr_eval_layers", "k_batch_gkr_eval_terms", "k_batch_gkr_eval_fold"):
        assert rows[(False, kernel, 0, 0)][1] == 0 and rows[(False, kernel, 0, 0)][3] == 0, "no scratch, no static LDS: " + kernel
    older = [k for k in rows if k[0]]
    assert len(older) >= 1 + 4 + 4 + 2, "k_batch_gkr, k_batch_gkr_phase, k_batch_gkr_terms and k_batch_gkr_fold of the parent"
    for k in older:
        assert rows[(False,) + k[1:]] == rows[k], k
