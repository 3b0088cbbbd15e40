"""CPU tests of the host side of sc_gkr_layer_next_batch (an existing GKR batch handle onto the next layer's inputs): the prototype under
its own marker SC_API_GKRL against the shim's declaration and the ctypes table, by the rules of tests/test_gkr_batch_rounds_host.py; the
export; the three older scanners, none of which may see the name; the wrappers of every mirror; the plan's name and place; the restage
kernel's resource figures; and what the call answers without a handle.  The values themselves are tests/test_gpu_gkr_next_layer.py's."""
import ctypes as C
import os
import re

import sumcheck_amd as sc
from sumcheck_amd import _lib
from tests import test_gkr_batch_rounds_host as GR
from tests import test_rust_shim as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sc_gkr_layer_next_batch"
HDR = open(os.path.join(ROOT, "include", "sumcheck_hip.h")).read()
PARAMS = ["*mut sc_gkr_batch_prover", "*const *const u64", "*const *const u64", "*const u64", "*const *const u64", "*const *const u64", "*const *const u64", "u32"]


def _header_prototypes():
    """the SC_API_GKRL prototypes, parameter types in the shim's spelling (tests/test_rust_shim.py's mapping plus the handle's opaque type)"""
    old = dict(RS.C_BASE)
    RS.C_BASE["sc_gkr_batch_prover"] = "sc_gkr_batch_prover"
    try:
        protos = {}
        for m in re.finditer(r"SC_API_GKRL\s+([^;(]+?)\b(sc_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", HDR, re.S):
            ret, name, params = m.group(1).strip(), m.group(2), " ".join(m.group(3).split())
            plist = [RS.c_type_to_rust(re.match(r"(.*?)([A-Za-z_][A-Za-z_0-9]*)$", prm.strip()).group(1)) for prm in params.split(",")]
            protos[name] = (plist, None if ret == "void" else RS.c_type_to_rust(ret))
        return protos
    finally:
        RS.C_BASE.clear()
        RS.C_BASE.update(old)


def test_the_symbol_is_declared_exported_and_in_its_own_signature_table():
    protos = _header_prototypes()
    assert set(protos) == {NAME} == set(_lib.SIGNATURES_GKRL)
    assert protos[NAME] == (PARAMS, "c_int")
    assert re.search(r"#define SC_API_GKRL SC_API\b", HDR) and not NAME.startswith("sc_gkr_batch_")
    version_line = HDR.split("#define SC_ABI_VERSION 5", 1)[1].split("\n", 1)[0]
    assert NAME in version_line, "an addition within ABI version 5: the version line names it"
    assert hasattr(C.CDLL(_lib.SO_PATH), NAME)
    res, args = _lib.SIGNATURES_GKRL[NAME]
    assert res is C.c_int and len(args) == len(PARAMS)
    assert NAME not in _lib.SIGNATURES and NAME not in _lib.SIGNATURES_EXT and NAME not in _lib.SIGNATURES_GKRB
    assert sc.lib().sc_abi_version() == 5
    assert "New inputs: a new handle" not in HDR, "sc_gkr_batch_prover_reset's comment points at the new call"


def test_none_of_the_older_scanners_sees_the_name():
    """tests/test_rust_shim.py reads `SC_API` prototypes, tests/test_batch_rounds_host.py `SC_API_EXT` ones, tests/test_gkr_batch_rounds_host.py
    `SC_API_GKRB` ones and the shim's `sc_gkr_batch_` declarations: each asserts a closed set"""
    for marker in ("SC_API", "SC_API_EXT", "SC_API_GKRB"):
        names = [m.group(2) for m in re.finditer(marker + r"\s+([^;(]+?)\b(sc_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", HDR, re.S)]
        assert names and NAME not in names, marker
    assert set(GR._header_prototypes()) == set(GR.NAMES)
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
    assert re.search(r"pub fn gkr_next_layer_batch<F: Limbs4>\(", rs)


def test_every_mirror_wraps_it_and_the_integration_guide_names_them():
    hpp = open(os.path.join(ROOT, "include", "sumcheck_amd.hpp")).read()
    assert NAME in hpp and re.search(r"void next_layer\(", hpp)
    assert callable(sc.GKRBatchProverState.next_layer)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in (NAME, "next_layer", "gkr_next_layer_batch"):
        assert name in doc, name


def test_a_null_handle_is_a_bad_argument():
    assert sc.lib().sc_gkr_layer_next_batch(None, None, None, None, None, None, None, 0) == _lib.SC_ERR_BAD_ARG
    assert "null" in sc.lib().sc_last_error().decode()


def test_the_plan_sits_between_the_two_bucketed_gkr_plans():
    names = list(_lib.plan_stats())
    i = names.index("batch.gkr_next_layer")
    assert names[i - 1] == "gkr.bucketed_grouped" and names[i + 1] == "gkr.bucketed_counted"
    assert len(names) == sc.lib().sc_plan_count() and "batch.gkr_next_layer" in HDR


def test_the_restage_kernel_is_built_and_uses_no_scratch():
    from sumcheck_amd import build
    src = open(os.path.join(ROOT, "sumcheck_amd", "csrc", "kernels_batch_gkr_rounds.hip")).read()
    assert "kernels_batch_gkr_rounds.hip" in build.SOURCES and "void k_batch_gkr_restage(" in src
    prof = open(os.path.join(ROOT, "profiles", "gkr_next_layer_kernel_resources.txt")).read()
    m = re.search(r"^k_batch_gkr_restage\S* VGPR (\d+) AGPR 0 scratch (\d+) occ (\d+) LDS (\d+)$", prof, re.M)
    assert m and int(m.group(2)) == 0 and int(m.group(4)) == 0 and int(m.group(1)) <= 64, "no scratch, no LDS"
