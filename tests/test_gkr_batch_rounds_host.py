"""CPU tests of the host side of the batched interactive GKR rounds (sc_gkr_batch_prover_*): the symbols through every mirror (header,
library, ctypes table, C++ header, Rust shim -- its declarations checked against the header's prototypes with tests/test_rust_shim.py's
rules, as tests/test_batch_rounds_host.py checks its own family), the two launch plans, the kernels' resource figures, and the argument
checks of sc_gkr_batch_prover_init, which run before any HIP call and before the device count is asked -- so they behave the same with
and without a device.  The values themselves are tests/test_gpu_gkr_batch_rounds.py's."""
import ctypes as C
import os
import re

import numpy as np

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib
from tests import test_rust_shim as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"sc_gkr_batch_prover_init": 10, "sc_gkr_batch_prove_round": 4, "sc_gkr_batch_prover_finish": 5, "sc_gkr_batch_prover_state": 6,
         "sc_gkr_batch_prover_reset": 1, "sc_gkr_batch_prover_free": 1}
HDR = open(os.path.join(ROOT, "include", "sumcheck_hip.h")).read()
P_LIMBS = np.array([0xffffffff00000001, 0x53bda402fffe5bfe, 0x3339d80809a1d805, 0x73eda753299d7d48], dtype=np.uint64)  # p itself: not canonical


def _header_prototypes():
    """the SC_API_GKRB prototypes, parameter types in the shim's spelling (tests/test_rust_shim.py's mapping plus the new opaque type)"""
    old = dict(RS.C_BASE)
    RS.C_BASE["sc_gkr_batch_prover"] = "sc_gkr_batch_prover"
    try:
        protos = {}
        for m in re.finditer(r"SC_API_GKRB\s+([^;(]+?)\b(sc_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", HDR, re.S):
            ret, name, params = m.group(1).strip(), m.group(2), " ".join(m.group(3).split())
            plist = [RS.c_type_to_rust(re.match(r"(.*?)([A-Za-z_][A-Za-z_0-9]*)$", prm.strip()).group(1)) for prm in params.split(",")]
            protos[name] = (plist, None if ret == "void" else RS.c_type_to_rust(ret))
        return protos
    finally:
        RS.C_BASE.clear()
        RS.C_BASE.update(old)


def test_the_symbols_are_declared_exported_and_in_the_signature_table():
    protos = _header_prototypes()
    assert set(protos) == set(NAMES) == set(_lib.SIGNATURES_GKRB)
    assert all(name.startswith("sc_gkr_batch_") for name in NAMES)
    assert re.search(r"#define SC_API_GKRB SC_API\b", HDR) and "typedef struct sc_gkr_batch_prover sc_gkr_batch_prover;" in HDR
    version_line = HDR.split("#define SC_ABI_VERSION 5", 1)[1].split("\n", 1)[0]
    assert "sc_gkr_batch_prover_" in version_line, "additions within ABI version 5: the version line names the family"
    so = C.CDLL(_lib.SO_PATH)
    for name, n_args in NAMES.items():
        assert hasattr(so, name), name
        assert len(protos[name][0]) == n_args and len(_lib.SIGNATURES_GKRB[name][1]) == n_args, name
        assert (_lib.SIGNATURES_GKRB[name][0] is None) == (protos[name][1] is None), name
        assert name not in _lib.SIGNATURES and name not in _lib.SIGNATURES_EXT
    assert protos["sc_gkr_batch_prove_round"] == (["*mut sc_gkr_batch_prover", "*const u64", "u32", "*mut u64"], "c_int")
    assert protos["sc_gkr_batch_prover_init"][0] == ["u32", "u32", "*const *const u64", "*const *const u64", "*const u64", "*const *const u64", "*const *const u64",
                                                     "*const *const u64", "u32", "*mut *mut sc_gkr_batch_prover"]
    assert sc.lib().sc_abi_version() == 5


def test_neither_older_scanner_sees_the_family():
    """the header-vs-shim scanner reads `SC_API` prototypes, tests/test_batch_rounds_host.py `SC_API_EXT` ones: the third marker is neither,
    its own #define line included"""
    for marker in ("SC_API", "SC_API_EXT"):
        names = [m.group(2) for m in re.finditer(marker + r"\s+([^;(]+?)\b(sc_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", HDR, re.S)]
        assert names and not [x for x in names if x in NAMES], marker


def test_the_shim_declares_them_as_the_header_does_and_wraps_them():
    rs = open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()
    protos, ext = _header_prototypes(), {}
    for block in re.findall(r'extern "C" \{(.*?)\n\}', rs, re.S):
        for m in re.finditer(r"\bfn (sc_gkr_batch_[a-z0-9_]+)\s*\((.*?)\)\s*(?:->\s*([^;]+?))?\s*;", block, re.S):
            assert not re.search(r"pub\s+fn " + m.group(1) + r"\b", block), "private declarations: the shim's pub externs are SC_API prototypes"
            params = " ".join(m.group(2).split())
            ext[m.group(1)] = ([p.split(":", 1)[1].strip() for p in params.split(",") if p.strip()], m.group(3).strip() if m.group(3) else None)
    assert set(ext) == set(NAMES)
    for name, (rp, rr) in ext.items():
        assert (rp, rr) == protos[name], f"{name}: shim {rp} -> {rr}, header {protos[name]}"
    assert re.search(r"pub struct sc_gkr_batch_prover \{\s*_private: \[u8; 0\],\s*\}", rs)
    for fn in ("gkr_prover_init_batch", "gkr_prove_round_batch", "gkr_finish_batch"):
        assert re.search(r"pub fn " + fn + r"<F: Limbs4>\(", rs), fn
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "gkr_prover_init_batch" in doc and "sc_gkr_batch_prover_" in doc


def test_the_python_and_cpp_mirrors_wrap_them():
    hpp = open(os.path.join(ROOT, "include", "sumcheck_amd.hpp")).read()
    for name in list(NAMES) + ["class GKRBatchProverState", "static GKRBatchProverState prover_init_batch(", "prove_round(", "finish("]:
        assert name in hpp, name
    assert callable(sc.GKRRoundSumcheck.prover_init_batch)
    for attr in ("prove_round", "finish", "round", "randomness", "tables", "reset", "close"):
        assert hasattr(sc.GKRBatchProverState, attr), attr


def test_the_two_plans_sit_immediately_in_front_of_gkr_sharded():
    names = list(_lib.plan_stats())
    i = names.index("gkr.sharded")
    assert names[i - 2:i] == ["batch.gkr_rounds_one_block", "batch.gkr_rounds_serial"]
    assert names[i - 3] == "gkr.coeff_from_bound_table" and len(names) == sc.lib().sc_plan_count()
    assert "batch.gkr_rounds_one_block" in HDR and "batch.gkr_rounds_serial" in HDR, "the header's policy comment names both plans"


def test_the_kernel_source_is_built_and_uses_no_scratch():
    from sumcheck_amd import build
    assert "kernels_batch_gkr_rounds.hip" in build.SOURCES and "gkr_batch_rounds.hip" in build.SOURCES
    prof = open(os.path.join(ROOT, "profiles", "gkr_batch_rounds_kernel_resources.txt")).read()
    for phase in (1, 2):
        m = re.search(r"^k_batch_gkr_phaseILi%d\S* VGPR (\d+) AGPR 0 scratch (\d+) " % phase, prof, re.M)
        assert m and int(m.group(2)) == 0 and int(m.group(1)) <= 128, phase


# ---- the argument checks: the same status with and without a device -----------------------------------------------------------------
def _args(n, dim, seed=500, nnz=None):
    N = 1 << dim
    keep = []
    for i in range(n):
        k = N if nnz is None else nnz
        idx = np.ascontiguousarray(np.random.default_rng(seed + i).integers(0, 1 << (3 * dim), size=k, dtype=np.uint64)) if dim else np.zeros(k, np.uint64)
        keep.append([idx, cref.synth_table(seed + i, 1, max(k, 1)), cref.synth_table(seed + i, 2, N), cref.synth_table(seed + i, 3, N), cref.synth_table(seed + i, 4, max(dim, 1))])
    return keep


def _init(keep, n, dim, null=None, out=True):
    def ptrs(col):
        return (C.c_void_p * max(n, 1))(*[a[col].ctypes.data for a in keep[:n]])
    cols = [ptrs(0), ptrs(1), (C.c_uint64 * max(n, 1))(*[a[0].shape[0] for a in keep[:n]]), ptrs(2), ptrs(3), ptrs(4)]
    if null is not None:
        cols[null] = None
    h = C.c_void_p()
    rc = sc.lib().sc_gkr_batch_prover_init(n, dim, cols[0], cols[1], cols[2], cols[3], cols[4], cols[5], 0, C.byref(h) if out else None)
    msg = sc.lib().sc_last_error().decode()
    if rc == _lib.SC_OK:
        sc.lib().sc_gkr_batch_prover_free(h)
    else:
        assert not h.value, "a failed init leaves no handle behind"
    return rc, msg


def test_null_arguments_and_an_empty_batch_are_bad_arguments():
    keep = _args(2, 3)
    for null in range(6):
        rc, msg = _init(keep, 2, 3, null=null)
        assert rc == _lib.SC_ERR_BAD_ARG and "null" in msg, (null, msg)
    rc, msg = _init(keep, 2, 3, out=False)
    assert rc == _lib.SC_ERR_BAD_ARG and "null" in msg
    rc, msg = _init(keep, 0, 3)
    assert rc == _lib.SC_ERR_BAD_ARG and "n == 0" in msg, msg
    L = sc.lib()
    buf = np.zeros((8, 4), np.uint64)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.sc_gkr_batch_prove_round(None, None, 0, p) == _lib.SC_ERR_BAD_ARG
    assert L.sc_gkr_batch_prover_finish(None, p, 0, p, p) == _lib.SC_ERR_BAD_ARG
    assert L.sc_gkr_batch_prover_state(None, 0, None, None, None, None) == _lib.SC_ERR_BAD_ARG
    assert L.sc_gkr_batch_prover_reset(None) == _lib.SC_ERR_BAD_ARG
    L.sc_gkr_batch_prover_free(None)  # like free(NULL)


def test_a_constant_and_a_dim_beyond_64_bit_indices():
    rc, msg = _init(_args(2, 0), 2, 0)
    assert rc == _lib.SC_ERR_CONSTANT_POLY and msg == "instance 0: Attempt to prove a constant.", msg
    keep = _args(1, 2)
    rc, msg = _init(keep, 1, 22)  # (checked before any array is read)
    assert rc == _lib.SC_ERR_BAD_ARG and msg.startswith("instance 0: dim 22"), msg


def test_a_non_canonical_g_and_a_host_index_out_of_range_name_their_instance():
    keep = _args(4, 3)
    keep[2][4] = keep[2][4].copy()
    keep[2][4][1] = P_LIMBS
    keep[3][4] = keep[3][4].copy()
    keep[3][4][0] = P_LIMBS
    rc, msg = _init(keep, 4, 3)
    assert rc == _lib.SC_ERR_BAD_ARG and msg == "instance 2: g[1] is not a canonical field element", msg
    keep = _args(4, 3)
    for i, bit in ((1, 9), (3, 63)):  # a bit at 3 dim and above
        keep[i][0] = keep[i][0].copy()
        keep[i][0][5] |= np.uint64(1) << np.uint64(bit)
    rc, msg = _init(keep, 4, 3)
    assert rc == _lib.SC_ERR_BAD_ARG and msg == "instance 1: f1 index 5 out of range", msg
    keep[1][0][5] &= np.uint64((1 << 9) - 1)
    rc, msg = _init(keep, 4, 3)
    assert rc == _lib.SC_ERR_BAD_ARG and msg.startswith("instance 3: f1 index 5"), msg


def test_a_valid_batch_needs_a_device():
    keep = _args(3, 4)
    rc, msg = _init(keep, 3, 4)
    if sc.lib().sc_device_count() > 0:
        assert rc == _lib.SC_OK, msg
    else:
        assert rc == _lib.SC_ERR_HIP and "no HIP device visible" in msg and "no CPU fallback" in msg
