"""Cases for tests/test_gpu_host_tables.py -- the two paths that exist only for HOST tables (sumcheck_amd/csrc/protocol.hip):

  streamed handles      sc_prover_init_streamed / launch_round_streamed: the tables stay on the host, rounds 1 and 2 pull them chunk by chunk
                        through a two-slot staging ring;
  staged initialisation staged_copy_and_round1 (policy "staged_init"): sc_prover_init over host tables copies them in chunks on two copy
                        streams and computes round 1 under the copy.

The GPU tests assert which plan counters move; each expectation rests on an inequality on the case's size and shape.  This file builds the
cases and states the inequalities.  Its constants are READ from the sources (a changed threshold fails tests/test_host_table_cases_host.py; it
does not silently move a case onto another path)."""
import ctypes as C
import os
import re
import types

import numpy as np

from oracle import cref
from tests import fe_model as fm
from tests import helpers as H

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sumcheck_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _ints(name, pattern):
    """the integers the (unique) match of `pattern` in csrc/`name` captures"""
    found = re.findall(pattern, _src(name))
    assert len(found) == 1, f"{name}: {len(found)} matches of {pattern!r}: the rule this file mirrors has changed"
    return [int(g) for g in (found[0] if isinstance(found[0], tuple) else (found[0],))]


K_MAX_ROUND_PRODS = _ints("kernels.h", r"constexpr int kMaxRoundProds = (\d+);")[0]       # products one merged big-round launch takes
K_ROUND_TREE_GRID = _ints("lane_sum.hpp", r"constexpr int kRoundTreeGrid = (\d+);")[0]
K_BLOCK = _ints("lane_sum.hpp", r"constexpr int kBlock = (\d+);")[0]
K_MAX_GRID = _ints("lane_sum.hpp", r"constexpr int kMaxGrid = (\d+);")[0]
K_MAX_FUSED_M = _ints("batch_shape.hpp", r"constexpr int kMaxFusedM = (\d+);")[0]          # beyond: k_sum_generic
K_MAX_SMALL_TABLES = _ints("batch_shape.hpp", r"constexpr int kMaxSmallTables = (\d+);")[0]
K_META_PRODS = _ints("batch_shape.hpp", r"constexpr int kMetaProds = (\d+);")[0]
# abi.hip, prover_build
MERGE_MAX_M = _ints("abi.hip", r"prod_offsets\[k \+ 1\] - d->prod_offsets\[k\] > (\d+)\) p->merge_rounds = false;")[0]
STREAM_MIN_NV = _ints("abi.hip", r"\(d->flags & SC_TABLES_STREAM\) && p->nv >= (\d+);")[0]
CHUNK_MIN_LOG2 = _ints("abi.hip", r"cl = std::max\((\d+)u, std::min\(cl, p->nv\)\);")[0]
CHUNK_DEFAULT_LOG2 = _ints("abi.hip", r"p->stream_chunk_request \? p->stream_chunk_request : (\d+)u;")[0]
# protocol.hip, staged_init_applies / staged_copy_and_round1
STAGED_MIN_NV = _ints("protocol.hip", r"p->nv >= (\d+) && p->K > 0 && p->K <= \(uint32_t\)scd::kMetaProds;")[0]
SIX_CHUNK_NV, LEVELS_BIG, LEVELS_SMALL = _ints("protocol.hip", r"int levels = p->nv >= (\d+) \? (\d+) : (\d+);")
_G_LINE = re.findall(r"int G = (n_pairs >= .*?);", _src("protocol.hip"))
assert len(_G_LINE) == 1
STAGED_GRID_LADDER = [(int(a), int(b)) for a, b in re.findall(r"n_pairs >= \(1ULL << (\d+)\) \? (\d+)", _G_LINE[0])]  # (log2 pairs, blocks)
STAGED_GRID_FLOOR = int(re.search(r": (\d+)$", _G_LINE[0]).group(1))

P = fm.P
SEED = 0x57AB


# ---- the rules ------------------------------------------------------------------------------------------------------------------------------
def clamp(v, lo, hi):
    return max(lo, min(v, hi))


def is_streamed(nv):
    """abi.hip: SC_TABLES_STREAM streams from 2^11 entries on; below, the tables are silently copied"""
    return nv >= STREAM_MIN_NV


def chunk_log2(nv, request):
    """abi.hip: request 0 is the default; the chunk is clamped to [2^10, the table]"""
    return clamp(request if request else CHUNK_DEFAULT_LOG2, CHUNK_MIN_LOG2, nv)


def n_chunks(nv, request):
    return 1 << (nv - chunk_log2(nv, request))


def is_merged(shapes):
    """abi.hip: merge_rounds -- one launch of the merged big-round kernel takes the whole list"""
    return 0 < len(shapes) <= K_MAX_ROUND_PRODS and all(len(sh) <= MERGE_MAX_M for sh in shapes)


def is_staged(nv, shapes, host=True, borrow=False, policy=1):
    """protocol.hip, staged_init_applies (K <= kMetaProds follows from merged: kMaxRoundProds <= kMetaProds)"""
    return bool(policy) and is_merged(shapes) and host and not borrow and nv >= STAGED_MIN_NV


def staged_chunks(nv):
    return (LEVELS_BIG if nv >= SIX_CHUNK_NV else LEVELS_SMALL) + 1


def grid_for_pairs(n_pairs):
    return clamp((n_pairs + K_BLOCK - 1) // K_BLOCK, 1, K_MAX_GRID)


def staged_sections(nv, K):
    """staged_copy_and_round1 -> [(first entry, entries, blocks)] per chunk: halves, quarters, ... and the last two of equal size"""
    n, n_pairs = 1 << nv, 1 << (nv - 1)
    G = next((g for lg, g in STAGED_GRID_LADDER if n_pairs >= (1 << lg)), STAGED_GRID_FLOOR)
    if K == 1:
        G = min(G, K_ROUND_TREE_GRID)
    G = min(G, grid_for_pairs(n_pairs))
    levels = LEVELS_BIG if nv >= SIX_CHUNK_NV else LEVELS_SMALL
    if levels == 5 and G % 8 == 0:
        sec = [G // 4, G // 8, G // 8, G // 8, G // 8, G // 4]
    else:
        levels = 2
        while levels > 0 and G % (1 << levels):
            levels -= 1
        sec = [G >> (c + 1 if c < levels else levels) for c in range(levels + 1)]
    out = []
    for c, g in enumerate(sec):
        sh = c + 1 if c < levels else levels
        out.append((n - (n >> c), n >> sh, g))
    return out


def sub_arm(shape):
    """launch_round_streamed's per-product path: which kernel a product of this length gets"""
    M = len(shape)
    return "tree" if M <= MERGE_MAX_M else "node_by_node" if M <= K_MAX_FUSED_M else "generic"


def referenced(shapes):
    return sorted({t for sh in shapes for t in sh})


# ---- the shapes -----------------------------------------------------------------------------------------------------------------------------
BASE = [[0, 1, 2], [1, 1], [2]]                                   # a shared table, a repeated factor, a single-table product
FOURTEEN_PAIRS = [[i % 4, (i + 1) % 4] for i in range(14)]        # more products than the merged launch takes: per-product trees
TEN_FACTORS = [[0, 1, 2, 0, 1, 2, 0, 1, 2, 0], [2]]               # k_sum_generic over per-slot pointer sets, beside a tree
THREE_ARMS = [[0, 1, 2], [0, 1, 2, 3, 1, 2], [0, 1, 2, 3, 0, 1, 2, 3, 0, 1]] + [[i % 4, (i + 2) % 4] for i in range(10)]  # K = 13
THIRTY_SIX = [[3 * i, 3 * i + 1, 3 * i + 2] for i in range(12)]   # U = 36: more tables than one pointer block holds

# name -> (nv, chunk request, shapes, tables).  The S4 cases leave table 1 out of every product: their descriptor is built through raw_desc()
STREAMED = {
    "S1-threshold": (11, 10, BASE, 3),
    "S1-below": (10, 10, BASE, 3),
    "S3a-64-chunks": (16, 10, BASE, 3),
    "S3b-fourteen-pairs": (14, 10, FOURTEEN_PAIRS, 4),
    "S3c-ten-factors": (14, 11, TEN_FACTORS, 3),
    "S4-unreferenced-merged": (13, 11, [[0, 2, 3], [2, 2], [3]], 4),     # table 1 is in no product
    "S4-unreferenced-five": (13, 11, [[0, 2, 3, 0, 2]], 4),
    "S5-three-arms": (13, 10, THREE_ARMS, 4),
    "S6-extreme-merged": (12, 10, [[0, 0, 1], [1, 2]], 3),
    "S6-extreme-generic": (12, 10, TEN_FACTORS, 3),
    "S7-reset": (13, 11, BASE, 3),
    "S8-thirty-six": (12, 10, THIRTY_SIX, 36),
}
CLAMP_NV, CLAMP_REQUESTS = 12, (1, 10, 12, 63)                    # S2
PINNED_CASES = ("S3a-64-chunks", "S3b-fourteen-pairs", "S3c-ten-factors")
UNREFERENCED = {"S4-unreferenced-merged": 1, "S4-unreferenced-five": 1, "T6-unreferenced": 1}  # case -> the table no product names

LADDER_SHAPE = [[0, 1, 2], [2, 2], [0]]                           # T1: a shared table, a repeated factor, a single-table product
LADDER_NV = (17, 18, 20, 21)
K1 = {"pair-22": (22, [[0, 1]]), "pair-19": (19, [[0, 1]]), "square-19": (19, [[0, 0]]), "single-18": (18, [[0]])}  # T2
EDGE_NV = 18
TWELVE_PAIRS = [[i % 4, (i + 1) % 4] for i in range(12)]
THIRTEEN_PAIRS = [[i % 4, (i + 1) % 4] for i in range(13)]
# T3: name -> (shapes, mode, staged_init policy)
EDGES = {
    "K12": (TWELVE_PAIRS, "host", 1),
    "K13": (THIRTEEN_PAIRS, "host", 1),
    "M4": ([[0, 1, 2, 3]], "host", 1),
    "M5": ([[0, 1, 2, 3, 0]], "host", 1),
    "policy-off": (LADDER_SHAPE, "host", 0),
    "device": (LADDER_SHAPE, "device", 1),
    "borrowed": (LADDER_SHAPE, "borrow", 1),
}
C3 = [[0, 1, 2, 3], [4, 5, 6], [7, 8], [9]]                       # T5: config 3's shape; table 9 lags in a device-table proof
T6 = (18, [[0, 2, 3], [2, 2], [3]], 4)                            # table 1 is in no product


def n_named(shapes):
    return max(max(sh) for sh in shapes) + 1


def first_occurrence_order(shapes):
    """the shapes name their tables in the order add_product flattens them: the wrapper's descriptor is the oracle's"""
    seen = [t for sh in shapes for t in sh]
    return sorted(set(seen), key=seen.index) == list(range(n_named(shapes)))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def synth_tables(nv, n, seed=SEED):
    return [cref.synth_table(seed + nv, s, 1 << nv) for s in range(n)]


def synth_coefs(nv, shapes, seed=SEED):
    return cref.synth_table(seed + nv, 1000, len(shapes))


def synth_challenges(nv, seed=SEED):
    return cref.synth_table(seed + nv, 2000, nv)


def extreme_tables(nv, n, seed=SEED):
    """n tables whose STORED entries are drawn from {0, 1, p - 1}; the last one is p - 1 throughout"""
    vals = np.stack([H.raw_limbs(v) for v in (0, 1, P - 1)])
    rng = np.random.default_rng(seed + nv)
    pick = [rng.integers(0, 3, size=1 << nv) for _ in range(n - 1)] + [np.full(1 << nv, 2)]
    return [np.ascontiguousarray(vals[p]) for p in pick]


def extreme_challenges(n):
    """the challenges p - 1, 0, 1, p - 1, ... (standard form -> as the API takes them)"""
    return H.mont_challenges([(P - 1, 0, 1)[j % 3] for j in range(n)])


def oracle_desc(nv, shapes, tabs, coefs):
    """the oracle's descriptor with the tables AS NUMBERED (an unreferenced table keeps its place)"""
    return cref.PolyDesc(nv, [(coefs[k], list(sh)) for k, sh in enumerate(shapes)], tabs)


def oracle_rounds(nv, shapes, tabs, coefs, chal, export_after=(), last=None):
    """cref.Prover under the given challenges -> (messages, {round: its tables after that round})"""
    op = cref.Prover(oracle_desc(nv, shapes, tabs, coefs), threads=cref.max_threads())
    want, otabs = [], {}
    for j in range(last or nv):
        want.append(op.prove_round(None if j == 0 else chal[j - 1]))
        if j + 1 in export_after:
            otabs[j + 1] = op.state()[1]
    op.close()
    return want, otabs


def oracle_proof(nv, shapes, tabs, coefs):
    """the oracle's Fiat-Shamir proof, round by round in cref.ml_prove's order (PolynomialInfo, then message -> challenge)"""
    desc = oracle_desc(nv, shapes, tabs, coefs)
    op, rng = cref.Prover(desc, threads=cref.max_threads()), cref.Rng()
    rng.feed_poly_info(desc.max_multiplicands, nv)
    proof, r = [], None
    for _ in range(nv):
        proof.append(op.prove_round(r))
        rng.feed_prover_msg(proof[-1])
        r = rng.sample_fr()
    op.close()
    return np.stack(proof)


# ---- helpers the wrapper does not offer -------------------------------------------------------------------------------------------------------
def pinned_like(tab):
    """a copy of `tab` in page-locked host memory -> (the torch tensor that owns the pages, a numpy uint64 view onto them)"""
    import torch
    t = torch.empty(tab.shape, dtype=torch.int64, pin_memory=True)
    assert t.is_pinned() and t.is_contiguous()
    view = t.numpy().view(np.uint64)
    view[:] = tab
    assert view.ctypes.data == t.data_ptr() and view.flags["C_CONTIGUOUS"]
    return t, view


def raw_desc(nv, shapes, coefs, table_ptrs, flags=0):
    """an sc_poly_desc by ctypes: n_tables = len(table_ptrs), which may exceed what the products name (the Python wrapper flattens the
    tables OUT OF the products and cannot express that) -> (descriptor, what keeps its arrays alive)"""
    from sumcheck_amd._lib import PolyDesc
    coeffs = np.ascontiguousarray(np.asarray(coefs, dtype=np.uint64).reshape(-1, 4)[: len(shapes)])
    offs, idx = [0], []
    for sh in shapes:
        idx.extend(int(t) for t in sh)
        offs.append(len(idx))
    assert max(idx) < len(table_ptrs)
    offsets, indices = np.asarray(offs, dtype=np.uint32), np.asarray(idx, dtype=np.uint32)
    tabs = (C.c_void_p * len(table_ptrs))(*[int(p) for p in table_ptrs])
    d = PolyDesc()
    d.num_vars, d.max_multiplicands, d.n_products = nv, max(len(sh) for sh in shapes), len(shapes)
    d.coeffs = coeffs.ctypes.data_as(C.POINTER(C.c_uint64))
    d.prod_offsets = offsets.ctypes.data_as(C.POINTER(C.c_uint32))
    d.prod_indices = indices.ctypes.data_as(C.POINTER(C.c_uint32))
    d.n_tables = len(table_ptrs)
    d.tables = C.cast(tabs, C.POINTER(C.c_void_p))
    d.flags = flags
    return d, (coeffs, offsets, indices, tabs)


def raw_prover(nv, shapes, coefs, tabs, streamed_chunk_log2=None):
    """sc_prover_init[_streamed] over raw_desc(host tables) -> a sumcheck_amd.ProverState on the handle (the tables stay alive with it)"""
    import sumcheck_amd as sc
    from sumcheck_amd import _lib
    d, keep = raw_desc(nv, shapes, coefs, [t.ctypes.data for t in tabs])
    h = C.c_void_p()
    if streamed_chunk_log2 is not None:
        _lib.check(sc.lib().sc_prover_init_streamed(C.byref(d), int(streamed_chunk_log2), C.byref(h)))
    else:
        _lib.check(sc.lib().sc_prover_init(C.byref(d), C.byref(h)))
    like = types.SimpleNamespace(products=[(np.asarray(coefs[k], dtype=np.uint64), list(sh)) for k, sh in enumerate(shapes)], num_variables=nv,
                                 max_multiplicands=d.max_multiplicands, flattened_ml_extensions=list(tabs))
    st = sc.ProverState(h, like)
    st._keep = (keep, list(tabs))
    return st
