"""Shared test helpers: golden fixture loading and building identical inputs for the oracle and the HIP path."""
import glob
import json
import os

import numpy as np

from oracle import cref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def hx(s: str) -> int:
    return int(s, 16)


def load(name: str) -> dict:
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def ml_cases():
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "ml_*.json")))


def gkr_cases():
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "gkr_*.json")))


def mont(vals) -> np.ndarray:
    return cref.ints_to_mont([hx(v) if isinstance(v, str) else v for v in vals])


def golden_tables(case: dict):
    """all tables of a golden ML case as Montgomery limb arrays (by original table id)"""
    return [mont(t) for t in case["tables"]]


def oracle_desc(case: dict) -> cref.PolyDesc:
    tabs = golden_tables(case)
    flat = [tabs[i] for i in case["flattened_table_ids"]]
    prods = [(mont([c])[0], ix) for c, ix in case["products"]]
    return cref.PolyDesc(case["nv"], prods, flat)


def hip_poly(case: dict, device=None):
    """build a sumcheck_amd.ListOfProductsOfPolynomials from a golden case through add_product (exercising de-duplication)"""
    import sumcheck_amd as sc
    tabs = golden_tables(case)
    if device is not None:
        import torch
        mles = [sc.DenseMultilinearExtension(case["nv"], torch.from_numpy(t.view(np.int64)).to(device)) for t in tabs]
    else:
        mles = [sc.DenseMultilinearExtension(case["nv"], t) for t in tabs]
    coeffs = {tuple(ix): c for c, ix in case["products"]}
    poly = sc.ListOfProductsOfPolynomials(case["nv"])
    for k, shape in enumerate(case["shapes"]):
        c = mont([case["products"][k][0]])[0]
        poly.add_product([mles[i] for i in shape], c)
    return poly, mles


def random_case(rng: np.random.Generator, nv: int, shapes, n_tables: int, seed: int):
    """synthetic (SplitMix64) tables + coefficients -> (cref.PolyDesc builder inputs)"""
    tabs = [cref.synth_table(seed, s, 1 << nv) for s in range(n_tables)]
    coefs = cref.synth_table(seed, 1000, len(shapes))
    return tabs, coefs


def desc_from(nv, shapes, tabs, coefs) -> cref.PolyDesc:
    """flatten like add_product does (first-occurrence order)"""
    order, remap = [], {}
    prods = []
    for k, sh in enumerate(shapes):
        ix = []
        for t in sh:
            if t not in remap:
                remap[t] = len(order)
                order.append(t)
            ix.append(remap[t])
        prods.append((coefs[k], ix))
    return cref.PolyDesc(nv, prods, [tabs[t] for t in order])


def hip_poly_from(nv, shapes, tabs, coefs, device=None):
    import sumcheck_amd as sc
    if device is not None:
        import torch
        mles = [sc.DenseMultilinearExtension(nv, torch.from_numpy(t.view(np.int64)).to(device)) for t in tabs]
    else:
        mles = [sc.DenseMultilinearExtension(nv, t) for t in tabs]
    poly = sc.ListOfProductsOfPolynomials(nv)
    for k, sh in enumerate(shapes):
        poly.add_product([mles[i] for i in sh], coefs[k])
    return poly, mles


# ---- sc_debug_fe_op (kernels_selftest.hip): one lane per element through one primitive of the carry-free arithmetic -------------------------
FE_DEV = "cuda:0"


def fe_dev_limbs(rows):
    """rows of int32 limbs (any row length that is a multiple of 9) -> device tensor"""
    import torch
    return torch.from_numpy(np.asarray(rows, dtype=np.int64).astype(np.int32)).contiguous().to(FE_DEV)


def fe_dev_words(vals):
    """values in [0, 2^256) as 8 words in a 9-int row"""
    import torch
    rows = np.asarray([[(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)] + [0] for v in vals], dtype=np.uint32)
    return torch.from_numpy(rows.view(np.int32)).contiguous().to(FE_DEV)


def fe_run_op(op, n, a, b=None, c=None, d=None, params=(), aux_tail=None):
    """sc_debug_fe_op(op) over n elements -> (n, 9) int32 on the host; params: aux[0..3], aux_tail: the u64 words behind them"""
    import ctypes as C
    import torch
    import sumcheck_amd as sc
    f = sc.lib().sc_debug_fe_op  # (a debug entry: exported, not declared in _lib.SIGNATURES)
    f.restype = C.c_int
    f.argtypes = [C.c_int] + [C.c_void_p] * 6 + [C.c_uint64]
    aux = list(params) + [0] * (4 - len(params))
    aux_np = np.asarray([x & 0xFFFFFFFFFFFFFFFF for x in aux], dtype=np.uint64)
    if aux_tail is not None:
        aux_np = np.concatenate([aux_np, np.asarray(aux_tail, dtype=np.uint64).reshape(-1)])
    aux_t = torch.from_numpy(aux_np.view(np.int64)).to(FE_DEV)
    out = torch.full((n, 9), 0x5A5A5A5A, dtype=torch.int32, device=FE_DEV)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    rc = f(op, ptr(a), ptr(b), ptr(c), ptr(d), ptr(aux_t), ptr(out), n)
    assert rc == 0, f"sc_debug_fe_op({op}) returned {rc}"
    return out.cpu().numpy()


def fe_as_fr(out_row) -> int:
    return sum(int(np.uint32(w)) << (32 * i) for i, w in enumerate(out_row[:8]))
