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


def merge_repeated(idx, vals):
    """a sparse list whose indices may repeat -> (sorted distinct indices, the sums of their values): the map the oracle takes"""
    idx = np.asarray(idx, dtype=np.uint64).reshape(-1)
    order = np.argsort(idx, kind="stable")
    si, sv = idx[order], np.asarray(vals, dtype=np.uint64).reshape(-1, 4)[order]
    ui, start = np.unique(si, return_index=True)
    if ui.shape[0] == si.shape[0]:
        return si, sv
    ints = cref.mont_to_ints(sv)
    merged = [sum(ints[a:b]) % cref.P for a, b in zip(start, list(start[1:]) + [len(si)])]
    return ui, cref.ints_to_mont(merged)


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


# ---- tables whose lazily bound entries reach the ends of their range (tests/fe_model.py: sinking_table, selector_table), at any size --------
def raw_limbs(v: int) -> np.ndarray:
    """the 4 x u64 limbs of the integer v: as a table entry, the element whose STORED (Montgomery) form is v; as a challenge, to_mont's result"""
    assert 0 <= v < (1 << 256)
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def _sub256(a: np.ndarray, b: int) -> np.ndarray:
    """(n, 4) u64 minus the integer b, row by row; the caller guarantees no row goes below zero"""
    out = np.empty_like(a)
    borrow = np.zeros(a.shape[0], dtype=np.uint64)
    for k in range(4):
        bk = np.uint64((b >> (64 * k)) & 0xFFFFFFFFFFFFFFFF)
        t = a[:, k] - bk
        out[:, k] = t - borrow
        borrow = ((a[:, k] < bk) | (t < borrow)).astype(np.uint64)
    assert not borrow.any(), "an entry below zero: c < m sum s_j"
    return out


def sinking_table_limbs(nv: int, s, m: int, c: int) -> np.ndarray:
    """fe_model.sinking_table as the (2^nv, 4) array the API and the oracle take, by doubling: the upper half is the lower minus m s_j"""
    assert len(s) == nv and m >= 1 and m * sum(s) <= c < (1 << 256)
    tab = raw_limbs(c).reshape(1, 4)
    for sj in s:
        tab = np.concatenate([tab, _sub256(tab, m * sj)])
    return np.ascontiguousarray(tab)


def selector_table_limbs(nv: int, s, sel: int, m: int, c: int, flip: bool = False) -> np.ndarray:
    """fe_model.selector_table, likewise"""
    from tests import fe_model as fm
    half = sinking_table_limbs(nv - 1, list(s[:sel]) + list(s[sel + 1:]), m, c).reshape(1 << (nv - 1 - sel), 1 << sel, 4)
    out = np.empty((1 << (nv - 1 - sel), 2, 1 << sel, 4), dtype=np.uint64)
    out[:, 1 if flip else 0] = half
    out[:, 0 if flip else 1] = raw_limbs(fm.P - 1)
    return np.ascontiguousarray(out.reshape(1 << nv, 4))


def assert_entries_match(tab: np.ndarray, entry_of, seed: int = 1, samples: int = 300):
    """the array against the big-integer formula entry_of(index) at the ends and at `samples` random indices"""
    rng = np.random.default_rng(seed)
    n = tab.shape[0]
    for x in [0, 1, n // 2 - 1, n // 2, n - 2, n - 1] + [int(i) for i in rng.integers(0, n, size=samples)]:
        got = sum(int(tab[x, k]) << (64 * k) for k in range(4))
        assert got == entry_of(x), f"entry {x}"


def sinking_entry(s, m: int, c: int):
    """index -> c - m sum_j x_j s_j, the formula itself"""
    return lambda x: c - m * sum(sj for j, sj in enumerate(s) if (x >> j) & 1)


def selector_entry(s, sel: int, m: int, c: int, flip: bool = False):
    from tests import fe_model as fm
    const_bit = 0 if flip else 1
    return lambda x: fm.P - 1 if (x >> sel) & 1 == const_bit else c - m * sum(sj for j, sj in enumerate(s) if j != sel and (x >> j) & 1)


def mont_challenges(r_std) -> np.ndarray:
    """standard-form challenges -> (len, 4) as the API takes them"""
    from tests import fe_model as fm
    return np.stack([raw_limbs(fm.to_mont(r)) for r in r_std])


# ---- thread ranks on one GPU (tests/test_gpu_sharded_edges.py) ---------------------------------------------------------------------------------
RANKS_BROKEN = []  # why no further rank may start in this process: a rank thread that never came back, or a rank that met a HIP error


def run_ranks(G: int, work, timeout: float = 150.0, on_error=None):
    """work(rank) on one thread per rank -> [its results].  Every thread is joined against ONE deadline; afterwards no thread may be alive
    and no rank may have raised.  A rank that hangs or meets a HIP error ends every later run_ranks of the process before it starts a
    thread: nothing more goes to a GPU that may be in a bad state.  on_error(): called by a failing rank, to let its peers out of an
    exchange they would otherwise wait in."""
    import threading
    import time
    import traceback
    import pytest
    if RANKS_BROKEN:
        pytest.fail(f"not started: {RANKS_BROKEN[0]}")
    out = [None] * G

    def body(rank):
        try:
            out[rank] = ("ok", work(rank))
        except BaseException as e:  # noqa: BLE001
            out[rank] = ("error", f"rank {rank}: {e}\n{traceback.format_exc()}")
            if on_error is not None:
                on_error()

    ts = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(G)]
    for t in ts:
        t.start()
    deadline = time.monotonic() + timeout
    for t in ts:
        t.join(timeout=max(0.0, deadline - time.monotonic()))
    alive = [r for r, t in enumerate(ts) if t.is_alive()]
    if alive:
        RANKS_BROKEN.append(f"ranks {alive} of an earlier test were still running after {timeout:.0f} s")
    errors = [o[1] for o in out if o is not None and o[0] == "error"]
    if any("[sc_status 6]" in e for e in errors):  # SC_ERR_HIP
        RANKS_BROKEN.append("a rank of an earlier test met a HIP error: " + errors[0].splitlines()[0])
    assert not alive, f"ranks {alive} did not finish within {timeout:.0f} s"
    assert not errors, "\n".join(errors)
    assert all(o is not None for o in out)
    return [o[1] for o in out]


class RecordingExchange:
    """sharded.ThreadExchange's in-process host transport with every call written down: allreduce_words[rank] and allgather_bytes[rank] list
    the sizes of that rank's calls, in order.  (The proof's bits do not depend on where a sharded proof stops sharding; the calls do.)"""

    def __init__(self, world: int):
        from sumcheck_amd import sharded
        self.world = world
        self._ex = sharded.ThreadExchange(world)
        self.clear()

    def clear(self):
        self.allreduce_words = [[] for _ in range(self.world)]
        self.allgather_bytes = [[] for _ in range(self.world)]

    def abort(self):
        """a rank has failed: its peers leave the barrier at once instead of waiting out its timeout"""
        self._ex._bar.abort()

    def comm(self, rank: int):
        from sumcheck_amd import sharded
        base = self._ex

        def allreduce(a):
            self.allreduce_words[rank].append(int(a.shape[0]))
            tot = np.zeros_like(a)
            for x in base._exchange(rank, a):
                tot += x
            return tot

        def allgather(b):
            self.allgather_bytes[rank].append(int(b.shape[0]))
            return np.concatenate(base._exchange(rank, b))

        return sharded.HostComm(rank, self.world, allreduce, allgather)
