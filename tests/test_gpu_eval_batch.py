"""GPU tests of sc_poly_evaluate_batch (ListOfProductsOfPolynomials.evaluate_batch) and sc_gkr_subclaim_batch
(GKRRoundSumcheck.evaluate_subclaims_batch, GKRRoundSumcheckSubClaim.verify_subclaim_batch): the oracle queries of a whole batch in one
call.  Every instance of every batch is compared with the oracle -- cref.poly_evaluate and cref.fix_variables for the dense side,
cref.sparse_fix_variables at the full point and pyoracle's big-integer evaluation for f1: none sampled, none skipped."""
import numpy as np
import pytest

import sumcheck_amd as sc
from oracle import cref
from oracle import pyoracle as po
from sumcheck_amd import _lib, field
from tests import helpers as H

pytestmark = pytest.mark.gpu

NV_MAX = 14  # the dense kernel's envelope (include/sumcheck_hip.h)
DIM_MAX, NNZ_PER_CELL_MAX = 9, 64  # the GKR kernel's: sc_gkr_prove_batch's
GOLDEN_SHAPES = {"c1": "ml_nv3_c1shape.json", "c2": "ml_nv7_c2shape.json", "c3": "ml_nv6_c3shape.json", "shared": "ml_nv6_shared.json", "deg12": "ml_nv5_deg12.json"}
EXTREMES = cref.ints_to_mont([0, 1, po.P - 1])


def shapes_of(name):
    return H.load(GOLDEN_SHAPES[name])["shapes"]


def _n_tables(shapes):
    return max(max(s) for s in shapes) + 1


def make_ml_batch(n, nv, shapes, seed, device="cuda:0", share_every=0, extreme=False):
    """n instances of one structure -> (polys, oracle descriptors, points).  share_every = k > 0: instance i (i % k != 0) reads the
    even tables of instance i - i % k (the same objects, the same pointers); extreme: entries and points drawn from {0, 1, p - 1}"""
    nt = _n_tables(shapes)
    rng = np.random.default_rng(seed)
    if extreme:
        tabs = EXTREMES[rng.integers(0, 3, size=(n, nt, 1 << nv))]
        points = EXTREMES[rng.integers(0, 3, size=(n, nv))]
    else:
        tabs = np.stack([np.stack([cref.synth_table(seed + 7919 * i, s, 1 << nv) for s in range(nt)]) for i in range(n)])  # (n, nt, 2^nv, 4)
        points = cref.synth_table(seed, 5000, n * nv).reshape(n, nv, 4)
    tabs = np.ascontiguousarray(tabs, dtype=np.uint64)
    coefs = [cref.synth_table(seed + 7919 * i, 1000, len(shapes)) for i in range(n)]
    if device is not None:
        import torch
        big = torch.from_numpy(tabs.view(np.int64)).to(device)
        torch.cuda.synchronize()
    mles = [[sc.DenseMultilinearExtension(nv, big[i, s] if device is not None else tabs[i, s]) for s in range(nt)] for i in range(n)]
    polys, descs = [], []
    for i in range(n):
        src = [i - i % share_every if (share_every and s % 2 == 0) else i for s in range(nt)]
        poly = sc.ListOfProductsOfPolynomials(nv)
        for k, sh in enumerate(shapes):
            poly.add_product([mles[src[t]][t] for t in sh], coefs[i][k])
        polys.append(poly)
        descs.append(H.desc_from(nv, shapes, [tabs[src[t], t] for t in range(nt)], coefs[i]))
    return polys, descs, np.ascontiguousarray(points, dtype=np.uint64)


def ml_oracle(descs, points):
    """-> per instance (value, per-table values) from cref.poly_evaluate and cref.fix_variables"""
    out = []
    for d, pt in zip(descs, points):
        tv = np.stack([cref.fix_variables(t, pt).reshape(4) for t in d.tables])
        out.append((cref.poly_evaluate(d, pt), tv))
    return out


def assert_ml_equals(polys, points, want):
    got, tv = sc.ListOfProductsOfPolynomials.evaluate_batch(polys, points, return_table_values=True)
    assert got.shape == (len(want), 4) and tv.shape[0] == len(want)
    for i, (wv, wt) in enumerate(want):
        assert np.array_equal(tv[i], wt), f"instance {i}: table values differ from cref.fix_variables"
        assert np.array_equal(got[i], wv), f"instance {i}: value differs from cref.poly_evaluate"
    assert np.array_equal(sc.ListOfProductsOfPolynomials.evaluate_batch(polys, points), got)
    return got, tv


def ml_plans():
    p = _lib.plan_stats()
    return p["batch.eval_one_block"], p["batch.eval_serial"]


def gkr_plans():
    p = _lib.plan_stats()
    return p["batch.gkr_eval_one_block"], p["batch.gkr_eval_serial"]


# ---- ML parity ------------------------------------------------------------------------------------------------------------------------
def _ml_cases():
    for name in GOLDEN_SHAPES:
        for nv in (0, 1, 2, 3, 4, 7, 10, NV_MAX):
            for n in (1, 2, 256):
                if (n == 256 and nv not in (0, 3, 7)) or (nv == NV_MAX and name in ("c3", "deg12") and n > 1):
                    continue
                yield pytest.param(name, nv, n, id=f"{name}-nv{nv}-n{n}")


@pytest.mark.parametrize("name,nv,n", list(_ml_cases()))
def test_ml_parity_with_the_oracle(name, nv, n):
    """the golden shapes from zero variables to the envelope's top, device tables, under the default policy; a batch of hundreds runs in the kernel"""
    polys, descs, points = make_ml_batch(n, nv, shapes_of(name), 81000 + 97 * nv + n)
    want = ml_oracle(descs, points)
    b0, s0 = ml_plans()
    assert_ml_equals(polys, points, want)
    b1, s1 = ml_plans()
    assert (b1 - b0) + (s1 - s0) == 2 and (b1 - b0 == 2 or n < 256), "one plan per call; hundreds of instances within the envelope run in the kernel"


@pytest.mark.parametrize("device", ["cuda:0", None], ids=["device", "host"])
@pytest.mark.parametrize("name", list(GOLDEN_SHAPES))
def test_ml_host_and_device_tables_both_plans(name, device):
    for nv, n in ((0, 3), (2, 5), (6, 13), (9, 4)):
        polys, descs, points = make_ml_batch(n, nv, shapes_of(name), 82000 + nv, device=device)
        want = ml_oracle(descs, points)
        with _lib.policy(batch=2):
            b0, s0 = ml_plans()
            got = assert_ml_equals(polys, points, want)
            assert ml_plans() == (b0 + 2, s0), "within the envelope the kernel takes the batch"
        with _lib.policy(batch=0):
            b0, s0 = ml_plans()
            got0 = assert_ml_equals(polys, points, want)
            assert ml_plans() == (b0, s0 + 2)
        assert got[0].tobytes() == got0[0].tobytes() and got[1].tobytes() == got0[1].tobytes()


def test_ml_more_instances_than_the_device_holds_workgroups():
    """1200 instances x 3 tables = 3600 workgroups: several times what 256 CUs hold at once"""
    polys, descs, points = make_ml_batch(1200, 5, shapes_of("c2"), 83000)
    want = ml_oracle(descs, points)
    b0, s0 = ml_plans()
    assert_ml_equals(polys, points, want)
    assert ml_plans() == (b0 + 2, s0)


@pytest.mark.parametrize("device", ["cuda:0", None], ids=["device", "host"])
def test_ml_tables_repeated_across_instances(device):
    for name, nv, n in (("c2", 6, 24), ("shared", 5, 9), ("c3", 4, 16)):
        polys, descs, points = make_ml_batch(n, nv, shapes_of(name), 84000 + nv, device=device, share_every=4)
        want = ml_oracle(descs, points)
        with _lib.policy(batch=2):
            b0, s0 = ml_plans()
            assert_ml_equals(polys, points, want)
            assert ml_plans() == (b0 + 2, s0)
    poly = polys[0]  # ONE polynomial for every instance: only the points differ
    want = ml_oracle([descs[0]] * 7, points[:7])
    with _lib.policy(batch=2):
        assert_ml_equals([poly] * 7, points[:7], want)


@pytest.mark.parametrize("device", ["cuda:0", None], ids=["device", "host"])
def test_ml_extreme_entries_and_points(device):
    """entries and points from {0, 1, p - 1}: the carry-free binds at their bounds"""
    for name, nv, n in (("c2", 1, 9), ("c1", 3, 9), ("shared", 6, 12), ("c3", 8, 5), ("deg12", 5, 6), ("c2", NV_MAX, 2)):
        polys, descs, points = make_ml_batch(n, nv, shapes_of(name), 85000 + nv, device=device, extreme=True)
        want = ml_oracle(descs, points)
        for pol in (2, 0):
            with _lib.policy(batch=pol):
                assert_ml_equals(polys, points, want)


def test_ml_beyond_the_envelope_the_serial_plan_gives_the_same_bits():
    polys, descs, points = make_ml_batch(3, NV_MAX + 1, shapes_of("c2"), 86000)
    want = ml_oracle(descs, points)
    with _lib.policy(batch=2):
        b0, s0 = ml_plans()
        assert_ml_equals(polys, points, want)
        assert ml_plans() == (b0, s0 + 2)
    polys, descs, points = make_ml_batch(3, NV_MAX, shapes_of("c2"), 86001)  # exactly at the top: the kernel
    want = ml_oracle(descs, points)
    with _lib.policy(batch=2):
        b0, s0 = ml_plans()
        assert_ml_equals(polys, points, want)
        assert ml_plans() == (b0 + 2, s0)


# ---- GKR parity -----------------------------------------------------------------------------------------------------------------------
def make_f1(dim, seed, variant="random", nnz=None):
    """(indices, values) of one wiring predicate: random (any order), repeated (every index several times), zeros (half the values zero)"""
    N = 1 << dim
    nnz = 2 * N if nnz is None else nnz
    rng = np.random.default_rng(seed)
    if variant == "repeated":
        pool = rng.integers(0, 1 << (3 * dim), size=max(nnz // 3, 1), dtype=np.uint64)
        idx = pool[rng.integers(0, pool.shape[0], size=nnz)]
    else:
        idx = rng.integers(0, 1 << (3 * dim), size=nnz, dtype=np.uint64)
    vals = cref.synth_table(seed, 1, nnz) if nnz else np.zeros((0, 4), np.uint64)
    if variant == "zeros" and nnz:
        vals = vals.copy()
        vals[::2] = 0
    return np.ascontiguousarray(idx, dtype=np.uint64), vals


def make_gkr_batch(n, dim, seed, device="cuda:0", variant="random", nnz=None, shared_f1=False, ragged=False):
    N = 1 << dim
    raw = []
    for i in range(n):
        k = [0, 1, N // 2, N, 3 * N, 8 * N][i % 6] if ragged else nnz
        f1 = make_f1(dim, seed + 31 * (0 if shared_f1 else i), variant, k)
        raw.append((f1[0], f1[1], cref.synth_table(seed + 7919 * i, 2, N), cref.synth_table(seed + 7919 * i, 3, N), cref.synth_table(seed + 7919 * i, 4, dim)))
    if device is not None:
        import torch
        td = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(device)
    else:
        td = lambda a: a
    shared = None
    f1s, f2s, f3s = [], [], []
    for idx, vals, f2, f3, g in raw:
        if shared_f1 and shared is not None:
            f1s.append(shared)  # ONE object, one pair of pointers for every instance
        else:
            f1s.append(sc.SparseMultilinearExtension(3 * dim, td(idx), td(vals)))
            shared = f1s[-1]
        f2s.append(sc.DenseMultilinearExtension(dim, td(f2)))
        f3s.append(sc.DenseMultilinearExtension(dim, td(f3)))
    if device is not None:
        import torch
        torch.cuda.synchronize()
    uv = cref.synth_table(seed, 6000, n * 2 * dim).reshape(n, 2, dim, 4)
    return {"n": n, "dim": dim, "raw": raw, "f1s": f1s, "f2s": f2s, "f3s": f3s, "gs": [r[4] for r in raw], "uv": uv}


def _one_table(dim, t):
    return cref.PolyDesc(dim, [(cref.ints_to_mont([1])[0], [0])], [t])


def gkr_oracle(b):
    """-> (n, 4, 4): f1(g,u,v) from cref.sparse_fix_variables at the full point (repeated indices merged first, as a map built by
    insertion-with-add holds them) -- and checked against pyoracle's big-integer evaluation --, f2(u) and f3(v) from cref.poly_evaluate,
    and their product"""
    dim = b["dim"]
    out = np.zeros((b["n"], 4, 4), np.uint64)
    for i, (idx, vals, f2, f3, g) in enumerate(b["raw"]):
        u, v = b["uv"][i, 0], b["uv"][i, 1]
        guv = np.concatenate([g, u, v])
        merged = {}
        for k, val in zip(idx.tolist(), cref.mont_to_ints(vals) if len(idx) else []):
            merged[k] = (merged.get(k, 0) + val) % po.P
        keys = sorted(merged)
        oi, ov = cref.sparse_fix_variables(np.array(keys, dtype=np.uint64), cref.ints_to_mont([merged[k] for k in keys]) if keys else np.zeros((0, 4), np.uint64), guv)
        a1 = ov[0] if len(oi) else np.zeros(4, np.uint64)
        big = po.sparse_evaluate(merged, 3 * dim, cref.mont_to_ints(guv))
        assert cref.mont_to_ints(a1.reshape(1, 4))[0] == big, f"instance {i}: the two oracles disagree on f1(g,u,v)"
        a2, a3 = cref.poly_evaluate(_one_table(dim, f2), u), cref.poly_evaluate(_one_table(dim, f3), v)
        out[i, 0], out[i, 1], out[i, 2] = a1, a2, a3
        out[i, 3] = cref.ints_to_mont([big * cref.mont_to_ints(a2.reshape(1, 4))[0] % po.P * cref.mont_to_ints(a3.reshape(1, 4))[0] % po.P])[0]
    return out


def assert_gkr_equals(b, want):
    got = sc.GKRRoundSumcheck.evaluate_subclaims_batch(b["f1s"], b["f2s"], b["f3s"], b["gs"], b["uv"])
    assert got.shape == want.shape
    for i in range(b["n"]):
        for j, what in enumerate(("f1(g,u,v)", "f2(u)", "f3(v)", "the product")):
            assert np.array_equal(got[i, j], want[i, j]), f"instance {i}: {what} differs from the oracle's"
    return got


@pytest.mark.parametrize("dim", list(range(1, DIM_MAX + 2)))
def test_gkr_parity_with_the_oracle(dim):
    """every dim of the envelope and one beyond (the serial plan), nnz = 2 x 2^dim, device inputs, under the default policy"""
    b = make_gkr_batch(5 if dim <= DIM_MAX else 2, dim, 91000 + dim)
    want = gkr_oracle(b)
    b0, s0 = gkr_plans()
    assert_gkr_equals(b, want)
    b1, s1 = gkr_plans()
    assert (b1 - b0) + (s1 - s0) == 1 and (dim <= DIM_MAX or s1 == s0 + 1), "one plan per call; beyond the envelope the serial plan"


@pytest.mark.parametrize("n", [1, 2, 256, 1000])
def test_gkr_batch_sizes(n):
    b = make_gkr_batch(n, 5, 92000 + n, nnz=32)
    want = gkr_oracle(b)
    b0, s0 = gkr_plans()
    assert_gkr_equals(b, want)
    if n >= 256:
        assert gkr_plans() == (b0 + 1, s0), "a batch of hundreds of instances within the envelope runs in the kernel"


@pytest.mark.parametrize("device", ["cuda:0", None], ids=["device", "host"])
@pytest.mark.parametrize("variant,kw", [("random", {}), ("repeated", {}), ("zeros", {}), ("random", {"nnz": 0}), ("repeated", {"nnz": "8N"}), ("random", {"shared_f1": True}),
                                        ("random", {"ragged": True})], ids=["random", "repeated", "zeros", "nnz0", "repeated8N", "shared_f1", "ragged"])
def test_gkr_f1_variants_device_and_host_inputs_both_plans(variant, kw, device):
    """unordered lists, repeated indices, zero values, empty lists, one f1 for every instance: the kernel and the serial plan give the oracle's bits"""
    for dim, n in ((1, 5), (4, 13), (7, 6), (9, 3)):
        kw2 = dict(kw)
        if kw2.get("nnz") == "8N":
            kw2["nnz"] = 8 << dim
        b = make_gkr_batch(n, dim, 93000 + dim, device=device, variant=variant, **kw2)
        want = gkr_oracle(b)
        with _lib.policy(batch=2):
            b0, s0 = gkr_plans()
            got = assert_gkr_equals(b, want)
            assert gkr_plans() == (b0 + 1, s0)
        with _lib.policy(batch=0):
            b0, s0 = gkr_plans()
            got0 = assert_gkr_equals(b, want)
            assert gkr_plans() == (b0, s0 + 1)
        assert got.tobytes() == got0.tobytes()


def test_gkr_beyond_the_envelope_the_serial_plan_gives_the_same_bits():
    for dim, n, nnz in ((DIM_MAX + 1, 2, None), (3, 4, (NNZ_PER_CELL_MAX << 3) + 1)):
        b = make_gkr_batch(n, dim, 94000 + dim, nnz=nnz)
        want = gkr_oracle(b)
        with _lib.policy(batch=2):
            b0, s0 = gkr_plans()
            assert_gkr_equals(b, want)
            assert gkr_plans() == (b0, s0 + 1), (dim, nnz)
    b = make_gkr_batch(3, 4, 94500, nnz=NNZ_PER_CELL_MAX << 4)  # exactly at the cap: the kernel
    want = gkr_oracle(b)
    with _lib.policy(batch=2):
        b0, s0 = gkr_plans()
        assert_gkr_equals(b, want)
        assert gkr_plans() == (b0 + 1, s0)


@pytest.mark.parametrize("pol", [2, 0])
def test_gkr_a_device_resident_index_out_of_range_is_detected_never_followed(pol):
    import torch
    n, dim = 12, 5
    b = make_gkr_batch(n, dim, 95000)
    want = gkr_oracle(b)
    for i, bit in ((7, 3 * dim), (9, 63)):
        idx = b["raw"][i][0].copy()
        idx[3] |= np.uint64(1) << np.uint64(bit)
        b["f1s"][i] = sc.SparseMultilinearExtension(3 * dim, torch.from_numpy(idx.view(np.int64)).to("cuda:0"), b["f1s"][i].values)
    torch.cuda.synchronize()
    with _lib.policy(batch=pol):
        with pytest.raises(sc.SumcheckError) as e:
            sc.GKRRoundSumcheck.evaluate_subclaims_batch(b["f1s"], b["f2s"], b["f3s"], b["gs"], b["uv"])
    assert e.value.code == _lib.SC_ERR_BAD_ARG and e.value.msg.startswith("instance 7: f1 has an index out of range"), e.value.msg
    assert want.shape == (n, 4, 4)


# ---- policy -----------------------------------------------------------------------------------------------------------------------------
def test_policy_batch_selects_the_plan_and_never_the_bits():
    polys, descs, points = make_ml_batch(40, 6, shapes_of("c2"), 96000)
    want = ml_oracle(descs, points)
    b = make_gkr_batch(40, 6, 96500)
    gwant = gkr_oracle(b)
    outs = {}
    for pol in (0, 1, 2):
        with _lib.policy(batch=pol):
            m0, g0 = ml_plans(), gkr_plans()
            v, tv = assert_ml_equals(polys, points, want)
            ge = assert_gkr_equals(b, gwant)
            m1, g1 = ml_plans(), gkr_plans()
        outs[pol] = v.tobytes() + tv.tobytes() + ge.tobytes()
        dm, dg = (m1[0] - m0[0], m1[1] - m0[1]), (g1[0] - g0[0], g1[1] - g0[1])
        if pol == 0:
            assert dm == (0, 2) and dg == (0, 1), "policy 0: always the serial plan"
        elif pol == 2:
            assert dm == (2, 0) and dg == (1, 0), "policy 2: the kernel for every n that fits"
        else:
            assert sum(dm) == 2 and sum(dg) == 1, "policy 1: one plan per call"
    assert outs[0] == outs[1] == outs[2]


def test_the_work_areas_are_shared_with_the_batched_provers_and_released():
    """evaluate, prove, evaluate over one staging area; sc_release_caches in between; a cache limit of zero keeps nothing"""
    from tests import test_gpu_batch as TB
    ppolys, pdescs = TB.make_batch(30, 6, TB.C2, 97000)
    pwant = TB.oracle_all(pdescs)
    polys, descs, points = make_ml_batch(30, 6, shapes_of("c2"), 97100, device=None)
    want = ml_oracle(descs, points)
    with _lib.policy(batch=2):
        for _ in range(2):
            assert_ml_equals(polys, points, want)
            TB.assert_batch_equals(ppolys, pwant)
            assert sc.lib().sc_release_caches() == 0
        try:
            assert sc.lib().sc_set_cache_limit(0) == 0
            b0, s0 = ml_plans()
            assert_ml_equals(polys, points, want)
            assert ml_plans() == (b0 + 2, s0)
        finally:
            assert sc.lib().sc_set_cache_limit(16 << 30) == 0


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", ["cuda:0", None], ids=["device", "host"])
def test_prove_batch_verify_evaluate_batch(device):
    """MLSumcheck.prove_batch -> verify per instance -> ONE evaluate_batch at the subclaims' points equals every expected_evaluation"""
    n, nv, shapes = 48, 8, shapes_of("c3")
    polys, descs, _ = make_ml_batch(n, nv, shapes, 98000, device=device)
    proofs = sc.MLSumcheck.prove_batch(polys)
    subs = [sc.MLSumcheck.verify(polys[i].info(), sc.MLSumcheck.extract_sum(proofs[i]), proofs[i]) for i in range(n)]
    points = np.stack([s.point for s in subs])
    got, _ = assert_ml_equals(polys, points, ml_oracle(descs, points))
    for i in range(n):
        assert np.array_equal(got[i], subs[i].expected_evaluation), f"instance {i}: the oracle query does not meet the subclaim"


@pytest.mark.parametrize("device", ["cuda:0", None], ids=["device", "host"])
def test_gkr_prove_batch_verify_verify_subclaim_batch(device):
    """GKRRoundSumcheck.prove_batch(return_uv) -> verify -> ONE verify_subclaim_batch: all true; one entry of one f3 changed: exactly that one false"""
    n, dim = 24, 7
    b = make_gkr_batch(n, dim, 99000, device=device)
    rngs = [sc.Blake2b512Rng.setup() for _ in range(n)]
    proofs, uv = sc.GKRRoundSumcheck.prove_batch(rngs, b["f1s"], b["f2s"], b["f3s"], b["gs"], return_uv=True)
    subs = [sc.GKRRoundSumcheck.verify(sc.Blake2b512Rng.setup(), dim, proofs[i], proofs[i].extract_sum()) for i in range(n)]
    for i in range(n):
        assert np.array_equal(subs[i].u, uv[i, 0]) and np.array_equal(subs[i].v, uv[i, 1])
    b["uv"] = uv
    want = gkr_oracle(b)
    assert_gkr_equals(b, want)
    for i in range(n):
        assert np.array_equal(want[i, 3], subs[i].expected_evaluation), f"instance {i}: the oracle's product does not meet the subclaim"
    assert sc.GKRRoundSumcheckSubClaim.verify_subclaim_batch(subs, b["f1s"], b["f2s"], b["f3s"], b["gs"]) == [True] * n
    bad = 17
    f3 = b["raw"][bad][3].copy()
    f3[5] = field.add(f3[5], field.ONE)
    if device is not None:
        import torch
        f3_bad = sc.DenseMultilinearExtension(dim, torch.from_numpy(f3.view(np.int64)).to(device))
        torch.cuda.synchronize()
    else:
        f3_bad = sc.DenseMultilinearExtension(dim, f3)
    f3s = list(b["f3s"])
    f3s[bad] = f3_bad
    assert sc.GKRRoundSumcheckSubClaim.verify_subclaim_batch(subs, b["f1s"], b["f2s"], f3s, b["gs"]) == [i != bad for i in range(n)]
