"""GPU tests of sc_gkr_prove_batch (GKRRoundSumcheck.prove_batch): many small GKR round proofs in one call.  Every instance of every batch
is compared with the oracle (cref.gkr_prove) on the proof, on (u, v) and on the next sample of the continued transcript: none sampled,
none skipped."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib
from tests import helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM_MAX, NNZ_PER_CELL_MAX = 9, 64  # the batched kernel's envelope (include/sumcheck_hip.h)


def make_f1(dim, seed, variant="random", nnz=None):
    """(indices, values) of one wiring predicate.  variant: random (any order, distinct where 2^(3 dim) allows), sorted (index order),
    repeated (every index several times), zeros (half the values zero)"""
    N = 1 << dim
    nnz = N if nnz is None else nnz
    rng = np.random.default_rng(seed)
    if variant == "repeated":
        pool = rng.integers(0, 1 << (3 * dim), size=max(nnz // 3, 1), dtype=np.uint64)
        idx = pool[rng.integers(0, pool.shape[0], size=nnz)]
    else:
        idx = rng.integers(0, 1 << (3 * dim), size=nnz, dtype=np.uint64)
    if variant == "sorted":
        idx = np.sort(idx)
    vals = cref.synth_table(seed, 1, nnz) if nnz else np.zeros((0, 4), np.uint64)
    if variant == "zeros" and nnz:
        vals = vals.copy()
        vals[::2] = 0
    return np.ascontiguousarray(idx, dtype=np.uint64), vals


def make_batch(n, dim, seed, device="cuda:0", variant="random", nnz=None, shared_f1=False, ragged=False, feed=None):
    """n instances of one dim -> dict with the library's objects and the host arrays the oracle takes"""
    N = 1 << dim
    raw = []
    for i in range(n):
        k = nnz
        if ragged:
            k = [0, 1, N // 2, N, 3 * N, 8 * N][i % 6]
        f1 = make_f1(dim, seed + 31 * (0 if shared_f1 else i), variant, k)
        raw.append((f1[0], f1[1], cref.synth_table(seed + 7919 * i, 2, N), cref.synth_table(seed + 7919 * i, 3, N), cref.synth_table(seed + 7919 * i, 4, dim)))
    if device is not None:
        import torch
        td = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(device)
    else:
        td = lambda a: a
    shared = None
    f1s, f2s, f3s = [], [], []
    for i, (idx, vals, f2, f3, g) in enumerate(raw):
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
    rngs, orngs = [], []
    for i in range(n):
        r, o = sc.Blake2b512Rng.setup(), cref.Rng()
        if feed:
            r.feed(feed % i)
            o.feed_bytes(feed % i)
        rngs.append(r)
        orngs.append(o)
    return {"n": n, "dim": dim, "raw": raw, "rngs": rngs, "orngs": orngs, "f1s": f1s, "f2s": f2s, "f3s": f3s, "gs": [r[4] for r in raw]}


def fresh_rngs(b, feed=None):
    b["rngs"], b["orngs"] = [], []
    for i in range(b["n"]):
        r, o = sc.Blake2b512Rng.setup(), cref.Rng()
        if feed:
            r.feed(feed % i)
            o.feed_bytes(feed % i)
        b["rngs"].append(r)
        b["orngs"].append(o)


def oracle_all(b):
    """-> per instance (proof, uv, the continued transcript's next sample)"""
    out = []
    for i, (idx, vals, f2, f3, g) in enumerate(b["raw"]):
        proof, uv = cref.gkr_prove(idx, vals, b["dim"], f2, f3, g, rng=b["orngs"][i], threads=1)
        out.append((proof, uv, b["orngs"][i].sample_fr()))
    return out


def assert_batch_equals(b, want):
    got, uv = sc.GKRRoundSumcheck.prove_batch(b["rngs"], b["f1s"], b["f2s"], b["f3s"], b["gs"], return_uv=True)
    assert len(got) == len(want) == b["n"]
    for i, (wp, wuv, wnext) in enumerate(want):
        g1 = np.stack([m.evaluations for m in got[i].phase1_sumcheck_msgs])
        g2 = np.stack([m.evaluations for m in got[i].phase2_sumcheck_msgs])
        assert np.array_equal(g1, wp[0]), f"instance {i}: phase one's messages differ from the oracle's"
        assert np.array_equal(g2, wp[1]), f"instance {i}: phase two's messages differ from the oracle's"
        assert np.array_equal(uv[i], wuv), f"instance {i}: (u, v) differs from the oracle's"
        assert np.array_equal(b["rngs"][i].sample_fr(), wnext), f"instance {i}: the transcript after the proof"
    return got


def plans():
    p = _lib.plan_stats()
    return p["batch.gkr_one_block"], p["batch.gkr_serial"]


def stats():
    out = (C.c_uint64 * 8)()
    _lib.check(sc.lib().sc_library_stats(out, 8))
    return [int(x) for x in out]


def _parity_cases():
    for dim in (1, 2, 5, 8, 9):
        for n in (1, 2, 7, 256, 1000):
            if n >= 256 and dim > 5:
                continue
            yield pytest.param(dim, n, id=f"dim{dim}-n{n}")


@pytest.mark.parametrize("dim,n", list(_parity_cases()))
def test_parity_with_the_oracle(dim, n):
    """from one variable to the largest dim one block holds; n = 1000 exceeds what is resident (the ticket)"""
    b = make_batch(n, dim, 61000 + 97 * dim + n)
    want = oracle_all(b)
    b0, s0 = plans()
    assert_batch_equals(b, want)
    b1, s1 = plans()
    if n >= 256:  # (below the measured crossover the call may choose either plan: only the bits are checked)
        assert b1 == b0 + 1 and s1 == s0, "a batch of hundreds of instances within the envelope runs in the batched kernel"


@pytest.mark.parametrize("dim", [2, 9])
@pytest.mark.parametrize("n", [1, 2])
def test_the_batched_kernel_forced_for_the_smallest_batches(dim, n):
    b = make_batch(n, dim, 62000 + dim)
    want = oracle_all(b)
    with _lib.policy(batch=2):
        b0, s0 = plans()
        assert_batch_equals(b, want)
        assert plans() == (b0 + 1, s0)
    fresh_rngs(b)
    with _lib.policy(batch=0):
        b0, s0 = plans()
        assert_batch_equals(b, want)
        assert plans() == (b0, s0 + 1)


@pytest.mark.parametrize("device", ["cuda:0", None])
@pytest.mark.parametrize("variant,kw", [("random", {}), ("sorted", {}), ("repeated", {}), ("zeros", {}), ("random", {"nnz": 0}), ("random", {"nnz": "8N"}),
                                        ("repeated", {"nnz": "8N"}), ("random", {"shared_f1": True}), ("random", {"ragged": True})],
                         ids=["random", "sorted", "repeated", "zeros", "nnz0", "nnz8N", "repeated8N", "shared_f1", "ragged"])
def test_f1_variants_device_and_host_inputs_both_plans(variant, kw, device):
    for dim, n in ((1, 5), (4, 13), (7, 12), (9, 3)):
        kw2 = dict(kw)
        if kw2.get("nnz") == "8N":
            kw2["nnz"] = 8 << dim
        b = make_batch(n, dim, 63000 + dim, device=device, variant=variant, **kw2)
        want = oracle_all(b)
        with _lib.policy(batch=2):
            b0, s0 = plans()
            assert_batch_equals(b, want)
            assert plans() == (b0 + 1, s0), "within the envelope (nnz up to 8 x 2^dim and beyond) the kernel takes the batch"
        fresh_rngs(b)
        with _lib.policy(batch=0):
            assert_batch_equals(b, want)


def test_callers_transcripts_with_prior_feeds_are_continued_identically_under_both_plans():
    n, dim = 40, 6
    for pol in (2, 0):
        b = make_batch(n, dim, 64000, feed=b"a GKR layer's transcript before instance %d")
        want = oracle_all(b)
        with _lib.policy(batch=pol):
            assert_batch_equals(b, want)
        for i in range(n):
            assert b["rngs"][i].fill_bytes(64) == b["orngs"][i].fill_bytes(64), f"instance {i}: the transcript after the proof"


def test_beyond_the_envelope_the_serial_plan_gives_the_same_bits():
    for dim, n, nnz in ((11, 3, None), (DIM_MAX + 1, 2, None), (3, 4, (NNZ_PER_CELL_MAX << 3) + 1)):
        b = make_batch(n, dim, 65000 + dim, nnz=nnz)
        want = oracle_all(b)
        with _lib.policy(batch=2):
            b0, s0 = plans()
            assert_batch_equals(b, want)
            assert plans() == (b0, s0 + 1), (dim, nnz)
    b = make_batch(3, 4, 65500, nnz=NNZ_PER_CELL_MAX << 4)  # exactly at the cap: the kernel
    want = oracle_all(b)
    with _lib.policy(batch=2):
        b0, s0 = plans()
        assert_batch_equals(b, want)
        assert plans() == (b0 + 1, s0)


def test_device_side_waits_off_takes_the_serial_plan():
    b = make_batch(9, 6, 66000)
    want = oracle_all(b)
    with _lib.policy(batch=2, pipeline=0):
        b0, s0 = plans()
        assert_batch_equals(b, want)
        assert plans() == (b0, s0 + 1)


def test_the_serial_plan_while_an_interactive_handle_holds_the_tail_slot():
    """an interactive handle's patient resident kernel is on the GPU: the batch does not wait for the slot"""
    nv, nt, shapes = 13, 4, [[0, 1, 2], [3, 3]]
    tabs = [cref.synth_table(7400, s, 1 << nv) for s in range(nt)]
    coefs = cref.synth_table(7400, 1000, len(shapes))
    op = cref.Prover(H.desc_from(nv, shapes, tabs, coefs), threads=4)
    chal = cref.synth_table(7400, 2000, nv)
    poly, _ = H.hip_poly_from(nv, shapes, tabs, coefs, device="cuda:0")
    a = sc.IPForMLSumcheck.prover_init(poly, borrow=True)
    _lib.check(sc.lib().sc_prover_set_resident(a._h, 1 << 20))
    b = make_batch(9, 6, 67000)
    want = oracle_all(b)
    v = None
    for i in range(nv):
        got = sc.IPForMLSumcheck.prove_round(a, v).evaluations
        assert np.array_equal(got, op.prove_round(None if v is None else v.randomness)), i
        v = sc.VerifierMsg(chal[i])
        if i in (3, 7):  # a's kernel is resident from its first late round on
            fresh_rngs(b)
            with _lib.policy(batch=2):
                b0, s0 = plans()
                busy0 = stats()[1]
                assert_batch_equals(b, want)
                assert plans() == (b0, s0 + 1) and stats()[1] > busy0
    a.close()


def test_an_expired_device_side_wait_is_proved_again_inside_the_call():
    """wait_spins = 1 (process-wide: a subprocess): blocks give their instances up before the host has answered; the call proves those
    again by the serial plan with device-side waits off and still returns the oracle's bits.  The library's designed status path with
    bounded waits -- run once."""
    code = r'''
import numpy as np, sumcheck_amd as sc
from sumcheck_amd import _lib
from tests import test_gpu_gkr_batch as T
_lib.set_policy("wait_spins", 1)
_lib.set_policy("batch", 2)
b = T.make_batch(64, 6, 68000)
want = T.oracle_all(b)
r0 = T.stats()[5]
b0, s0 = T.plans()
T.assert_batch_equals(b, want)
print("RETRIES", T.stats()[5] - r0, "PLANS", T.plans()[0] - b0, T.plans()[1] - s0)
'''
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    words = r.stdout.split()
    assert "RETRIES" in words and int(words[words.index("RETRIES") + 1]) > 0, r.stdout + r.stderr[-500:]
    assert int(words[words.index("PLANS") + 1]) == 1, r.stdout


@pytest.mark.parametrize("pol", [2, 0])
def test_a_device_resident_index_out_of_range_is_detected_never_followed(pol):
    """the index has a bit at 3 dim and above: the check in front of the proofs catches it (the kernel itself masks every index it uses);
    no caller transcript has moved"""
    import torch
    n, dim = 12, 5
    b = make_batch(n, dim, 69000, feed=b"before instance %d")
    for i, bit in ((7, 3 * dim), (9, 63)):
        idx = b["raw"][i][0].copy()
        idx[3] |= np.uint64(1) << np.uint64(bit)
        b["f1s"][i] = sc.SparseMultilinearExtension(3 * dim, torch.from_numpy(idx.view(np.int64)).to("cuda:0"), b["f1s"][i].values)
    torch.cuda.synchronize()
    with _lib.policy(batch=pol):
        with pytest.raises(sc.SumcheckError) as e:
            sc.GKRRoundSumcheck.prove_batch(b["rngs"], b["f1s"], b["f2s"], b["f3s"], b["gs"])
    assert e.value.code == _lib.SC_ERR_BAD_ARG and e.value.msg.startswith("instance 7: f1 has an index out of range"), e.value.msg
    for i in range(n):
        assert np.array_equal(b["rngs"][i].sample_fr(), b["orngs"][i].sample_fr()), f"instance {i}: the failed call advanced the transcript"


def test_caches_release_limit_and_no_growth():
    import torch
    b = make_batch(300, 5, 70000)
    want = oracle_all(b)
    assert_batch_equals(b, want)
    assert sc.lib().sc_release_caches() == 0
    fresh_rngs(b)
    b0, s0 = plans()
    assert_batch_equals(b, want)
    assert plans() == (b0 + 1, s0)
    try:
        assert sc.lib().sc_set_cache_limit(0) == 0
        for _ in range(2):  # nothing is kept between calls: the call allocates and frees its own
            fresh_rngs(b)
            assert_batch_equals(b, want)
        assert plans() == (b0 + 3, s0)
    finally:
        assert sc.lib().sc_set_cache_limit(16 << 30) == 0
    fresh_rngs(b)
    assert_batch_equals(b, want)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(10):
        fresh_rngs(b)
        assert_batch_equals(b, want)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free1 >= free0, "repeated batches of one size must not grow device memory"
    assert sc.lib().sc_release_caches() == 0


def test_an_ml_batch_and_a_gkr_batch_share_the_work_areas():
    """the two entry points alternate over one set of pages, mailboxes and tags"""
    from tests import test_gpu_batch as TB
    polys, descs = TB.make_batch(50, 6, TB.GKR, 71000)
    want_ml = TB.oracle_all(descs)
    b = make_batch(50, 6, 71500)
    want = oracle_all(b)
    for _ in range(3):
        TB.assert_batch_equals(polys, want_ml)
        fresh_rngs(b)
        assert_batch_equals(b, want)


def test_every_proof_of_a_batch_verifies():
    n, dim = 20, 7
    b = make_batch(n, dim, 72000, device=None)
    want = oracle_all(b)
    got = assert_batch_equals(b, want)
    for i in range(n):
        sub = sc.GKRRoundSumcheck.verify(sc.Blake2b512Rng.setup(), dim, got[i], got[i].extract_sum())
        assert np.array_equal(sub.u, want[i][1][0]) and np.array_equal(sub.v, want[i][1][1])
        assert sub.verify_subclaim(b["f1s"][i], b["f2s"][i], b["f3s"][i], b["gs"][i]), i
