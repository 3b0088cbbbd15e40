"""GPU tests of sc_ml_prove_batch (MLSumcheck.prove_batch): many small independent proofs in one call.  Every instance of every batch is
compared with the oracle (cref.ml_prove on H.desc_from(...)): proofs AND randomness, none sampled, none skipped."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import sumcheck_amd as sc
from oracle import cref
from oracle import pyoracle as po
from sumcheck_amd import _lib, field
from tests import helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C2 = [[0, 1, 2]]
GKR = [[0, 1]]
TWO = [[0, 1, 2], [1, 3]]
SQUARED = [[0, 1, 2], [2, 2]]
C3 = [[0, 1, 2, 3], [4, 5, 6], [7, 8], [9]]
SIX = [[0, 1, 2, 3, 4, 5]]
# the largest num_vars one block's LDS holds (144 KB: finalize scratch + 48 B per entry and table): three or four tables 2^9, the GKR
# phases' two 2^10, six tables or config 3's ten 2^8
ENVELOPE = {"c2": (C2, 9), "gkr": (GKR, 10), "two": (TWO, 9), "squared": (SQUARED, 9), "c3": (C3, 8), "six": (SIX, 8)}


def _n_tables(shapes):
    return max(max(s) for s in shapes) + 1


def make_batch(n, nv, shapes, seed, device="cuda:0", coefs=None):
    """n instances of one structure, tables and coefficients each instance's own -> (polys, oracle descriptors)"""
    nt = _n_tables(shapes)
    tabs = np.stack([np.stack([cref.synth_table(seed + 7919 * i, s, 1 << nv) for s in range(nt)]) for i in range(n)])  # (n, nt, 2^nv, 4)
    if coefs is None:
        coefs = [cref.synth_table(seed + 7919 * i, 1000, len(shapes)) for i in range(n)]
    descs = [H.desc_from(nv, shapes, list(tabs[i]), coefs[i]) for i in range(n)]
    if device is not None:
        import torch
        big = torch.from_numpy(tabs.view(np.int64)).to(device)
        torch.cuda.synchronize()
    polys = []
    for i in range(n):
        mles = [sc.DenseMultilinearExtension(nv, big[i, s] if device is not None else tabs[i, s]) for s in range(nt)]
        poly = sc.ListOfProductsOfPolynomials(nv)
        for k, sh in enumerate(shapes):
            poly.add_product([mles[t] for t in sh], coefs[i][k])
        polys.append(poly)
    return polys, descs


def oracle_all(descs, rngs=None):
    return [cref.ml_prove(d, rng=rngs[i] if rngs else None, threads=1) for i, d in enumerate(descs)]


def assert_batch_equals(polys, want, rngs=None):
    got, rand = sc.MLSumcheck.prove_batch(polys, rngs=rngs, return_randomness=True)
    assert len(got) == len(want)
    for i, (wp, wr) in enumerate(want):
        assert np.array_equal(np.stack([m.evaluations for m in got[i]]), wp), f"instance {i}: proof differs from the oracle's"
        assert np.array_equal(rand[i], wr), f"instance {i}: randomness differs from the oracle's"
    return got


def plans():
    p = _lib.plan_stats()
    return p["batch.one_block"], p["batch.serial"]


def stats():
    out = (C.c_uint64 * 8)()
    _lib.check(sc.lib().sc_library_stats(out, 8))
    return [int(x) for x in out]


def _parity_cases():
    for name, (shapes, nv_max) in ENVELOPE.items():
        for nv in (1, 2, 5, nv_max):
            for n in (1, 2, 7, 256, 1000):
                if n >= 256 and nv > 5:
                    continue
                yield pytest.param(shapes, nv, n, id=f"{name}-nv{nv}-n{n}")


@pytest.mark.parametrize("shapes,nv,n", list(_parity_cases()))
def test_parity_with_the_oracle(shapes, nv, n):
    """every shape of the envelope, from one variable to the largest one block holds; n = 1000 exceeds what is resident (the ticket)"""
    polys, descs = make_batch(n, nv, shapes, 41000 + 97 * nv + n)
    b0, s0 = plans()
    assert_batch_equals(polys, oracle_all(descs))
    b1, s1 = plans()
    if n >= 256:  # (below the measured crossover the call may choose either plan: only the bits are checked)
        assert b1 == b0 + 1 and s1 == s0, "a batch of hundreds of instances within the envelope runs in the batched kernel"


@pytest.mark.parametrize("name", list(ENVELOPE))
@pytest.mark.parametrize("n", [1, 2])
def test_the_batched_kernel_forced_for_the_smallest_batches(name, n):
    """policy batch = 2: the batched kernel whatever n, at the envelope's largest size and at two variables"""
    shapes, nv_max = ENVELOPE[name]
    for nv in (2, nv_max):
        polys, descs = make_batch(n, nv, shapes, 43000 + nv)
        with _lib.policy(batch=2):
            b0, s0 = plans()
            assert_batch_equals(polys, oracle_all(descs))
            assert plans() == (b0 + 1, s0)


def test_callers_transcripts_are_continued_like_sc_ml_prove_continues_them():
    n, nv = 40, 6
    polys, descs = make_batch(n, nv, TWO, 44000)
    for pol in (2, 0):  # both plans
        rngs, orngs = [], []
        for i in range(n):
            r, o = sc.Blake2b512Rng.setup(), cref.Rng()
            r.feed(b"batched transcript %d" % i)
            o.feed_bytes(b"batched transcript %d" % i)
            rngs.append(r)
            orngs.append(o)
        with _lib.policy(batch=pol):
            assert_batch_equals(polys, oracle_all(descs, orngs), rngs=rngs)
        for i in range(n):
            assert rngs[i].fill_bytes(64) == orngs[i].fill_bytes(64), f"instance {i}: the transcript after the proof"


def test_host_tables_give_the_same_bits_as_device_tables():
    n, nv = 33, 7
    want = None
    for device in ("cuda:0", None):
        polys, descs = make_batch(n, nv, C2, 45000, device=device)
        want = want or oracle_all(descs)
        with _lib.policy(batch=2):
            b0, s0 = plans()
            assert_batch_equals(polys, want)
            assert plans() == (b0 + 1, s0)


def test_per_instance_coefficients_including_zero_one_and_p_minus_one():
    n, nv = 24, 5
    special = [0, 1, po.P - 1]
    coefs = []
    for i in range(n):
        c = cref.synth_table(46000 + i, 1000, len(SQUARED)).copy()
        c[i % 2] = H.mont([special[i % 3]])[0]
        if i == 5:
            c[:] = H.mont([0, 0])
        coefs.append(c)
    polys, descs = make_batch(n, nv, SQUARED, 46000, coefs=coefs)
    want = oracle_all(descs)
    for pol in (2, 0):
        with _lib.policy(batch=pol):
            assert_batch_equals(polys, want)


def test_the_serial_plan_gives_the_same_bits():
    n, nv = 12, 6
    polys, descs = make_batch(n, nv, C2, 47000)
    want = oracle_all(descs)
    for kv in ({"batch": 0}, {"batch": 2, "pipeline": 0}):
        with _lib.policy(**kv):
            b0, s0 = plans()
            assert_batch_equals(polys, want)
            assert plans() == (b0, s0 + 1), kv
    # beyond the envelope: config 3's shape at 2^11 entries (ten tables do not fit one block's LDS), one product of ten multiplicands
    for shapes, nv_big, n_big in ((C3, 11, 3), ([[0, 1, 2, 3, 4, 5, 6, 7, 8, 9]], 6, 5)):
        polys, descs = make_batch(n_big, nv_big, shapes, 47500 + nv_big)
        with _lib.policy(batch=2):
            b0, s0 = plans()
            assert_batch_equals(polys, oracle_all(descs))
            assert plans() == (b0, s0 + 1), shapes


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
    polys, descs = make_batch(9, 6, GKR, 48000)
    want = oracle_all(descs)
    v = None
    for i in range(nv):
        got = sc.IPForMLSumcheck.prove_round(a, v).evaluations
        assert np.array_equal(got, op.prove_round(None if v is None else v.randomness)), i
        v = sc.VerifierMsg(chal[i])
        if i in (3, 7):  # a's kernel is resident from its first late round on
            with _lib.policy(batch=2):
                b0, s0 = plans()
                busy0 = stats()[1]
                assert_batch_equals(polys, want)
                assert plans() == (b0, s0 + 1) and stats()[1] > busy0
    a.close()


def test_an_expired_device_side_wait_is_proved_again_inside_the_call():
    """wait_spins = 1 (process-wide: a subprocess): blocks give their instances up before the host has answered; the call proves those
    again by the serial plan with device-side waits off and still returns the oracle's bits.  The library's designed status path with
    bounded waits -- run once."""
    code = r'''
import ctypes as C
import numpy as np, sumcheck_amd as sc
from sumcheck_amd import _lib
from tests import test_gpu_batch as T
_lib.set_policy("wait_spins", 1)
_lib.set_policy("batch", 2)
polys, descs = T.make_batch(64, 6, T.C2, 49000)
want = T.oracle_all(descs)
r0 = T.stats()[5]
b0, s0 = T.plans()
T.assert_batch_equals(polys, want)
print("RETRIES", T.stats()[5] - r0, "PLANS", T.plans()[0] - b0, T.plans()[1] - s0)
'''
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    words = r.stdout.split()
    assert "RETRIES" in words and int(words[words.index("RETRIES") + 1]) > 0, r.stdout + r.stderr[-500:]
    assert int(words[words.index("PLANS") + 1]) == 1, r.stdout


def test_a_batch_loop_beside_whole_proofs_on_another_thread():
    polys, descs = make_batch(256, 6, C2, 50000)
    want = oracle_all(descs)
    nv, shapes, nt = 15, [[0, 1, 2], [3]], 4
    tabs = [cref.synth_table(50100, s, 1 << nv) for s in range(nt)]
    coefs = cref.synth_table(50100, 1000, len(shapes))
    want_big, _ = cref.ml_prove(H.desc_from(nv, shapes, tabs, coefs), threads=4)
    poly, _ = H.hip_poly_from(nv, shapes, tabs, coefs, device="cuda:0")
    out = [None, None]
    stop = threading.Event()

    def batch_worker():
        try:
            for _ in range(20):
                assert_batch_equals(polys, want)
            out[0] = 0
        except Exception as e:
            out[0] = repr(e)
        finally:
            stop.set()

    def whole_worker():
        try:
            st = sc.IPForMLSumcheck.prover_init(poly, borrow=True)
            bad = reps = 0
            while reps < 40 or not stop.is_set():
                st.reset()
                bad += not np.array_equal(np.asarray(st.prove()).reshape(want_big.shape), want_big)
                reps += 1
                if reps >= 4000:
                    break
            st.close()
            out[1] = bad
        except Exception as e:
            out[1] = repr(e)

    ts = [threading.Thread(target=batch_worker), threading.Thread(target=whole_worker)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=600)
    assert out == [0, 0], out


def test_caches_release_limit_and_no_growth():
    import torch
    polys, descs = make_batch(300, 5, TWO, 51000)
    want = oracle_all(descs)
    assert_batch_equals(polys, want)
    assert sc.lib().sc_release_caches() == 0
    try:
        assert sc.lib().sc_set_cache_limit(0) == 0
        b0, s0 = plans()
        assert_batch_equals(polys, want)  # nothing is kept between calls: the call allocates and frees its own
        assert_batch_equals(polys, want)
        assert plans() == (b0 + 2, s0)
    finally:
        assert sc.lib().sc_set_cache_limit(16 << 30) == 0
    assert_batch_equals(polys, want)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(10):
        assert_batch_equals(polys, want)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free1 >= free0, "repeated batches of one size must not grow device memory"
    assert sc.lib().sc_release_caches() == 0


def test_every_proof_of_a_batch_verifies_with_its_claimed_sum():
    n, nv = 50, 7
    polys, descs = make_batch(n, nv, C3, 52000)
    want = oracle_all(descs)
    got = assert_batch_equals(polys, want)
    for i in range(n):
        claimed = field.add(want[i][0][0][0], want[i][0][0][1])  # the oracle's P_1(0) + P_1(1)
        sub = sc.MLSumcheck.verify(polys[i].info(), claimed, got[i])
        assert np.array_equal(polys[i].evaluate(sub.point), sub.expected_evaluation), i
