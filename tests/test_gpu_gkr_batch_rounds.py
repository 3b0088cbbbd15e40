"""GPU tests of the batched interactive GKR rounds (sc_gkr_batch_prover_*: GKRRoundSumcheck.prover_init_batch / GKRBatchProverState): the
2 dim rounds of n small GKRRoundSumcheck::prove under the CALLER's challenges, one call per round.  Two oracles:
  (a) the walk with arbitrary challenges, composed from oracle/cref.py -- gkr_phase_one, a Prover over (h_g, f2), f2(u) by fix_variables,
      gkr_phase_two, f3 * f2(u) entry by entry (fr_binop), a second Prover over (f1_gu, f2(u) f3).  Fed cref.gkr_prove's own challenges it
      reproduces cref.gkr_prove's messages bit for bit (test 2 checks exactly that through the handle);
  (b) cref.gkr_prove under Blake2b.
Every message of every round of every instance of every batch is compared: none sampled, none skipped."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib
from tests import test_gpu_gkr_batch as T
from tests.test_gpu_gkr_batch import make_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = cref.P
ONE = cref.ints_to_mont([1])[0]
EDGE = cref.ints_to_mont([0, 1, P - 1])  # the field's 0, 1 and -1 as the library stores them
P_LIMBS = np.array([(P >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)  # p itself: the smallest non-canonical pattern


def raw(v):
    """the stored limbs of value v (whatever field element that is): p - 1 is the largest canonical pattern"""
    assert 0 <= v < P
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def plans():
    p = _lib.plan_stats()
    return p["batch.gkr_rounds_one_block"], p["batch.gkr_rounds_serial"]


def challenges(n, dim, seed, edge_instance=0):
    """(2 dim, n, 4): challenge [j][i] follows message j of instance i (the last one goes to finish) -- all distinct, but for ONE instance
    position j is 0, 1 or p - 1 in turn"""
    chal = cref.synth_table(seed, 77, 2 * dim * n).reshape(2 * dim, n, 4).copy()
    if edge_instance is not None:
        for j in range(2 * dim):
            chal[j, min(edge_instance, n - 1)] = EDGE[j % 3]
    return chal


class Walk:
    """oracle (a) for ONE instance: messages (2 dim, 3, 4), the provers' tables after the round calls in `states`, (f1(g,u,v), f2(u), f2(u) f3(v))"""

    def __init__(self, inst, dim, chal, states=()):
        idx, vals, f2, f3, g = inst
        N = 1 << dim
        desc = lambda a, b: cref.PolyDesc(dim, [(ONE, [0, 1])], [a, b])
        h_g, gi, gv = cref.gkr_phase_one(idx, vals, dim, f3, g)
        self.msgs, self.states = [], {}
        p = cref.Prover(desc(h_g, f2))
        for t in range(dim):
            self.msgs.append(p.prove_round(None if t == 0 else chal[t - 1]))
            if t + 1 in states:
                self.states[t + 1] = p.state()[1]
        p.close()
        u = np.ascontiguousarray(chal[:dim])
        f2u = cref.fix_variables(f2, u)[0]
        f1gu = cref.gkr_phase_two(gi, gv, dim, u)
        t1 = np.stack([cref.fr_binop("mul", f3[e], f2u) for e in range(N)])  # mod.rs:71-75
        p = cref.Prover(desc(f1gu, t1))
        for r in range(dim):
            self.msgs.append(p.prove_round(None if r == 0 else chal[dim + r - 1]))
            if dim + r + 1 in states:
                self.states[dim + r + 1] = p.state()[1]
        p.close()
        v = np.ascontiguousarray(chal[dim:2 * dim])
        self.msgs = np.stack(self.msgs)
        self.final = np.stack([cref.fix_variables(f1gu, v)[0], f2u, cref.fix_variables(t1, v)[0]])


def state_rounds(dim):
    return sorted({1, dim, dim + 1, 2 * dim - 1} & set(range(1, 2 * dim + 1)))


def walks(raw_insts, dim, chal, states=()):
    return [Walk(inst, dim, np.ascontiguousarray(chal[:, i]), states) for i, inst in enumerate(raw_insts)]


def init(b):
    return sc.GKRRoundSumcheck.prover_init_batch(b["f1s"], b["f2s"], b["f3s"], b["gs"])


def drive(st, chal, want, states=(), shared=False, label=""):
    """all 2 dim rounds and finish against the walks; -> (messages (n, 2 dim, 3, 4), uv, final)"""
    n, dim = st.n, st.dim
    msgs = []
    for t in range(2 * dim):
        r = None if t == 0 else (chal[t - 1][0] if shared else chal[t - 1])
        got = st.prove_round(r, shared=shared and t > 0)
        w = np.stack([want[i].msgs[t] for i in range(n)])
        bad = np.nonzero((got != w).any(axis=(1, 2)))[0]
        assert np.array_equal(got, w), f"{label}round call {t}: messages differ from the walk's, first for instance {bad[:1]}"
        msgs.append(got)
        assert st.round == t + 1
        if t + 1 in states:
            for i in range(n):
                assert np.array_equal(st.tables(i), want[i].states[t + 1]), f"{label}after round call {t}: the two tables of instance {i}"
    last = chal[2 * dim - 1]
    uv, fin = st.finish(last[0] if shared else last, shared=shared)
    for i in range(n):
        ci = chal[:, 0] if shared else chal[:, i]
        assert np.array_equal(uv[i].reshape(2 * dim, 4), ci), f"{label}uv of instance {i}"
        assert np.array_equal(st.randomness(i), ci), f"{label}randomness of instance {i}"
        assert np.array_equal(fin[i], want[i].final), f"{label}finish's triple of instance {i}"
    return np.stack(msgs, axis=1), uv, fin


# ---- 1. every round equals the walk ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _parity_oracle(dim, n):
    """shared by the device and the host case of a shape: the walk depends on the seeds only"""
    b = make_batch(n, dim, 81000 + 97 * dim + n, device=None, ragged=True)
    chal = challenges(n, dim, 82000 + dim + n, edge_instance=n // 2)
    chal.setflags(write=False)
    return chal, walks(b["raw"], dim, chal, state_rounds(dim))


@pytest.mark.parametrize("device", ["cuda:0", None], ids=["device", "host"])
@pytest.mark.parametrize("n", [1, 3, 67])
@pytest.mark.parametrize("dim", [1, 2, 5, 8, 9])
def test_every_round_equals_the_walk(dim, n, device):
    """one variable; fewer cells than a wavefront; fewer than a block; exactly kTsBlock cells; two strides per lane.  Ragged lists: nnz in
    {0, 1, N/2, N, 3N, 8N} across the instances"""
    chal, want = _parity_oracle(dim, n)
    b = make_batch(n, dim, 81000 + 97 * dim + n, device=device, ragged=True)
    b0, s0 = plans()
    st = init(b)
    drive(st, chal, want, state_rounds(dim))
    st.close()
    assert plans() == (b0 + 2 * dim, s0), "every round call of a batch within the envelope is counted once, on the batched plan"


# ---- 2. the caller's transcripts reproduce sc_gkr_prove_batch -------------------------------------------------------------------------
def prove_with_transcripts(st, rngs):
    """mod.rs:111-133 with the caller's n transcripts: feed the message, sample the challenge -> (proofs (n, 2, dim, 3, 4), uv, final)"""
    n, dim = st.n, st.dim
    r, msgs = None, []
    for t in range(2 * dim):
        got = st.prove_round(r)
        msgs.append(got)
        r = np.empty((n, 4), np.uint64)
        for i in range(n):
            rngs[i].feed(sc.ProverMsg(got[i]))
            r[i] = rngs[i].sample_fr()
    uv, fin = st.finish(r)
    return np.stack(msgs, axis=1).reshape(n, 2, dim, 3, 4), uv, fin


@pytest.mark.parametrize("dim", [4, 9])
@pytest.mark.parametrize("variant,kw", [("repeated", {}), ("zeros", {}), ("sorted", {}), ("random", {"shared_f1": True})], ids=["repeated", "zeros", "sorted", "shared_f1"])
def test_the_callers_transcripts_reproduce_the_batched_proof(variant, kw, dim):
    n = 5
    b = make_batch(n, dim, 83000 + dim, variant=variant, feed=b"a layer's transcript before instance %d", **kw)
    want = T.oracle_all(b)  # cref.gkr_prove under Blake2b: (proof, uv, next sample)
    mine = []
    for i in range(n):
        mine.append(sc.Blake2b512Rng.setup())
        mine[i].feed(b"a layer's transcript before instance %d" % i)
    st = init(b)
    proofs, uv, _ = prove_with_transcripts(st, mine)
    st.close()
    for i, (wp, wuv, wnext) in enumerate(want):
        assert np.array_equal(proofs[i], wp), f"instance {i}: the proof differs from cref.gkr_prove's"
        assert np.array_equal(uv[i], wuv), f"instance {i}: (u, v)"
        assert np.array_equal(mine[i].sample_fr(), wnext), f"instance {i}: the transcript after the proof"
    got = T.assert_batch_equals(b, want)  # ... and GKRRoundSumcheck.prove_batch over the same inputs gives the same
    for i in range(n):
        assert np.array_equal(np.stack([m.evaluations for m in got[i].phase1_sumcheck_msgs + got[i].phase2_sumcheck_msgs]), proofs[i].reshape(2 * dim, 3, 4))


# ---- 3. a shared challenge -----------------------------------------------------------------------------------------------------------
def test_a_shared_challenge_equals_the_same_challenge_n_times():
    n, dim = 4, 3
    b = make_batch(n, dim, 84000)
    chal = challenges(n, dim, 84001, edge_instance=None)
    same = np.repeat(chal[:, :1], n, axis=1)
    want = walks(b["raw"], dim, same)
    st = init(b)
    shared, uv_s, fin_s = drive(st, chal, want, shared=True, label="shared: ")
    st.reset()
    each, uv_e, fin_e = drive(st, same, want, label="n times: ")
    st.close()
    assert np.array_equal(shared, each) and np.array_equal(uv_s, uv_e) and np.array_equal(fin_s, fin_e)


# ---- 4. finish's triple --------------------------------------------------------------------------------------------------------------
def test_finishs_triple_is_the_subclaims_oracle_values():
    n, dim = 6, 5
    b = make_batch(n, dim, 85000, variant="repeated")
    want = T.oracle_all(b)
    mine = [sc.Blake2b512Rng.setup() for _ in range(n)]
    st = init(b)
    proofs, uv, fin = prove_with_transcripts(st, mine)
    st.close()
    ev = sc.GKRRoundSumcheck.evaluate_subclaims_batch(b["f1s"], b["f2s"], b["f3s"], b["gs"], uv)  # f1(g,u,v), f2(u), f3(v), their product
    for i in range(n):
        assert np.array_equal(proofs[i], want[i][0]), i
        assert np.array_equal(fin[i, 0], ev[i, 0]), f"instance {i}: f1(g,u,v)"
        assert np.array_equal(fin[i, 1], ev[i, 1]), f"instance {i}: f2(u)"
        assert np.array_equal(fin[i, 2], cref.fr_binop("mul", ev[i, 1], ev[i, 2])), f"instance {i}: f2(u) f3(v)"
        prod = cref.fr_binop("mul", fin[i, 0], fin[i, 2])
        assert np.array_equal(prod, ev[i, 3]), f"instance {i}: the product"
        proof = sc.gkr_round_sumcheck.GKRProof([sc.ProverMsg(m) for m in proofs[i, 0]], [sc.ProverMsg(m) for m in proofs[i, 1]])
        sub = sc.GKRRoundSumcheck.verify(sc.Blake2b512Rng.setup(), dim, proof, proof.extract_sum())
        assert np.array_equal(prod, sub.expected_evaluation), f"instance {i}: the verifier's expected evaluation"


# ---- 5. all terms in one cell --------------------------------------------------------------------------------------------------------
def test_all_terms_in_one_cell_at_the_ends_of_the_range():
    """nnz = 64 x 2^4 at dim 4, every index with the same x (phase one's cell) and the same y (phase two's), values and f3 all p - 1: the
    accumulator at its fullest; f2 and the challenges from {0, 1, p - 1}: the bound entries at the ends of their range"""
    n, dim = 3, 4
    N, nnz = 1 << dim, 64 << dim
    pm1 = raw(P - 1)
    ends = np.stack([raw(0), raw(1), pm1])
    rng = np.random.default_rng(86000)
    insts = []
    for i in range(n):
        x, y = (5 + i) % N, (11 + 3 * i) % N
        z = rng.integers(0, N, size=nnz, dtype=np.uint64)
        idx = np.ascontiguousarray(z | np.uint64(x << dim) | np.uint64(y << (2 * dim)))
        vals = np.repeat(pm1[None], nnz, axis=0)
        f2 = ends[rng.integers(0, 3, size=N)]
        f3 = np.repeat(pm1[None], N, axis=0)
        insts.append((idx, vals, np.ascontiguousarray(f2), np.ascontiguousarray(f3), cref.synth_table(86000 + i, 4, dim)))
    chal = ends[rng.integers(0, 3, size=(2 * dim, n))]
    want = walks(insts, dim, chal, state_rounds(dim))
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")
    f1s = [sc.SparseMultilinearExtension(3 * dim, td(a[0]), td(a[1])) for a in insts]
    f2s = [sc.DenseMultilinearExtension(dim, td(a[2])) for a in insts]
    f3s = [sc.DenseMultilinearExtension(dim, td(a[3])) for a in insts]
    torch.cuda.synchronize()
    b0, s0 = plans()
    st = sc.GKRRoundSumcheck.prover_init_batch(f1s, f2s, f3s, [a[4] for a in insts])
    drive(st, chal, want, state_rounds(dim))
    st.close()
    assert plans() == (b0 + 2 * dim, s0), "exactly at the cap of 64 non-zeros per cell: the kernel"


# ---- 6. the serial plan --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n,nnz,pol,direct", [(5, 3, None, 0, 1), (10, 2, None, 1, 1), (3, 3, 65 << 3, 1, 1), (5, 3, None, 0, 0)],
                         ids=["policy0-dim5", "dim10", "nnz65x8-dim3", "policy0-dim5-list_form"])
def test_the_serial_plan_gives_the_same_bits(dim, n, nnz, pol, direct):
    """policy "batch" = 0; beyond the envelope in dim and in nnz; and the dense tables through the list form (policy "gkr_direct" = 0)
    instead of the bucketed kernels -- sc_gkr_prove's two routes"""
    b = make_batch(n, dim, 87000 + dim, nnz=nnz, variant="repeated" if nnz or not direct else "random", ragged=not direct)
    chal = challenges(n, dim, 87500 + dim)
    want = walks(b["raw"], dim, chal, state_rounds(dim))
    with _lib.policy(batch=pol, gkr_direct=direct):
        b0, s0 = plans()
        l0 = _lib.plan_stats()["gkr.list_form"]
        st = init(b)
        drive(st, chal, want, state_rounds(dim))  # (the plan was chosen when the handle was built)
        assert plans() == (b0, s0 + 2 * dim), "only the serial counter moves, once per round call"
        assert direct or _lib.plan_stats()["gkr.list_form"] > l0
        st.reset()
        drive(st, chal, want, label="after a reset: ")
    st.close()


# ---- 7. misuse -----------------------------------------------------------------------------------------------------------------------
def _raises(code, fn, *a, **kw):
    with pytest.raises(sc.SumcheckError) as e:
        fn(*a, **kw)
    assert e.value.code == code, e.value.msg
    return e.value.msg


@pytest.mark.parametrize("pol", [1, 0], ids=["one_block", "serial"])
def test_misuse_maps_to_the_status_codes_and_leaves_the_handle_where_it_was(pol):
    n, dim = 4, 3
    b = make_batch(n, dim, 88000)
    chal = challenges(n, dim, 88001)
    want = walks(b["raw"], dim, chal)
    with _lib.policy(batch=pol):
        st = init(b)
    msg = lambda t: np.stack([want[i].msgs[t] for i in range(n)])
    _raises(_lib.SC_ERR_FIRST_ROUND_HAS_MSG, st.prove_round, chal[0])
    _raises(_lib.SC_ERR_NOT_ACTIVE, st.finish, chal[0])  # too early
    assert np.array_equal(st.prove_round(None), msg(0))
    _raises(_lib.SC_ERR_MISSING_MSG, st.prove_round, None)
    bad = chal[0].copy()
    bad[2] = P_LIMBS
    assert _raises(_lib.SC_ERR_BAD_ARG, st.prove_round, bad) == "instance 2: challenge is not canonical"
    assert st.round == 1 and st.randomness(0).shape[0] == 0
    for t in range(1, 2 * dim):
        if t == dim:  # the same at the phase change
            _raises(_lib.SC_ERR_MISSING_MSG, st.prove_round, None)
            _raises(_lib.SC_ERR_NOT_ACTIVE, st.finish, chal[t - 1])
        assert np.array_equal(st.prove_round(chal[t - 1]), msg(t)), t
    _raises(_lib.SC_ERR_NOT_ACTIVE, st.prove_round, chal[2 * dim - 1])  # after 2 dim rounds
    assert _raises(_lib.SC_ERR_BAD_ARG, st.finish, bad) == "instance 2: challenge is not canonical"
    uv, fin = st.finish(chal[2 * dim - 1])
    for i in range(n):
        assert np.array_equal(uv[i].reshape(2 * dim, 4), chal[:, i]) and np.array_equal(fin[i], want[i].final), i
    _raises(_lib.SC_ERR_NOT_ACTIVE, st.finish, chal[2 * dim - 1])
    _raises(_lib.SC_ERR_NOT_ACTIVE, st.prove_round, chal[0])
    st.close()


@pytest.mark.parametrize("pol", [1, 0], ids=["one_block", "serial"])
def test_a_device_resident_index_out_of_range_fails_at_init_never_followed(pol):
    n, dim = 9, 5
    b = make_batch(n, dim, 89000)
    for i, bit in ((6, 3 * dim), (8, 63)):
        idx = b["raw"][i][0].copy()
        idx[3] |= np.uint64(1) << np.uint64(bit)
        b["f1s"][i] = sc.SparseMultilinearExtension(3 * dim, torch.from_numpy(idx.view(np.int64)).to("cuda:0"), b["f1s"][i].values)
    torch.cuda.synchronize()
    before = plans()
    with _lib.policy(batch=pol):
        msg = _raises(_lib.SC_ERR_BAD_ARG, init, b)
    assert msg.startswith("instance 6: f1 has an index out of range"), msg
    assert plans() == before, "no round is ever launched"


# ---- 8. reset, two handles, released caches ------------------------------------------------------------------------------------------
def test_reset_two_handles_and_released_caches():
    n, dim = 5, 6
    ba, bb = make_batch(n, dim, 90000, ragged=True), make_batch(n, dim, 90500, variant="repeated")
    c1, c2 = challenges(n, dim, 90001), challenges(n, dim, 90002, edge_instance=3)
    wa1, wa2, wb = walks(ba["raw"], dim, c1), walks(ba["raw"], dim, c2), walks(bb["raw"], dim, c2)
    sa, sb = init(ba), init(bb)
    first, _, _ = drive(sa, c1, wa1)
    sa.reset()
    assert sa.round == 0 and sa.randomness(0).shape[0] == 0
    again, _, _ = drive(sa, c1, wa1, label="the same challenges after a reset: ")
    assert np.array_equal(first, again)
    sa.reset()
    # two handles in turn, other challenges for the first; the caches are released in the middle of both proofs
    for t in range(2 * dim):
        ga = sa.prove_round(None if t == 0 else c2[t - 1])
        gb = sb.prove_round(None if t == 0 else c2[t - 1])
        assert np.array_equal(ga, np.stack([w.msgs[t] for w in wa2])), f"handle a, round call {t}"
        assert np.array_equal(gb, np.stack([w.msgs[t] for w in wb])), f"handle b, round call {t}"
        if t == dim - 1:
            assert sc.lib().sc_release_caches() == 0
    _, fa = sa.finish(c2[2 * dim - 1])
    _, fb = sb.finish(c2[2 * dim - 1])
    for i in range(n):
        assert np.array_equal(fa[i], wa2[i].final) and np.array_equal(fb[i], wb[i].final), i
    sa.close()
    sb.close()


# ---- the C++ mirror ------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_reproduces_gkr_prove():
    """GKRRoundSumcheck::prover_init_batch / GKRBatchProverState of include/sumcheck_amd.hpp driven by Blake2b transcripts against
    GKRRoundSumcheck::prove, built the way tests/test_batch_rounds_host.py builds its mirror program"""
    from tests import test_cpp_mirror as M
    src = os.path.join(ROOT, "tests", "cpp", "test_gkr_batch_rounds_mirror.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "test_gkr_batch_rounds_mirror.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, "-o", out, "-L", M.LIBDIR, "-lsumcheck_hip", f"-Wl,-rpath,{M.LIBDIR}",
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([out], capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ALL TESTS PASSED" in r.stdout, r.stdout + r.stderr
