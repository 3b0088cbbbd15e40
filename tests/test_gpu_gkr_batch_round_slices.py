"""GPU tests of the sliced plan of the batched interactive GKR rounds (policy "batch_slices" = 1, plan batch.gkr_rounds_slices:
k_batch_gkr_terms + k_batch_gkr_fold for the two initialisations, k_batch_round_slices + k_batch_round_fin for the rounds beyond one
block's LDS, k_batch_round behind them) at dim 10 .. 16.  The oracle is the Walk of tests/test_gpu_gkr_batch_rounds.py: every message of
every round of every instance is compared bit for bit, the two tables after round calls {1, dim, dim + 1, 2 dim - 1}, finish's triple;
nothing is sampled.  Every test runs under the key and asserts which counters moved: the new plan 2 dim times per proof, the other two GKR
round plans not at all."""
import functools

import numpy as np
import pytest
import torch

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib
from tests import fe_model as fm
from tests import helpers as H
from tests import test_gpu_gkr_batch as T
from tests import test_gpu_gkr_batch_rounds as R
from tests.test_gpu_gkr_batch import make_batch

pytestmark = pytest.mark.gpu
P = cref.P
PM1 = R.raw(P - 1)


def plans():
    """(slices, one block, serial) of the GKR round handles; the ML handle's two work-area plans, which must not move"""
    p = _lib.plan_stats()
    return (p.get("batch.gkr_rounds_slices"), p["batch.gkr_rounds_one_block"], p["batch.gkr_rounds_serial"]), (p["batch.rounds_slices"], p["batch.rounds_one_block"])


def moved(before, slices=0, one_block=0, serial=0):
    (s0, b0, r0), ml0 = before
    (s1, b1, r1), ml1 = plans()
    assert (s1, b1, r1) == (s0 + slices, b0 + one_block, r0 + serial), "the GKR round plans' counters"
    assert ml1 == ml0, "batch.rounds_slices and batch.rounds_one_block belong to sc_batch_prove_round"


def td(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def batch_of(insts, dim):
    """instances (idx, vals, f2, f3, g) as host arrays -> make_batch's dict over device inputs"""
    b = {"n": len(insts), "dim": dim, "raw": insts, "gs": [a[4] for a in insts]}
    b["f1s"] = [sc.SparseMultilinearExtension(3 * dim, td(a[0]), td(a[1])) for a in insts]
    b["f2s"] = [sc.DenseMultilinearExtension(dim, td(a[2])) for a in insts]
    b["f3s"] = [sc.DenseMultilinearExtension(dim, td(a[3])) for a in insts]
    torch.cuda.synchronize()
    return b


# ---- 1. every round equals the walk ---------------------------------------------------------------------------------------------------
SHAPES = [(10, 1, True), (10, 6, True), (11, 1, True), (11, 6, True), (13, 2, False), (16, 2, False)]


@functools.lru_cache(maxsize=None)
def _parity_oracle(dim, n, ragged):
    b = make_batch(n, dim, 91000 + 97 * dim + n, device=None, ragged=ragged)
    chal = R.challenges(n, dim, 92000 + dim + n, edge_instance=n // 2)  # one instance's challenges cycle through 0, 1, p - 1
    chal.setflags(write=False)
    return chal, R.walks(b["raw"], dim, chal, R.state_rounds(dim))


@pytest.mark.parametrize("dim,n,ragged,device", [s + (d,) for s in SHAPES for d in (["cuda:0", None] if s[0] <= 11 else ["cuda:0"])],
                         ids=lambda v: {None: "host", "cuda:0": "device"}.get(v, str(v)))
def test_every_round_equals_the_walk(dim, n, ragged, device):
    """dim 10: the new initialisation, no sliced round; 11: the first sliced rounds, four slices; 13; 16: the limit, 128 slices, 48-bit
    indices.  Ragged lists at 10 / 11: nnz in {0, 1, N/2, N, 3N, 8N} across six instances, a lone instance with an empty list"""
    chal, want = _parity_oracle(dim, n, ragged)
    b = make_batch(n, dim, 91000 + 97 * dim + n, device=device, ragged=ragged)
    with _lib.policy(batch_slices=1):
        before = plans()
        st = R.init(b)
        R.drive(st, chal, want, R.state_rounds(dim))
        st.close()
        moved(before, slices=2 * dim)


# ---- 2. a shared challenge -----------------------------------------------------------------------------------------------------------
def test_a_shared_challenge_equals_the_same_challenge_n_times():
    n, dim = 3, 11
    b = make_batch(n, dim, 93000, ragged=True)
    chal = R.challenges(n, dim, 93001, edge_instance=None)
    same = np.repeat(chal[:, :1], n, axis=1)
    want = R.walks(b["raw"], dim, same)
    with _lib.policy(batch_slices=1):
        before = plans()
        st = R.init(b)
        shared, uv_s, fin_s = R.drive(st, chal, want, shared=True, label="shared: ")
        st.reset()
        each, uv_e, fin_e = R.drive(st, same, want, label="n times: ")
        st.close()
        moved(before, slices=4 * dim)
    assert np.array_equal(shared, each) and np.array_equal(uv_s, uv_e) and np.array_equal(fin_s, fin_e)


# ---- 3. collisions and extremes ------------------------------------------------------------------------------------------------------
def test_every_term_of_an_instance_in_one_cell_and_g_at_the_ends():
    """dim 10.  Instance 0: all 64 x 2^10 non-zeros on one x and one y with value p - 1 -- one cell's lanes at their largest and every
    atomic of a phase on the same eight addresses; instance 1: g from {0, 1, p - 1} and every other value zero; instance 2: g all p - 1
    (eq(g, z) non-zero for every z) over a list with repeated indices"""
    dim = 10
    N, nnz = 1 << dim, 64 << dim
    rng = np.random.default_rng(94000)
    z = rng.integers(0, N, size=nnz, dtype=np.uint64)
    idx = np.ascontiguousarray(z | np.uint64(777 << dim) | np.uint64(1023 << (2 * dim)))
    insts = [(idx, np.repeat(PM1[None], nnz, axis=0), cref.synth_table(94000, 2, N), np.repeat(PM1[None], N, axis=0), cref.synth_table(94000, 4, dim))]
    i1, v1 = T.make_f1(dim, 94001, "zeros", 2 * N)
    insts.append((i1, v1, cref.synth_table(94001, 2, N), cref.synth_table(94001, 3, N), np.ascontiguousarray(R.EDGE[np.arange(dim) % 3])))
    i2, v2 = T.make_f1(dim, 94002, "repeated", 3 * N)
    insts.append((i2, v2, cref.synth_table(94002, 2, N), cref.synth_table(94002, 3, N), np.repeat(PM1[None], dim, axis=0)))
    chal = R.challenges(3, dim, 94003, edge_instance=1)
    want = R.walks(insts, dim, chal, R.state_rounds(dim))
    b = batch_of(insts, dim)
    with _lib.policy(batch_slices=1):
        before = plans()
        st = R.init(b)
        R.drive(st, chal, want, R.state_rounds(dim))
        st.close()
        moved(before, slices=2 * dim)


def test_the_first_and_the_last_index_at_dim_16():
    """an entry at index 0 and one at 2^48 - 1 (every component at its largest: the last cell, the last f3 entry, the last eq entries),
    both twice, among random ones; g from {0, 1, p - 1}"""
    dim = 16
    N = 1 << dim
    idx, vals = T.make_f1(dim, 95000, "random", N // 4)
    idx = idx.copy()
    idx[[0, 5, 1000, N // 4 - 1]] = [0, (1 << 48) - 1, 0, (1 << 48) - 1]
    insts = [(np.ascontiguousarray(idx), vals, cref.synth_table(95000, 2, N), cref.synth_table(95000, 3, N), np.ascontiguousarray(R.EDGE[(np.arange(dim) + 2) % 3]))]
    chal = R.challenges(1, dim, 95001, edge_instance=None)
    want = R.walks(insts, dim, chal, R.state_rounds(dim))
    b = batch_of(insts, dim)
    with _lib.policy(batch_slices=1):
        before = plans()
        st = R.init(b)
        R.drive(st, chal, want, R.state_rounds(dim))
        st.close()
        moved(before, slices=2 * dim)


# ---- 4. f2 at the end of its range ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [11, 16])
def test_f2_sinks_to_the_end_of_its_range_at_the_phase_change(dim):
    """f2 a sinking table under the u challenges: after k binds its entries are at -k p, so the two entries the phase change binds with
    u_{dim-1} -- the operands of k_batch_gkr_fold<2>'s fe_mul_u -- are at -(dim - 1) p, the lower end of their range"""
    N = 1 << dim
    s, r = fm.sinking_challenges(dim, 96000 + dim)
    m, c = 3, 3 * sum(s) + 11
    f2 = H.sinking_table_limbs(dim, s, m, c)
    H.assert_entries_match(f2, H.sinking_entry(s, m, c), seed=dim)
    idx, vals = T.make_f1(dim, 96100 + dim, "random", N)
    insts = [(idx, vals, f2, cref.synth_table(96200 + dim, 3, N), cref.synth_table(96200 + dim, 4, dim))]
    chal = R.challenges(1, dim, 96300 + dim, edge_instance=None)
    chal[:dim, 0] = H.mont_challenges(r)
    want = R.walks(insts, dim, chal, R.state_rounds(dim))
    b = batch_of(insts, dim)
    with _lib.policy(batch_slices=1):
        before = plans()
        st = R.init(b)
        R.drive(st, chal, want, R.state_rounds(dim))
        st.close()
        moved(before, slices=2 * dim)


# ---- 5. the handle -------------------------------------------------------------------------------------------------------------------
def test_reset_two_handles_and_a_refused_challenge_at_the_phase_change():
    n, dim = 2, 11
    ba, bb = make_batch(n, dim, 97000, nnz=3 << dim), make_batch(n, dim, 97500, variant="repeated")
    c1, c2 = R.challenges(n, dim, 97001), R.challenges(n, dim, 97002, edge_instance=1)
    wa1, wa2, wb = R.walks(ba["raw"], dim, c1), R.walks(ba["raw"], dim, c2, [dim]), R.walks(bb["raw"], dim, c2)
    with _lib.policy(batch_slices=1):
        before = plans()
        sa, sb = R.init(ba), R.init(bb)
    # (the plan was chosen when the handles were built: the key may go back to its default)
    R.drive(sa, c1, wa1)
    sa.reset()
    assert sa.round == 0 and sa.randomness(0).shape[0] == 0
    moved(before, slices=2 * dim)
    for t in range(2 * dim):  # two handles in turn, other challenges for the first
        if t == dim:  # a non-canonical challenge at the phase change: nothing moves, phase two is not built over it
            bad = c2[t - 1].copy()
            bad[1] = R.P_LIMBS
            mid = plans()
            tabs = [sa.tables(i) for i in range(n)]
            assert R._raises(_lib.SC_ERR_BAD_ARG, sa.prove_round, bad) == "instance 1: challenge is not canonical"
            assert sa.round == dim and sa.randomness(0).shape[0] == dim - 1 and plans() == mid
            for i in range(n):
                assert np.array_equal(sa.tables(i), tabs[i]) and np.array_equal(tabs[i], wa2[i].states[dim]), i
        ga = sa.prove_round(None if t == 0 else c2[t - 1])
        gb = sb.prove_round(None if t == 0 else c2[t - 1])
        assert np.array_equal(ga, np.stack([w.msgs[t] for w in wa2])), f"handle a, round call {t}"
        assert np.array_equal(gb, np.stack([w.msgs[t] for w in wb])), f"handle b, round call {t}"
    _, fa = sa.finish(c2[2 * dim - 1])
    _, fb = sb.finish(c2[2 * dim - 1])
    for i in range(n):
        assert np.array_equal(fa[i], wa2[i].final) and np.array_equal(fb[i], wb[i].final), i
    sa.close()
    sb.close()
    moved(before, slices=6 * dim)


# ---- 6. the envelope's edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,nnz,pol,expect", [(17, None, {"batch_slices": 1}, "serial"), (10, (64 << 10) + 1, {"batch_slices": 1}, "serial"), (10, None, {}, "serial"),
                                                (10, None, {"batch_slices": 1, "batch": 0}, "serial"), (9, None, {"batch_slices": 1}, "one_block"),
                                                (10, 64 << 10, {"batch_slices": 1}, "slices")],
                         ids=["dim17", "nnz-cap-plus-1", "key-default", "batch0", "dim9", "nnz-cap"])
def test_the_envelopes_edges_give_the_walks_messages_on_their_plan(dim, nnz, pol, expect):
    n = 1 if dim == 17 else 2
    b = make_batch(n, dim, 98000 + dim, nnz=nnz, variant="repeated" if nnz else "random")
    chal = R.challenges(n, dim, 98500 + dim)
    want = R.walks(b["raw"], dim, chal)
    with _lib.policy(**pol):
        before = plans()
        st = R.init(b)
        R.drive(st, chal, want)
        st.close()
        moved(before, **{expect: 2 * dim})


# ---- 7. a device-resident index out of range -----------------------------------------------------------------------------------------
def test_a_device_resident_index_out_of_range_fails_at_init_never_followed():
    n, dim = 4, 10
    b = make_batch(n, dim, 99000)
    for i, bit in ((2, 3 * dim), (3, 63)):
        idx = b["raw"][i][0].copy()
        idx[3] |= np.uint64(1) << np.uint64(bit)
        b["f1s"][i] = sc.SparseMultilinearExtension(3 * dim, td(idx), b["f1s"][i].values)
    torch.cuda.synchronize()
    with _lib.policy(batch_slices=1):
        before = plans()
        msg = R._raises(_lib.SC_ERR_BAD_ARG, R.init, b)
        moved(before)
    assert msg.startswith("instance 2: f1 has an index out of range"), msg


# ---- 8. the caller's transcripts reproduce cref.gkr_prove ----------------------------------------------------------------------------
def test_the_callers_transcripts_reproduce_the_oracles_proof():
    n, dim = 3, 11
    b = make_batch(n, dim, 99500, ragged=True, feed=b"a layer's transcript before instance %d")
    want = T.oracle_all(b)  # cref.gkr_prove under Blake2b: (proof, uv, next sample)
    mine = []
    for i in range(n):
        mine.append(sc.Blake2b512Rng.setup())
        mine[i].feed(b"a layer's transcript before instance %d" % i)
    with _lib.policy(batch_slices=1):
        before = plans()
        st = R.init(b)
        proofs, uv, _ = R.prove_with_transcripts(st, mine)
        st.close()
        moved(before, slices=2 * dim)
    for i, (wp, wuv, wnext) in enumerate(want):
        assert np.array_equal(proofs[i], wp), f"instance {i}: the proof differs from cref.gkr_prove's"
        assert np.array_equal(uv[i], wuv), f"instance {i}: (u, v)"
        assert np.array_equal(mine[i].sample_fr(), wnext), f"instance {i}: the transcript after the proof"
