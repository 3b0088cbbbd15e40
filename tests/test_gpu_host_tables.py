"""The two paths that exist only for HOST tables (sumcheck_amd/csrc/protocol.hip), at their chunk, shape and memory edges:

  S  streamed handles (sc_prover_init_streamed, launch_round_streamed): two chunks and the nv = 11 threshold, the clamp of the chunk request,
     PINNED tables (the copies then really overlap the kernels: the ring's ev_copied / ev_consumed waits order them), a table that no product
     names, the three per-product kernels in one polynomial, tables of 0, 1 and p - 1, a reset onto new tables, 36 tables;
  T  staged initialisation (staged_copy_and_round1): the sizes either side of nv = 18 and of the six-chunk split at 21, K = 1 under the capped
     grid, one table (one copy stream), the edges of the merged shape, the cached round 1 discarded by a caller that wants lanes, a reset onto
     host tables behind a lagging device-table proof, an unreferenced table.

Every message is compared bit for bit with the oracle's (cref.Prover under fixed challenges; the Fiat-Shamir proof with cref.Prover and
cref.Rng), the exported tables with its .state().  The plan counters are read around every call.  big.streamed moves once per call of
launch_round_streamed (rounds 1 and 2 of a streamed handle); big.staged_round1 once per staged_copy_and_round1 (an init or a reset);
big.merged.round1 / big.merged.bind_chain once per LAUNCH of the merged kernel, so they count the chunks of a merged shape.
tests/host_table_cases.py states the inequality behind every expectation."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib, sharded
from tests import helpers as H
from tests import host_table_cases as HT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VM = sc.VerifierMsg
LAG = ("big.lag_class_round", "big.lag_catch_up", "big.lag_materialize")


def moved_since(before):
    after = _lib.plan_stats()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


@functools.lru_cache(maxsize=None)
def synth(nv, n, seed=HT.SEED):
    """synthetic tables, once per (size, count, seed); never written to (every test checks that at its end)"""
    return tuple(HT.synth_tables(nv, n, seed))


@pytest.fixture(scope="module", autouse=True)
def free_the_tables():
    yield
    synth.cache_clear()


def in_memory(tabs, memory):
    """-> (arrays the library will read, the pinned tensors that own them or None): copies, so that the shared tables stay as they are"""
    if memory == "pageable":
        return [t.copy() for t in tabs], None
    pairs = [HT.pinned_like(t) for t in tabs]
    return [v for _, v in pairs], [t for t, _ in pairs]


def host_poly(nv, shapes, arrays, coefs, owners=None):
    """the wrapper's polynomial over host arrays; with pinned owners: the library is handed the pinned pages themselves"""
    poly, mles = H.hip_poly_from(nv, shapes, arrays, coefs)
    for u, m in enumerate(mles):
        assert m.data_ptr() == arrays[u].ctypes.data
        if owners is not None:
            assert m.data_ptr() == owners[u].data_ptr() and owners[u].is_pinned()
    assert [id(m) for m in poly.flattened_ml_extensions] == [id(m) for m in mles], "the shapes name their tables in first-occurrence order"
    return poly


def assert_tables(st, want_tabs, what):
    got = st.flattened_ml_extensions
    assert len(got) == len(want_tabs)
    for u, t in enumerate(got):
        assert np.array_equal(t.evaluations, want_tabs[u]), f"table {u} {what}"


def drive(st, chal, want, otabs, last):
    """rounds 1 .. last through sc_prove_round: every message, and the tables after the rounds of `otabs`, against the oracle's
    -> the plan counters each round's call moved"""
    per_round = []
    for j in range(last):
        before = _lib.plan_stats()
        got = sc.IPForMLSumcheck.prove_round(st, None if j == 0 else VM(chal[j - 1])).evaluations
        per_round.append(moved_since(before))
        assert np.array_equal(got, want[j]), f"round {j + 1}"
        if j + 1 in otabs:
            assert_tables(st, otabs[j + 1], f"after round {j + 1}")
    return per_round


def assert_unchanged(arrays, tabs):
    for u, (a, t) in enumerate(zip(arrays, tabs)):
        assert np.array_equal(a, t), f"the caller's table {u} was written to"


def table_ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


# ---- S: streamed handles ----------------------------------------------------------------------------------------------------------------------
def streamed_counters(per_round, nv, chunk, shapes, streams=True):
    """launch_round_streamed runs for rounds 1 and 2 alone; a merged shape is one launch of the merged kernel per chunk"""
    n = HT.n_chunks(nv, chunk)
    for j, m in enumerate(per_round):
        assert m.get("big.streamed", 0) == (1 if streams and j < 2 else 0), f"round {j + 1}: {m}"
    if streams and HT.is_merged(shapes):
        assert per_round[0].get("big.merged.round1", 0) == n, f"round 1 in {n} chunks: {per_round[0]}"
        assert per_round[1].get("big.merged.bind_chain", 0) == n and "big.merged.bind" not in per_round[1], f"round 2 in {n} chunks: {per_round[1]}"
    elif streams:
        assert not any(k.startswith("big.merged") for m in per_round[:2] for k in m), per_round[:2]


def run_streamed(st, nv, chunk, shapes, tabs, coefs, chal, arrays, proofs=1, streams=True):
    """the interactive rounds with the tables after rounds 1, 2 and 3; then `proofs` Fiat-Shamir proofs on the rewound handle"""
    want, otabs = HT.oracle_rounds(nv, shapes, tabs, coefs, chal, (1, 2, 3))
    per_round = drive(st, chal, want, otabs, nv)
    streamed_counters(per_round, nv, chunk, shapes, streams)
    proof = HT.oracle_proof(nv, shapes, tabs, coefs)
    for i in range(proofs):
        before = _lib.plan_stats()
        st.reset()
        got = st.prove(sc.Blake2b512Rng.setup())
        assert np.array_equal(got, proof), f"reset + prove {i + 1}: the Fiat-Shamir proof differs from the oracle's"
        assert moved_since(before).get("big.streamed", 0) == (2 if streams else 0)
    assert_unchanged(arrays, tabs)
    return want, otabs


@pytest.mark.parametrize("name", ["S1-threshold", "S1-below"])
def test_two_chunks_at_the_streaming_threshold(name):
    """nv = 11, chunk 2^10: the smallest table that streams, in two chunks -- each ring slot used once, the `c >= 2` waits never run.
    nv = 10 with the same request is silently a copying handle (big.streamed does not move) that rewinds like a streamed one: reset() with
    NULL tables copies the remembered host tables in again (host_tabs)."""
    nv, chunk, shapes, nt = HT.STREAMED[name]
    tabs, coefs, chal = synth(nv, nt), HT.synth_coefs(nv, shapes), HT.synth_challenges(nv)
    arrays, _ = in_memory(tabs, "pageable")
    st = sc.IPForMLSumcheck.prover_init(host_poly(nv, shapes, arrays, coefs), streamed_chunk_log2=chunk)
    run_streamed(st, nv, chunk, shapes, tabs, coefs, chal, arrays, proofs=2, streams=HT.is_streamed(nv))
    st.close()


def test_the_chunk_request_is_clamped():
    """nv = 12 under the requests 1, 10, 12 and 63: 2^10 (four chunks) twice and the whole table (one chunk) twice -- the same bits"""
    nv, shapes = HT.CLAMP_NV, HT.BASE
    tabs, coefs, chal = synth(nv, 3), HT.synth_coefs(nv, shapes), HT.synth_challenges(nv)
    seen = []
    for request in HT.CLAMP_REQUESTS:
        arrays, _ = in_memory(tabs, "pageable")
        st = sc.IPForMLSumcheck.prover_init(host_poly(nv, shapes, arrays, coefs), streamed_chunk_log2=request)
        want, otabs = run_streamed(st, nv, request, shapes, tabs, coefs, chal, arrays)  # (counts the chunks: big.merged.round1)
        st.close()
        seen.append((np.stack(want), otabs))
    for msgs, otabs in seen[1:]:
        assert np.array_equal(msgs, seen[0][0]) and all(np.array_equal(otabs[j], seen[0][1][j]) for j in (1, 2, 3))


@pytest.mark.parametrize("memory", ["pageable", "pinned"])
@pytest.mark.parametrize("name", HT.PINNED_CASES)
def test_streaming_from_pinned_memory(name, memory):
    """the same tables from pageable and from page-locked memory.  From pinned pages hipMemcpyAsync returns at once and the copy engine runs
    beside the kernels: what keeps a chunk's copy from overwriting a slot still being read is the ring's ev_consumed wait, what keeps a
    kernel off a slot still being filled its ev_copied wait; the generic arm's per-slot pointer set is guarded by a host-side wait on
    ev_consumed.  64 chunks of three tables (merged), 16 chunks of fourteen small launches, 8 chunks of k_sum_generic; three proofs back to
    back on the handle, so that slots and events are reused across proofs."""
    nv, chunk, shapes, nt = HT.STREAMED[name]
    tabs, coefs, chal = synth(nv, nt), HT.synth_coefs(nv, shapes), HT.synth_challenges(nv)
    arrays, owners = in_memory(tabs, memory)
    assert (owners is not None) == (memory == "pinned")
    st = sc.IPForMLSumcheck.prover_init(host_poly(nv, shapes, arrays, coefs, owners), streamed_chunk_log2=chunk)
    run_streamed(st, nv, chunk, shapes, tabs, coefs, chal, arrays, proofs=3)
    st.close()


@pytest.mark.parametrize("name", ["S4-unreferenced-merged", "S4-unreferenced-five"])
def test_streamed_table_that_no_product_names(name):
    """four tables of which the products name three (the C ABI permits it; the descriptor is built by ctypes).  Round 2 binds the odd table
    chunk by chunk with k_fix into the canonical layout while -- in the merged arm -- the others are stored packed; every later round binds
    it on (the state machine).  Every message, and every table after rounds 1, 2 and 3, the unreferenced one among them."""
    nv, chunk, shapes, nt = HT.STREAMED[name]
    u = HT.UNREFERENCED[name]
    tabs, coefs, chal = synth(nv, nt), HT.synth_coefs(nv, shapes), HT.synth_challenges(nv)
    arrays, _ = in_memory(tabs, "pageable")
    st = HT.raw_prover(nv, shapes, coefs, arrays, streamed_chunk_log2=chunk)
    _, otabs = run_streamed(st, nv, chunk, shapes, tabs, coefs, chal, arrays)
    for j in (2, 3):  # (the oracle's treatment of the table is pinned by tests/test_host_table_cases_host.py)
        assert np.array_equal(otabs[j][u], cref.fix_variables(tabs[u], chal[: j - 1]))
    st.close()


def test_three_per_product_kernels_in_one_streamed_polynomial():
    """K = 13, so no merged launch: per chunk, k_fix binds every table, then a product tree ([0, 1, 2] and ten pairs), the carry-free
    node-by-node kernel (six factors) and k_sum_generic (ten factors, through the slot's pointer set) sum over shared tables"""
    name = "S5-three-arms"
    nv, chunk, shapes, nt = HT.STREAMED[name]
    tabs, coefs, chal = synth(nv, nt), HT.synth_coefs(nv, shapes), HT.synth_challenges(nv)
    arrays, _ = in_memory(tabs, "pageable")
    st = sc.IPForMLSumcheck.prover_init(host_poly(nv, shapes, arrays, coefs), streamed_chunk_log2=chunk)
    run_streamed(st, nv, chunk, shapes, tabs, coefs, chal, arrays)
    st.close()


@pytest.mark.parametrize("name", ["S6-extreme-merged", "S6-extreme-generic"])
def test_streamed_extreme_values(name):
    """tables of 0, 1 and p - 1 (one of them p - 1 throughout) under the challenges p - 1, 0, 1, p - 1, ...: round 2 binds canonical host
    entries chunk by chunk into packed blocks (merged, with a repeated factor) or with k_fix in front of k_sum_generic"""
    nv, chunk, shapes, nt = HT.STREAMED[name]
    tabs, coefs, chal = HT.extreme_tables(nv, nt), HT.synth_coefs(nv, shapes), HT.extreme_challenges(nv)
    arrays, _ = in_memory(tabs, "pageable")
    st = sc.IPForMLSumcheck.prover_init(host_poly(nv, shapes, arrays, coefs), streamed_chunk_log2=chunk)
    run_streamed(st, nv, chunk, shapes, tabs, coefs, chal, arrays)
    st.close()


def test_streamed_reset_onto_new_host_tables():
    """a proof abandoned after round 1, sc_prover_reset(h, NEW host tables, 0), and the proof over the second set; in between a reset that
    names device tables is refused (SC_ERR_BAD_ARG) and leaves the handle as it was: round 2 goes on"""
    nv, chunk, shapes, nt = HT.STREAMED["S7-reset"]
    tabs_a, tabs_b = synth(nv, nt), synth(nv, nt, HT.SEED + 0x100)
    coefs, chal = HT.synth_coefs(nv, shapes), HT.synth_challenges(nv)
    arr_a, _ = in_memory(tabs_a, "pageable")
    arr_b, _ = in_memory(tabs_b, "pageable")
    want_a, _ = HT.oracle_rounds(nv, shapes, tabs_a, coefs, chal, last=1)
    want_b, otabs_b = HT.oracle_rounds(nv, shapes, tabs_b, coefs, chal, (1, 2, 3))
    st = sc.IPForMLSumcheck.prover_init(host_poly(nv, shapes, arr_a, coefs), streamed_chunk_log2=chunk)
    before = _lib.plan_stats()
    assert np.array_equal(sc.IPForMLSumcheck.prove_round(st, None).evaluations, want_a[0]), "round 1 over the first set"
    ptrs_b = table_ptrs(arr_b)
    _lib.check(sc.lib().sc_prover_reset(st._h, ptrs_b, 0))
    assert st.round == 0
    assert np.array_equal(sc.IPForMLSumcheck.prove_round(st, None).evaluations, want_b[0]), "round 1 over the second set"
    assert_tables(st, otabs_b[1], "after round 1 (the second set, still on the host)")
    assert sc.lib().sc_prover_reset(st._h, ptrs_b, _lib.SC_TABLES_ON_DEVICE) == _lib.SC_ERR_BAD_ARG, "streamed tables are host tables"
    assert st.round == 1
    for j in range(1, nv):
        got = sc.IPForMLSumcheck.prove_round(st, VM(chal[j - 1])).evaluations
        assert np.array_equal(got, want_b[j]), f"round {j + 1} over the second set"
        if j + 1 in otabs_b:
            assert_tables(st, otabs_b[j + 1], f"after round {j + 1}")
    assert moved_since(before).get("big.streamed", 0) == 3
    st.reset()
    assert np.array_equal(st.prove(sc.Blake2b512Rng.setup()), HT.oracle_proof(nv, shapes, tabs_b, coefs)), "reset + prove over the second set"
    assert_unchanged(arr_a, tabs_a)
    assert_unchanged(arr_b, tabs_b)
    st.close()


def test_thirty_six_tables_streamed_through_the_merged_launch():
    """twelve three-factor products over 36 tables: more tables than one pointer block holds, so the handle keeps canonical bound tables and
    the later rounds go through device-side pointers; rounds 1 and 2 are the merged launch over the ring, chunk by chunk"""
    nv, chunk, shapes, nt = HT.STREAMED["S8-thirty-six"]
    tabs, coefs, chal = synth(nv, nt), HT.synth_coefs(nv, shapes), HT.synth_challenges(nv)
    arrays, _ = in_memory(tabs, "pageable")
    st = sc.IPForMLSumcheck.prover_init(host_poly(nv, shapes, arrays, coefs), streamed_chunk_log2=chunk)
    run_streamed(st, nv, chunk, shapes, tabs, coefs, chal, arrays)
    st.close()


# ---- T: staged initialisation -----------------------------------------------------------------------------------------------------------------
def init_counters(moved, nv, staged):
    """a staged init is ONE big.staged_round1 and one launch of round 1's merged kernel per chunk; any other init launches nothing"""
    assert moved.get("big.staged_round1", 0) == (1 if staged else 0), moved
    assert moved.get("big.merged.round1", 0) == (HT.staged_chunks(nv) if staged else 0), moved


def run_staged(nv, shapes, tabs, coefs, memory="pageable", mode="host", policy=1):
    """prover_init, rounds 1 .. 4 with the tables after each of them, then a one-shot proof of a fresh polynomial over the same tables"""
    staged = HT.is_staged(nv, shapes, host=mode == "host", borrow=mode == "borrow", policy=policy)
    chal = HT.synth_challenges(nv)
    want, otabs = HT.oracle_rounds(nv, shapes, tabs, coefs, chal, (1, 2, 3, 4), last=4)
    arrays, owners = in_memory(tabs, memory) if mode == "host" else (None, None)

    def make_poly():
        if mode == "host":
            return host_poly(nv, shapes, arrays, coefs, owners)
        poly, _ = H.hip_poly_from(nv, shapes, list(tabs), coefs, device=DEV)
        torch.cuda.synchronize()
        return poly

    with _lib.policy(staged_init=policy):
        poly = make_poly()
        before = _lib.plan_stats()
        st = sc.IPForMLSumcheck.prover_init(poly, borrow=mode == "borrow")
        init_counters(moved_since(before), nv, staged)
        per_round = drive(st, chal, want, otabs, 4)
        # the cached message is taken: round 1 launches nothing; otherwise round 1 is a launch
        assert ("big.merged.round1" in per_round[0]) == (not staged and HT.is_merged(shapes)), per_round[0]
        assert not any("big.staged_round1" in m for m in per_round), per_round
        st.close()
        before = _lib.plan_stats()
        proof = sc.MLSumcheck.prove(make_poly())  # (a handle out of the pool is RESET onto the tables: the staged pass again)
        assert moved_since(before).get("big.staged_round1", 0) == (1 if staged else 0)
    assert np.array_equal(np.stack([m.evaluations for m in proof]), HT.oracle_proof(nv, shapes, tabs, coefs)), "the one-shot proof differs from the oracle's"
    if arrays is not None:
        assert_unchanged(arrays, tabs)


@pytest.mark.parametrize("memory", ["pageable", "pinned"])
@pytest.mark.parametrize("nv", HT.LADDER_NV)
def test_staged_init_size_ladder(nv, memory):
    """[[0, 1, 2], [2, 2], [0]] at nv = 17 (not staged), 18 (the first size: chunks of 1/2, 1/4, 1/4), 20 and 21 (the first six-chunk
    split: 1/2 ... 1/32, 1/32), from pageable and from pinned tables"""
    run_staged(nv, HT.LADDER_SHAPE, synth(nv, 3), HT.synth_coefs(nv, HT.LADDER_SHAPE), memory)


@pytest.mark.parametrize("name", list(HT.K1))
def test_staged_init_of_one_product(name):
    """K = 1: [[0, 1]] at nv = 22, where the grid is capped to kRoundTreeGrid and cut 192/96/96/96/96/192, and at nv = 19; [[0, 0]]: one
    table, so the second copy stream records nothing; [[0]]: a single-table product alone.  From pinned tables."""
    nv, shapes = HT.K1[name]
    nt = HT.n_named(shapes)
    run_staged(nv, shapes, synth(nv, nt), HT.synth_coefs(nv, shapes), "pinned")


@pytest.mark.parametrize("name", list(HT.EDGES))
def test_staged_init_at_the_edges_of_the_merged_shape(name):
    """nv = 18: twelve products stage and thirteen do not, four factors do and five do not; nor does anything under staged_init = 0, from
    device tables or over borrowed ones -- the oracle's bits in all seven"""
    shapes, mode, policy = HT.EDGES[name]
    nv = HT.EDGE_NV
    run_staged(nv, shapes, synth(nv, HT.n_named(shapes)), HT.synth_coefs(nv, shapes), mode=mode, policy=policy)


def staged_handle(nv, shapes, tabs, coefs):
    arrays, _ = in_memory(tabs, "pageable")
    before = _lib.plan_stats()
    st = sc.IPForMLSumcheck.prover_init(host_poly(nv, shapes, arrays, coefs))
    init_counters(moved_since(before), nv, True)
    return st, arrays


def test_partial_round_discards_the_cached_round_one():
    """the first call behind a staged init is sc_prove_round_partial: the caller wants lanes, the cached message is dropped and round 1 is
    computed again over the resident tables (one launch of the merged kernel); folded with sc_wide_reduce it is the oracle's round 1, and
    rounds 2 .. 4 go on as ordinary calls"""
    nv, shapes = 18, HT.LADDER_SHAPE
    tabs, coefs, chal = synth(nv, 3), HT.synth_coefs(nv, shapes), HT.synth_challenges(nv)
    want, otabs = HT.oracle_rounds(nv, shapes, tabs, coefs, chal, (1, 2, 3, 4), last=4)
    st, arrays = staged_handle(nv, shapes, tabs, coefs)
    lanes = torch.zeros((st.max_multiplicands + 1, 8), dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    before = _lib.plan_stats()
    _lib.check(sc.lib().sc_prove_round_partial(st._h, None, C.c_void_p(lanes.data_ptr())))
    moved = moved_since(before)
    torch.cuda.synchronize()  # (the handle works on a stream of its own)
    assert np.array_equal(sharded.wide_reduce(lanes.cpu().numpy().view(np.uint64)), want[0]), "round 1, computed again"
    assert moved.get("big.merged.round1", 0) == 1 and "big.staged_round1" not in moved, moved
    assert st.round == 1
    assert_tables(st, otabs[1], "after round 1")
    for j in range(1, 4):
        got = sc.IPForMLSumcheck.prove_round(st, VM(chal[j - 1])).evaluations
        assert np.array_equal(got, want[j]), f"round {j + 1}"
        assert_tables(st, otabs[j + 1], f"after round {j + 1}")
    st.close()
    assert_unchanged(arrays, tabs)


def test_reset_before_the_cached_round_one_is_taken():
    """sc_prover_reset with the same host tables straight after a staged init, before any round: the staged pass runs again, its message
    replaces the cached one, and the proof is the oracle's"""
    nv, shapes = 18, HT.LADDER_SHAPE
    tabs, coefs = synth(nv, 3), HT.synth_coefs(nv, shapes)
    proof = HT.oracle_proof(nv, shapes, tabs, coefs)
    st, arrays = staged_handle(nv, shapes, tabs, coefs)
    before = _lib.plan_stats()
    _lib.check(sc.lib().sc_prover_reset(st._h, table_ptrs(arrays), 0))
    init_counters(moved_since(before), nv, True)
    before = _lib.plan_stats()
    got = st.prove(sc.Blake2b512Rng.setup())
    assert np.array_equal(got, proof), "the Fiat-Shamir proof differs from the oracle's"
    assert "big.merged.round1" not in moved_since(before), "round 1 was the cached message"
    st.close()
    assert_unchanged(arrays, tabs)


@pytest.mark.parametrize("rounds", [3, 2])
def test_staged_reset_behind_a_lagging_proof(rounds):
    """config 3's shape at nv = 18 from DEVICE tables in copy mode: table 9 lags through round 2 (a class round) and is caught up in front
    of round 3.  The proof is abandoned after round 3 -- or after round 2, the table still lagging -- and the handle reset onto HOST tables:
    the staged pass runs before the lagging state is cleared.  Then back onto device tables, where the table lags again."""
    nv, shapes = 18, HT.C3
    tabs_d, tabs_h = synth(nv, 10), synth(nv, 10, HT.SEED + 0x200)
    coefs, chal = HT.synth_coefs(nv, shapes), HT.synth_challenges(nv)
    want, _ = HT.oracle_rounds(nv, shapes, tabs_d, coefs, chal, last=rounds)
    poly, mles = H.hip_poly_from(nv, shapes, list(tabs_d), coefs, device=DEV)
    torch.cuda.synchronize()
    before = _lib.plan_stats()
    st = sc.IPForMLSumcheck.prover_init(poly)
    init_counters(moved_since(before), nv, False)
    before = _lib.plan_stats()
    drive(st, chal, want, {}, rounds)
    moved = moved_since(before)
    assert moved.get(LAG[0], 0) == 1 and moved.get(LAG[1], 0) + moved.get(LAG[2], 0) == (1 if rounds == 3 else 0), moved

    arrays, _ = in_memory(tabs_h, "pageable")
    before = _lib.plan_stats()
    _lib.check(sc.lib().sc_prover_reset(st._h, table_ptrs(arrays), 0))
    init_counters(moved_since(before), nv, True)
    before = _lib.plan_stats()
    got = st.prove(sc.Blake2b512Rng.setup())
    moved = moved_since(before)
    assert np.array_equal(got, HT.oracle_proof(nv, shapes, tabs_h, coefs)), "the proof over the host tables differs from the oracle's"
    assert not any(moved.get(k, 0) for k in LAG), f"round 1 was the cached message: nothing decides to lag ({moved})"

    dev_ptrs = (C.c_void_p * len(mles))(*[m.data_ptr() for m in mles])
    before = _lib.plan_stats()
    _lib.check(sc.lib().sc_prover_reset(st._h, dev_ptrs, _lib.SC_TABLES_ON_DEVICE))
    init_counters(moved_since(before), nv, False)
    got = st.prove(sc.Blake2b512Rng.setup())
    moved = moved_since(before)
    assert np.array_equal(got, HT.oracle_proof(nv, shapes, tabs_d, coefs)), "the proof over the device tables differs from the oracle's"
    assert moved.get(LAG[0], 0) == 1 and moved.get(LAG[1], 0) + moved.get(LAG[2], 0) == 1, moved
    st.close()
    assert_unchanged(arrays, tabs_h)


def test_staged_table_that_no_product_names():
    """nv = 18, four host tables of which the products name three: the staged pass copies all four, the rounds bind the odd one on"""
    nv, shapes, nt = HT.T6
    u = HT.UNREFERENCED["T6-unreferenced"]
    tabs, coefs, chal = synth(nv, nt), HT.synth_coefs(nv, shapes), HT.synth_challenges(nv)
    want, otabs = HT.oracle_rounds(nv, shapes, tabs, coefs, chal, (1, 2, 3, 4), last=4)
    arrays, _ = in_memory(tabs, "pageable")
    before = _lib.plan_stats()
    st = HT.raw_prover(nv, shapes, coefs, arrays)
    init_counters(moved_since(before), nv, True)
    drive(st, chal, want, otabs, 4)
    for j in (2, 3, 4):
        assert np.array_equal(otabs[j][u], cref.fix_variables(tabs[u], chal[: j - 1]))
    before = _lib.plan_stats()
    _lib.check(sc.lib().sc_prover_reset(st._h, table_ptrs(arrays), 0))
    init_counters(moved_since(before), nv, True)
    assert np.array_equal(st.prove(sc.Blake2b512Rng.setup()), HT.oracle_proof(nv, shapes, tabs, coefs)), "reset + prove"
    st.close()
    assert_unchanged(arrays, tabs)
