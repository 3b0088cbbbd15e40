"""sc_ml_prove_sharded at every place where the cut between its sharded and its replicated rounds can fall (protocol.hip: sharded_tail_m,
sharded_tail), which policy "shard_gather_log2" moves and no other test sets:

  A  the threshold ladder on ONE handle per rank: m = 14, 0, 9, 13, 1, 14 -- every step rebuilds the tail prover and the exchange buffers;
  B  k >= glog and the step above it;  C  shards of one and two variables;  D  streamed shards (two local rounds at least);
  E  the peer-to-peer communicator on these, on a group of 16 and on a 64-word message through both inbox halves;
  F  0, 1 and p - 1 through the lanes of 16 ranks;  G  big rounds and a table that would lag, before sharded small rounds;
  H  sharded GKR with m = 0 in both phases.

G thread ranks in this process on GPU 0.  Every rank's proof and randomness equal the unsharded oracle's (cref.ml_prove) bit for bit -- but
those bits do not depend on where the cut fell.  So the host-transport cases run over a transport that writes every call down: exactly nl
all-reduces of 8 D words and one all-gather of U 2^m 32 bytes per rank and proof, (nl, m) from tests/sharded_cases.py (whose rule
tests/test_sharded_cases_host.py holds against a hand-written table).  The peer-to-peer cases cannot count; each has a host-transport twin
of the same (G, nv, shape, glog) here.  The plan counters sharded.host / sharded.p2p and sharded.gather_tail move by G per proof.

The policy is process-wide: set in the main thread before the ranks start, restored in `finally`.  Every rank thread is joined against a
deadline; a rank that hangs or meets a HIP error ends the file's remaining tests before they start a thread (helpers.run_ranks)."""
import functools
import itertools

import numpy as np
import pytest

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib, sharded
from tests import helpers as H
from tests import sharded_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEY = "shard_gather_log2"
LAG = ("big.lag_class_round", "big.lag_catch_up", "big.lag_materialize")
SHARDED = ("sharded.host", "sharded.p2p", "sharded.rccl_direct", "sharded.rccl_publish")
_GROUP = itertools.count(9001)  # peer-to-peer group ids no other file uses


def moved_since(before):
    after = _lib.plan_stats()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(tables, coefficients, oracle proof, oracle randomness), once per case; never written to"""
    c = SC.CASES[name]
    tabs, coefs = SC.inputs(name)
    want, wrand = SC.oracle_proof(c.nv, c.shapes, tabs, coefs)
    _SUMS[name] = [int(t.sum(dtype=np.uint64)) for t in tabs]
    return tabs, coefs, want, wrand


_SUMS = {}


def assert_inputs_untouched(name):
    """a streamed shard is read where the cache keeps it"""
    for u, t in enumerate(case_inputs(name)[0]):
        assert int(t.sum(dtype=np.uint64)) == _SUMS[name][u], f"{name}: the caller's table {u} was written to"


@pytest.fixture(scope="module", autouse=True)
def free_the_inputs():
    yield
    case_inputs.cache_clear()
    assert _lib.get_policy(KEY) == SC.GLOG_DEFAULT, "a test left the policy moved"


def assert_exchanges(rec, G, f, what):
    """every rank: nl all-reduces of 8 D words, then one all-gather of U 2^m 32 bytes (none with one rank)"""
    for r in range(G):
        assert rec.allreduce_words[r] == ([f["words"]] * f["nl"] if G > 1 else []), f"{what}, rank {r}: all-reduces {rec.allreduce_words[r]}, want {f['nl']} of {f['words']} words"
        assert rec.allgather_bytes[r] == ([f["gather_bytes"]] if G > 1 else []), f"{what}, rank {r}: all-gathers {rec.allgather_bytes[r]}, want one of {f['gather_bytes']} bytes"


def assert_counters(moved, G, transport, what, proofs=1):
    mine = "sharded.host" if transport == "host" else "sharded.p2p"
    assert moved.get(mine, 0) == G * proofs and all(moved.get(k, 0) == 0 for k in SHARDED if k != mine), f"{what}: {moved}"
    assert moved.get("sharded.gather_tail", 0) == (G * proofs if G > 1 else 0), f"{what}: {moved}"


class Ranks:
    """G ranks' handles and communicators, kept across steps: every step runs on fresh threads (helpers.run_ranks) under the policy the main
    thread has set; the FIRST step's threads build the handles (sc_set_device per thread, as a Rust host would)"""

    def __init__(self, G, nv, shapes, tabs, coefs, transport, chunk=None):
        self.G, self.nv, self.shapes, self.tabs, self.coefs, self.transport, self.chunk = G, nv, shapes, tabs, coefs, transport, chunk
        self.k, self.n_loc = SC.log2(G), (1 << nv) // G
        self.rec = H.RecordingExchange(G) if transport == "host" else None
        self.gid = next(_GROUP)
        self.state = [None] * G
        self.failed = False

    def shard(self, rank):
        return [np.ascontiguousarray(t[rank * self.n_loc:(rank + 1) * self.n_loc]) for t in self.tabs]

    def _enter(self, rank):
        _lib.check(sc.lib().sc_set_device(0))
        if self.state[rank] is None:
            eng = sharded.HipShardEngine(self.nv - self.k, self.shapes, self.coefs, self.shard(rank), DEV, borrow=True, streamed_chunk_log2=self.chunk)
            comm = self.rec.comm(rank) if self.rec is not None else sharded.P2PComm(self.gid, rank, self.G, DEV)
            self.state[rank] = (eng, comm)
        return self.state[rank]

    def run(self, work):
        try:
            return H.run_ranks(self.G, lambda rank: work(rank, *self._enter(rank)), on_error=self.rec.abort if self.rec is not None else None)
        except BaseException:
            self.failed = True
            raise

    def prove(self, glog, want, wrand, what):
        """one sharded proof per rank under policy glog (set by the caller's main thread): bits, exchanges, counters"""
        assert _lib.get_policy(KEY) == glog
        f = SC.facts(self.G, self.nv, self.shapes, glog, streamed=self.chunk is not None)
        if self.rec is not None:
            self.rec.clear()
        before = _lib.plan_stats()

        def work(rank, eng, comm):
            eng.reset()
            if self.transport == "p2p":
                comm.selftest()
            return sharded.prove_sharded_library(eng, comm, self.nv)

        res = self.run(work)
        moved = moved_since(before)
        for r, (proof, rand) in enumerate(res):
            assert np.array_equal(proof, want), f"{what}, rank {r}: the proof differs from the oracle's"
            assert np.array_equal(rand, wrand), f"{what}, rank {r}: the randomness differs from the oracle's"
        assert_counters(moved, self.G, self.transport, what)
        if self.rec is not None:
            assert_exchanges(self.rec, self.G, f, what)
        return moved

    def close(self):
        """main thread, after the last step; a group that failed is left alone (closing synchronises with a GPU that may not answer)"""
        if self.failed:
            return
        for st in self.state:
            if st is not None:
                st[1].close()
                st[0].close()


def run_case(name, transport, glogs=None):
    """the case's (G, nv, shape, inputs) on one handle per rank under each policy of `glogs` (default: the case's own)"""
    c = SC.CASES[name]
    tabs, coefs, want, wrand = case_inputs(name)
    ranks = Ranks(c.G, c.nv, c.shapes, tabs, coefs, transport, c.chunk)
    old = _lib.get_policy(KEY)
    try:
        for glog in glogs or (c.glog,):
            _lib.set_policy(KEY, glog)
            ranks.prove(glog, want, wrand, f"{name} over {transport} at glog = {glog}")
    finally:
        _lib.set_policy(KEY, old)
        ranks.close()
    assert_inputs_untouched(name)


def test_the_policy_takes_1_to_15():
    L = sc.lib()
    old = _lib.get_policy(KEY)
    try:
        assert old == SC.GLOG_DEFAULT
        for bad in (SC.GLOG_MIN - 1, SC.GLOG_MAX + 1):
            assert L.sc_set_policy(KEY.encode(), bad) == _lib.SC_ERR_BAD_ARG and _lib.get_policy(KEY) == old
        for good in (SC.GLOG_MIN, SC.GLOG_MAX):
            assert L.sc_set_policy(KEY.encode(), good) == 0 and _lib.get_policy(KEY) == good
    finally:
        _lib.set_policy(KEY, old)


# ---- A: the threshold ladder ------------------------------------------------------------------------------------------------------------------
def test_threshold_ladder_on_one_handle():
    """G = 2, nv = 17 (round 1 is a big round): proofs back to back on the same handles under glog = 15, 1, 10, 14, 2, 15 -- (m, nl) =
    (14, 2), (0, 16), (9, 7), (13, 3), (1, 15), (14, 2).  Every change of m frees and rebuilds the tail prover and the three exchange buffers
    (sharded_tail); the last step returns to a size used before.  A stale tail prover or buffer of the previous size gives a wrong proof."""
    assert [SC.CASES[n].glog for n in SC.LADDER_ORDER] == [15, 1, 10, 14, 2, 15]
    assert len({(SC.CASES[n].G, SC.CASES[n].nv, str(SC.CASES[n].shapes)) for n in SC.LADDER_ORDER}) == 1
    run_case("A-15", "host", glogs=[SC.CASES[n].glog for n in SC.LADDER_ORDER])


# ---- B, C, D and the twins of E: one proof's cut each --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["B-2", "B-3", "B-4"])
def test_ranks_at_and_above_the_gather_threshold(name):
    """G = 8: glog = 2 and 3 (k >= glog) gather one element per table and rank, glog = 4 two"""
    run_case(name, "host")


def test_gather_threshold_steps_on_one_handle():
    """B again, on the same handles: m = 0, 0, 1 -- the middle step reuses the tail prover, the last rebuilds it"""
    run_case("B-2", "host", glogs=[2, 3, 4])


@pytest.mark.parametrize("name", ["C-2x1", "C-8x1", "C-16x1", "C-4x2-15", "C-4x2-1"])
def test_smallest_shards(name):
    """shards of one variable (two entries per table: the nv_local - 1 clamp gives m = 0 at the default policy; launch_gather_to_tables at
    per = 1 is a pure transposition rank <-> table) and of two (m = 1 at the default, 0 at glog = 1)"""
    run_case(name, "host")


@pytest.mark.parametrize("name", ["D-15", "D-3"])
def test_streamed_shards(name):
    """nv_local = 11, the smallest table that streams: at glog = 15 the streamed clamp leaves two local rounds (m = 9, where a resident shard
    would keep one); at glog = 3, rounds 1-2 stream and seven resident rounds are sharded behind them (m = 2)"""
    run_case(name, "host")


@pytest.mark.parametrize("name", ["E-16-15", "E-16-1", "E-seven"])
def test_host_twins_of_the_peer_to_peer_cases(name):
    """the largest group (16 ranks) at both ends of the policy, and a product of seven tables (D = 8: a 64-word message) over six sharded rounds"""
    run_case(name, "host")


def test_one_rank_never_exchanges():
    """G = 1: no all-reduce, no all-gather, no tail, whatever the policy"""
    nv, shapes = 6, SC.SMALL
    tabs = [cref.synth_table(SC.SEED, s, 1 << nv) for s in range(3)]
    coefs = cref.synth_table(SC.SEED, 1000, len(shapes))
    want, wrand = SC.oracle_proof(nv, shapes, tabs, coefs)
    ranks = Ranks(1, nv, shapes, tabs, coefs, "host")
    old = _lib.get_policy(KEY)
    try:
        for glog in (15, 1):
            _lib.set_policy(KEY, glog)
            assert SC.cut(1, nv, glog) == (nv, 0)
            ranks.prove(glog, want, wrand, f"one rank at glog = {glog}")
    finally:
        _lib.set_policy(KEY, old)
        ranks.close()


# ---- E: peer to peer ----------------------------------------------------------------------------------------------------------------------------
def test_peer_to_peer_threshold_ladder_ends():
    """A over sharded.P2PComm on one handle: glog = 15 (two sharded rounds, one of them big) and 1 (all sixteen, fourteen of them latency-bound
    rounds whose lanes the small-round kernels write), a group self-test before each proof"""
    run_case("A-15", "p2p", glogs=[15, 1])


@pytest.mark.parametrize("name", ["B-3", "E-16-15", "E-16-1", "E-seven"])
def test_peer_to_peer_cases(name):
    """k = glog on 8 ranks; 16 ranks (kP2PMaxRanks: every slot of the inbox layout in use) at both ends of the policy; a 64-word message (a
    full inbox slot) through six sharded rounds, so each inbox half is used three times"""
    c = SC.CASES[name]
    assert c.G <= SC.K_P2P_MAX_RANKS and SC.case_facts(name)["words"] <= SC.K_P2P_WORDS
    run_case(name, "p2p")


# ---- F: extreme values through the lanes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transport", ["host", "p2p"])
@pytest.mark.parametrize("name", SC.F_NAMES)
def test_extreme_values_through_sixteen_ranks_lanes(name, transport):
    """16 ranks, all four local rounds sharded.  p - 1 at every shard's entry 0 (as an element and as a stored word) and 0 elsewhere: every
    rank's message at node 0 is p - 1, the reduced lanes 16 times its limbs; the same with one rank's shard all zero (15 times); tables
    drawn from {0, 1, p - 1}.  Under [[0]] and under [[0, 0, 0]]."""
    run_case(name, transport)


# ---- G: big rounds, a single-table product, late sharded rounds --------------------------------------------------------------------------------------
def test_big_rounds_then_sharded_small_rounds_and_no_lagging_under_lanes():
    """G = 2, nv = 19, config 3's shape: three big rounds per shard, and table 9 (a product of its own) would lag in an ordinary proof.  Round 1
    with lanes never activates lagging (launch_round: !d_wide), so the lag counters stand still through the sharded proofs at glog = 15
    (nl = 4: one small round sharded) and 12 (nl = 7).  Then, on the same handles: an ordinary whole proof of the shard's own polynomial,
    which DOES lag, against the oracle on the shard's tables; reset; the sharded proof again."""
    c15, c12 = SC.CASES["G-15"], SC.CASES["G-12"]
    assert (c15.G, c15.nv, c15.shapes) == (c12.G, c12.nv, c12.shapes)
    tabs, coefs, want, wrand = case_inputs("G-15")
    nvl = c15.nv - 1
    ranks = Ranks(c15.G, c15.nv, c15.shapes, tabs, coefs, "host")
    old = _lib.get_policy(KEY)
    try:
        for glog in (15, 12, 15):
            _lib.set_policy(KEY, glog)
            moved = ranks.prove(glog, want, wrand, f"G at glog = {glog}")
            assert not any(k in moved for k in LAG), f"a sharded proof let a table lag: {moved}"
        # the shard's own polynomial, as an ordinary proof on the same handle
        local = [cref.ml_prove(H.desc_from(nvl, c15.shapes, ranks.shard(r), coefs), threads=cref.max_threads()) for r in range(c15.G)]
        before = _lib.plan_stats()

        def whole(rank, eng, comm):
            eng.reset()
            rng = sc.Blake2b512Rng.setup()
            rng.feed(sc.PolynomialInfo(eng.D - 1, nvl))
            return eng.prove_rounds(rng, nvl)

        res = ranks.run(whole)
        moved = moved_since(before)
        for r, (msgs, ch) in enumerate(res):
            assert np.array_equal(msgs, local[r][0]) and np.array_equal(ch, local[r][1]), f"rank {r}: the ordinary proof of its shard"
        assert moved.get("big.lag_class_round", 0) > 0, f"the ordinary proof was meant to lag: {moved}"
        assert not any(k in moved for k in SHARDED + ("sharded.gather_tail",)), moved
        _lib.set_policy(KEY, 12)
        moved = ranks.prove(12, want, wrand, "G at glog = 12, behind a lagging proof")
        assert not any(k in moved for k in LAG), moved
    finally:
        _lib.set_policy(KEY, old)
        ranks.close()
    assert_inputs_untouched("G-15")


# ---- H: sharded GKR -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gkr_oracle(dim):
    idx, vals, f2, f3, g = SC.gkr_inputs(dim)
    return (idx, vals, f2, f3, g) + tuple(cref.gkr_prove(idx, vals, dim, f2, f3, g, threads=4))


@pytest.mark.parametrize("transport", ["host", "p2p"])
@pytest.mark.parametrize("name", list(SC.GKR))
def test_sharded_gkr_at_both_ends_of_the_policy(name, transport):
    """sharded_gkr.prove_sharded at G = 4, dim = 9: both phases are sharded proofs over two tables.  glog = 2: m = 0 in both (seven sharded
    rounds each); glog = 15: one.  Messages, u and v equal cref.gkr_prove's; over the host transport each phase all-gathers once."""
    from sumcheck_amd import sharded_gkr
    G, dim, glog = SC.GKR[name]
    f = SC.case_facts(name)
    idx, vals, f2, f3, g, want, wuv = gkr_oracle(dim)
    rec = H.RecordingExchange(G) if transport == "host" else None
    gid = next(_GROUP)
    before = _lib.plan_stats()

    def work(rank):
        _lib.check(sc.lib().sc_set_device(0))
        comm = rec.comm(rank) if rec is not None else sharded.P2PComm(gid, rank, G, DEV)
        if rec is None:
            comm.selftest()
        f1 = sc.SparseMultilinearExtension(3 * dim, np.ascontiguousarray(idx[rank::G]), np.ascontiguousarray(vals[rank::G]))
        res = sharded_gkr.prove_sharded(comm, sc.Blake2b512Rng.setup(), f1, sc.DenseMultilinearExtension(dim, f2), sc.DenseMultilinearExtension(dim, f3), g)
        comm.close()
        return res

    old = _lib.get_policy(KEY)
    try:
        _lib.set_policy(KEY, glog)
        res = H.run_ranks(G, work, on_error=rec.abort if rec is not None else None)
    finally:
        _lib.set_policy(KEY, old)
    moved = moved_since(before)
    for r, (m1, m2, u, v) in enumerate(res):
        assert np.array_equal(m1, want[0]) and np.array_equal(m2, want[1]), f"rank {r}"
        assert np.array_equal(u, wuv[0]) and np.array_equal(v, wuv[1]), f"rank {r}"
    assert_counters(moved, G, transport, name, proofs=2)
    assert moved.get("gkr.sharded", 0) == G
    if rec is not None:
        for r in range(G):  # (the initialisations all-reduce whole tables: 2^dim x 8 words; the rounds, 8 D = 24)
            assert [w for w in rec.allreduce_words[r] if w == f["words"]] == [f["words"]] * (2 * f["nl"]), f"rank {r}: {rec.allreduce_words[r]}"
            assert rec.allgather_bytes[r] == [f["gather_bytes"]] * 2, f"rank {r}: {rec.allgather_bytes[r]}"
