"""Cases for tests/test_gpu_sharded_edges.py -- where a sharded proof (sc_ml_prove_sharded, sumcheck_amd/csrc/protocol.hip) stops sharding.

A rank runs its first nl rounds sharded, one integer all-reduce of the round message (8 D words) per round; it binds once more and all-gathers
what is left of every shard (2^m entries per table and rank: U 2^m 32 bytes); the last m + log2 G rounds run replicated on a tail prover.
sharded_tail_m and sharded_proof_body decide the cut, with k = log2 G:

    glog = clamp(policy "shard_gather_log2", 1, 15)
    m    = 0                                          if k == 0
    m    = min(k >= glog ? 0 : glog - k, nv_local - 1)  otherwise
    m    = min(m, nv_local - 2)                       for a streamed shard with nv_local >= 2
    nl   = nv_local - m

cut() restates the rule; CASES is the table the GPU tests run; every case states the inequality it rests on (`why`, checked by
tests/test_sharded_cases_host.py over the names of facts()).  The constants are READ from the sources: a changed default, range or
threshold fails the host test; it does not silently move a case to the other side of its edge."""
import collections
import os
import re

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


# abi.hip, kPolicyDefs: {name, default, lowest, highest}
GLOG_DEFAULT, GLOG_MIN, GLOG_MAX = _ints("abi.hip", r'\{"shard_gather_log2", (\d+), (\d+), (\d+)\}')
K_SMALL_ROUND_PAIRS = 1 << _ints("kernels.h", r"constexpr uint64_t kSmallRoundPairs = 1u << (\d+);")[0]  # more pairs than this: a big round
K_P2P_MAX_RANKS, K_P2P_WORDS = _ints("kernels.h", r"constexpr int kP2PMaxRanks = (\d+), kP2PWords = (\d+);")
# protocol.hip: the clamp sharded_tail_m applies to the policy, and the streamed shard's two local rounds
TAIL_CLAMP_LO, TAIL_CLAMP_HI = _ints("protocol.hip", r"std::max<int64_t>\(scd::policy\(scd::kPolShardGatherLog2\), (\d+)\), (\d+)\);")
STREAMED_LOCAL_ROUNDS = _ints("protocol.hip", r"if \(p->streamed && p->nv >= 2\) m = std::min\(m, p->nv - (\d+)\);")[0]
STREAM_MIN_NV = _ints("abi.hip", r"\(d->flags & SC_TABLES_STREAM\) && p->nv >= (\d+);")[0]  # smaller tables are silently copied

P = fm.P
SEED = 0x5AED


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------
def log2(G):
    assert G > 0 and G & (G - 1) == 0, "the number of ranks is a power of two"
    return G.bit_length() - 1


def cut(G, nv_local, glog, streamed=False):
    """-> (nl, m): the sharded rounds, and log2 of the entries per table a rank still holds at the gather"""
    k = log2(G)
    glog = max(TAIL_CLAMP_LO, min(glog, TAIL_CLAMP_HI))
    if k == 0:
        m = 0
    else:
        m = min(0 if k >= glog else glog - k, nv_local - 1)
    if streamed and nv_local >= 2:
        m = min(m, nv_local - STREAMED_LOCAL_ROUNDS)
    return nv_local - m, m


# ---- the shapes -----------------------------------------------------------------------------------------------------------------------------
LADDER = [[0, 1, 2], [3, 3], [1]]                          # A: a shared table, a repeated factor, a single-table product; 4 tables
PAIR = [[0, 1], [1]]                                       # B
SMALL = [[0, 1, 2], [1]]                                   # C
TRIPLE = [[0, 1, 2]]                                       # D
SEVEN = [[0, 1, 2, 3, 4, 5, 6]]                            # E: D = 8, a message of 64 words
ONE = [[0]]                                                # F
CUBE = [[0, 0, 0]]                                         # F
C3 = [[0, 1, 2, 3], [4, 5, 6], [7, 8], [9]]                # G: config 3's shape; table 9 lags in an ordinary proof

Case = collections.namedtuple("Case", "name G nv shapes glog chunk tables why")


def _c(name, G, nv, shapes, glog, why, chunk=None, tables="synth"):
    return Case(name, G, nv, shapes, glog, chunk, tables, why)


# `why` is an expression over facts(case).  Host-transport cases, by name; the peer-to-peer cases (P2P) run the same (G, nv, shape, glog).
_CASES = [
    # A: the threshold ladder on one handle (nv_local = 16: round 1 has 2^15 pairs, a big round), in the order the test runs it
    _c("A-15", 2, 17, LADDER, 15, "(m, nl) == (14, 2) and m == glog - k < nv_local - 1 and big_rounds == 1"),
    _c("A-1", 2, 17, LADDER, 1, "(m, nl) == (0, 16) and k >= glog and big_rounds == 1"),
    _c("A-10", 2, 17, LADDER, 10, "(m, nl) == (9, 7) and m == glog - k"),
    _c("A-14", 2, 17, LADDER, 14, "(m, nl) == (13, 3) and m == glog - k"),
    _c("A-2", 2, 17, LADDER, 2, "(m, nl) == (1, 15) and m == glog - k == 1"),
    # B: k >= glog and the step above it
    _c("B-2", 8, 9, PAIR, 2, "m == 0 and k > glog"),
    _c("B-3", 8, 9, PAIR, 3, "m == 0 and k == glog"),
    _c("B-4", 8, 9, PAIR, 4, "m == 1 and k == glog - 1"),
    # C: the smallest shards.  nv_local = 1: the nv_local - 1 clamp alone gives m = 0, whatever the policy
    _c("C-2x1", 2, 2, SMALL, GLOG_DEFAULT, "nv_local == 1 and m == 0 == nv_local - 1 < glog - k and nl == 1"),
    _c("C-8x1", 8, 4, SMALL, GLOG_DEFAULT, "nv_local == 1 and m == 0 == nv_local - 1 < glog - k and nl == 1"),
    _c("C-16x1", 16, 5, SMALL, GLOG_DEFAULT, "nv_local == 1 and m == 0 == nv_local - 1 < glog - k and nl == 1 and G == kP2PMaxRanks"),
    _c("C-4x2-15", 4, 4, SMALL, GLOG_DEFAULT, "nv_local == 2 and m == 1 == nv_local - 1 < glog - k and nl == 1"),
    _c("C-4x2-1", 4, 4, SMALL, 1, "nv_local == 2 and m == 0 and k >= glog and nl == 2"),
    # D: streamed shards (nv_local = 11 is the smallest table that streams)
    _c("D-15", 2, 12, TRIPLE, GLOG_DEFAULT, "nv_local == stream_min_nv and (m, nl) == (9, 2) and m == nv_local - 2 < nv_local - 1 < glog - k", chunk=11),
    _c("D-3", 2, 12, TRIPLE, 3, "nv_local == stream_min_nv and (m, nl) == (2, 9) and m == glog - k < nv_local - 2", chunk=11),
    # E: the twins of the peer-to-peer cases that are not in A or B
    _c("E-16-15", 16, 8, SMALL, GLOG_DEFAULT, "G == kP2PMaxRanks and (m, nl) == (3, 1) and m == nv_local - 1 < glog - k"),
    _c("E-16-1", 16, 8, SMALL, 1, "G == kP2PMaxRanks and (m, nl) == (0, 4) and k >= glog"),
    _c("E-seven", 4, 8, SEVEN, 1, "words == kP2PWords and D == 8 and (m, nl) == (0, 6) and k >= glog"),
    # F: extreme values through the lanes (G = 16: every lane is the sum of 16 limbs), all four local rounds sharded
    _c("F-one-spike", 16, 8, ONE, 1, "G == kP2PMaxRanks and (m, nl) == (0, 4) and U == 1", tables="spike"),
    _c("F-cube-spike", 16, 8, CUBE, 1, "G == kP2PMaxRanks and (m, nl) == (0, 4) and U == 1 and D == 4", tables="spike"),
    _c("F-one-raw-spike", 16, 8, ONE, 1, "G == kP2PMaxRanks and (m, nl) == (0, 4) and U == 1", tables="raw-spike"),
    _c("F-cube-raw-spike", 16, 8, CUBE, 1, "G == kP2PMaxRanks and (m, nl) == (0, 4) and U == 1", tables="raw-spike"),
    _c("F-one-spike-hole", 16, 8, ONE, 1, "G == kP2PMaxRanks and (m, nl) == (0, 4)", tables="spike-hole"),
    _c("F-cube-spike-hole", 16, 8, CUBE, 1, "G == kP2PMaxRanks and (m, nl) == (0, 4)", tables="spike-hole"),
    _c("F-one-drawn", 16, 8, ONE, 1, "G == kP2PMaxRanks and (m, nl) == (0, 4)", tables="drawn"),
    _c("F-cube-drawn", 16, 8, CUBE, 1, "G == kP2PMaxRanks and (m, nl) == (0, 4)", tables="drawn"),
    # G: three big rounds, a single-table product whose table would lag, sharded rounds behind the big ones
    _c("G-15", 2, 19, C3, GLOG_DEFAULT, "nv_local == 18 and big_rounds == 3 and (m, nl) == (14, 4) and nl > big_rounds"),
    _c("G-12", 2, 19, C3, 12, "nv_local == 18 and big_rounds == 3 and (m, nl) == (11, 7) and m == glog - k"),
]
CASES = {c.name: c for c in _CASES}
assert len(CASES) == len(_CASES)

LADDER_ORDER = ("A-15", "A-1", "A-10", "A-14", "A-2", "A-15")   # every step changes m; the last returns to a size used before
F_NAMES = tuple(n for n in CASES if n.startswith("F-"))
HOLE_RANK = 5                                                   # F: the rank whose shard is all zero
# the peer-to-peer cases: each runs its host-transport twin's (G, nv, shape, tables, glog), which pins (nl, m) by counting the exchanges
P2P = ("A-15", "A-1", "B-3", "E-16-15", "E-16-1", "E-seven") + F_NAMES

# H: sharded GKR (sharded_gkr.prove_sharded): (G, dim, glog); each phase is a sharded proof over two tables of dim variables
GKR = {"H-2": (4, 9, 2), "H-15": (4, 9, GLOG_DEFAULT)}
GKR_WHY = {"H-2": "(m, nl) == (0, 7) and k >= glog", "H-15": "(m, nl) == (6, 1) and m == nv_local - 1 < glog - k"}
GKR_TABLES, GKR_D = 2, 3

# the whole-proof tests of tests/test_gpu_sharded.py, all at the default policy: (G, nv) -> (nl, m)
EXISTING = {(2, 13): (1, 11), (4, 19): (4, 13), (2, 20): (5, 14), (8, 6): (1, 2), (8, 12): (1, 8)}


def n_tables(shapes):
    return max(max(sh) for sh in shapes) + 1


def big_rounds(nv_local):
    """the local rounds with more than kSmallRoundPairs pairs (round j of a shard has 2^(nv_local - j) pairs)"""
    return sum(1 for j in range(1, nv_local + 1) if (1 << (nv_local - j)) > K_SMALL_ROUND_PAIRS)


def facts(G, nv, shapes_or_none, glog, streamed=False, U=None, D=None):
    """everything a case's expectations are: the names its `why` may use"""
    k = log2(G)
    nv_local = nv - k
    nl, m = cut(G, nv_local, glog, streamed)
    U = n_tables(shapes_or_none) if U is None else U
    D = max(len(sh) for sh in shapes_or_none) + 1 if D is None else D
    return dict(G=G, k=k, nv=nv, nv_local=nv_local, glog=glog, nl=nl, m=m, tail=m + k, U=U, D=D, words=8 * D, gather_bytes=U * (1 << m) * 32,
                big_rounds=big_rounds(nv_local), kP2PWords=K_P2P_WORDS, kP2PMaxRanks=K_P2P_MAX_RANKS, stream_min_nv=STREAM_MIN_NV)


def case_facts(name):
    if name in GKR:
        G, dim, glog = GKR[name]
        return facts(G, dim, None, glog, U=GKR_TABLES, D=GKR_D)
    c = CASES[name]
    return facts(c.G, c.nv, c.shapes, c.glog, streamed=c.chunk is not None)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def _one():
    return cref.ints_to_mont([1])[0]


def spike_table(G, nv, value_limbs, hole=None):
    """value at every shard's entry 0 (none in shard `hole`), 0 elsewhere"""
    n_loc = (1 << nv) // G
    t = np.zeros((1 << nv, 4), dtype=np.uint64)
    for g in range(G):
        if g != hole:
            t[g * n_loc] = value_limbs
    return t


def drawn_table(nv, seed=SEED):
    """STORED entries drawn from {0, 1, p - 1}"""
    vals = np.stack([H.raw_limbs(v) for v in (0, 1, P - 1)])
    return np.ascontiguousarray(vals[np.random.default_rng(seed + nv).integers(0, 3, size=1 << nv)])


def inputs(name):
    """-> (tables, coefficients) of a case.  F's spikes: the ELEMENT p - 1 ("spike": x^3 = x, so both shapes' messages at node 0 are p - 1
    per rank) or the STORED word p - 1 ("raw-spike": under [[0]] every rank's lanes at node 0 are the limbs of p - 1, the largest a lane
    gets); their coefficient is one, so that the message is the table's entry itself."""
    c = CASES[name]
    nt = n_tables(c.shapes)
    if c.tables == "synth":
        seed = SEED + c.nv * 64 + c.G
        return [cref.synth_table(seed, s, 1 << c.nv) for s in range(nt)], cref.synth_table(seed, 1000, len(c.shapes))
    assert nt == 1 and len(c.shapes) == 1
    coefs = _one().reshape(1, 4)
    if c.tables == "drawn":
        return [drawn_table(c.nv)], coefs
    value = H.raw_limbs(P - 1) if c.tables.startswith("raw") else cref.ints_to_mont([P - 1])[0]
    return [spike_table(c.G, c.nv, value, HOLE_RANK if c.tables.endswith("hole") else None)], coefs


def oracle_proof(nv, shapes, tabs, coefs):
    """cref.ml_prove on the unsharded tables -> (proof, randomness)"""
    return cref.ml_prove(H.desc_from(nv, shapes, tabs, coefs), threads=cref.max_threads())


def gkr_inputs(dim, seed=SEED):
    """-> (f1's distinct indices, its values, f2, f3, g)"""
    rng = np.random.default_rng(seed + dim)
    n = 1 << dim
    d = np.uint64(dim)
    idx = np.unique(rng.integers(0, n, size=3 * n, dtype=np.uint64) | (rng.integers(0, n, size=3 * n, dtype=np.uint64) << d)
                    | (rng.integers(0, 4, size=3 * n, dtype=np.uint64) << (d + d)))[: 2 * n]
    return idx, cref.synth_table(seed + dim, 1, idx.shape[0]), cref.synth_table(seed + dim, 6, n), cref.synth_table(seed + dim, 3, n), cref.synth_table(seed + dim, 4, dim)
