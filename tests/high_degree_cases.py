"""Product lists of 14 to 40 multiplicands for tests/test_gpu_high_degree.py, and the arithmetic their expected launch plans rest on.

The GPU tests assert which plan counters move; each of those expectations follows from an inequality on the list's shape.  This file builds the
shapes and states the inequalities (the constants mirror sumcheck_amd/csrc: kernels.h, batch_shape.hpp, finalize_device.hpp), so that
tests/test_high_degree_host.py can check without a GPU that every shape lies on the side of its threshold the GPU test means it to."""
import numpy as np

from oracle import cref
from tests import fe_model as fm
from tests import helpers as H

K_MAX_FUSED_M = 8         # batch_shape.hpp: kMaxFusedM -- longer products run node by node in saturated arithmetic in the latency-bound rounds
K_MAX_WIDE_M = 12         # kernels.h: kMaxWideM -- the longest product a tree (big rounds) or the LDS-resident tail takes
K_MAX_SMALL_TABLES = 32   # batch_shape.hpp: kMaxSmallTables -- table pointers that fit a kernel argument
K_META_PRODS = 16         # batch_shape.hpp: kMetaProds
K_META_COMBOS = 24        # kernels.h: kMetaCombos -- (product, node) combinations that fit a kernel argument
K_META_SLOTS = 48         # kernels.h: kMetaSlots
K_FIN_LDS_MAX = 48 * 1024 # finalize_device.hpp: kFinLdsMax
K_SMALL_ROUND_PAIRS = 1 << 14  # kernels.h: kSmallRoundPairs -- a round of more pairs is a big round

LADDER = (14, 19, 20, 23, 24, 31, 32, 33, 37, 38, 40)  # one product of M multiplicands at nv = 11
LADDER_NV = 11
PLAIN_LAUNCHES = (23, 24, 37, 38)                      # ... repeated under pipeline = 0: either side of has_meta and of the finalize's LDS bound


def one_product(M):
    """one product of M factors: distinct tables up to 32 of them, beyond that M factors over 32 tables (table i % 32) -> (shapes, tables)"""
    if M <= K_MAX_SMALL_TABLES:
        return [list(range(M))], M
    return [[i % K_MAX_SMALL_TABLES for i in range(M)]], K_MAX_SMALL_TABLES


BIG_NV = 17  # rounds 1 and 2 are big (2^16 and 2^15 pairs)
BIG_SHAPES = {
    "14-distinct": ([list(range(14))], 14),
    "24-over-16": ([[i % 16 for i in range(24)]], 16),          # tables 0 .. 7 squared, 8 .. 15 once
    "38-over-32": one_product(38),
    "mixed-D21": ([list(range(20)), [0, 1], [2], [3] * 9], 20),  # k_sum_generic beside two trees (M = 2, 1) and a wide16 product (M = 9)
}
EXPONENT_SHAPES = {"0^33": ([[0] * 33], 1), "0^20.1^13": ([[0] * 20 + [1] * 13], 2)}
FORTY_TABLES = ([list(range(40))], 40)


def n_tables(shapes):
    return max(max(sh) for sh in shapes) + 1


def max_mult(shapes):
    return max(len(sh) for sh in shapes)


def degree(shapes):
    """D: evaluations per round message"""
    return max_mult(shapes) + 1


def n_combos(shapes):
    """(product, node) combinations: sum of M_k + 1"""
    return sum(len(sh) + 1 for sh in shapes)


def n_slots(shapes):
    """distinct tables per product, summed"""
    return sum(len(set(sh)) for sh in shapes)


def has_meta(shapes):
    """abi.hip, prover_build: the round metadata travels as a kernel argument"""
    return n_combos(shapes) <= K_META_COMBOS and n_slots(shapes) <= K_META_SLOTS


def fin_lds_bytes(shapes):
    """the finalize's node sums, products and per-product messages: K D (D + 2) elements of 32 bytes"""
    D = degree(shapes)
    return len(shapes) * D * (D + 2) * 32


def tail_shape_ok(shapes):
    """protocol.hip: the persistent kernels (k_tail_rounds, the resident kernel) can take the list's latency-bound rounds"""
    return (n_tables(shapes) <= K_MAX_SMALL_TABLES and has_meta(shapes) and len(shapes) <= K_META_PRODS and fin_lds_bytes(shapes) <= K_FIN_LDS_MAX)


def tail_slices_ok(shapes):
    """... out of LDS (k_tail_slices): never beyond kMaxWideM multiplicands"""
    return tail_shape_ok(shapes) and max_mult(shapes) <= K_MAX_WIDE_M


def finalize_plan(shapes):
    """kernels.hip, launch_finalize, for a handle with its records on the host and the multi-block counter (every handle of these tests)"""
    if fin_lds_bytes(shapes) > K_FIN_LDS_MAX:
        return "finalize.no_lds"
    return "finalize.multi_block" if len(shapes) <= K_META_PRODS else "finalize.one_block"


def small_plan(shapes):
    """protocol.hip, launch_round: a latency-bound round launched after its challenge"""
    if n_tables(shapes) > K_MAX_SMALL_TABLES:
        return "small.ptrs"
    return "small.launched" if has_meta(shapes) else "small.combos_table"


def big_rounds(nv):
    return sum(1 for j in range(1, nv + 1) if (1 << (nv - j)) > K_SMALL_ROUND_PAIRS)


def synth_case(nv, shapes, seed):
    """tables and coefficients from the oracle's generator; the shapes name their tables in first-occurrence order, as add_product flattens them"""
    seen = [t for sh in shapes for t in sh]
    assert sorted(set(seen), key=seen.index) == list(range(n_tables(shapes)))
    tabs = [cref.synth_table(seed, s, 1 << nv) for s in range(n_tables(shapes))]
    coefs = cref.synth_table(seed, 1000, len(shapes))
    return tabs, coefs


EXTREMES = (0, 1, fm.P - 1)


def extreme_tables(nv, n, seed, all_top=False):
    """n tables whose STORED entries are drawn from {0, 1, p - 1} (all_top: every entry p - 1)"""
    vals = np.stack([H.raw_limbs(v) for v in EXTREMES])
    rng = np.random.default_rng(seed)
    pick = [np.full(1 << nv, 2) if all_top else rng.integers(0, 3, size=1 << nv) for _ in range(n)]
    return [np.ascontiguousarray(vals[p]) for p in pick]


def extreme_challenges(n):
    """the challenges 0, 1, p - 1, 0, 1, ... (standard form -> as the API takes them)"""
    return H.mont_challenges([EXTREMES[j % 3] for j in range(n)])
