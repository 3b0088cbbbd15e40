"""The packed internal table format on the GPU (fe_device.hpp / f29_pack.hpp): bound tables of the big rounds in 32 bytes an entry.
The smallest shapes that reach every new path: round 2 packs from canonical tables, round 3 reads packed and writes packed, the resident
tail makes its first load from packed tables, the five-multiplicand tree binds into the format, a state export converts it back -- each
against the oracle, bit for bit -- and a round-trip / range-rule self-test of the device code against the Python model
(tests/f29_pack_model.py) on the format's corners."""
import random

import numpy as np
import pytest
import torch

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib
from tests import f29_pack_model as pk
from tests import fe_model as fm
from tests import helpers as H
from tests.test_gpu_lazy_entries import interactive, poly_of, selector, sinking

pytestmark = pytest.mark.gpu
P = fm.P
VM = sc.VerifierMsg
C3 = [[0, 1, 2, 3], [4, 5, 6], [7, 8], [9]]
OP_F29_ROUND_TRIP, OP_F29_SETTLE = 19, 20  # kernels_selftest.hip: FeOp


def moved_plans(before):
    after = _lib.plan_stats()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def fiat_shamir_against_the_oracle(nv, shapes, seed):
    nt = max(max(sh) for sh in shapes) + 1
    tabs = [cref.synth_table(seed, t, 1 << nv) for t in range(nt)]
    coefs = cref.synth_table(seed, 1000, len(shapes))
    want, _ = cref.ml_prove(H.desc_from(nv, shapes, tabs, coefs), threads=cref.max_threads())
    poly = poly_of(nv, shapes, tabs, coefs)
    before = _lib.plan_stats()
    proof = sc.MLSumcheck.prove(poly)
    moved = moved_plans(before)
    got = np.stack([m.evaluations for m in proof])
    bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
    assert bad.size == 0, f"rounds {(bad + 1).tolist()} differ from the oracle's"
    return moved


def test_config3_shape_nv18_packs_in_round_2_streams_in_round_3_and_hands_over_to_the_tail():
    moved = fiat_shamir_against_the_oracle(18, C3, 0xF29018)
    print(moved)
    assert moved.get("big.store_f29", 0) == 2, "rounds 2 and 3 must store their bound tables in the internal format"
    assert moved.get("big.claim_identity", 0) > 0
    # (sc_ml_prove counts its k_tail_slices launch as tail.slices8; resident.slices is the same kernel under sc_prove_round and is asserted
    # by the interactive test below)
    assert moved.get("tail.slices8", 0) == 1 and moved.get("tail.rounds", 0) == 0, "the tail must start from the packed tables in one k_tail_slices launch"


# ---- both branches of the range rule in the big rounds, one entry at the decision point in each ------------------------------------------------
def near_decision_table(nv, s, m, binds):
    """a sinking table whose entries sit AT the range rule's decision point in bind number `binds` (1: round 2, canonical -> packed; 2: round 3,
    packed -> packed).  A bind's term is m 2^232 - p (limb 8: m - PH - 1) and the rule reads limb 8 of the un-normalised sum: with
    c = K 2^232 + eps, K = PH + 1 - RULE_TOP - binds m and 0 < eps < m s_(binds + 1), the pair at index 0 reads exactly -RULE_TOP (kept) and the
    pair whose entries carry -m s_(binds + 1) reads one less (p is added); both values are 0.34 * 2^232 above -p / 2."""
    K = fm.PH + 1 - pk.RULE_TOP - binds * m
    c = (K << 232) + (m * s[binds]) // 2
    return H.sinking_table_limbs(nv, s, m, c), c


def model_entries_after(c, m, s, r, binds):
    """the model's first four entries of the table after `binds` binds -> per bind: [(value before the rule, added)]"""
    n = 1 << (binds + 2)
    cur = [fm.limbs_of(c - m * sum(sj for j, sj in enumerate(s) if (x >> j) & 1)) for x in range(n)]
    log = []
    for k in range(binds):
        nxt, row = [], []
        for b in range(len(cur) // 2):
            raw = fm.fe_add(cur[2 * b], fm.fe_mul_bind(fm.fe_sub(cur[2 * b + 1], cur[2 * b]), r[k]))
            new, added = pk.settle(raw)
            assert pk.packable(new)
            row.append((fm.value(raw), added))
            nxt.append(new)
        cur = nxt
        log.append(row)
    return log


def test_interactive_nv18_range_rule_both_branches_and_the_extreme_tables():
    nv = 18
    s, r = fm.sinking_challenges(nv, 76000)
    m_a, m_b = 2, 3
    tab_a, c_a = near_decision_table(nv, s, m_a, 1)
    tab_b, c_b = near_decision_table(nv, s, m_b, 2)
    # the CPU model: in round 2's bind table A has neighbouring pairs on either side of the decision point, within 2^232 of it; table B likewise in round 3's
    for c, m, binds in ((c_a, m_a, 1), (c_b, m_b, 2)):
        row = model_entries_after(c, m, s, r, binds)[binds - 1]
        assert {added for _, added in row} == {False, True}, "both branches of the range rule"
        assert min(abs(v + P // 2) for v, _ in row) < (1 << 232), "an entry within 2^232 of -p / 2"
    n = 1 << nv
    zeros = np.zeros((n, 4), dtype=np.uint64)
    pm1 = np.ascontiguousarray(np.broadcast_to(H.raw_limbs(P - 1), (n, 4)))
    alt = np.ascontiguousarray(np.where((np.arange(n) % 2 == 0)[:, None], zeros[:1], pm1[:1]))
    alt_rev = np.ascontiguousarray(np.where((np.arange(n) % 2 == 1)[:, None], zeros[:1], pm1[:1]))
    tabs = [tab_a, selector(nv, s, 1, 1, False), selector(nv, s, 2, 2, True), tab_b, zeros, pm1, alt, sinking(nv, s, 7), alt_rev, selector(nv, s, 2, 5, False)]
    moved = interactive(nv, C3, tabs, H.mont_challenges(r), lazy_big_binds=2)
    assert moved.get("big.claim_identity", 0) > 0


def test_five_multiplicands_nv17_bind_into_the_packed_format_in_the_wide_tree():
    moved = fiat_shamir_against_the_oracle(17, [[0, 1, 2, 3, 4]], 0xF29017)
    print(moved)
    assert moved.get("big.wide", 0) > 0, "the big rounds must run in the tree kernel for five to eight multiplicands"
    assert moved.get("big.store_f29", 0) >= 1, "and store their bound tables in the internal format"


def test_state_export_after_round_2_converts_packed_tables_to_canonical():
    nv = 18
    tabs = [cref.synth_table(0xF29E, t, 1 << nv) for t in range(10)]
    coefs = cref.synth_table(0xF29E, 1000, len(C3))
    chal = cref.synth_table(0xF29E, 2000, 2)
    chal[:, 3] &= np.uint64(0x0FFFFFFFFFFFFFFF)  # canonical: below p
    op = cref.Prover(H.desc_from(nv, C3, tabs, coefs), threads=cref.max_threads())
    want = [op.prove_round(None), op.prove_round(chal[0])]
    _, otabs, rnd = op.state()
    op.close()
    poly = poly_of(nv, C3, tabs, coefs)
    before = _lib.plan_stats()
    st = sc.IPForMLSumcheck.prover_init(poly)
    got = [sc.IPForMLSumcheck.prove_round(st, None).evaluations, sc.IPForMLSumcheck.prove_round(st, VM(chal[0])).evaluations]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert moved_plans(before).get("big.store_f29", 0) == 1, "round 2 must have left packed tables"
    exported = st.flattened_ml_extensions
    assert st.round == rnd == 2 and len(exported) == len(otabs)
    for u, t in enumerate(exported):
        assert np.array_equal(t.evaluations, otabs[u]), f"bound table {u} after round 2"
    # the export leaves the handle as it was: round 3 reads the packed tables
    op2 = cref.Prover(H.desc_from(nv, C3, tabs, coefs), threads=cref.max_threads())
    for rr in (None, chal[0]):
        op2.prove_round(rr)
    assert np.array_equal(sc.IPForMLSumcheck.prove_round(st, VM(chal[1])).evaluations, op2.prove_round(chal[1]))
    op2.close()
    st.close()


# ---- the device code against the model -----------------------------------------------------------------------------------------------------------
def test_round_trip_self_test_on_the_corners():
    """one block of entries (128, the layout's granule): stored with fe_store_f29 by lane i, loaded back with fe_load_f29 by a second launch"""
    rng = random.Random(fm.SEED + 50)
    rows = pk.corner_limbs()
    rows += [[rng.randint(0, fm.MASK) for _ in range(8)] + [rng.randint(pk.TOP_LO, pk.TOP_HI)] for _ in range(128 - len(rows))]
    assert len(rows) == 128 and all(pk.packable(l) for l in rows)
    scratch = torch.zeros((128, 8), dtype=torch.int32, device=H.FE_DEV)
    got = H.fe_run_op(OP_F29_ROUND_TRIP, 128, H.fe_dev_limbs(rows), b=scratch)
    for i, l in enumerate(rows):
        assert pk.unpack(pk.pack(l)) == l
        assert got[i].tolist() == l, f"entry {i}: {l}"
    # the table itself: entry e's chunk `half` at uint4 index (2 (e & 1) + half) * 64 + col(e >> 1), holding the model's words
    table = scratch.cpu().numpy().view(np.uint32).reshape(256, 4)
    for e, l in enumerate(rows):
        q = e >> 1
        col = ((q & 63) >> 1) | ((q & 1) << 5)
        w = pk.pack(l)
        for half in (0, 1):
            assert table[(2 * (e & 1) + half) * 64 + col].tolist() == w[4 * half:4 * half + 4], f"entry {e}, half {half}"


def test_range_rule_on_the_device_matches_the_model():
    rng = random.Random(fm.SEED + 51)
    rows = []
    for top in (-pk.RULE_TOP - 2, -pk.RULE_TOP - 1, -pk.RULE_TOP, -pk.RULE_TOP + 1, 0, fm.PH, -fm.PH - 1, -2 * fm.PH - 2):
        rows += [[low] * 8 + [top] for low in (0, fm.MASK, 2 * fm.MASK)]
        rows += [[rng.randint(0, 2 * fm.MASK) for _ in range(8)] + [top] for _ in range(60)]
    rows += [[rng.randint(0, 2 * fm.MASK) for _ in range(8)] + [rng.randint(-(1 << 24), 1 << 24)] for _ in range(1000)]
    got = H.fe_run_op(OP_F29_SETTLE, len(rows), H.fe_dev_limbs(rows))
    for i, l in enumerate(rows):
        want, _ = pk.settle(l)
        assert got[i].tolist() == want, f"row {i}: {l}"
