"""Without a GPU: what tests/test_gpu_host_tables.py leans on.

  * every case of tests/host_table_cases.py lies on the side of its threshold the GPU test means it to (streamed from nv = 11, the chunk count
    2^(nv - clamp(request, 10, nv)), merged up to 12 products of at most 4 factors, staged from nv = 18 over host tables, three chunks up to
    nv = 20 and six from 21) -- with the constants as the sources have them;
  * the C oracle (oracle/oracle.c through cref) against the big-integer oracle (oracle/pyoracle.py) on every shape shrunk to nv = 5 or 6,
    message by message and table by table: a table that no product names is bound like any other (also against cref.fix_variables), tables
    of 0, 1 and p - 1 under the challenges p - 1, 0, 1."""
import numpy as np
import pytest

from oracle import cref
from oracle import pyoracle as po
from tests import host_table_cases as HT

I = cref.mont_to_ints


def test_the_constants_are_the_sources():
    assert (HT.K_MAX_ROUND_PRODS, HT.MERGE_MAX_M, HT.K_MAX_FUSED_M, HT.K_MAX_SMALL_TABLES) == (12, 4, 8, 32)
    assert (HT.STREAM_MIN_NV, HT.CHUNK_MIN_LOG2, HT.STAGED_MIN_NV, HT.SIX_CHUNK_NV, HT.K_ROUND_TREE_GRID) == (11, 10, 18, 21, 768)
    assert (HT.LEVELS_BIG, HT.LEVELS_SMALL) == (5, 2) and HT.K_MAX_ROUND_PRODS <= HT.K_META_PRODS
    assert HT.STAGED_GRID_LADDER == [(21, 1024), (20, 768), (18, 384), (17, 256)] and HT.STAGED_GRID_FLOOR == 192


def test_streamed_cases_stream_in_the_chunks_they_claim():
    want_chunks = {"S1-threshold": 2, "S1-below": 1, "S3a-64-chunks": 64, "S3b-fourteen-pairs": 16, "S3c-ten-factors": 8, "S4-unreferenced-merged": 4,
                   "S4-unreferenced-five": 4, "S5-three-arms": 8, "S6-extreme-merged": 4, "S6-extreme-generic": 4, "S7-reset": 4, "S8-thirty-six": 4}
    assert set(want_chunks) == set(HT.STREAMED)
    for name, (nv, chunk, shapes, nt) in HT.STREAMED.items():
        assert HT.is_streamed(nv) == (name != "S1-below"), name
        assert HT.n_chunks(nv, chunk) == 1 << (nv - HT.clamp(chunk, 10, nv)) == want_chunks[name], name
        assert (1 << HT.chunk_log2(nv, chunk)) // 2 >= 512, "the bound half of a chunk keeps whole F29 blocks of 128 entries"
        assert nt == HT.n_named(shapes) and (HT.referenced(shapes) == list(range(nt))) == (name not in HT.UNREFERENCED), name
        if name not in HT.UNREFERENCED:
            assert HT.first_occurrence_order(shapes), name
    assert HT.STREAM_MIN_NV == 11 and not HT.is_streamed(10) and HT.is_streamed(11), "S1 stands on both sides of the threshold"
    # S2: the request is clamped to [10, nv]
    assert [HT.chunk_log2(HT.CLAMP_NV, q) for q in HT.CLAMP_REQUESTS] == [10, 10, 12, 12]
    assert [HT.n_chunks(HT.CLAMP_NV, q) for q in HT.CLAMP_REQUESTS] == [4, 4, 1, 1]
    assert HT.chunk_log2(18, 0) == 18 and HT.chunk_log2(30, 0) == HT.CHUNK_DEFAULT_LOG2 == 22


def test_streamed_cases_take_the_arms_they_claim():
    merged = {name for name, (_, _, shapes, _) in HT.STREAMED.items() if HT.is_merged(shapes)}
    assert merged == {"S1-threshold", "S1-below", "S3a-64-chunks", "S4-unreferenced-merged", "S6-extreme-merged", "S7-reset", "S8-thirty-six"}
    assert len(HT.FOURTEEN_PAIRS) == 14 > HT.K_MAX_ROUND_PRODS and {HT.sub_arm(sh) for sh in HT.FOURTEEN_PAIRS} == {"tree"}
    assert [HT.sub_arm(sh) for sh in HT.TEN_FACTORS] == ["generic", "tree"]
    assert [HT.sub_arm(sh) for sh in HT.STREAMED["S4-unreferenced-five"][2]] == ["node_by_node"]
    arms = [HT.sub_arm(sh) for sh in HT.THREE_ARMS]
    assert len(HT.THREE_ARMS) == 13 == HT.K_MAX_ROUND_PRODS + 1 and arms[:3] == ["tree", "node_by_node", "generic"] and set(arms[3:]) == {"tree"}
    assert [len(sh) for sh in HT.THREE_ARMS[:3]] == [3, 6, 10] and HT.referenced(HT.THREE_ARMS) == [0, 1, 2, 3], "the products share four tables"
    assert len(HT.THIRTY_SIX) == 12 and HT.n_named(HT.THIRTY_SIX) == 36 > HT.K_MAX_SMALL_TABLES and HT.is_merged(HT.THIRTY_SIX)
    assert [0, 0, 1] in HT.STREAMED["S6-extreme-merged"][2]
    for name, u in HT.UNREFERENCED.items():
        nv, shapes, nt = HT.T6 if name.startswith("T6") else (HT.STREAMED[name][0], HT.STREAMED[name][2], HT.STREAMED[name][3])
        assert nt == 4 and HT.referenced(shapes) == [t for t in range(nt) if t != u], name


def test_staged_cases_stage_where_they_claim():
    for nv in HT.LADDER_NV:
        assert HT.is_staged(nv, HT.LADDER_SHAPE) == (nv >= 18), nv
    assert 17 in HT.LADDER_NV and 18 in HT.LADDER_NV, "both sides of the first size that stages"
    assert [HT.staged_chunks(nv) for nv in (18, 19, 20, 21, 22)] == [3, 3, 3, 6, 6] and 20 in HT.LADDER_NV and 21 in HT.LADDER_NV
    for name, (nv, shapes) in HT.K1.items():
        assert len(shapes) == 1 and HT.is_staged(nv, shapes), name
    want = {"K12": True, "K13": False, "M4": True, "M5": False, "policy-off": False, "device": False, "borrowed": False}
    for name, (shapes, mode, pol) in HT.EDGES.items():
        assert HT.is_staged(HT.EDGE_NV, shapes, host=mode == "host", borrow=mode == "borrow", policy=pol) == want[name], name
        assert HT.first_occurrence_order(shapes), name
    assert len(HT.TWELVE_PAIRS) == HT.K_MAX_ROUND_PRODS == len(HT.THIRTEEN_PAIRS) - 1 and HT.n_named(HT.TWELVE_PAIRS) == 4
    assert [len(HT.EDGES[k][0][0]) for k in ("M4", "M5")] == [HT.MERGE_MAX_M, HT.MERGE_MAX_M + 1]
    assert HT.is_staged(HT.T6[0], HT.T6[1]) and HT.is_staged(18, HT.C3) and HT.first_occurrence_order(HT.C3)


def test_staged_sections_cover_the_tables_and_the_grid():
    """the chunks are a half, a quarter, ... and two last ones of equal size; the sections of the grid add up to it"""
    for nv, K in [(18, 3), (18, 1), (19, 1), (20, 3), (21, 3), (22, 1), (22, 4)]:
        sec = HT.staged_sections(nv, K)
        assert len(sec) == HT.staged_chunks(nv)
        assert sec[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(sec, sec[1:])) and sec[-1][0] + sec[-1][1] == 1 << nv
        assert sec[-1][1] == sec[-2][1] == (1 << nv) >> (len(sec) - 1)
    assert [g for _, _, g in HT.staged_sections(22, 1)] == [192, 96, 96, 96, 96, 192], "K = 1: the grid is capped to kRoundTreeGrid"
    assert [g for _, _, g in HT.staged_sections(22, 4)] == [256, 128, 128, 128, 128, 256]
    assert [g for _, _, g in HT.staged_sections(21, 3)] == [192, 96, 96, 96, 96, 192]  # 2^20 pairs: 768 blocks
    assert [g for _, _, g in HT.staged_sections(18, 3)] == [128, 64, 64] and [g for _, _, g in HT.staged_sections(20, 3)] == [192, 96, 96]


# ---- the oracle on the shapes, small ----------------------------------------------------------------------------------------------------------
def _small_shapes():
    out = {name: (shapes, nt, "extreme" if name.startswith("S6") else "synth") for name, (_, _, shapes, nt) in HT.STREAMED.items()}
    out["T1-ladder"] = (HT.LADDER_SHAPE, 3, "synth")
    for name, (_, shapes) in HT.K1.items():
        out["T2-" + name] = (shapes, HT.n_named(shapes), "synth")
    for name, (shapes, _, _) in HT.EDGES.items():
        out["T3-" + name] = (shapes, HT.n_named(shapes), "synth")
    out["T5-config3"] = (HT.C3, 10, "synth")
    out["T6-unreferenced"] = (HT.T6[1], HT.T6[2], "synth")
    return out


SMALL = _small_shapes()


@pytest.mark.parametrize("name", sorted(SMALL))
def test_c_oracle_equals_big_integers_on_every_shape(name):
    shapes, nt, kind = SMALL[name]
    nv = 5 if max(len(sh) for sh in shapes) > 4 or nt > 8 else 6
    tabs = HT.extreme_tables(nv, nt) if kind == "extreme" else HT.synth_tables(nv, nt)
    coefs = HT.synth_coefs(nv, shapes)
    chal = HT.extreme_challenges(nv) if kind == "extreme" else HT.synth_challenges(nv)
    if kind == "extreme":
        seen = {v for t in tabs for v in (sum(int(e[k]) << (64 * k) for k in range(4)) for e in t)}
        assert seen == {0, 1, HT.P - 1} and all(int(x) == HT.P - 1 for x in [sum(int(e[k]) << (64 * k) for k in range(4)) for e in tabs[-1]])
        assert I(chal)[:4] == [HT.P - 1, 0, 1, HT.P - 1]
    st = po.ProverState()  # (built by hand: its ListOfProductsOfPolynomials flattens the tables out of the products)
    st.flattened_ml_extensions = [I(t) for t in tabs]
    st.list_of_products = [(I(coefs[k].reshape(1, 4))[0], list(sh)) for k, sh in enumerate(shapes)]
    st.num_vars, st.max_multiplicands = nv, max(len(sh) for sh in shapes)
    op = cref.Prover(HT.oracle_desc(nv, shapes, tabs, coefs), threads=2)
    ichal = I(chal)
    for j in range(nv):
        want = po.prove_round(st, None if j == 0 else ichal[j - 1])
        got = op.prove_round(None if j == 0 else chal[j - 1])
        assert I(got) == want, f"round {j + 1}"
        _, otabs, rnd = op.state()
        assert rnd == j + 1 and len(otabs) == nt
        for u in range(nt):
            assert I(otabs[u]) == st.flattened_ml_extensions[u], f"table {u} after round {j + 1}"
            if j:  # ... an unreferenced one among them: bound with every challenge so far, like the rest
                assert np.array_equal(otabs[u], cref.fix_variables(tabs[u], chal[:j])), f"table {u} after round {j + 1} against fix_variables"
    op.close()
    if name in HT.UNREFERENCED:
        u = HT.UNREFERENCED[name]
        assert all(u not in sh for sh in shapes) and u < nt
