"""GPU tests of sc_gkr_layers_eval_batch (GKRRoundSumcheck.evaluate_layers_batch): the values of a circuit's layers, computed on the device.
Every output is compared element for element with the big-integer definition of tests/gkr_layers_eval_cases.py; every test also ties an
output to the oracle through the claim identity -- the first message of cref.gkr_prove over the layer's inputs at a random g sums to
cref.fix_variables(output, g), the multilinear extension of the evaluated layer -- and asserts which of the two plan counters moved."""
import ctypes as C

import numpy as np
import pytest
import torch

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib
from tests import gkr_layers_eval_cases as K
from tests import test_gpu_gkr_batch_rounds as R
from tests import test_gpu_gkr_next_layer as NL

pytestmark = pytest.mark.gpu
P = cref.P
FULL = K.MAX_NNZ_PER_CELL << K.MAX_DIM  # 64 x 2^9: the longest list of the one-block plan
PATTERN = 0x5A5A5A5A5A5A5A5A


def counters():
    p = _lib.plan_stats()
    return p[K.ONE_BLOCK], p[K.CELLS]


def moved(before, one_block=0, cells=0):
    assert counters() == (before[0] + one_block, before[1] + cells), "one_block / cells"


def evaluate(insts, dim, device="cuda:0", **pol):
    """insts: per instance (layers [(idx, vals)], f2, f3) as host arrays; arrays that are the same object go in as the same object.
    -> out[k][i] as host arrays.  The inputs are compared with copies afterwards: a call changes nothing of the caller's"""
    put = NL.td if device is not None else (lambda a: a)
    seen = {}

    def once(a):
        if id(a) not in seen:
            seen[id(a)] = (put(a), a.copy())
        return seen[id(a)][0]

    n_layers = len(insts[0][0])
    f1 = [[sc.SparseMultilinearExtension(3 * dim, once(inst[0][k][0]), once(inst[0][k][1])) for inst in insts] for k in range(n_layers)]
    f2s = [sc.DenseMultilinearExtension(dim, once(inst[1])) for inst in insts]
    f3s = [sc.DenseMultilinearExtension(dim, once(inst[2])) for inst in insts]
    if device is not None:
        torch.cuda.synchronize()
    with _lib.policy(**pol):
        out = sc.GKRRoundSumcheck.evaluate_layers_batch(f1, f2s, f3s)
    for now, then in seen.values():
        host = now.cpu().numpy().view(np.uint64).reshape(then.shape) if device is not None else now
        assert np.array_equal(host, then), "an input changed"
    assert all(m.on_device == (device is not None) and m.num_vars == dim for layer in out for m in layer)
    return [[(m.evaluations.cpu().numpy().view(np.uint64) if device is not None else m.evaluations).reshape(-1, 4) for m in layer] for layer in out], out


def check(insts, dim, got):
    for i, inst in enumerate(insts):
        want = K.define_layers(inst[0], inst[1], inst[2], dim)
        for k, w in enumerate(want):
            bad = np.nonzero((got[k][i] != w).any(axis=1))[0]
            assert np.array_equal(got[k][i], w), f"layer {k} instance {i}: {bad.shape[0]} cells differ from the definition, first {bad[:3]}"


def claim(idx, vals, dim, a, b, out, seed):
    """the claim a layer's sumcheck starts from, both sides in the oracle's arithmetic: P(0) + P(1) of cref.gkr_prove's first message
    against the multilinear extension of the device's output at g"""
    g = cref.synth_table(seed, 4, dim)
    proof, _ = cref.gkr_prove(idx, vals, dim, a, b, g)
    assert np.array_equal(cref.fr_binop("add", proof[0, 0, 0], proof[0, 0, 1]), cref.fix_variables(out, g)[0]), "P(0) + P(1) is not the layer's extension at g"


# ---- 1. one block per instance -------------------------------------------------------------------------------------------------------
def _one_block_insts(dim, n):
    N = 1 << dim
    if n == 1:
        return [([K.wiring(dim, 61000 + dim, 3 * N, "repeated")], cref.synth_table(61100 + dim, 2, N), cref.synth_table(61100 + dim, 3, N))]
    shared = K.wiring(dim, 61200 + dim, 3 * N, "repeated")  # one wiring for instances 0 and 1; then none at all, one, zeros kept in the list
    lists = [shared, shared, K.wiring(dim, 0, 0), K.wiring(dim, 61300 + dim, 1), K.wiring(dim, 61400 + dim, N + 1, "zeros")]
    return [([lists[i]], cref.synth_table(61500 + 10 * dim + i, 2, N), cref.synth_table(61500 + 10 * dim + i, 3, N)) for i in range(n)]


@pytest.mark.parametrize("device", ["cuda:0", None], ids=["device", "host"])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("dim", [1, 2, 5, 9])
def test_one_block_equals_the_definition(dim, n, device):
    """dim 1: two cells; 2; 5: fewer cells than lanes; 9: the LDS full, two strides of cells per lane.  Lists of 0, 1 and 3 x 2^dim
    non-zeros with repeated indices, zero values kept in the list, one wiring shared by two instances"""
    insts = _one_block_insts(dim, n)
    before = counters()
    got, _ = evaluate(insts, dim, device, batch=2)
    moved(before, one_block=1)
    check(insts, dim, got)
    assert n == 1 or (not got[0][2].any() and got[0][1].any()), "an empty list gives zero"
    claim(*insts[0][0][0], dim, insts[0][1], insts[0][2], got[0][0], 61900 + dim)


def test_one_block_at_the_ends_of_its_envelope():
    """dim 9: exactly 64 x 2^9 non-zeros; and all 64 x 2^9 terms of an instance in ONE cell with v = f2 = f3 = p - 1, the fullest lanes the
    plan admits: the cell is -(64 x 2^9) mod p"""
    dim = K.MAX_DIM
    N = 1 << dim
    idx, vals, table = K.one_cell(dim, FULL, 345, 62000)
    insts = [([K.wiring(dim, 62001, FULL, "random")], cref.synth_table(62002, 2, N), cref.synth_table(62002, 3, N)), ([(idx, vals)], table, table)]
    before = counters()
    got, _ = evaluate(insts, dim, batch=2)
    moved(before, one_block=1)
    check(insts, dim, got)
    assert cref.mont_to_ints(got[0][1][345:346]) == [P - FULL] and not np.delete(got[0][1], 345, axis=0).any()
    claim(idx, vals, dim, table, table, got[0][1], 62003)


def test_tables_and_values_from_the_ends_of_the_field():
    dim, n = 5, 3
    insts = [([K.wiring(dim, 63000 + i, 3 << dim, "edge")], K.edge_table(dim, 63100 + i), K.edge_table(dim, 63200 + i)) for i in range(n)]
    before = counters()
    got, _ = evaluate(insts, dim, batch=2)
    moved(before, one_block=1)
    check(insts, dim, got)
    assert all(g[0].any() for g in zip(*got)), "something to compare"
    claim(*insts[1][0][0], dim, insts[1][1], insts[1][2], got[0][1], 63300)


# ---- 2. the plan boundary ------------------------------------------------------------------------------------------------------------
def test_one_non_zero_beyond_the_one_block_plan_runs_as_cells_with_the_same_bits():
    dim = K.MAX_DIM
    N = 1 << dim
    idx, vals = K.wiring(dim, 64000, FULL + 1, "random")
    f2, f3 = cref.synth_table(64001, 2, N), cref.synth_table(64001, 3, N)
    before = counters()
    head, _ = evaluate([([(np.ascontiguousarray(idx[:FULL]), np.ascontiguousarray(vals[:FULL]))], f2, f3)], dim, batch=2)
    moved(before, one_block=1)
    full, _ = evaluate([([(idx, vals)], f2, f3)], dim, batch=2)
    moved(before, one_block=1, cells=1)
    check([([(idx, vals)], f2, f3)], dim, full)
    extra = K.define_layer(idx[FULL:], cref.mont_to_ints(vals[FULL:]), dim, cref.mont_to_ints(f2), cref.mont_to_ints(f3))
    z = int(idx[FULL]) & (N - 1)
    assert extra[z] != 0
    want = head[0][0].copy()
    want[z] = cref.fr_binop("add", want[z], cref.ints_to_mont([extra[z]])[0])
    assert np.array_equal(full[0][0], want), "the one-block plan's bits over the first 64 x 2^9 terms, plus the extra one"
    claim(idx, vals, dim, f2, f3, full[0][0], 64002)


@pytest.mark.parametrize("dim,pol", [(K.MAX_DIM + 1, 2), (5, 0)], ids=["dim10-small", "dim5-batch0"])
def test_beyond_the_dim_or_under_policy_batch_0_the_cells_plan_runs(dim, pol):
    N = 1 << dim
    insts = [([K.wiring(dim, 65000 + dim + i, 40 + i, "random")], cref.synth_table(65100 + i, 2, N), cref.synth_table(65100 + i, 3, N)) for i in range(2)]
    before = counters()
    got, _ = evaluate(insts, dim, batch=pol)
    moved(before, cells=1)
    check(insts, dim, got)
    if pol == 0:
        again, _ = evaluate(insts, dim, batch=2)
        moved(before, one_block=1, cells=1)
        assert all(np.array_equal(a, b) for a, b in zip(got[0], again[0])), "both plans give the same bits"
    claim(*insts[0][0][0], dim, insts[0][1], insts[0][2], got[0][0], 65200 + dim)


# ---- 3. cells ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,device", [(10, "cuda:0"), (11, "cuda:0"), (11, None), (16, "cuda:0")], ids=["dim10-device", "dim11-device", "dim11-host", "dim16-device"])
def test_cells_equal_the_definition(dim, device):
    """n = 2, nnz = 2 x 2^dim; dim 10: the first dim beyond one block; 11: also from host arrays (the staging path); 16: 2^16 cells an instance"""
    N = 1 << dim
    insts = [([K.wiring(dim, 66000 + dim + i, 2 * N, "repeated" if i else "random")], cref.synth_table(66100 + dim + i, 2, N), cref.synth_table(66100 + dim + i, 3, N)) for i in range(2)]
    before = counters()
    got, _ = evaluate(insts, dim, device, batch=2)
    moved(before, cells=1)
    check(insts, dim, got)
    claim(*insts[1][0][0], dim, insts[1][1], insts[1][2], got[0][1], 66200 + dim)


def test_cells_at_dim_21_over_tables_made_on_the_device():
    """the largest dim: a few hundred non-zeros, among them index 0 and index 2^63 - 1 (every component 2^21 - 1); the expected table is the
    definition over the list's terms and zero in every other cell"""
    dim, nnz, seed = 21, 300, 67000
    N = 1 << dim
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, 1 << 63, size=nnz, dtype=np.uint64)
    idx[0], idx[1], idx[2], idx[3] = 0, (1 << 63) - 1, idx[10], idx[10]  # the ends of the range; an index three times
    vals = cref.synth_table(seed, 1, nnz)
    tabs = [torch.empty((N, 4), dtype=torch.int64, device="cuda:0") for _ in range(2)]
    for s, t in enumerate(tabs):
        _lib.check(sc.lib().sc_synth_table_device(seed, 2 + s, 0, N, C.c_void_p(t.data_ptr())))
    entry = lambda stream: (lambda e: cref.mont_to_ints(cref.synth_table(seed, stream, 1, first=e))[0])
    want = K.sparse_terms(idx, cref.mont_to_ints(vals), dim, entry(2), entry(3))
    f1 = sc.SparseMultilinearExtension(3 * dim, NL.td(idx), NL.td(vals))
    torch.cuda.synchronize()
    before = counters()
    out = sc.GKRRoundSumcheck.evaluate_layers_batch([[f1]], [sc.DenseMultilinearExtension(dim, tabs[0])], [sc.DenseMultilinearExtension(dim, tabs[1])])[0][0].evaluations
    moved(before, cells=1)
    cells = sorted(want)
    got = out[torch.tensor(cells, device="cuda:0")].cpu().numpy().view(np.uint64)
    assert np.array_equal(got, cref.ints_to_mont([want[z] for z in cells]))
    assert int((out != 0).any(dim=1).sum()) == sum(1 for z in cells if want[z]), "zero in every other cell"
    # the oracle's fold of the whole table at g against the extension of the expected cells
    g = cref.synth_table(seed + 1, 4, dim)
    gi = cref.mont_to_ints(g)
    ext = 0
    for z in cells:
        e = want[z]
        for j in range(dim):
            e = e * (gi[j] if (z >> j) & 1 else 1 - gi[j]) % P
        ext = (ext + e) % P
    assert cref.mont_to_ints(cref.fix_variables(out.cpu().numpy().view(np.uint64), g)) == [ext]


def test_cells_with_70000_terms_of_p_minus_1_in_one_cell():
    dim, terms = 10, 70000
    idx, vals, table = K.one_cell(dim, terms, 777, 68000)
    before = counters()
    got, _ = evaluate([([(idx, vals)], table, table)], dim, batch=2)
    moved(before, cells=1)
    assert cref.mont_to_ints(got[0][0][777:778]) == [P - terms] and not np.delete(got[0][0], 777, axis=0).any()
    claim(idx, vals, dim, table, table, got[0][0], 68001)


# ---- 4. several layers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 10])
def test_four_layers_and_the_handle_takes_a_layer_as_it_lies_on_the_device(dim):
    """wiring and nnz differ per layer and instance, one list empty; dim 3: all layers inside one launch; dim 10: per layer on one stream.
    out[1] then goes, unchanged and on the device, into a handle as f2s and f3s of layer 2"""
    N, n = 1 << dim, 2
    nnzs = [[3 * N, N + 1], [6 * N, 3 * N], [3 * N, 0], [3 * N + 1, 5]]  # [layer][instance]: dense enough that a deep layer still has values
    kinds = ["random", "repeated", "random", "random"]
    insts = [([K.wiring(dim, 69000 + 10 * k + i, nnzs[k][i], kinds[k]) for k in range(4)], cref.synth_table(69100 + i, 2, N), cref.synth_table(69100 + i, 3, N)) for i in range(n)]
    before = counters()
    got, out = evaluate(insts, dim, batch=2)
    moved(before, one_block=1 if dim == 3 else 0, cells=0 if dim == 3 else 1)
    check(insts, dim, got)
    assert got[3][0].any() and not got[2][1].any() and not got[3][1].any(), "every layer has values; an empty layer, and what reads it, is zero"
    for k in (1, 2, 3):
        claim(*insts[0][0][k], dim, got[k - 1][0], got[k - 1][0], got[k][0], 69200 + k)
    gs = [cref.synth_table(69300 + i, 4, dim) for i in range(n)]
    f1s = [sc.SparseMultilinearExtension(3 * dim, NL.td(insts[i][0][2][0]), NL.td(insts[i][0][2][1])) for i in range(n)]
    torch.cuda.synchronize()
    chal = R.challenges(n, dim, 69400)
    want = R.walks([(insts[i][0][2][0], insts[i][0][2][1], got[1][i], got[1][i], gs[i]) for i in range(n)], dim, chal)
    with _lib.policy(batch=2, batch_slices=1):
        st = sc.GKRRoundSumcheck.prover_init_batch(f1s, out[1], out[1], gs)
    msgs, _, _ = R.drive(st, chal, want)
    st.close()
    for i in range(n):
        assert np.array_equal(cref.fr_binop("add", msgs[i, 0, 0], msgs[i, 0, 1]), cref.fix_variables(got[2][i], gs[i])[0]), "the handle's claim is layer 2's extension at g"


# ---- 5. refusals on the device -------------------------------------------------------------------------------------------------------
def test_an_index_out_of_range_in_a_device_list_is_found_before_anything_is_written():
    dim, n, n_layers = 3, 2, 3
    N = 1 << dim
    insts = K.circuit(n, dim, n_layers, 70000, [2 * N, N, 3 * N])
    bad = insts[1][0][2][0].copy()
    bad[5] |= np.uint64(1) << np.uint64(3 * dim)
    lists = [[(insts[i][0][k][0] if (k, i) != (2, 1) else bad, insts[i][0][k][1]) for i in range(n)] for k in range(n_layers)]
    keep = [[(NL.td(a), NL.td(b)) for a, b in layer] for layer in lists]
    f2, f3 = [NL.td(inst[1]) for inst in insts], [NL.td(inst[2]) for inst in insts]
    outs = [torch.full((N, 4), PATTERN, dtype=torch.int64, device="cuda:0") for _ in range(n * n_layers)]
    torch.cuda.synchronize()
    ptrs = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    nnz = (C.c_uint64 * (n * n_layers))(*[int(a.numel()) for layer in keep for a, _ in layer])
    args = (n, dim, n_layers, ptrs([a for layer in keep for a, _ in layer]), ptrs([b for layer in keep for _, b in layer]), nnz, ptrs(f2), ptrs(f3), _lib.SC_TABLES_ON_DEVICE, ptrs(outs))
    before = counters()
    assert sc.lib().sc_gkr_layers_eval_batch(*args) == _lib.SC_ERR_BAD_ARG
    assert sc.lib().sc_last_error().decode() == "layer 2 instance 1: f1 has an index out of range"
    moved(before)
    assert all(bool((t == PATTERN).all()) for t in outs), "no output has been written"
    keep[2][1][0][5] = int(insts[1][0][2][0][5])  # the index in range again: the same arrays evaluate
    torch.cuda.synchronize()
    assert sc.lib().sc_gkr_layers_eval_batch(*args) == _lib.SC_OK
    moved(before, one_block=1)
    got = [[outs[k * n + i].cpu().numpy().view(np.uint64) for i in range(n)] for k in range(n_layers)]
    check(insts, dim, got)
    claim(*insts[1][0][2], dim, got[1][1], got[1][1], got[2][1], 70001)


# ---- 6. the claim identity against the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 9, 10])
def test_the_claim_a_layers_sumcheck_starts_from_is_the_extension_of_the_evaluated_layer(dim):
    """for random g, cref.gkr_prove's first message satisfies P(0) + P(1) = cref.fix_variables(out, g): the provers, evaluate and the new
    kernels tied together through the oracle"""
    N = 1 << dim
    insts = [([K.wiring(dim, 71000 + dim + i, 2 * N, "random")], cref.synth_table(71100 + dim + i, 2, N), cref.synth_table(71100 + dim + i, 3, N)) for i in range(2)]
    before = counters()
    got, _ = evaluate(insts, dim, batch=2)
    moved(before, one_block=int(dim <= K.MAX_DIM), cells=int(dim > K.MAX_DIM))
    for i, inst in enumerate(insts):
        for s in range(2):
            claim(*inst[0][0], dim, inst[1], inst[2], got[0][i], 71200 + 10 * i + s)


# ---- 7. a circuit end to end ---------------------------------------------------------------------------------------------------------
def _transcript_challenge(rng, msgs):
    for m in msgs:
        rng.feed_prover_msg(m)
    return rng.sample_fr()


def _prove_layer(st, rng):
    """2 dim round calls and finish under the test's transcript, one challenge shared by all instances -> (first message, u, v, final)"""
    first, r = None, None
    for t in range(2 * st.dim):
        msgs = st.prove_round(r, shared=r is not None)
        first = msgs if t == 0 else first
        r = _transcript_challenge(rng, msgs)
    uv, fin = st.finish(r, shared=True)
    return first, uv[0, 0], uv[0, 1], fin


@pytest.mark.parametrize("dim", [3, 9])
def test_a_circuit_of_three_layers_is_evaluated_and_proved_back_to_its_inputs(dim):
    n, n_layers = 4, 3
    N = 1 << dim
    insts = K.circuit(n, dim, n_layers, 72000 + dim, [N + 1, 2 * N, 3 * N], "random")  # (the output layer, which the handle is built over, has the longest lists: every later layer fits the handle's copy)
    before = counters()
    got, W = evaluate(insts, dim, batch=2)  # W[k][i] stay on the device: the handle reads them there
    moved(before, one_block=1)
    f1 = [[sc.SparseMultilinearExtension(3 * dim, NL.td(inst[0][k][0]), NL.td(inst[0][k][1])) for inst in insts] for k in range(n_layers)]
    inputs2, inputs3 = [sc.DenseMultilinearExtension(dim, NL.td(inst[1])) for inst in insts], [sc.DenseMultilinearExtension(dim, NL.td(inst[2])) for inst in insts]
    torch.cuda.synchronize()
    rng = cref.Rng()
    rng.feed_bytes(b"gkr layers end to end")
    at = lambda table, point: cref.fix_variables(table, point)[0]
    mul, add = (lambda a, b: cref.fr_binop("mul", a, b)), (lambda a, b: cref.fr_binop("add", a, b))
    # the output layer: one point
    g = np.stack([rng.sample_fr() for _ in range(dim)])
    with _lib.policy(batch=2):
        st = sc.GKRRoundSumcheck.prover_init_batch(f1[2], W[1], W[1], [g] * n)
    first, u, v, fin = _prove_layer(st, rng)
    for i in range(n):
        assert np.array_equal(add(first[i, 0], first[i, 1]), at(got[2][i], g)), f"output layer, instance {i}: the claim is W(g)"
    claims = [sc.GKRRoundSumcheckSubClaim(u, v, mul(fin[i, 0], fin[i, 2])) for i in range(n)]
    assert sc.GKRRoundSumcheckSubClaim.verify_subclaim_batch(claims, f1[2], W[1], W[1], [g] * n) == [True] * n
    # every deeper layer: the claim stands at the two points the layer above ended on
    below = {1: (W[0], W[0], got[1]), 0: (inputs2, inputs3, got[0])}
    for k in (1, 0):
        alpha, beta = rng.sample_fr(), rng.sample_fr()
        coeffs = [np.stack([alpha, beta])] * n
        st.next_layer(below[k][0], below[k][1], [u] * n, f1[k], g2s=[v] * n, coeffs=coeffs)
        gu, gv = u, v
        first, u, v, fin = _prove_layer(st, rng)
        for i in range(n):
            want = add(mul(alpha, at(below[k][2][i], gu)), mul(beta, at(below[k][2][i], gv)))
            assert np.array_equal(add(first[i, 0], first[i, 1]), want), f"layer {k}, instance {i}: the claim is alpha W(u) + beta W(v)"
            if k == 1 and i == 0:
                flipped = below[k][2][i].copy()
                flipped[N // 2, 2] ^= np.uint64(1)
                other = add(mul(alpha, at(flipped, gu)), mul(beta, at(flipped, gv)))
                assert not np.array_equal(add(first[i, 0], first[i, 1]), other), "a flipped limb in the evaluated layer fails the claim check"
        claims = [sc.GKRRoundSumcheckSubClaim(u, v, mul(fin[i, 0], fin[i, 2])) for i in range(n)]
        assert sc.GKRRoundSumcheckSubClaim.verify_subclaim_two_point_batch(claims, f1[k], below[k][0], below[k][1], [gu] * n, [gv] * n, coeffs) == [True] * n
    st.close()
    for i, inst in enumerate(insts):  # the last layer ends on the INPUT tables
        assert np.array_equal(fin[i, 1], at(inst[1], u)) and np.array_equal(fin[i, 2], mul(at(inst[1], u), at(inst[2], v))), f"instance {i}: f2(u), f2(u) f3(v) of the inputs"
