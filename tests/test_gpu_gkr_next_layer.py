"""GPU tests of sc_gkr_layer_next_batch (GKRBatchProverState.next_layer): an existing GKR batch handle onto the next layer's inputs without
a rebuild.  The oracle is the Walk of tests/test_gpu_gkr_batch_rounds.py (composed from oracle/cref.py) under the same challenges: every
message of every round of every instance, the tables after round calls {1, dim, dim + 1, 2 dim - 1}, (u, v) and finish's triple are
compared bit for bit, for every layer a handle is put onto.  Handles are built under policy "batch" = 2 unless a case says otherwise."""
import ctypes as C
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
from tests import test_gpu_gkr_batch_rounds as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEXT = "batch.gkr_next_layer"


def td(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def counters():
    p = _lib.plan_stats()
    return p[NEXT], p["batch.gkr_rounds_one_block"], p["batch.gkr_rounds_slices"], p["batch.gkr_rounds_serial"]


def moved(before, next_layer=0, one_block=0, slices=0, serial=0):
    assert counters() == (before[0] + next_layer, before[1] + one_block, before[2] + slices, before[3] + serial), "next_layer / one_block / slices / serial"


def raw_layer(n, dim, seed, nnzs, variant="random"):
    """n instances (idx, vals, f2, f3, g) as host arrays; nnzs[i] non-zeros"""
    N = 1 << dim
    out = []
    for i in range(n):
        idx, vals = T.make_f1(dim, seed + 31 * i, variant, nnzs[i])
        out.append((idx, vals, cref.synth_table(seed + 7919 * i, 2, N), cref.synth_table(seed + 7919 * i, 3, N), cref.synth_table(seed + 7919 * i, 4, dim)))
    return out


def objects(insts, dim, device="cuda:0"):
    """instances as host arrays -> the library's objects (make_batch's keys), on the host (device=None) or on the GPU"""
    put = td if device is not None else (lambda a: a)
    b = {"n": len(insts), "dim": dim, "raw": insts, "gs": [a[4] for a in insts]}
    b["f1s"] = [sc.SparseMultilinearExtension(3 * dim, put(a[0]), put(a[1])) for a in insts]
    b["f2s"] = [sc.DenseMultilinearExtension(dim, put(a[2])) for a in insts]
    b["f3s"] = [sc.DenseMultilinearExtension(dim, put(a[3])) for a in insts]
    if device is not None:
        torch.cuda.synchronize()
    return b


def init(b, **pol):
    with _lib.policy(**({"batch": 2} if not pol else pol)):
        return R.init(b)


def onto(st, b, keep_f1=False):
    st.next_layer(b["f2s"], b["f3s"], b["gs"], None if keep_f1 else b["f1s"])
    assert st.round == 0 and st.randomness(0).shape[0] == 0


def nnz_a(n, dim):
    N = 1 << dim
    return [[2 * N, 3 * N, N, 8 * N, N // 2 + 1][i % 5] for i in range(n)]


def nnz_b(n, dim):
    """against nnz_a: none at all (nothing stale may be read), fewer, as many"""
    a = nnz_a(n, dim)
    return [[0, a[i] // 2 - 1, a[i]][i % 3] for i in range(n)]


@functools.lru_cache(maxsize=None)
def two_layers(dim, n, seed=0):
    """layers A and B of one shape, their challenges and walks: shared by every case over that shape (the walks depend on the seeds only)"""
    A, B = raw_layer(n, dim, 61000 + seed + 97 * dim + n, nnz_a(n, dim), "repeated"), raw_layer(n, dim, 62000 + seed + 97 * dim + n, nnz_b(n, dim))
    ca, cb = R.challenges(n, dim, 63000 + seed + dim + n, edge_instance=n // 2), R.challenges(n, dim, 64000 + seed + dim + n, edge_instance=0)
    for c in (ca, cb):
        c.setflags(write=False)
    states = R.state_rounds(dim)
    return A, B, ca, cb, R.walks(A, dim, ca, states), R.walks(B, dim, cb, states)


def a_b_a(st, a, b, ca, cb, wa, wb, dim, first=None):
    """layer A is proved (or `first` is its proof); onto B, proved; back onto A's arrays: the same bits as the first time"""
    states = R.state_rounds(dim)
    if first is None:
        first = R.drive(st, ca, wa, states, label="layer A: ")
    onto(st, b)
    R.drive(st, cb, wb, states, label="layer B: ")
    onto(st, a)
    again = R.drive(st, ca, wa, states, label="layer A again: ")
    for x, y in zip(first, again):
        assert np.array_equal(x, y), "the second proof of layer A differs from the first"


# ---- 1. A and B on one handle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", ["cuda:0", None], ids=["device", "host"])
@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("dim", [3, 9])
def test_two_layers_on_one_handle(dim, n, device):
    """dim 9: the one-block envelope's end.  Everything of B is new; its lists are empty, shorter than and as long as A's"""
    A, B, ca, cb, wa, wb = two_layers(dim, n)
    a, b = objects(A, dim, device), objects(B, dim, device)
    st = init(a)
    before = counters()
    a_b_a(st, a, b, ca, cb, wa, wb, dim)
    st.close()
    moved(before, next_layer=2, one_block=3 * 2 * dim)


# ---- 2. called in every state --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["fresh", "phase_two", "finished"])
def test_called_in_every_state(state):
    dim, n = 4, 3
    A, B, ca, cb, wa, wb = two_layers(dim, n)
    a, b = objects(A, dim), objects(B, dim)
    st = init(a)
    if state == "phase_two":  # round call dim + 1 has been answered: phase two's area is live
        for t in range(dim + 1):
            st.prove_round(None if t == 0 else ca[t - 1])
        assert st.round == dim + 1
    elif state == "finished":
        R.drive(st, ca, wa)
    ref = init(a)
    first = R.drive(ref, ca, wa, R.state_rounds(dim), label="a handle of its own: ")
    ref.close()
    a_b_a(st, a, b, ca, cb, wa, wb, dim, first=first)
    st.close()


# ---- 3. the wiring kept --------------------------------------------------------------------------------------------------------------
def test_the_wiring_kept_one_f1_for_all_f2_and_f3_one_array_a_shared_challenge():
    dim, n = 5, 4
    N = 1 << dim
    idx, vals = T.make_f1(dim, 65000, "random", 3 * N)
    layers = []
    for k in range(3):
        tabs = [cref.synth_table(65100 + 10 * k + i, 2, N) for i in range(n)]
        layers.append([(idx, vals, tabs[i], tabs[i], cref.synth_table(65200 + 10 * k + i, 4, dim)) for i in range(n)])
    f1 = sc.SparseMultilinearExtension(3 * dim, td(idx), td(vals))
    objs = []
    for insts in layers:
        dense = [sc.DenseMultilinearExtension(dim, td(a[2])) for a in insts]
        objs.append({"f1s": [f1] * n, "f2s": dense, "f3s": dense, "gs": [a[4] for a in insts], "raw": insts})
    torch.cuda.synchronize()
    chal = R.challenges(n, dim, 65300, edge_instance=None)
    same = np.repeat(chal[:, :1], n, axis=1)
    st = init(objs[0])
    before = counters()
    R.drive(st, chal, R.walks(layers[0], dim, same), shared=True, label="layer 0: ")
    for k in (1, 2):
        onto(st, objs[k], keep_f1=True)
        R.drive(st, chal, R.walks(layers[k], dim, same, R.state_rounds(dim)), R.state_rounds(dim), shared=True, label=f"layer {k}, wiring kept: ")
    # f2 and f3 no longer one array: 2 n distinct tables where init laid out n -- refused, and the handle is still layer 2's
    other = [sc.DenseMultilinearExtension(dim, td(a[3])) for a in layers[1]]
    torch.cuda.synchronize()
    msg = R._raises(_lib.SC_ERR_BAD_ARG, st.next_layer, objs[1]["f2s"], other, objs[1]["gs"])
    assert "build a new handle" in msg and str(2 * n * N * 32 + _f1_bytes(3 * N)) in msg and str(n * N * 32 + _f1_bytes(3 * N)) in msg, msg
    st.reset()
    R.drive(st, chal, R.walks(layers[2], dim, same), shared=True, label="layer 2 after a refused call: ")
    st.close()
    moved(before, next_layer=2, one_block=4 * 2 * dim)


def _f1_bytes(nnz):
    """an index list and its values in a handle's copy: each rounded up to 256 bytes"""
    up = lambda v: (v + 255) // 256 * 256
    return up(nnz * 8) + up(nnz * 32)


# ---- 4. unaligned sources ------------------------------------------------------------------------------------------------------------
def test_device_arrays_at_an_8_byte_offset_and_odd_lists():
    """every device array of both layers starts 8 bytes into a larger buffer (a uint64_t * is only 8-byte aligned) and every list has an
    odd number of entries: the smallest shape at which a 16-byte copy goes wrong"""
    dim, n = 3, 2
    N = 1 << dim
    A, B = raw_layer(n, dim, 66000, [2 * N + 1, N + 1]), raw_layer(n, dim, 66500, [2 * N - 1, 1])

    def shifted(a):
        flat = np.ascontiguousarray(a).view(np.int64).reshape(-1)
        big = torch.zeros(flat.shape[0] + 3, dtype=torch.int64, device="cuda:0")
        assert big.data_ptr() % 16 == 0
        big[1:1 + flat.shape[0]] = torch.from_numpy(flat).to("cuda:0")
        out = big[1:1 + flat.shape[0]].view(np.asarray(a).shape)
        assert out.data_ptr() % 16 == 8 and out.is_contiguous()
        return out

    def objs(insts):
        b = {"raw": insts, "gs": [a[4] for a in insts]}
        b["f1s"] = [sc.SparseMultilinearExtension(3 * dim, shifted(a[0]), shifted(a[1])) for a in insts]
        b["f2s"] = [sc.DenseMultilinearExtension(dim, shifted(a[2])) for a in insts]
        b["f3s"] = [sc.DenseMultilinearExtension(dim, shifted(a[3])) for a in insts]
        return b

    a, b = objs(A), objs(B)
    torch.cuda.synchronize()
    ca, cb = R.challenges(n, dim, 66001), R.challenges(n, dim, 66002)
    st = init(a)
    a_b_a(st, a, b, ca, cb, R.walks(A, dim, ca, R.state_rounds(dim)), R.walks(B, dim, cb, R.state_rounds(dim)), dim)
    st.close()


# ---- 5. the sliced plan --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [10, 11])
def test_the_sliced_plan(dim):
    """dim 10: only the initialisation is sliced; 11: rounds 0 and 1 too.  Layer A has one cell that takes 4 x 2^dim terms per phase, layer B
    a sparse list: cells that were not zeroed would show"""
    n = 2
    N = 1 << dim
    rng = np.random.default_rng(67000 + dim)
    A = []
    for i in range(n):
        z = rng.integers(0, N, size=4 * N, dtype=np.uint64)
        idx = np.ascontiguousarray(z | np.uint64((77 + i) << dim) | np.uint64((1000 - i) << (2 * dim)))
        A.append((idx, cref.synth_table(67100 + i, 1, 4 * N), cref.synth_table(67100 + i, 2, N), cref.synth_table(67100 + i, 3, N), cref.synth_table(67100 + i, 4, dim)))
    B = raw_layer(n, dim, 67500 + dim, [N // 8, 0])
    ca, cb = R.challenges(n, dim, 67001 + dim), R.challenges(n, dim, 67002 + dim, edge_instance=1)
    wa, wb = R.walks(A, dim, ca, R.state_rounds(dim)), R.walks(B, dim, cb, R.state_rounds(dim))
    a, b = objects(A, dim), objects(B, dim)
    st = init(a, batch=2, batch_slices=1)
    before = counters()
    a_b_a(st, a, b, ca, cb, wa, wb, dim)
    st.close()
    moved(before, next_layer=2, slices=3 * 2 * dim)


# ---- 6. the serial plan --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,pol", [(10, {"batch": 2}), (4, {"batch": 0})], ids=["dim10-no-key", "dim4-batch0"])
def test_the_serial_plan_gives_the_same_bits(dim, pol):
    n = 2 if dim == 10 else 3
    A, B, ca, cb, wa, wb = two_layers(dim, n)
    a, b = objects(A, dim), objects(B, dim)
    st = init(a, **pol)
    before = counters()
    a_b_a(st, a, b, ca, cb, wa, wb, dim)  # (dim 4, n 3: the walks test_called_in_every_state holds the work-area handle to)
    st.close()
    moved(before, serial=3 * 2 * dim)


# ---- 7. three layers chained ---------------------------------------------------------------------------------------------------------
def test_three_layers_chained_under_one_transcript_per_instance():
    """layer k + 1's g is layer k's u; every challenge comes from the instance's Blake2b transcript, which runs through all three layers"""
    dim, n = 5, 4
    N = 1 << dim
    layers = [raw_layer(n, dim, 68000 + 500 * k, [[2 * N, N, 3 * N, N // 2][(i + k) % 4] for i in range(n)]) for k in range(3)]
    mine, theirs, verifiers = [], [], []
    for i in range(n):
        mine.append(sc.Blake2b512Rng.setup())
        verifiers.append(sc.Blake2b512Rng.setup())
        theirs.append(cref.Rng())
        mine[i].feed(b"circuit %d" % i)
        verifiers[i].feed(b"circuit %d" % i)
        theirs[i].feed_bytes(b"circuit %d" % i)
    st, u = None, None
    before = counters()
    for k, insts in enumerate(layers):
        if u is not None:
            insts = [(a[0], a[1], a[2], a[3], np.ascontiguousarray(u[i])) for i, a in enumerate(insts)]
        b = objects(insts, dim)
        if st is None:
            st = init(b)
        else:
            onto(st, b)
        proofs, uv, fin = R.prove_with_transcripts(st, mine)
        subclaims = []
        for i, (idx, vals, f2, f3, g) in enumerate(insts):
            wp, wuv = cref.gkr_prove(idx, vals, dim, f2, f3, g, rng=theirs[i], threads=1)
            assert np.array_equal(proofs[i], wp) and np.array_equal(uv[i], wuv), f"layer {k}, instance {i}: the proof differs from cref.gkr_prove's"
            proof = sc.gkr_round_sumcheck.GKRProof([sc.ProverMsg(m) for m in proofs[i, 0]], [sc.ProverMsg(m) for m in proofs[i, 1]])
            sub = sc.GKRRoundSumcheck.verify(verifiers[i], dim, proof, proof.extract_sum())
            assert np.array_equal(sub.u, uv[i, 0]) and np.array_equal(sub.v, uv[i, 1]), f"layer {k}, instance {i}: the verifier's point"
            assert np.array_equal(cref.fr_binop("mul", fin[i, 0], fin[i, 2]), sub.expected_evaluation), f"layer {k}, instance {i}: finish's triple"
            subclaims.append(sub)
        assert all(sc.GKRRoundSumcheckSubClaim.verify_subclaim_batch(subclaims, b["f1s"], b["f2s"], b["f3s"], b["gs"])), f"layer {k}: the subclaims"
        u = uv[:, 0]
    st.close()
    for i in range(n):
        assert np.array_equal(mine[i].sample_fr(), theirs[i].sample_fr()), f"instance {i}: the transcript after three layers"
    moved(before, next_layer=2, one_block=3 * 2 * dim)


# ---- 8. errors leave the handle where it was -----------------------------------------------------------------------------------------
def test_errors_in_the_middle_of_phase_one_leave_the_handle_where_it_was():
    dim, n = 4, 3
    N = 1 << dim
    A, B, ca, cb, wa, wb = two_layers(dim, n)
    a, b = objects(A, dim), objects(B, dim)
    st = init(a)
    for t in range(2):
        assert np.array_equal(st.prove_round(None if t == 0 else ca[t - 1]), np.stack([w.msgs[t] for w in wa]))
    before = counters()

    def with_f1(i, idx, vals):
        f1s = list(b["f1s"])
        f1s[i] = sc.SparseMultilinearExtension(3 * dim, td(idx), td(vals))
        torch.cuda.synchronize()
        return f1s

    # a list longer than the bytes init reserved (within the plan's limit): both byte counts
    k = nnz_a(n, dim)[0] + 64
    longer = T.make_f1(dim, 69000, "repeated", k)
    msg = R._raises(_lib.SC_ERR_BAD_ARG, st.next_layer, b["f2s"], b["f3s"], b["gs"], with_f1(0, *longer))
    reserved = sum(_f1_bytes(x) for x in nnz_a(n, dim)) + 2 * n * N * 32
    needed = _f1_bytes(k) + sum(_f1_bytes(x) for x in nnz_b(n, dim)[1:]) + 2 * n * N * 32
    assert "build a new handle" in msg and f"{needed} bytes" in msg and f"reserved {reserved}" in msg, msg
    # more than 64 x 2^dim non-zeros: another plan's shape
    over = T.make_f1(dim, 69001, "repeated", 64 * N + 1)
    msg = R._raises(_lib.SC_ERR_BAD_ARG, st.next_layer, b["f2s"], b["f3s"], b["gs"], with_f1(1, *over))
    assert msg.startswith("instance 1: nnz %d" % (64 * N + 1)) and "batch.gkr_rounds_serial" in msg and "build a new handle" in msg, msg
    # a non-canonical g
    gs = [g.copy() for g in b["gs"]]
    gs[2][1] = R.P_LIMBS
    assert R._raises(_lib.SC_ERR_BAD_ARG, st.next_layer, b["f2s"], b["f3s"], gs, b["f1s"]) == "instance 2: g[1] is not a canonical field element"
    # f1_idx without f1_vals and nnz
    ptrs = lambda vals: (C.c_void_p * n)(*[C.cast(v, C.c_void_p) for v in vals])
    keep = [np.ascontiguousarray(g) for g in b["gs"]]
    args = [ptrs([C.c_void_p(m.data_ptr()) for m in b["f2s"]]), ptrs([C.c_void_p(m.data_ptr()) for m in b["f3s"]]), ptrs([g.ctypes.data for g in keep])]
    idx_p = ptrs([f._ptrs()[0] for f in b["f1s"]])
    nnz = (C.c_uint64 * n)(*[f.nnz for f in b["f1s"]])
    for f1_args in ((idx_p, None, None), (None, None, nnz), (idx_p, None, nnz)):
        assert sc.lib().sc_gkr_layer_next_batch(st._h, *f1_args, *args, _lib.SC_TABLES_ON_DEVICE) == _lib.SC_ERR_BAD_ARG
        assert "all NULL" in sc.lib().sc_last_error().decode()
    # host arrays for a handle built over device arrays
    h = objects(B, dim, device=None)
    assert "flags" in R._raises(_lib.SC_ERR_BAD_ARG, st.next_layer, h["f2s"], h["f3s"], h["gs"], h["f1s"])
    # a device-resident index with bit 3 dim set: found on the device, over the caller's arrays, never followed
    idx = B[1][0].copy()
    idx[2] |= np.uint64(1) << np.uint64(3 * dim)
    msg = R._raises(_lib.SC_ERR_BAD_ARG, st.next_layer, b["f2s"], b["f3s"], b["gs"], with_f1(1, idx, B[1][1]))
    assert msg.startswith("instance 1: f1 has an index out of range"), msg
    # ... and the proof in progress goes on with the same bits
    moved(before)
    assert st.round == 2 and np.array_equal(st.randomness(1), ca[:1, 1])
    for t in range(2, 2 * dim):
        assert np.array_equal(st.prove_round(ca[t - 1]), np.stack([w.msgs[t] for w in wa])), f"round call {t} after the refused calls"
        if t + 1 in R.state_rounds(dim):
            for i in range(n):
                assert np.array_equal(st.tables(i), wa[i].states[t + 1]), (t, i)
    uv, fin = st.finish(ca[2 * dim - 1])
    for i in range(n):
        assert np.array_equal(uv[i].reshape(2 * dim, 4), ca[:, i]) and np.array_equal(fin[i], wa[i].final), i
    onto(st, b)  # and the handle still takes a good layer
    R.drive(st, cb, wb, label="layer B after the refused calls: ")
    st.close()


# ---- 9. the plan counters ------------------------------------------------------------------------------------------------------------
def test_the_plan_counter_moves_once_per_successful_call_on_a_work_area_handle():
    dim, n = 4, 3
    A, B, ca, cb, wa, wb = two_layers(dim, n)
    a, b = objects(A, dim), objects(B, dim)
    before = counters()
    st = init(a)
    moved(before)
    onto(st, b)
    moved(before, next_layer=1)
    R.drive(st, cb, wb)
    moved(before, next_layer=1, one_block=2 * dim)  # the rounds are counted as after init
    gs = [g.copy() for g in a["gs"]]
    gs[0][0] = R.P_LIMBS
    R._raises(_lib.SC_ERR_BAD_ARG, st.next_layer, a["f2s"], a["f3s"], gs, a["f1s"])
    moved(before, next_layer=1, one_block=2 * dim)
    onto(st, a)
    moved(before, next_layer=2, one_block=2 * dim)
    st.close()
    serial = init(a, batch=0)
    onto(serial, b)
    R.drive(serial, cb, wb)
    serial.close()
    moved(before, next_layer=2, one_block=2 * dim, serial=2 * dim)


# ---- 10. the C++ mirror --------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_next_layer():
    """GKRBatchProverState::next_layer of include/sumcheck_amd.hpp: a program proves layer A, layer B and layer A again on one handle at
    dim 4 and prints its inputs, its challenges and every message; the messages are compared with the walks over what it printed"""
    from tests import test_cpp_mirror as M
    src = os.path.join(ROOT, "tests", "cpp", "test_gkr_next_layer_mirror.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "test_gkr_next_layer_mirror.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, "-o", out, "-L", M.LIBDIR, "-lsumcheck_hip", f"-Wl,-rpath,{M.LIBDIR}",
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-2000:] + r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        key, colon, words = line.partition(":")
        if colon:  # (an empty list prints no word)
            rows[key.strip()] = np.array([int(w, 16) for w in words.split()], dtype=np.uint64)
    dim, n = int(rows["dim"][0]), int(rows["n"][0])
    assert dim == 4 and n >= 2
    layers = {}
    for name in "AB":
        layers[name] = [(rows[f"{name} idx {i}"], rows[f"{name} vals {i}"].reshape(-1, 4), rows[f"{name} f2 {i}"].reshape(-1, 4), rows[f"{name} f3 {i}"].reshape(-1, 4),
                         rows[f"{name} g {i}"].reshape(dim, 4)) for i in range(n)]
    for p, name in enumerate("ABA"):
        chal = rows[f"pass {p} challenges"].reshape(2 * dim, n, 4)
        want = R.walks(layers[name], dim, chal)
        got = rows[f"pass {p} messages"].reshape(2 * dim, n, 3, 4)
        for i in range(n):
            assert np.array_equal(got[:, i], want[i].msgs), f"pass {p} (layer {name}), instance {i}: the messages differ from the walk's"
            assert np.array_equal(rows[f"pass {p} final"].reshape(n, 3, 4)[i], want[i].final), f"pass {p} (layer {name}), instance {i}: finish's triple"
    assert np.array_equal(rows["pass 0 challenges"], rows["pass 2 challenges"]) and np.array_equal(rows["pass 0 messages"], rows["pass 2 messages"])
