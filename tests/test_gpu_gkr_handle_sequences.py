"""GPU tests of the GKR batch handle (sc_gkr_batch_prover) under generated call sequences: tests/gkr_handle_sequences.py draws, per seed, two
handles of different configurations and a long mixed history -- rounds with per-instance and shared challenges, finish with and without its
outputs, state queries, resets, the four shapes of next, every refused call the header names, and between them policy changes, released
caches, one-shot calls of the other families and rounds of the other handle.  The sequence is replayed through GKRBatchProverState; after
EVERY operation the messages, (u, v), the final values, the round, every instance's randomness, the tables of a mul handle, the status and
the head of the text of a refused call, and the movement of every plan counter with "gkr" in its name are compared with what the model
expects -- the values bit for bit with the three walks (Walk, Walk2, WalkG) over the attempt's inputs and the challenges handed out.
Each seed runs with its handles' inputs where the seed put them (host or device) and once more with both swapped; the walks are shared.
A failure names the seed, the position and the sequence up to there; `python -m tests.gkr_handle_sequences SEED` prints all of it."""
import ctypes as C

import numpy as np
import pytest
import torch

import sumcheck_amd as sc
from oracle import cref
from sumcheck_amd import _lib
from sumcheck_amd.gkr_round_sumcheck import _dense_ptr
from sumcheck_amd.ml_sumcheck import _ptr
from tests import gkr_gates_cases as K
from tests import gkr_handle_sequences as S
from tests import test_gpu_batch as MB
from tests import test_gpu_eval_batch as EB
from tests import test_gpu_gkr_batch as T
from tests import test_gpu_gkr_gates as G
from tests import test_gpu_gkr_next_layer as NL

pytestmark = pytest.mark.gpu
STATUS = {name: getattr(_lib, name) for name in S.STATUS}  # the loader's constants (the host test compares them with the header's text)
POLICY_KEYS = ("batch", "batch_slices", "gkr_gates_fused")


def gkr_counters():
    return {k: v for k, v in _lib.plan_stats().items() if "gkr" in k}


def objects(spec, insts, device):
    """a layer's instances -> the library's objects; shared wiring: the last instance holds instance 0's OBJECTS (one pair of pointers)"""
    if spec.kind == "gates":
        b = G.objects(insts, device)
        lists = ("muls", "adds")
    else:
        b = NL.objects([a[:5] for a in insts], spec.dim, device)
        two = len(insts[0]) > 5
        b["g2s"], b["coeffs"] = ([a[5] for a in insts], [a[6] for a in insts]) if two else (None, None)
        lists = ("f1s",)
    if spec.shared:
        for k in lists:
            b[k][-1] = b[k][0]
    return b


def build(spec, b):
    with _lib.policy(**spec.pol):  # the policies are set only around the init call
        if spec.kind == "gates":
            return sc.GKRRoundSumcheck.prover_init_batch_gates(b["muls"], b["adds"], b["f2s"], b["f3s"], b["gs"], g2s=b["g2s"], coeffs=b["coeffs"])
        return sc.GKRRoundSumcheck.prover_init_batch(b["f1s"], b["f2s"], b["f3s"], b["gs"], g2s=b["g2s"], coeffs=b["coeffs"])


def onto(H, b, kept):
    """the handle's own next call over b"""
    if H.spec.kind == "gates":
        H.st.next_layer_gates(b["f2s"], b["f3s"], b["gs"], None if kept else b["muls"], None if kept else b["adds"], g2s=b["g2s"], coeffs=b["coeffs"])
    else:
        H.st.next_layer(b["f2s"], b["f3s"], b["gs"], None if kept else b["f1s"], g2s=b["g2s"], coeffs=b["coeffs"])


class Live:
    """a handle of the library and where the model says it is"""

    def __init__(self, spec, device, insts):
        self.spec, self.device = spec, "cuda:0" if device else None
        self.cur = objects(spec, insts, self.device)  # the layer in force
        self.st = build(spec, self.cur)
        self.round, self.received, self.attempt, self.exhausted = 0, 0, 0, False

    def restart(self):
        self.round, self.received, self.exhausted = 0, 0, False
        self.attempt += 1


class Replay:
    def __init__(self, seq, proofs, swapped):
        self.seq, self.proofs, self.pos = seq, proofs, -1
        self.saved = {k: _lib.get_policy(k) for k in POLICY_KEYS}
        self.live = []
        for h, spec in enumerate(seq.specs):
            before = gkr_counters()
            self.live.append(Live(spec, spec.device != swapped, S.layer_insts(spec, seq.handles[h].attempts[0].layer)))
            self.moved(before, seq.init_counters(h), spec, "init")

    def where(self, what=""):
        head = "\n".join(self.seq.text().split("\n")[:4 + max(self.pos, 0)])
        return f"seed {self.seq.seed}, operation {self.pos}: {what}\n{head}"

    def moved(self, before, want, spec, what):
        """exactly the counters in `want` moved; on a serial plan the dense tables take sc_gkr_prove's routes (gkr.*), whichever they are"""
        after = gkr_counters()
        for k in after:
            if k in want or not (k.startswith("gkr.") and spec.cls == "serial"):
                assert after[k] - before[k] == want.get(k, 0), self.where(f"{what}: plan counter {k} moved by {after[k] - before[k]}, the model says {want.get(k, 0)}")

    def refused(self, o, fn):
        status, text = self.seq.refusal(o)
        with pytest.raises(_lib.SumcheckError) as e:
            fn()
            pytest.fail(self.where(f"the call was accepted, the header says {status}"))
        assert e.value.code == STATUS[status], self.where(f"status {e.value.code} ({e.value.msg}), the header says {status}")
        assert e.value.msg.startswith(text), self.where(f"the text is '{e.value.msg}', expected to begin '{text}'")
        return e.value.msg

    def raw(self, fn, *args):
        """a C call the wrappers cannot make, as an exception like theirs"""
        def call():
            _lib.check(fn(*args))
        return call

    def check_state(self, H, h):
        st, n = H.st, H.spec.n
        assert st.round == H.round, self.where(f"handle {h}: round {st.round}, the model says {H.round}")
        for i in range(n):
            got = st.randomness(i)
            want = self.proofs[(h, H.attempt)].chal[:H.received, i] if H.received else np.zeros((0, 4), np.uint64)
            assert np.array_equal(got, want), self.where(f"handle {h}: the randomness of instance {i}")

    # ---- one operation ----
    def run(self, o, top=True):
        if top:
            self.pos += 1
        if o.op == "env_other_round":
            self.run(o.params["step"], top=False)
            self.check_state(self.live[o.h], o.h)
            return
        H, spec, seq = self.live[o.h], self.seq.specs[o.h], self.seq
        st, n, dim, p = H.st, spec.n, spec.dim, o.params
        assert (o.round, o.attempt) == (H.round, H.attempt) and o.state == S.state_class(H.round, dim, H.exhausted), self.where("the replay lost the model")
        proof = self.proofs.get((o.h, o.attempt))
        filler = cref.synth_table(4242 + self.pos, 77, n)  # canonical challenges for calls that must be refused before they are read
        cur = H.cur
        before = gkr_counters()
        if o.op in ("round", "round_shared"):
            t = o.round
            r = None if t == 0 else np.ascontiguousarray(proof.chal[t - 1, 0] if o.op == "round_shared" else proof.chal[t - 1])
            got = st.prove_round(r, shared=o.op == "round_shared")
            bad = np.nonzero((got != proof.msgs(t)).any(axis=(1, 2)))[0]
            assert np.array_equal(got, proof.msgs(t)), self.where(f"round call {t}: the messages differ from the walk's, instances {bad}")
            H.round, H.received = t + 1, t
        elif o.op == "finish":
            last = np.ascontiguousarray(proof.chal[2 * dim - 1, 0] if p["shared"] else proof.chal[2 * dim - 1])
            uv = np.zeros((n, 2, dim, 4), np.uint64) if p["outputs"] in ("both", "uv") else None
            fin = np.zeros((n, 3, 4), np.uint64) if p["outputs"] in ("both", "final") else None
            _lib.check(sc.lib().sc_gkr_batch_prover_finish(st._h, _ptr(last), 1 if p["shared"] else 0, None if uv is None else _ptr(uv), None if fin is None else _ptr(fin)))
            assert uv is None or np.array_equal(uv, proof.uv), self.where("finish: (u, v)")
            assert fin is None or np.array_equal(fin, proof.final), self.where("finish: the final values differ from the walk's")
            H.received, H.exhausted = 2 * dim, True
        elif o.op == "state":
            for i in range(n):
                if spec.kind == "gates":
                    with pytest.raises(_lib.SumcheckError) as e:
                        st.tables(i)
                    assert e.value.code == STATUS["SC_ERR_BAD_ARG"] and e.value.msg.startswith("tables_out: a gate handle exports no tables"), self.where(e.value.msg)
                elif not H.exhausted:
                    assert np.array_equal(st.tables(i), proof.tables(i, H.round)), self.where(f"the two tables of instance {i} after {H.round} round calls")
        elif o.op == "reset":
            st.reset()
            H.restart()
        elif o.op.startswith("next_"):
            H.cur = objects(spec, S.layer_insts(spec, p["layer"]), H.device)
            onto(H, H.cur, "_kept_" in o.op)
            H.restart()
        elif o.op == "ref_first_has_msg":
            self.refused(o, lambda: st.prove_round(filler))
        elif o.op == "ref_missing_msg":
            self.refused(o, lambda: st.prove_round(None))
        elif o.op == "ref_round_after_end":
            self.refused(o, lambda: st.prove_round(filler))
        elif o.op == "ref_bad_challenge":
            bad = filler.copy()
            bad[p["instance"]] = S.P_LIMBS
            self.refused(o, (lambda: st.finish(bad)) if o.state == "awaiting_finish" else (lambda: st.prove_round(bad)))
        elif o.op == "ref_finish_early":
            self.refused(o, lambda: st.finish(filler))
        elif o.op == "ref_other_next":
            other = st.next_layer if spec.kind == "gates" else st.next_layer_gates
            self.refused(o, lambda: other(cur["f2s"], cur["f3s"], cur["gs"]))
        elif o.op in ("ref_mixed_wiring", "ref_flags"):
            flags = _lib.SC_TABLES_ON_DEVICE if H.device else 0
            ptrs = lambda vals: (C.c_void_p * n)(*[C.cast(v, C.c_void_p) for v in vals])
            tail = [ptrs([_dense_ptr(m) for m in cur["f2s"]]), ptrs([_dense_ptr(m) for m in cur["f3s"]]), ptrs([_ptr(np.ascontiguousarray(g)) for g in cur["gs"]])]
            wiring = []
            for f1s in ([cur["muls"], cur["adds"]] if spec.kind == "gates" else [cur["f1s"]]):
                wiring += [ptrs([f._ptrs()[0] for f in f1s]), ptrs([f._ptrs()[1] for f in f1s]), (C.c_uint64 * n)(*[f.nnz for f in f1s])]
            if o.op == "ref_mixed_wiring":
                wiring[p["hole"]] = None
            else:  # the flag alone differs: kept wiring, and the call is refused before any array is read
                wiring, flags = [None] * len(wiring), flags ^ _lib.SC_TABLES_ON_DEVICE
            if spec.kind == "gates":
                msg = self.refused(o, self.raw(sc.lib().sc_gkr_gates_next_batch, st._h, *wiring, *tail, None, None, flags))
            else:
                msg = self.refused(o, self.raw(sc.lib().sc_gkr_layer_next_batch, st._h, *wiring, *tail, flags))
            assert o.op != "ref_flags" or msg.startswith("flags: the handle was built over " + ("device" if H.device else "host") + " arrays"), self.where(msg)
        elif o.op == "ref_bad_point":
            i, which = p["instance"], p["which"]
            gs = [np.array(g, dtype=np.uint64, copy=True) for g in cur["gs"]]
            g2s = [cref.synth_table(p["seed"] + i2, 5, dim).copy() for i2 in range(n)]
            coeffs = [cref.synth_table(p["seed"] + i2, 6, 2).copy() for i2 in range(n)]
            if which == "g":
                gs[i][0] = S.P_LIMBS
            elif which == "g2":
                g2s[i][dim - 1] = S.P_LIMBS
            else:
                coeffs[i][1] = S.P_LIMBS
            b = dict(cur, gs=gs, g2s=None if which == "g" else g2s, coeffs=None if which == "g" else coeffs)
            self.refused(o, lambda: onto(H, b, True))
        elif o.op in ("ref_over_limit", "ref_overflow"):
            init_nnz = seq.handles[o.h].init_nnz
            if o.op == "ref_overflow":  # every list 64 entries longer than init's: 512 B of indices and 2 KiB of values beyond any padding
                grow = lambda nnz: [a + 64 for a in nnz]
            else:
                at = 0 if spec.shared and p["instance"] == n - 1 else p["instance"]  # (shared wiring: the last instance's list is instance 0's)
                grow = lambda nnz: S.shared_nnz(spec, [(S.MAX_NNZ_PER_CELL << dim) + 1 if i == at else a for i, a in enumerate(nnz)])
            if spec.kind == "mul":
                nnz = grow(init_nnz)
            else:
                which = p.get("which")
                nnz = (grow(init_nnz[0]) if which != "add" else list(init_nnz[0]), grow(init_nnz[1]) if which != "mul" else list(init_nnz[1]))
            b = objects(spec, S.layer_insts(spec, S.Layer(p["seed"], p["seed"] + 1, nnz, False)), H.device)
            self.refused(o, lambda: onto(H, b, False))
        elif o.op == "env_policies":
            for k, v in spec.other_policies().items():
                _lib.set_policy(k, v)
        elif o.op == "env_release":
            assert sc.lib().sc_release_caches() == 0
        elif o.op == "env_oneshot":
            self.oneshot(p["which"], p["dim"], p["seed"])
            after = gkr_counters()
            assert all(after[k] == before[k] for k in S.HANDLE_COUNTERS), self.where("a one-shot call moved a counter of the handle's plans")
        else:
            raise AssertionError(o.op)
        if o.op != "env_oneshot":
            self.moved(before, seq.counters(o), spec, o.op)
        for h, L in enumerate(self.live):
            if h == o.h or o.op.startswith("env_"):
                self.check_state(L, h)

    def oneshot(self, which, dim, seed):
        """one small call of another family against that call's own oracle, as its own tests compare it"""
        N = 1 << dim
        if which == "prove":
            b = T.make_batch(1, dim, seed)
            (wp, _, wnext), = T.oracle_all(b)
            got = sc.GKRRoundSumcheck.prove(b["rngs"][0], b["f1s"][0], b["f2s"][0], b["f3s"][0], b["gs"][0])
            assert np.array_equal(np.stack([m.evaluations for m in got.phase1_sumcheck_msgs]), wp[0]) and np.array_equal(np.stack([m.evaluations for m in got.phase2_sumcheck_msgs]), wp[1]), self.where("sc_gkr_prove")
            assert np.array_equal(b["rngs"][0].sample_fr(), wnext), self.where("sc_gkr_prove: the transcript")
        elif which == "prove_batch":
            b = T.make_batch(3, dim, seed, ragged=True)
            T.assert_batch_equals(b, T.oracle_all(b))
        elif which == "evaluate_subclaims":
            b = EB.make_gkr_batch(2, dim, seed)
            EB.assert_gkr_equals(b, EB.gkr_oracle(b))
        elif which == "ml_prove_batch":
            polys, descs = MB.make_batch(3, dim, MB.C2, seed)
            MB.assert_batch_equals(polys, MB.oracle_all(descs))
        else:
            gates = which == "evaluate_layers_gates"
            empty = (np.zeros(0, np.uint64), np.zeros((0, 4), np.uint64))
            layers = [[(K.wiring(dim, seed + 10 * k + i, 2 * N + 1), K.wiring(dim, seed + 10 * k + i + 5, N + 1) if gates else empty) for i in range(2)] for k in range(2)]
            f2s, f3s = [cref.synth_table(seed + i, 2, N) for i in range(2)], [cref.synth_table(seed + i, 3, N) for i in range(2)]
            want = [K.define_layers([layers[0][i], layers[1][i]], f2s[i], f3s[i]) for i in range(2)]
            cref.fix_variables(want[0][1], cref.synth_table(seed, 4, dim))  # (the oracle's own reading of an expected layer)
            if gates:
                got = G.evaluate(layers, f2s, f3s, dim, **{k: _lib.get_policy(k) for k in POLICY_KEYS})
            else:
                sp = lambda lst: sc.SparseMultilinearExtension(3 * dim, NL.td(lst[0]), NL.td(lst[1]))
                dense = lambda a: sc.DenseMultilinearExtension(dim, NL.td(a))
                out = sc.GKRRoundSumcheck.evaluate_layers_batch([[sp(w[0]) for w in layer] for layer in layers], [dense(a) for a in f2s], [dense(a) for a in f3s])
                got = [[G.host(m) for m in layer] for layer in out]
            for i in range(2):
                for k in range(2):
                    assert np.array_equal(got[k][i], want[i][k]), self.where(f"{which}: layer {k}, instance {i}")

    def close(self):
        for k, v in self.saved.items():
            _lib.set_policy(k, v)
        for L in self.live:
            L.st.close()


@pytest.mark.parametrize("placement", ["drawn", "swapped"])
@pytest.mark.parametrize("seed", S.SEEDS)
def test_a_generated_sequence_matches_the_model_after_every_operation(seed, placement):
    seq, proofs = S.sequence(seed), S.oracle(seed)  # (the walks of a seed are computed once, for both placements)
    run = None
    try:
        run = Replay(seq, proofs, placement == "swapped")
        for o in seq.ops:
            run.run(o)
    finally:
        if run is not None:
            run.close()
