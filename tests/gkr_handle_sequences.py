"""A model of the GKR batch handle (sc_gkr_batch_prover: include/sumcheck_hip.h) as a state machine, and a generator of call sequences checked
against it.  Needs no GPU and imports nothing of the library: the oracle (oracle/cref.py), the two lib-free case modules, and the header's text.

A SEQUENCE is a seed, two handles of different configurations and a list of operations, each drawn from those legal in the state the model
is in.  The seven configurations, each built under the policies that select it (set only around the init call):
    mul/one_block  mul/slices  mul/serial  gates/one_block  gates/composed/one_block  gates/composed/slices  gates/composed/serial
The model's state classes are fresh (round 0), phase_one (0 < round < dim), phase_change (round = dim), phase_two (dim < round < 2 dim),
awaiting_finish (round = 2 dim) and exhausted.  OPS lists the operations; LEGAL says in which state classes each is drawn; every operation
carries the outcome the model expects: for a successful call the proof it belongs to (an ATTEMPT: a layer's inputs and a matrix of challenges,
begun by init, reset or next) and the round it answers, for a refused call the status and the head of the text, and after it the state is
what it was.  The expected VALUES come from the three walks -- Walk (tests/test_gpu_gkr_batch_rounds.py), Walk2 (tests/gkr_two_point_cases.py),
WalkG (tests/gkr_gates_cases.py) -- run over each attempt's inputs and the challenges the model handed out (oracle(), at the end); nothing of
the library under test feeds them.

STEERING.  Every choice comes from a splitmix64 stream of the seed.  A draw prefers (state class, operation) and (configuration, operation)
pairs the sequence has not made yet, most of all the pairs this seed WANTS -- a fifth of all pairs, a function of the seed, the handle and
the pair alone: for handle 0 a residue class that runs through all five over the seeds of one configuration, for handle 1 a hash --, so that
a list of seeds spreads over the pairs; where nothing wanted is left in a state the handle moves on (a round, finish, or -- exhausted -- a
reset or next).  A sequence is 56 operations, and 3 dim more for every handle of dim 10 or 11, whose proofs are 2 dim rounds long.  tests/test_gkr_handle_sequences_host.py states what the committed SEEDS must reach.

    python -m tests.gkr_handle_sequences SEED        prints the sequence readably"""
import functools
import os
import re
import sys

import numpy as np

from oracle import cref
from tests import gkr_gates_cases as K
from tests import gkr_two_point_cases as K2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = cref.P
P_LIMBS = np.array([(P >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)  # p itself: the smallest non-canonical pattern
HDR = open(os.path.join(ROOT, "include", "sumcheck_hip.h")).read()
STATUS = {name: int(v) for name, v in re.findall(r"\b(SC_OK|SC_ERR_[A-Z_]+) = (\d+)", HDR)}  # the header's enum, by its text
MAX_NNZ_PER_CELL = K.MAX_NNZ_PER_CELL

# The committed list: 0 .. 41 are every ordered pair of configurations (handle 0's is seed % 7), 83 reaches the three pairs they leave.
# tests/test_gkr_handle_sequences_host.py asserts what the list reaches, and a hash of every sequence's text.
SEEDS = tuple(range(42)) + (83,)

# ---- the configurations ------------------------------------------------------------------------------------------------------------------
SMALL, BIG = (1, 2, 3, 5), (10, 11)
R1, RS, RSER = "batch.gkr_rounds_one_block", "batch.gkr_rounds_slices", "batch.gkr_rounds_serial"
G1, GC, NEXT, TWO = K.ONE_BLOCK, K.COMPOSED, "batch.gkr_next_layer", "batch.gkr_two_point"
HANDLE_COUNTERS = (R1, RS, RSER, G1, GC, NEXT, TWO)


def _pol(batch, slices, fused):
    return {"batch": batch, "batch_slices": slices, "gkr_gates_fused": fused}


# name -> kind, class (work areas / the serial plan underneath), the ways to build it (dims, policies), the counters a round call moves
CONFIGS = {
    "mul/one_block": ("mul", "work", [(SMALL, _pol(2, 0, 1))], (R1,)),
    "mul/slices": ("mul", "work", [(BIG, _pol(2, 1, 1))], (RS,)),
    "mul/serial": ("mul", "serial", [(SMALL, _pol(0, 0, 1)), ((10,), _pol(2, 0, 1)), (SMALL, _pol(0, 0, 1))], (RSER,)),
    "gates/one_block": ("gates", "work", [(SMALL, _pol(2, 0, 1))], (G1,)),
    "gates/composed/one_block": ("gates", "work", [(SMALL, _pol(2, 0, 0))], (GC, R1)),
    "gates/composed/slices": ("gates", "work", [(BIG, _pol(2, 1, 1))], (GC, RS)),
    "gates/composed/serial": ("gates", "serial", [((10,), _pol(2, 0, 1)), (SMALL, _pol(0, 0, 1)), (SMALL, _pol(0, 1, 0))], (GC, RSER)),
}
CONFIG_NAMES = tuple(CONFIGS)
WORK_AREA_HANDLES = ("mul/one_block", "mul/slices", "gates/one_block", "gates/composed/one_block", "gates/composed/slices")  # a list beyond 64 x 2^dim is refused
COUNTS_NEXT = ("mul/one_block", "mul/slices", "gates/composed/one_block", "gates/composed/slices")  # batch.gkr_next_layer: a (inner) handle with work areas
COUNTS_TWO = tuple(c for c in CONFIG_NAMES if c != "gates/one_block")  # batch.gkr_two_point: sc_gkr_two_point_* ran, the handle's own or the inner one's

# ---- states and operations ---------------------------------------------------------------------------------------------------------------
STATES = ("fresh", "phase_one", "phase_change", "phase_two", "awaiting_finish", "exhausted")
_ANY = frozenset(STATES)
_RUNNING = frozenset(STATES[:4])
_CHALLENGED = frozenset(STATES[1:4])
LEGAL = {
    "round": _RUNNING, "round_shared": _CHALLENGED,
    "finish": {"awaiting_finish"},                                     # (outputs: both, uv alone, the final values alone, neither -- in turn)
    "state": _ANY, "reset": _ANY,
    "next_kept_one": _ANY, "next_kept_two": _ANY, "next_new_one": _ANY, "next_new_two": _ANY,
    # refused calls: the header's status, and the handle stays where it was
    "ref_first_has_msg": {"fresh"},                                    # a challenge on call 0
    "ref_missing_msg": _CHALLENGED | {"awaiting_finish"},              # no challenge on a later call
    "ref_round_after_end": {"awaiting_finish", "exhausted"},           # a round after 2 dim
    "ref_bad_challenge": _CHALLENGED | {"awaiting_finish"},            # a non-canonical challenge for one instance (awaiting_finish: handed to finish)
    "ref_finish_early": _RUNNING | {"exhausted"},                      # finish before 2 dim rounds (exhausted: a second finish)
    "ref_other_next": _ANY,                                            # the other family's next
    "ref_mixed_wiring": _ANY,                                          # some wiring arguments NULL, some given
    "ref_bad_point": _ANY,                                             # a non-canonical g, g2 or coefficient
    "ref_over_limit": _ANY,                                            # (handles with work areas) a new list of 64 x 2^dim + 1 entries
    "ref_flags": _ANY,                                                 # SC_TABLES_ON_DEVICE differing from init's
    "ref_overflow": _ANY,                                              # new wiring beyond the bytes reserved at init
    # the environment between handle calls: the handle must go on with the same bits
    "env_policies": _ANY, "env_release": _ANY, "env_oneshot": _ANY, "env_other_round": _ANY,
}
OPS = tuple(LEGAL)
ADVANCING = ("round", "round_shared", "finish")
FINISH_OUTPUTS = ("both", "uv", "final", "none")
REFUSED = tuple(op for op in OPS if op.startswith("ref_"))
ONESHOTS = ("prove", "prove_batch", "evaluate_layers", "evaluate_layers_gates", "evaluate_subclaims", "ml_prove_batch")
REFUSAL_STATUS = {"ref_first_has_msg": "SC_ERR_FIRST_ROUND_HAS_MSG", "ref_missing_msg": "SC_ERR_MISSING_MSG", "ref_round_after_end": "SC_ERR_NOT_ACTIVE",
                  "ref_bad_challenge": "SC_ERR_BAD_ARG", "ref_finish_early": "SC_ERR_NOT_ACTIVE", "ref_other_next": "SC_ERR_BAD_ARG", "ref_mixed_wiring": "SC_ERR_BAD_ARG",
                  "ref_bad_point": "SC_ERR_BAD_ARG", "ref_over_limit": "SC_ERR_BAD_ARG", "ref_flags": "SC_ERR_BAD_ARG", "ref_overflow": "SC_ERR_BAD_ARG"}


def legal(op, state, config):
    return state in LEGAL[op] and (op != "ref_over_limit" or config in WORK_AREA_HANDLES)


def legal_pairs(cls):
    """every (state class, operation) pair that is legal on some configuration of the class"""
    return [(s, op) for s in STATES for op in OPS if any(legal(op, s, c) for c in CONFIG_NAMES if CONFIGS[c][1] == cls)]


def state_class(rnd, dim, exhausted):
    if exhausted:
        return "exhausted"
    return "fresh" if rnd == 0 else "phase_one" if rnd < dim else "phase_change" if rnd == dim else "phase_two" if rnd < 2 * dim else "awaiting_finish"


# ---- the only source of choice -----------------------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def _mix(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


class Det:
    """splitmix64 over the seed"""

    def __init__(self, seed):
        self.s = _mix(seed)

    def below(self, k):
        self.s = (self.s + 0x9E3779B97F4A7C15) & _M64
        return _mix(self.s) % k

    def pick(self, seq):
        return seq[self.below(len(seq))]


def wanted(seed, h, state, op):
    """the pairs a seed's handle goes for first: about a fifth of all, a function of (seed, handle, pair) alone"""
    k = STATES.index(state) * len(OPS) + OPS.index(op)
    if h == 0:  # handle 0's configuration is seed % 7: over five seeds of one configuration the residues 3 j + c run through all of 0 .. 4
        return (k + seed // 7 * 3 + seed % 7) % 5 == 0
    return _mix(_mix(seed) ^ k) % 5 == 0


# ---- what a sequence is made of ------------------------------------------------------------------------------------------------------------
class Spec:
    """one handle: the configuration and how it is built, the shape, where the inputs live, the init layer"""

    def __init__(self, config, dim, n, pol, device, two_point, shared, seed):
        self.config, self.dim, self.n, self.pol, self.device, self.two_point, self.shared, self.seed = config, dim, n, pol, device, two_point, shared, seed
        self.kind, self.cls, _, self.round_counters = CONFIGS[config]

    def text(self):
        pol = " ".join(f"{k}={v}" for k, v in self.pol.items())
        return (f"{self.config} dim={self.dim} n={self.n} {'device' if self.device else 'host'} init={'two' if self.two_point else 'one'}-point"
                f"{' shared-wiring' if self.shared else ''} [{pol}]")

    def other_policies(self):
        """values other than those the handle was built under"""
        return {"batch": 0 if self.pol["batch"] else 2, "batch_slices": 1 - self.pol["batch_slices"], "gkr_gates_fused": 1 - self.pol["gkr_gates_fused"]}


class Layer:
    """a layer's inputs by their seeds: wseed and nnz describe the wiring (kept wiring: the former layer's), seed the tables and points.
    nnz: per instance (mul handle) or a pair of such lists (gates handle: mul, add)"""

    def __init__(self, seed, wseed, nnz, two_point):
        self.seed, self.wseed, self.nnz, self.two_point = seed, wseed, nnz, two_point


class Attempt:
    """a proof from round 0: a layer and the challenges the model hands out ((2 dim, n, 4); a shared position holds instance 0's for all)"""

    def __init__(self, layer, chal_seed):
        self.layer, self.chal_seed, self.shared = layer, chal_seed, set()


def ragged(n, dim, k):
    """per instance: none at all, one, three per cell, just over half a cell each, two per cell; a lone instance: three per cell"""
    N = 1 << dim
    return [3 * N - k % 2] if n == 1 else [[0, 1, 3 * N, N // 2 + 1, 2 * N][(i + k) % 5] for i in range(n)]


def _lists(spec, wseed, nnz, step):
    """n (indices, values) pairs with repeated indices; shared wiring: the last instance holds instance 0's arrays"""
    out = [K.wiring(spec.dim, wseed + 31 * i + step, nnz[i]) for i in range(spec.n)]
    if spec.shared:
        out[-1] = out[0]
    return out


def layer_insts(spec, layer):
    """the layer's instances as host arrays: (idx, vals, f2, f3, g[, g2, coef]) for a mul handle, K.Inst for a gates handle"""
    dim, N, s = spec.dim, 1 << spec.dim, layer.seed
    tabs = [(cref.synth_table(s + 7919 * i, 2, N), cref.synth_table(s + 7919 * i, 3, N), cref.synth_table(s + 7919 * i, 4, dim)) for i in range(spec.n)]
    second = [(cref.synth_table(s + 7919 * i, 5, dim), cref.synth_table(s + 7919 * i, 6, 2)) if layer.two_point else () for i in range(spec.n)]
    if spec.kind == "mul":
        f1 = _lists(spec, layer.wseed, layer.nnz, 0)
        return [f1[i] + tabs[i] + second[i] for i in range(spec.n)]
    muls, adds = _lists(spec, layer.wseed, layer.nnz[0], 0), _lists(spec, layer.wseed, layer.nnz[1], 17)
    return [K.Inst(muls[i], adds[i], *tabs[i], *second[i]) for i in range(spec.n)]


def shared_nnz(spec, nnz):
    nnz = list(nnz)
    if spec.shared:
        nnz[-1] = nnz[0]
    return nnz


def attempt_challenges(spec, attempt):
    dim, n = spec.dim, spec.n
    chal = cref.synth_table(attempt.chal_seed, 77, 2 * dim * n).reshape(2 * dim, n, 4).copy()
    if n > 1:  # one instance's challenges run through 0, 1 and p - 1
        for j in range(2 * dim):
            chal[j, n // 2] = K.EDGE[j % 3]
    for j in attempt.shared:
        chal[j, :] = chal[j, 0]
    chal.setflags(write=False)
    return chal


class Op:
    def __init__(self, h, op, state, rnd, attempt, **params):
        self.h, self.op, self.state, self.round, self.attempt, self.params = h, op, state, rnd, attempt, params

    def text(self):
        p = []
        for k, v in self.params.items():
            if isinstance(v, Layer):
                v = f"layer(seed={v.seed} wseed={v.wseed} nnz={v.nnz} {'two' if v.two_point else 'one'}-point)"
            elif isinstance(v, Op):
                v = f"<h{v.h} {v.state}@{v.round} {v.op}>"
            p.append(f"{k}={v}")
        return f"h{self.h} {self.state}@{self.round} {self.op}" + (" " + " ".join(p) if p else "")


class _Handle:
    """the model's state of one handle"""

    def __init__(self, spec, layer, attempt):
        self.spec, self.round, self.exhausted, self.layer, self.init_nnz = spec, 0, False, layer, layer.nnz
        self.attempts = [attempt]
        self.pending = set()  # refusal kinds since the last successful round of this proof

    @property
    def state(self):
        return state_class(self.round, self.spec.dim, self.exhausted)


class Sequence:
    def __init__(self, seed, n_ops=None):
        self.seed = seed
        d = Det(seed)
        a = CONFIG_NAMES[seed % 7]
        b = CONFIG_NAMES[(seed % 7 + 1 + (seed // 7) % 6) % 7]
        self.specs = [self._spec(d, c, h) for h, c in enumerate((a, b))]
        self.handles = []
        for h, spec in enumerate(self.specs):
            k = d.below(5)
            nnz = shared_nnz(spec, ragged(spec.n, spec.dim, k)) if spec.kind == "mul" else (shared_nnz(spec, ragged(spec.n, spec.dim, k)), shared_nnz(spec, ragged(spec.n, spec.dim, k + 1)))
            layer = Layer(spec.seed, spec.seed + 1, nnz, spec.two_point)
            self.handles.append(_Handle(spec, layer, Attempt(layer, spec.seed + 2)))
        self.ops, self.reached, self.confirmed = [], set(), set()  # reached: (state, op, class, config); confirmed: refusal kinds a successful round of the same proof followed
        self._seen_s, self._seen_c, self._fresh, self._finishes = set(), set(), 1000 * seed + 100, 0
        if n_ops is None:
            n_ops = 56 + sum(3 * s.dim for s in self.specs if s.dim >= 10)
        while len(self.ops) < n_ops:
            self._draw(d)

    def _spec(self, d, config, h):
        dims, pol = d.pick(CONFIGS[config][2])
        dim = d.pick(dims)
        n = d.pick((1, 2, 3, 5))
        return Spec(config, dim, n, pol, device=bool(d.below(2)), two_point=bool(d.below(2)), shared=n > 1 and d.below(3) == 0, seed=1000 * self.seed + 10 * h + 500)

    def _new_seed(self):
        self._fresh += 3
        return self._fresh

    # ---- one draw ----
    def _score(self, h, op):
        H = self.handles[h]
        s, spec = H.state, H.spec
        sc = 0
        unseen = (s, op, spec.cls) not in self._seen_s
        sc += 4 * unseen + 3 * ((spec.config, op) not in self._seen_c)
        if unseen and wanted(self.seed, h, s, op):
            sc += 10 - 2 * h
        left = any(legal(o, s, spec.config) and (s, o, spec.cls) not in self._seen_s and wanted(self.seed, h, s, o) for o in OPS if o not in ADVANCING)
        if op in ADVANCING:
            sc += 2 + (0 if left else 8) + (6 if H.pending - self.confirmed else 0)
        if s == "exhausted" and not left and (op == "reset" or op.startswith("next_")):
            sc += 8
        return sc

    def _draw(self, d):
        cands = [(h, op) for h in (0, 1) for op in OPS if legal(op, self.handles[h].state, self.handles[h].spec.config)]
        best = max(self._score(h, op) for h, op in cands)
        h, op = d.pick([c for c in cands if self._score(*c) == best])
        self.ops.append(self._make(d, h, op))

    def _mark(self, o):
        spec = self.specs[o.h]
        self._seen_s.add((o.state, o.op, spec.cls))
        self._seen_c.add((spec.config, o.op))
        self.reached.add((o.state, o.op, spec.cls, spec.config))

    def _make(self, d, h, op, nested=False):
        H = self.handles[h]
        spec, dim, n = H.spec, H.spec.dim, H.spec.n
        o = Op(h, op, H.state, H.round, len(H.attempts) - 1)
        self._mark(o)
        p = o.params
        if op in ("round", "round_shared"):
            if op == "round_shared":
                H.attempts[-1].shared.add(H.round - 1)
            H.round += 1
        elif op == "finish":
            p["outputs"] = "both" if nested else FINISH_OUTPUTS[(self.seed + self._finishes) % 4]
            self._finishes += not nested
            p["shared"] = d.below(3) == 0
            if p["shared"]:
                H.attempts[-1].shared.add(2 * dim - 1)
            H.exhausted = True
        if op in ADVANCING:
            self.confirmed |= H.pending
            H.pending = set()
        elif op == "reset":
            self._restart(H, H.layer)
        elif op.startswith("next_"):
            two, new = op.endswith("_two"), "_new_" in op
            if new:  # per instance no more non-zeros than init's, in init's pattern of repeated pointers
                k = d.below(3)
                shrink = lambda nnz: shared_nnz(spec, [[0, a // 2, a][(i + k) % 3] for i, a in enumerate(nnz)])
                nnz = shrink(H.init_nnz) if spec.kind == "mul" else (shrink(H.init_nnz[0]), shrink(H.init_nnz[1]))
                layer = Layer(self._new_seed(), self._new_seed(), nnz, two)
            else:
                layer = Layer(self._new_seed(), H.layer.wseed, H.layer.nnz, two)
            p["layer"] = layer
            self._restart(H, layer)
        elif op in REFUSED:
            if H.round < 2 * dim or H.state == "awaiting_finish":
                H.pending.add(op)
            if op in ("ref_bad_challenge", "ref_bad_point", "ref_over_limit"):
                p["instance"] = d.below(n)
            if op == "ref_bad_point":
                p["which"] = d.pick(("g", "g2", "coef"))
            if op == "ref_over_limit" and spec.kind == "gates":
                p["which"] = d.pick(("mul", "add"))
            if op in ("ref_over_limit", "ref_overflow", "ref_bad_point", "ref_other_next", "ref_flags", "ref_mixed_wiring"):
                p["seed"] = self._new_seed()
            if op == "ref_mixed_wiring":
                p["hole"] = d.below(3 if spec.kind == "mul" else 6)
        elif op == "env_oneshot":
            p["which"], p["seed"] = d.pick(ONESHOTS), self._new_seed()
            p["dim"] = d.pick([x for x in (2, 3, 4) if x not in (self.specs[0].dim, self.specs[1].dim)])
        elif op == "env_other_round":  # one successful step of the other handle: a round, or what its state leaves
            G = self.handles[1 - h]
            step = {"awaiting_finish": "finish", "exhausted": "reset"}.get(G.state, "round")
            p["step"] = self._make(d, 1 - h, step, nested=True)
        return o

    def _restart(self, H, layer):
        H.layer, H.round, H.exhausted, H.pending = layer, 0, False, set()
        H.attempts.append(Attempt(layer, self._new_seed()))

    # ---- what a refused call answers ----
    def refusal(self, o):
        """(status name, head of sc_last_error())"""
        spec = self.specs[o.h]
        p, gates, composed = o.params, spec.kind == "gates", spec.config.startswith("gates/composed")
        inner = "composed plan (inner instances 3 i + k): " if composed else ""
        limit = MAX_NNZ_PER_CELL << spec.dim
        first = lambda i: 0 if spec.shared and i == spec.n - 1 else i  # the lowest instance that holds instance i's wiring
        text = {
            "ref_first_has_msg": "first round should be prover first.",
            "ref_missing_msg": "verifier message is empty",
            "ref_round_after_end": "Prover is not active",
            "ref_bad_challenge": f"instance {p.get('instance')}: challenge is not canonical",
            "ref_finish_early": "finish needs a prover that has answered its last round",
            "ref_other_next": "the handle was built by sc_gkr_gates_init_batch" if gates else "the handle was not built by sc_gkr_gates_init_batch",
            "ref_mixed_wiring": "mul_idx, mul_vals, mul_nnz, add_idx, add_vals and add_nnz come together" if gates else "f1_idx, f1_vals and nnz come together",
            "ref_flags": "flags: the handle was built over ",  # (device or host: where the replay put the inputs)
            "ref_overflow": inner + "the layer's distinct arrays take ",
        }.get(o.op)
        if o.op == "ref_bad_point":
            i = p["instance"]
            text = {"g": f"instance {i}: g[0] is not a canonical field element", "g2": f"instance {i}: g2 is not canonical", "coef": f"instance {i}: coefficient is not canonical"}[p["which"]]
        if o.op == "ref_over_limit":
            i = first(p["instance"])
            if not gates:
                text = f"instance {i}: nnz {limit + 1} "
            elif composed:
                text = inner + f"instance {3 * i + (p['which'] == 'add')}: nnz {limit + 1} "
            else:
                text = f"instance {i}: {p['which']} nnz {limit + 1} is beyond the limit of plan batch.gkr_gates_one_block"
        return REFUSAL_STATUS[o.op], text

    # ---- the plan counters a successful call moves (every other batch.gkr_* counter stays; gkr.* only under a serial plan) ----
    def counters(self, o):
        spec = self.specs[o.h]
        if o.op in ("round", "round_shared"):
            return {c: 1 for c in spec.round_counters}
        if o.op.startswith("next_"):
            return {c: 1 for c, on in ((NEXT, spec.config in COUNTS_NEXT), (TWO, o.op.endswith("_two") and spec.config in COUNTS_TWO)) if on}
        return {}

    def init_counters(self, h):
        spec = self.specs[h]
        return {TWO: 1} if spec.two_point and spec.config in COUNTS_TWO else {}

    def text(self):
        lines = [f"seed {self.seed}"] + [f"handle {h}: {s.text()} nnz={self.handles[h].init_nnz}" for h, s in enumerate(self.specs)]
        return "\n".join(lines + [f"{k:02d} {o.text()}" for k, o in enumerate(self.ops)])


@functools.lru_cache(maxsize=None)
def sequence(seed):
    return Sequence(seed)


# ---- the expected values: the three walks over every attempt ---------------------------------------------------------------------------------
class Proof:
    """one attempt's inputs, challenges and walks: msgs(t) (n, 3, 4), uv (n, 2, dim, 4), final (n, 3, 4), tables(i, round) on a mul handle"""

    def __init__(self, spec, attempt):
        self.insts, self.chal = layer_insts(spec, attempt.layer), attempt_challenges(spec, attempt)
        dim, n = spec.dim, spec.n
        per = [np.ascontiguousarray(self.chal[:, i]) for i in range(n)]
        rounds = tuple(range(1, 2 * dim + 1))
        if spec.kind == "gates":
            self.walks = [K.WalkG(inst, per[i]) for i, inst in enumerate(self.insts)]
        elif attempt.layer.two_point:
            self.walks = [K2.Walk2(inst, dim, per[i], rounds) for i, inst in enumerate(self.insts)]
        else:
            from tests.test_gpu_gkr_batch_rounds import Walk  # (the module holds GPU tests: imported only where values are wanted)
            self.walks = [Walk(inst, dim, per[i], rounds) for i, inst in enumerate(self.insts)]
        self.uv = np.ascontiguousarray(np.transpose(self.chal, (1, 0, 2)).reshape(n, 2, dim, 4))
        self.final = np.stack([w.final for w in self.walks])

    def msgs(self, t):
        return np.stack([w.msgs[t] for w in self.walks])

    def tables(self, i, rnd):
        """the current phase's two tables after `rnd` round calls: round 0 holds what round 1 holds (nothing is bound before the first challenge)"""
        return self.walks[i].states[max(rnd, 1)]


@functools.lru_cache(maxsize=None)
def oracle(seed):
    """[handle][attempt] -> Proof, for the attempts that some operation asks a value of; shared by every variant of a seed's case"""
    seq = sequence(seed)
    used = {(o.h, o.attempt) for top in seq.ops for o in (top, top.params.get("step")) if o is not None and (o.op in ADVANCING or o.op == "state")}
    return {key: Proof(seq.specs[key[0]], seq.handles[key[0]].attempts[key[1]]) for key in sorted(used)}


if __name__ == "__main__":
    for arg in sys.argv[1:] or ["0"]:
        print(sequence(int(arg)).text())
