"""CPU tests of tests/gkr_handle_sequences.py, the generator of call sequences for the GKR batch handle and its model: what the committed seeds
reach (conditions, not measurements), that no sequence asks for an illegal successful call (re-derived here from the printed operations
alone), that every sequence's text is what it was when it was committed, that the statuses are the header's, and that the walks over a
sequence's attempts are consistent sumchecks under the challenges the model handed out.  The library's answers are
tests/test_gpu_gkr_handle_sequences.py's."""
import glob
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import cref
from sumcheck_amd import _lib
from tests import gkr_handle_sequences as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("work", "serial")

# sha256 of each committed seed's printed sequence, first 16 digits: a change to the generator shows here
TEXT_HASHES = {
    0: "c07069ac9a585127",
    1: "3e6e94f2df634cf2",
    2: "1d2744059d05b80c",
    3: "e4c4394c3737913a",
    4: "5ab92dde284f60ac",
    5: "412afe0a26b993e1",
    6: "871a680ac16cea95",
    7: "cfca35f360539ea6",
    8: "3a1de83f8691cfd4",
    9: "ffe93d650f02fdf4",
    10: "1fb1d898a059a68a",
    11: "e657bf214ff39350",
    12: "f4238be7da594387",
    13: "fa490ff9fd6f9fcb",
    14: "54a8932db8e2742e",
    15: "3b00e8cf92310ae1",
    16: "fdc107609f1ea3ec",
    17: "47a6a3abe067702d",
    18: "7ffd31a8cfc3163d",
    19: "ecc253abad70501d",
    20: "4d5eeb3a06af597d",
    21: "4d45cc470dba542c",
    22: "d36440e4e8ca84d9",
    23: "d0070667dc891ba9",
    24: "3c4ba109e18a7e59",
    25: "e0f6f1c568b6445f",
    26: "9e05ae6b99d9e7ef",
    27: "b1f30bb36149fd79",
    28: "6fb0a37e15d2f457",
    29: "9940a5d5865e03c5",
    30: "c141a8c4c8ba6f5c",
    31: "177767792c3f658e",
    32: "a657082cd6e13e21",
    33: "1cd432765ca52dc6",
    34: "6246d9e66bdc8970",
    35: "f983391dbe557326",
    36: "0d9fbed78f707529",
    37: "d01f2fb812b5c3ab",
    38: "ef132cd2ced35058",
    39: "d67e31f479b04bc1",
    40: "ab1e1ec2a668c379",
    41: "2ab549ed37475adc",
    83: "e57d70d61f9dcea6",
}


def _all():
    return [S.sequence(seed) for seed in S.SEEDS]


def _flat(seq):
    """every operation with the nested step of env_other_round behind it"""
    for o in seq.ops:
        yield o
        if "step" in o.params:
            yield o.params["step"]


# ---- what the committed seeds reach ----------------------------------------------------------------------------------------------------------
def test_every_legal_state_and_operation_is_reached_on_a_work_area_and_on_a_serial_configuration():
    reached = set().union(*[q.reached for q in _all()])
    for cls in CLASSES:
        have = {(state, op) for state, op, c, _ in reached if c == cls}
        missing = [p for p in S.legal_pairs(cls) if p not in have]
        assert not missing, (cls, missing)
    assert len(S.legal_pairs("work")) == len(S.legal_pairs("serial")) + len(S.STATES), "ref_over_limit, in every state, is a work-area handle's"
    assert {s for s, _ in S.legal_pairs("work")} == set(S.STATES) and {op for _, op in S.legal_pairs("serial")} == set(S.OPS) - {"ref_over_limit"}


def test_every_configuration_meets_every_operation():
    reached = set().union(*[q.reached for q in _all()])
    have = {(config, op) for _, op, _, config in reached}
    missing = [(c, op) for c in S.CONFIG_NAMES for op in S.OPS if (op != "ref_over_limit" or c in S.WORK_AREA_HANDLES) and (c, op) not in have]
    assert not missing, missing
    assert {q.specs[0].config for q in _all()} == set(S.CONFIG_NAMES) and all(q.specs[0].config != q.specs[1].config for q in _all())


def test_every_refused_call_is_followed_by_a_successful_round_of_the_same_proof():
    """recomputed from the operations: a refusal counts once a later round (awaiting finish: finish, the one call the proof has left) of the same
    handle answers before a reset or next begins another proof"""
    confirmed = set()
    for q in _all():
        pending = [set(), set()]
        for o in _flat(q):
            if o.op in S.REFUSED and o.state != "exhausted":
                pending[o.h].add(o.op)
            elif o.op in S.ADVANCING:
                confirmed |= pending[o.h]
                pending[o.h] = set()
            elif o.op == "reset" or o.op.startswith("next_"):
                pending[o.h] = set()
        assert confirmed >= q.confirmed
    assert confirmed == set(S.REFUSED), sorted(set(S.REFUSED) - confirmed)
    in_a_round = {o.op for q in _all() for o in _flat(q) if o.op in S.REFUSED and o.state in ("fresh", "phase_one", "phase_change", "phase_two")}
    assert in_a_round == set(S.REFUSED) - {"ref_round_after_end"}, "all but the round after 2 dim happen where a round follows"


def test_finish_is_called_with_and_without_each_output_on_both_kinds_and_both_classes():
    have = {(q.specs[o.h].kind, q.specs[o.h].cls, o.params["outputs"]) for q in _all() for o in q.ops if o.op == "finish"}
    assert have == {(k, c, v) for k in ("mul", "gates") for c in CLASSES for v in S.FINISH_OUTPUTS}
    assert {o.params["shared"] for q in _all() for o in q.ops if o.op == "finish"} == {True, False}


def test_the_shapes_and_forms_the_issue_names_are_all_drawn():
    specs = [s for q in _all() for s in q.specs]
    assert {s.dim for s in specs} == {1, 2, 3, 5, 10, 11} and {s.n for s in specs} == {1, 2, 3, 5}
    assert {(s.kind, s.device) for s in specs} == {(k, d) for k in ("mul", "gates") for d in (True, False)}
    assert {s.two_point for s in specs} == {True, False} and {s.shared for s in specs} == {True, False}
    assert all(s.dim <= 11 and s.n <= 5 for s in specs)
    assert any(0 in (q.handles[h].init_nnz if s.kind == "mul" else q.handles[h].init_nnz[0]) for q in _all() for h, s in enumerate(q.specs)), "an empty list"
    for config in S.CONFIG_NAMES:  # every way of building a configuration
        built = {tuple(sorted(s.pol.items())) for s in specs if s.config == config}
        assert built == {tuple(sorted(pol.items())) for _, pol in S.CONFIGS[config][2]}, config
    assert {o.params["which"] for q in _all() for o in q.ops if o.op == "env_oneshot"} == set(S.ONESHOTS)
    assert {o.params["which"] for q in _all() for o in q.ops if o.op == "ref_bad_point"} == {"g", "g2", "coef"}


# ---- no illegal successful call ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", S.SEEDS)
def test_no_sequence_asks_for_an_illegal_successful_call(seed):
    """the handle's rules, written out again: a round needs round < 2 dim and no finish behind it, the first takes no challenge and every later
    one takes one; finish needs exactly 2 dim rounds; new wiring is no longer than init's.  The state the generator printed is the one
    derived here"""
    q = S.sequence(seed)
    rnd, done, att = [0, 0], [False, False], [0, 0]
    for o in _flat(q):
        dim, h = q.specs[o.h].dim, o.h
        assert (o.round, o.attempt) == (rnd[h], att[h]) and o.state == S.state_class(rnd[h], dim, done[h]), o.text()
        assert S.legal(o.op, o.state, q.specs[h].config), o.text()
        if o.op == "round":
            assert not done[h] and rnd[h] < 2 * dim
            rnd[h] += 1
        elif o.op == "round_shared":
            assert not done[h] and 0 < rnd[h] < 2 * dim
            rnd[h] += 1
        elif o.op == "finish":
            assert not done[h] and rnd[h] == 2 * dim
            done[h] = True
        elif o.op == "reset" or o.op.startswith("next_"):
            rnd[h], done[h], att[h] = 0, False, att[h] + 1
            if "_new_" in o.op:
                init, new = q.handles[h].init_nnz, o.params["layer"].nnz
                pairs = zip(init, new) if q.specs[h].kind == "mul" else list(zip(init[0], new[0])) + list(zip(init[1], new[1]))
                assert all(b <= a for a, b in pairs), o.text()
            if "_kept_" in o.op:
                assert o.params["layer"].nnz == q.handles[h].attempts[att[h] - 1].layer.nnz and o.params["layer"].wseed == q.handles[h].attempts[att[h] - 1].layer.wseed
        elif o.op in S.REFUSED:  # a refused call is one the rules above refuse, or an argument error the header names
            if o.op == "ref_first_has_msg":
                assert rnd[h] == 0 and not done[h]
            if o.op == "ref_missing_msg":
                assert rnd[h] > 0 and not done[h]
            if o.op == "ref_round_after_end":
                assert done[h] or rnd[h] == 2 * dim
            if o.op == "ref_finish_early":
                assert done[h] or rnd[h] < 2 * dim
            status, text = q.refusal(o)
            assert status in S.STATUS and text
    assert all(len(q.handles[h].attempts) == att[h] + 1 for h in (0, 1))


# ---- the text, the statuses, the texts -----------------------------------------------------------------------------------------------------------
def test_the_sequence_text_of_every_seed_is_the_committed_one():
    got = {q.seed: hashlib.sha256(q.text().encode()).hexdigest()[:16] for q in _all()}
    assert got == TEXT_HASHES, "\n".join(f"    {s}: \"{h}\"," for s, h in got.items())
    assert S.Sequence(5).text() == S.sequence(5).text(), "a sequence is a function of its seed"
    r = subprocess.run([sys.executable, "-m", "tests.gkr_handle_sequences", "5"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip("\n") == S.sequence(5).text()


def test_the_statuses_are_the_headers_and_the_texts_are_in_the_sources():
    assert S.STATUS == {name: getattr(_lib, name) for name in S.STATUS} and len(S.STATUS) == 9
    assert set(S.REFUSAL_STATUS) == set(S.REFUSED) and set(S.REFUSAL_STATUS.values()) <= set(S.STATUS)
    for name in set(S.REFUSAL_STATUS.values()):  # each is a status the header gives these calls
        assert re.search(name + r"\b", S.HDR.split("typedef struct sc_gkr_batch_prover", 1)[1]) or name == "SC_ERR_NOT_ACTIVE" and "SC_ERR_NOT_ACTIVE after 2 x dim rounds" in S.HDR
    src = "".join(open(f).read() for f in sorted(glob.glob(os.path.join(ROOT, "sumcheck_amd", "csrc", "*.hip"))))
    heads = set()
    for q in _all():
        for o in _flat(q):
            if o.op in S.REFUSED:
                heads.add(re.sub(r"(?<![a-z])\d+", "#", q.refusal(o)[1]))
    assert len(heads) >= len(S.REFUSED)
    fmt = re.sub(r"%(llu|zu|u|s)", "#", src)
    for head in heads:  # with the numbers and names the format strings leave open
        variants = [head, head.replace("mul nnz", "# nnz").replace("add nnz", "# nnz"), head.replace("device arrays", "# arrays").replace("host arrays", "# arrays"),
                        head.replace(": g[", ": #[")]
        parts = [v.split("): ", 1)[-1] if v.startswith("composed plan") else v for v in variants]
        assert any(part.rstrip() in fmt for part in parts) and (not head.startswith("composed plan") or "composed plan (inner instances 3 i + k): " in src), head


# ---- the walks under the model's challenges ----------------------------------------------------------------------------------------------------
def test_the_walks_of_a_sequence_are_consistent_sumchecks_under_the_challenges_handed_out():
    """every message's p(0) + p(1) is the message before it at the challenge the model handed out for it; shared positions hold one challenge"""
    seed = next(s for s in S.SEEDS if all(x.dim <= 3 for x in S.sequence(s).specs) and {x.kind for x in S.sequence(s).specs} == {"mul", "gates"})
    q, proofs = S.sequence(seed), S.oracle(seed)
    assert proofs
    for (h, a), proof in proofs.items():
        spec, attempt = q.specs[h], q.handles[h].attempts[a]
        assert proof.chal.shape == (2 * spec.dim, spec.n, 4) and proof.uv.shape == (spec.n, 2, spec.dim, 4)
        for j in attempt.shared:
            assert all(np.array_equal(proof.chal[j, i], proof.chal[j, 0]) for i in range(spec.n))
        for i in range(spec.n):
            for t in range(1, 2 * spec.dim):
                m = proof.msgs(t)[i]
                assert np.array_equal(cref.fr_binop("add", m[0], m[1]), cref.interpolate_uni_poly(proof.msgs(t - 1)[i], proof.chal[t - 1, i])), (h, a, i, t)
            if spec.kind == "mul":
                assert proof.tables(i, 0).shape == (2, 1 << spec.dim, 4) and proof.tables(i, 2 * spec.dim).shape == (2, 2, 4)
