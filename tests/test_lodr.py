"""LODR without a GPU: the twin (tests/lodr_twin.py) against the twin it extends, its term against the C library's host automaton
(k2hip_ngram_lm_step) bit for bit, the recorded cases of tests/lodr_cases.py (acceptance, gaps, moved streams, no earlier accepted draw),
the score bound against LOGIT_TOL, a known answer on the planted model of tests/kat_model.py, and the rescoring order."""
import numpy as np
import pytest

import lodr_cases as cases
import parity
import rnn_lm_fusion_cases as fc
import rnn_lm_fusion_twin as ft
from lodr_twin import lodr_terms, lodr_total, rescored_order, twin_beam_search
from ngram_twin import TwinLm

f32 = np.float32


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    d = tmp_path_factory.mktemp("lodr")
    oras = {w: fc.make_oracle(d, w)[1] for w in ("tiny", "tiny165")}
    encs, lms = {}, {}

    def enc_of(which, base):
        if (which, base) not in encs:
            e = fc.encode(oras[which], fc.utterances(base))
            encs[(which, base)] = (e,) + cases.lodr_lm(oras[which], e)
        return encs[(which, base)]

    def lm_of(name, seed):
        if (name, seed) not in lms:
            lms[(name, seed)] = fc.make_lm(d, name, seed)
        return lms[(name, seed)]
    return oras, enc_of, lm_of


def same_run(a, b):
    assert (a["ys"], a["ts"]) == (b["ys"], b["ts"]) and f32(a["lp"]).tobytes() == f32(b["lp"]).tobytes()
    assert np.array_equal(a["idx"], b["idx"]) and np.array_equal(a["val"].view(np.uint32), b["val"].view(np.uint32))
    assert np.array_equal(a["gaps"], b["gaps"]) and np.array_equal(a["margins"].view(np.uint32), b["margins"].view(np.uint32))
    assert [(x["tokens"], x["timestamps"], x["score"]) for x in a["alts"]] == [(x["tokens"], x["timestamps"], x["score"]) for x in b["alts"]]


def test_off_is_the_fusion_twin(world):
    """lodr None, lscale 0 and (no neural LM, whatever lodr says): the twin this one extends, to the bit"""
    oras, enc_of, lm_of = world
    base, seed, ls, _, _ = cases.SEEDS[("A", 4)]
    enc, lodr, _ = enc_of("tiny", base)
    _, nlm, _ = lm_of("A", seed)
    for b in range(enc.shape[0]):
        want = ft.twin_beam_search(oras["tiny"], enc[b], 4, nlm=nlm, nscale=cases.SCALE, nbest=cases.NBEST)
        same_run(twin_beam_search(oras["tiny"], enc[b], 4, nlm=nlm, nscale=cases.SCALE, nbest=cases.NBEST), want)
        same_run(twin_beam_search(oras["tiny"], enc[b], 4, nlm=nlm, nscale=cases.SCALE, nbest=cases.NBEST, lodr=lodr, lscale=0.0), want)
        plain = ft.twin_beam_search(oras["tiny"], enc[b], 4, nbest=cases.NBEST)
        same_run(twin_beam_search(oras["tiny"], enc[b], 4, nbest=cases.NBEST, lodr=lodr, lscale=ls), plain)
        same_run(twin_beam_search(oras["tiny"], enc[b], 4, nlm=nlm, nscale=0.0, nbest=cases.NBEST, lodr=lodr, lscale=ls), plain)


def check_record(oras, enc_of, lm_of, name, beam, rec, what=None):
    """a recorded case: accepted, its gap, its moved streams, no accepted draw among the FIRST_CHECKED in front; the terms against the C
    library; the bound.  Returns the runs."""
    from k2transducerasr_amd import NgramLm
    which = cases.OPERATOR[name]
    ora = oras[which]
    base, seed, ls, gap, moved = rec
    extras_of = (lambda e: fc.together_extras(ora, e, what)) if what else (lambda e: {})
    enc, lodr, entries = enc_of(which, base)
    _, nlm, _ = lm_of(name, seed)
    runs, without = cases.run_case(ora, enc, beam, nlm, lodr, ls, extras_of(enc))
    ok, g = fc.accepted(runs)
    assert ok and abs(g - gap) <= 5e-7 * max(1.0, abs(gap) * 1e3), (g, gap)
    assert cases.moved_streams(runs, without) == moved
    order = cases.draws()
    at = order.index((base, seed, ls))
    for b2, s2, l2 in order[max(0, at - cases.FIRST_CHECKED): at]:
        e2, lodr2, _ = enc_of(which, b2)
        assert not fc.accepted(cases.run_case(ora, e2, beam, lm_of(name, s2)[1], lodr2, l2, extras_of(e2))[0])[0], (b2, s2, l2)
    # the terms: k2hip_ngram_lm_step times the scale, bit for bit (the weights are powers of two: scaling entry by entry, as the model
    # does, and scaling the unscaled step give the same float32), and their float32 sum is the rescoring's lodr_i
    clm = NgramLm(entries, ora.vocab_size)
    assert ls in (-0.25, -0.5, -1.0)
    nterms = 0
    for r in runs:
        for a in r["alts"]:
            s, acc = clm.start_state, f32(0)
            assert len(a["dl"]) == len(a["tokens"])
            for tok, term in zip(a["tokens"], a["dl"]):
                s, lp = clm.step(s, tok)
                assert f32(lp * f32(ls)).tobytes() == f32(term).tobytes(), (a["tokens"], tok)
                acc = f32(acc + f32(term))
                nterms += 1
            assert s == a["dst"]
            assert acc.tobytes() == lodr_total(lodr, ls, a["tokens"]).tobytes()
            assert [f32(x).tobytes() for x in lodr_terms(lodr, ls, a["tokens"])] == [f32(x).tobytes() for x in a["dl"]]
    assert nterms > 0
    # the bound
    S, T = cases.case_smax(runs), enc.shape[1]
    nmax = max(len(a["tokens"]) for r in runs for a in r["alts"])
    bound = cases.score_bound(T, nmax, S)
    assert parity.LOGIT_TOL >= 2 * bound, (bound, S, nmax)
    return runs


@pytest.mark.parametrize("name,beam", sorted(cases.SEEDS))
def test_operator_cases(world, name, beam):
    check_record(*world, name, beam, cases.SEEDS[(name, beam)])


@pytest.mark.parametrize("what", sorted(cases.TOGETHER))
def test_together_cases(world, what):
    oras, enc_of, _ = world
    check_record(*world, "A", 4, cases.TOGETHER[what], what)
    if what == "ngram":   # two automata of different sizes, so a swapped state array cannot pass for the right one
        enc, lodr, _ = enc_of("tiny", cases.TOGETHER[what][0])
        tri = fc.together_extras(oras["tiny"], enc, what)["lm"]
        assert tri.N == 3 and lodr.N == 2 and tri.num_states != lodr.num_states and tri.num_arcs != lodr.num_arcs


def test_the_feature_moves_something():
    assert cases.MOVED == sum(v[4] for v in cases.SEEDS.values()) >= 1
    assert any(v[4] > 0 for v in cases.SEEDS.values())


class FlatLm:
    """a neural LM stand-in whose next-token row is uniform: its term is the same for every real token"""

    def __init__(self, V):
        self.q = np.full(V, -np.log(V))

    def start(self):
        return 0, self.q

    def step(self, state, token):
        return state + 1, self.q


# The frames of ngram_twin.KAT_LM_FLIP: t0 offers 5 (1.0) against a slightly better 6 (1.1), t1 offers 7 (3.0), t2 blank (3.0); beam 2.
# Neural LM: flat (every real token earns n' = fl32(0.5 * -log 8)), so two hypotheses of equal length carry the same neural part.
# LODR LM: unigrams of 1, 3, 4, 5, 6, 7 at u = -4 each, the bigram (6, 7) at b = -1 with bow(6) = -0.5; weight -0.5, so the scaled terms
# are u' = +2 and b' = +0.5 (exact in float32): what the source-domain bi-gram finds LIKELY earns less.
#   t0: p(6) = 0.338, p(5) = 0.325: the selection is {6, 5}; both earn n' + u'.  [6] is a LODR state, [5] is not.
#   t1: the selection is the unbiased one, {[6]+7, [5]+7}.  [6, 7] earns the bigram b' = +0.5, [5, 7] the unigram u' = +2: [5, 7] is now
#       ahead by e^1.5 x 0.166 / 0.173 = 4.3 -- the mirror image of KAT_LM_FLIP, where the added bigram (5, 7) does the same.
#   t2: both take blank, as there; final pick [5, 7] instead of [6, 7], no merges on the way, so
#   score = log p(5 | t0) + log p(7 | t1, ctx [0, 5]) + log p(0 | t2, ctx [5, 7]) + 2 n' + u' + u'
KAT_LODR_FLIP = dict(lscale=-0.5, nscale=0.5,
                     entries=[((v,), -4.0, -0.5 if v == 6 else 0.0) for v in (1, 3, 4, 5, 6, 7)] + [((6, 7), -1.0, 0.0)])


def test_kat_lodr_flip(tmp_path):
    from kat_model import frames, write_kat_model
    from ngram_twin import KAT_LM_FLIP, kat_lm_flip_score
    from oracle import Oracle
    p = str(tmp_path / "kat.k2w")
    write_kat_model(p)
    ora = Oracle(p)
    K, D = KAT_LM_FLIP, KAT_LODR_FLIP
    enc = frames(K["rows"])
    nlm, lodr = FlatLm(8), TwinLm(D["entries"], 8)
    fused = twin_beam_search(ora, enc, K["beam"], nlm=nlm, nscale=D["nscale"])
    assert (fused["ys"], fused["ts"]) == K["plain"]          # the flat LM alone moves nothing
    r = twin_beam_search(ora, enc, K["beam"], nlm=nlm, nscale=D["nscale"], lodr=lodr, lscale=D["lscale"])
    assert (r["ys"], r["ts"]) == K["fused"]
    assert [float(x) for x in r["dl"]] == [2.0, 2.0]
    assert [float(x) for x in lodr_terms(lodr, D["lscale"], [6, 7])] == [2.0, 0.5]
    nterm = float(f32(D["nscale"] * -np.log(8.0)))
    # kat_lm_flip_score() = the three acoustic terms + (-2.0) + (-0.5) of its own LM
    want = kat_lm_flip_score() + 2.0 + 0.5 + 2 * nterm + 2.0 + 2.0
    assert abs(r["lp"] - want) < 1e-5, (r["lp"], want)


def test_rescoring_order():
    """lodr_twin.rescored_order against rnn_lm_twin.rescored_order: with zero LODR totals the same order and keys; a LODR total that
    outweighs the neural gain flips two entries; the CTC form does not divide by the length"""
    from rnn_lm_twin import rescored_order as base_order
    scores, lengths, lms = [-3.0, -3.2, -3.1], [3, 4, 3], [-6.0, -4.0, -5.0]
    for ctc in (False, True):
        assert rescored_order(scores, lengths, lms, 0.5, [0.0, 0.0, 0.0], ctc) == base_order(scores, lengths, lms, 0.5, ctc)
    order, keys = rescored_order(scores, lengths, lms, 0.5, [1.0, 0.25, 2.0], False)
    assert order == [2, 1, 0] and keys[2] == pytest.approx((-3.1 - 2.5 + 2.0) / 5)
    order, keys = rescored_order(scores, lengths, lms, 0.5, [1.0, 0.25, 2.0], True)
    assert order == [2, 1, 0] and keys[0] == pytest.approx(-3.0 - 3.0 + 1.0)
    # on a recorded list: the totals are those of the host walk, and the order is stable under exact ties
    lodr = TwinLm(KAT_LODR_FLIP["entries"], 8)
    tot = [float(lodr_total(lodr, -0.5, t)) for t in ([6, 7], [5, 7], [])]
    assert tot == [2.5, 4.0, 0.0]
    order, _ = rescored_order([-1.0, -1.0, -1.0], [2, 2, 0], [0.0, 0.0, 0.0], 0.5, [0.0, 0.0, 0.0], True)
    assert order == [0, 1, 2]
