"""Neural LM shallow fusion without a GPU: the Python twin (tests/rnn_lm_fusion_twin.py) against the twin it extends, against the LM's
own totals, against exhaustive enumeration on a toy problem, and the acceptance of the cases in tests/rnn_lm_fusion_cases.py that
test_rnn_lm_fusion_gpu.py runs the device on."""
import itertools

import numpy as np
import pytest

import ngram_twin
import parity
import rnn_lm_cases as lmc
import rnn_lm_fusion_cases as cases
import torch

from rnn_lm_fusion_twin import FusionLm, Oracle64, twin_batch, twin_beam_search
from rnn_lm_twin import Twin


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    d = tmp_path_factory.mktemp("fusion_cases")
    paths = {w: cases.make_oracle(d, w) for w in ("tiny", "tiny165")}
    oras = {w: po[1] for w, po in paths.items()}
    oras.update({w + "/64": Oracle64(*po) for w, po in paths.items()})
    made = {}

    def encs(which, base, seconds=cases.UTT_SECONDS):
        if (which, base, seconds) not in made:
            made[(which, base, seconds)] = cases.encode(oras[which], cases.utterances(base, seconds))
        return made[(which, base, seconds)]
    return d, oras, encs


def test_scale_zero_is_the_twin_it_extends(world):
    d, oras, encs = world
    _, nlm, _ = cases.make_lm(d, "A", 0)
    enc = encs("tiny", 50)
    for beam in (1, 4):
        for b in range(cases.STREAMS):
            want = ngram_twin.twin_beam_search(oras["tiny"], enc[b], beam)
            for kw in (dict(), dict(nlm=nlm, nscale=0.0)):
                got = twin_beam_search(oras["tiny"], enc[b], beam, **kw)
                assert (got["ys"], got["ts"]) == (want["ys"], want["ts"]) and np.float32(got["lp"]).tobytes() == np.float32(want["lp"]).tobytes()
                for k in ("idx", "val", "n", "margins"):
                    assert np.array_equal(got[k], want[k]), (beam, b, k)


@pytest.mark.parametrize("name,beam", sorted(cases.SEEDS))
def test_operator_cases_are_accepted_and_the_lm_part_is_the_lm_total(world, name, beam):
    """the recorded draw is accepted with the recorded gap and no earlier draw is; for every returned hypothesis the sum of its neural
    terms is scale x the LM twin's total without eos within total_bound(n); and the LM moves something"""
    d, oras, encs = world
    which = cases.OPERATOR[name]
    base, seed, gap = cases.SEEDS[(name, beam)]
    order = cases.draws()
    at = order.index((base, seed))
    for b_, s in order[max(at - cases.FIRST_CHECKED, 0): at + 1]:
        _, nlm, tw = cases.make_lm(d, name, s)
        enc = encs(which, b_)
        runs = twin_batch(oras[which], enc, beam, nlm=nlm, nscale=cases.SCALE, nbest=cases.NBEST)[4]
        ok, g = cases.accepted(runs)
        assert ok == ((b_, s) == (base, seed)), (name, beam, b_, s, g)
    assert abs(g - gap) <= 1e-3 * gap, (g, gap)
    check_score_bound(oras[which], oras[which + "/64"], enc, beam, nlm, runs)
    for r in runs:
        assert r["alts"][0]["tokens"] == r["ys"] and r["alts"][0]["timestamps"] == r["ts"]
        for a in r["alts"]:
            n = len(a["tokens"])
            assert abs(a["nl"] - cases.SCALE * tw.score(a["tokens"], with_eos=False)[0]) <= lmc.total_bound(n), (name, beam, a)
    plain = twin_batch(oras[which], enc, beam, nbest=cases.NBEST)[4]
    if beam >= 2:
        assert any([a["tokens"] for a in p["alts"]] != [a["tokens"] for a in r["alts"]] for p, r in zip(plain, runs)), "the LM moves no list"


def check_score_bound(ora, ora64, enc, beam, nlm, runs, **kw):
    """the float32 twin's own score error per frame against the same search in float64 stays within SCORE_E32, and the acceptance gap is
    at least twice the bound the device's scores are held to"""
    r64 = twin_batch(ora64, enc, beam, nlm=nlm, nscale=cases.SCALE, nbest=cases.NBEST, dtype=torch.float64, **kw)[4]
    T = enc.shape[1]
    for a, b in zip(runs, r64):
        assert [(x["tokens"], x["timestamps"]) for x in a["alts"]] == [(x["tokens"], x["timestamps"]) for x in b["alts"]]
        for x, y in zip(a["alts"], b["alts"]):
            assert abs(x["score"] - y["score"]) <= cases.SCORE_E32 * T, (x["score"], y["score"])
            assert len(x["tokens"]) == 0 or np.abs(x["token_log_probs"] - y["token_log_probs"]).max() <= cases.YP_TOL / 4
    n_max = max(len(a["tokens"]) for r in runs for a in r["alts"])
    assert parity.LOGIT_TOL >= 2 * cases.score_bound(T, n_max), (T, n_max, cases.score_bound(T, n_max))


def test_oracle64_restates_the_oracle(world):
    d, oras, encs = world
    rng = np.random.default_rng(0)
    for w in ("tiny", "tiny165"):
        o, o64 = oras[w], oras[w + "/64"]
        ctx = rng.integers(0, o.vocab_size, size=(16, 2))
        ctx[0] = 0
        e = encs(w, 50)[0][:16]
        assert np.abs(o64.joiner(e, o64.decoder(ctx)) - o.joiner(e, o.decoder(ctx))).max() <= 1e-5


def test_wide_case_record(world):
    """the wide case's utterances are the first 32 seeds from 200 up whose stream has no selection margin below LOGIT_TOL on the twin:
    every recorded stream is clear, every seed passed over is not"""
    from k2transducerasr_amd.synth import synth_utterance
    d, oras, _ = world
    w = cases.WIDE
    assert len(w["utt_seeds"]) == w["B"] and w["utt_seeds"] == sorted(w["utt_seeds"]) and w["utt_seeds"][0] >= 200 and w["tight_streams"] <= 2
    _, nlm, _ = cases.make_lm(d, w["lm"], w["seed"])
    seeds = list(range(200, w["utt_seeds"][-1] + 1))
    enc = cases.encode(oras["tiny"], [synth_utterance(u, w["seconds"]) for u in seeds])
    for u, e in zip(seeds, enc):
        mg = twin_beam_search(oras["tiny"], e, w["beam"], nlm=nlm, nscale=cases.SCALE)["margins"]
        assert (float(mg[:-1].min()) >= parity.LOGIT_TOL) == (u in w["utt_seeds"]), u


class ToyOracle:
    """V = 5 (blank 0, unk 2, real 1, 3, 4): logits = enc frame + a table row of the two-token context"""
    context_size, vocab_size = 2, 5

    def __init__(self, rng):
        self.table = rng.standard_normal((5, 5, 5)).astype(np.float32)

    def decoder(self, ctx):
        return np.asarray(ctx, np.int64)

    def joiner(self, enc, dec):
        return (np.asarray(enc, np.float32) + self.table[dec[:, 0], dec[:, 1]]).astype(np.float32)


def test_brute_force(tmp_path):
    """V = 5, T' = 3 and a beam that never prunes: the twin equals the enumeration of all 125 symbol paths in float64 -- every
    sequence, its merged score with the LM terms, and the pick"""
    from k2transducerasr_amd.synth import write_synthetic_rnn_lm
    scale, T = 0.7, 3
    for seed in range(3):
        rng = np.random.default_rng(seed)
        ora = ToyOracle(rng)
        enc = rng.standard_normal((T, 5)).astype(np.float32)
        nlm = FusionLm(Twin(write_synthetic_rnn_lm(str(tmp_path / f"toy{seed}.k2w"), 5, 8, 32, 2, seed), 2))
        got = twin_beam_search(ora, enc, beam=70, nlm=nlm, nscale=scale, nbest=70)
        states = {(): nlm.start()}
        total = {}
        for path in itertools.product(range(5), repeat=T):
            ys, lp = [], 0.0
            for t, v in enumerate(path):
                ctx = ([0, 0] + ys)[-2:]
                z = enc[t].astype(np.float64) + ora.table[ctx[0], ctx[1]].astype(np.float64)
                lp += z[v] - (z.max() + np.log(np.exp(z - z.max()).sum()))
                if v not in (0, 2):
                    lp += scale * states[tuple(ys)][1][v]
                    ys = ys + [v]
                    if tuple(ys) not in states:
                        states[tuple(ys)] = nlm.step(states[tuple(ys[:-1])][0], v)
            total[tuple(ys)] = np.logaddexp(total.get(tuple(ys), -np.inf), lp)
        assert {tuple(a["tokens"]) for a in got["alts"]} == set(total)
        for a in got["alts"]:
            assert abs(a["score"] - total[tuple(a["tokens"])]) <= 2e-5, (seed, a["tokens"])
        best = max(total, key=lambda k: total[k] / (len(k) + 2))
        assert tuple(got["ys"]) == best, seed


def test_recognizer_case_moves_half_the_streams(world):
    """fusion shows something: on the recognizer case the fused result differs from BOTH the plain search's and the rescored N-best
    list's top entry in at least half of the streams, and the case is accepted"""
    d, oras, encs = world
    rc = cases.RECOGNIZER
    _, nlm, tw = cases.make_lm(d, rc["lm"], rc["seed"])
    views, fused = cases.recognizer_views(oras["tiny"], encs("tiny", rc["base"], cases.REC_SECONDS), nlm, tw, rc["scale"], rc["beam"], rc["nbest"])
    moved = sum(f != p and f != r for p, r, f in views)
    ok, g = cases.accepted(fused)
    assert ok and abs(g - rc["gap"]) <= 1e-3 * rc["gap"], g
    assert moved == rc["moved"] and 2 * moved >= len(views)


@pytest.mark.parametrize("what", sorted(cases.TOGETHER))
def test_together_cases_are_accepted(world, what):
    d, oras, encs = world
    base, seed, gap = cases.TOGETHER[what]
    enc = encs("tiny", base)
    ex = cases.together_extras(oras["tiny"], enc, what)
    _, nlm, _ = cases.make_lm(d, "A", seed)
    kw = dict(lm=ex.get("lm"), scale=ex.get("scale", 0.0), graph=ex.get("graph"), nbest=cases.NBEST)
    runs = twin_batch(oras["tiny"], enc, 4, nlm=nlm, nscale=cases.SCALE, **kw)[4]
    ok, g = cases.accepted(runs)
    assert ok and abs(g - gap) <= 1e-3 * gap, g
    check_score_bound(oras["tiny"], oras["tiny/64"], enc, 4, nlm, runs, lm=ex.get("lm"), scale=ex.get("scale", 0.0), graph=ex.get("graph"))
    # both biases act: the result differs from the neural LM alone and from the other bias alone
    alone = twin_batch(oras["tiny"], enc, 4, nlm=nlm, nscale=cases.SCALE, nbest=cases.NBEST)[4]
    other = twin_batch(oras["tiny"], enc, 4, **kw)[4]
    lists = lambda rs: [[(a["tokens"], round(a["score"], 4)) for a in r["alts"]] for r in rs]   # noqa: E731
    assert lists(runs) != lists(alone) and lists(runs) != lists(other)
