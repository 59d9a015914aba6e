"""Host-side checks of tests/beam_bias_cases.py, the inputs tests/test_beam_bias_ties_gpu.py puts through the biased modified beam
search: the promises and the coverage on every committed draw, the new twin against beam_cases.twin where nothing biases, against the
older restatements on the oracle's operators (hotword_twin / ngram_twin) where something does, and the sensitivity of the cases -- every
deliberately wrong biased search (beam_bias_cases.BIAS_RULES) is told from the reference by at least one committed case per V, so each
of these mistakes in a kernel would fail the device test."""
import functools

import numpy as np
import pytest

import beam_bias_cases as bb
import beam_cases as bc
import hotword_twin
import ngram_twin
from hotword_twin import SCORE, TwinGraph
from ngram_twin import TwinLm


@functools.lru_cache(maxsize=None)
def reference(V, config, case, stream, beam):
    m = bb.cases(V)
    c = next(x for x in m.cases if x.name == case)
    bias = bb.biases(V)[config]
    return bb.twin(m.W, m.b, c.enc[stream], beam, np.float64, bias.graph, bias.lm)


def runs(m):
    return [(c, s, beam) for c in m.cases for s in range(c.enc.shape[0]) for beam in bb.BEAMS]


@pytest.mark.parametrize("V", bb.VS)
def test_promises_and_coverage(V):
    """coverage() on the committed draw: in all four configurations every ordering decision is an exact tie of equally formed scores
    or 10 x the extended bound apart, float32 and float64 alike in tokens, timestamps and order; every bias kind is counted at least
    once at every beam that admits it; the final-order promise holds on three quarters of the resumed test's prefixes."""
    m = bb.cases(V)
    cov = bb.coverage(V)
    for (config, beam), tot in cov.items():
        print(f"V={V} {config} beam={beam}: " + " ".join(f"{k}={v}" for k, v in tot.items() if v))
    for beam in bb.BEAMS:
        assert cov["both", beam]["ties"] >= 40
    worst = max(bb.score_bound(m.W, m.b, reference(V, cf, c.name, s, beam), c.enc.shape[1]) for cf in bb.CONFIGS for c, s, beam in runs(m))
    ok, n = bb.prefix_share(V)
    print(f"V={V}: score bound {worst:.3g}, token log-prob bound {bc.noise_terms(m.W, m.b)[0]:.3g}; {ok} of {n} prefix ends keep the final-order promise")
    assert worst < 1e-3


def test_the_biases_are_what_the_docstring_says():
    for V in bb.VS:
        b = bb.biases(V)
        plant = {c for cols in bc.groups(V).values() for c in cols}
        for which in ("A", "B"):
            ph = bb.phrases(V, which)
            assert all(1 <= len(p) <= 3 and set(p) <= plant - {bc.BLANK, bc.UNK} for p in ph) and {len(p) for p in ph} == {1, 2, 3}
        assert float(b["hw"].graph.c) == SCORE == 1.5 and b["lm"].graph is None and b["hw"].lm is None
        assert b["both"].graph is b["hw"].graph and b["both"].lm is b["lm"].lm is b["bothB"].lm
        lm = TwinLm(b["lm"].entries, V)
        assert lm.N == 3 and lm.start != 0
        for tab in (lm.lp, lm.bo):
            assert all(float(v) * 8 == int(float(v) * 8) for v in tab.values()), "multiples of 1 / 8"
        for tab in (b["lm"].lm.lp, b["lm"].lm.bo):
            assert all(float(v) * 16 == int(float(v) * 16) and abs(float(v)) <= 50 for v in tab.values())
        m = bb.cases(V)
        assert np.array_equal(m.W, bc.build(V).W) and np.array_equal(m.b, bc.build(V).b)
        for c in m.cases:
            assert c.enc.shape == (3, bb.T_FRAMES, bc.J) and c.enc.dtype == np.float32


@pytest.mark.parametrize("V", bb.VS)
def test_without_a_bias_the_twin_is_beam_cases_twin(V):
    """an empty graph and no LM: result for result what beam_cases.twin returns -- on beam_cases' committed frames and on this file's,
    in float64 and float32"""
    m, own = bc.build(V), bb.cases(V)
    empty = TwinGraph([], SCORE, V)
    for enc in [c.enc[s] for mm in (m, own) for c in mm.cases for s in range(c.enc.shape[0])]:
        for beam in bb.BEAMS:
            for dt in (np.float64, np.float32):
                want = bc.twin(m.W, m.b, enc, beam, dt)
                for graph in (None, empty):
                    got = bb.twin(m.W, m.b, enc, beam, dt, graph, None)
                    assert got["order"] == want["order"] and got["smax"] == want["smax"] and got["merges"] == want["merges"]
                    assert got["selected"] == want["selected"]
                    for a, w in zip(got["alts"], want["alts"]):
                        assert (a["tokens"], a["timestamps"], a["score"], a["norm"], a["sym"]) == (w["tokens"], w["timestamps"], w["score"], w["norm"], w["sym"])
                        assert np.array_equal(a["token_log_probs"], w["token_log_probs"])
                    for f, g in zip(got["frames"], want["frames"]):
                        assert np.array_equal(f["idx"], g["idx"]) and np.array_equal(f["val"], g["val"]) and f["merges"] == g["merges"]
                        assert f["n"] == g["n"] and f["sym"] == g["sym"]


@pytest.mark.parametrize("V", bb.VS)
def test_twin_equals_the_older_restatements_on_the_oracle(V, tmp_path):
    """hotword_twin.twin_beam_search / ngram_twin.twin_beam_search run the oracle's decoder and joiner with torch's log_softmax, topk
    and logaddexp in float32: this file's twin at float32 picks the same tokens and timestamps, and both scores lie within the bound
    of the float64 reference -- with the oracle's ONE chain of V additions in the sum of exponentials."""
    from oracle import Oracle
    m = bb.cases(V)
    p = str(tmp_path / f"bias_v{V}.k2w")
    m.write(p)
    ora = Oracle(p)
    worst = 0.0
    try:
        for config, bias in bb.biases(V).items():
            lm = TwinLm(bias.entries, V) if bias.entries else None
            for c, s, beam in runs(m):
                if config == "hw":
                    old = hotword_twin.twin_beam_search(ora, c.enc[s], beam, bias.graph)
                else:
                    old = ngram_twin.twin_beam_search(ora, c.enc[s], beam, lm, bb.SCALE, bias.graph)
                ref = reference(V, config, c.name, s, beam)
                new = bb.twin(m.W, m.b, c.enc[s], beam, np.float32, bias.graph, bias.lm)["alts"][0]
                bound = bb.score_bound(m.W, m.b, ref, c.enc.shape[1], chain=V)
                what = (V, config, c.name, s, beam)
                assert (old["ys"], old["ts"]) == (new["tokens"], new["timestamps"]) == (ref["alts"][0]["tokens"], ref["alts"][0]["timestamps"]), what
                for x in (old["lp"], new["score"]):
                    worst = max(worst, abs(x - ref["alts"][0]["score"]) / bound)
                    assert abs(x - ref["alts"][0]["score"]) <= bound, (what, x, ref["alts"][0]["score"], bound)
    finally:
        ora.close()
    print(f"V={V}: float32 twin and older restatements against float64, worst score difference {worst:.3f} of its bound")


@pytest.mark.parametrize("rule", bb.BIAS_RULES)
@pytest.mark.parametrize("V", bb.VS)
def test_every_wrong_variant_is_caught_at_every_vocabulary(V, rule):
    """the twin run with one rule of the bias broken -- the bonus added before the selection, no take-back, the take-back after the
    normalisation, a merged-in candidate's bonus dropped, a miss that falls to the root instead of the failure link, no reset on a
    commit, a back-off weight dropped, the LM state not advanced on a backed-off hit -- differs from the reference (tokens, timestamps,
    order, or a score by more than the bound) on at least one committed case: the cases would catch the mistake."""
    caught, n = bb.caught(V, rule)
    print(f"V={V} {rule}: told apart by {len(caught)} of {n} (configuration, case, stream, beam) runs")
    assert caught
