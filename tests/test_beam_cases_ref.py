"""Host-side checks of tests/beam_cases.py, the inputs tests/test_beam_ties_gpu.py puts through the modified beam search: the
generator's promises and coverage on every committed case, the float64 twin against the float32 C oracle and against nbest_twin_search
on the alternatives, and the sensitivity of the cases -- every deliberately wrong variant of the search (beam_cases.RULES) is told from
the reference by at least one committed case per V, so each of these mistakes in a kernel would fail the device test."""
import functools

import numpy as np
import pytest

import beam_cases as bc
from nbest_twin import nbest_twin_search


@functools.lru_cache(maxsize=None)
def model(V):
    return bc.build(V)


@functools.lru_cache(maxsize=None)
def reference(V, case, stream, beam):
    m = model(V)
    c = next(x for x in m.cases if x.name == case)
    return bc.twin(m.W, m.b, c.enc[stream], beam)


def runs(m):
    return [(c, s, beam) for c in m.cases for s in range(c.enc.shape[0]) for beam in bc.BEAMS]


@pytest.mark.parametrize("V", bc.VS)
def test_promises_and_coverage(V):
    """check_case on every committed case (through coverage): every ordering decision an exact tie of equally formed scores or 10 x the
    bound apart, float32 and float64 alike in tokens, timestamps and order, and every kind and duplicate position counted at least once at
    every beam that admits it.  The committed seed is the first that does all this."""
    m = model(V)
    cov = bc.coverage(m)
    for beam in bc.BEAMS:
        print(f"V={V} beam={beam}: " + " ".join(f"{k}={v}" for k, v in cov[beam].items() if v))
        assert cov[beam]["ties"] >= 40
    worst = max(bc.score_bound(m.W, m.b, reference(V, c.name, s, beam), c.enc.shape[1]) for c, s, beam in runs(m))
    print(f"V={V}: score bound {worst:.3g}, token log-prob bound {bc.noise_terms(m.W, m.b)[0]:.3g}")
    assert worst < 1e-3                                 # (a bound near the levels' spacing would leave no room for 10 x of it)
    assert bc.find_seed(V, bc.SEEDS[V] + 1)[0] == bc.SEEDS[V]


def test_the_model_is_what_the_docstring_says():
    for V in bc.VS:
        m = model(V)
        assert m.W.shape == (V, bc.J) and ((m.W != 0).sum(1) <= 1).all() and set(np.unique(m.W)) == {0.0, np.float32(bc.W_LEVER)}
        assert (m.b == np.float32(bc.FLOOR)).all()
        for d, cols in enumerate(m.groups.values()):
            assert (np.flatnonzero(m.W[:, d]) == sorted(cols)).all()
        assert int((~(m.W != 0).any(1)).sum()) >= V - 40    # the floor: several hundred columns without a weight
        for c in m.cases:
            assert c.enc.shape[0] <= 3 and c.enc.shape[1] <= 16 and c.enc.dtype == np.float32
    rep = model(400).cases[0]
    assert rep.name == "repeat" and all(np.array_equal(e[0], e[1]) for e in rep.enc)


@pytest.mark.parametrize("V", bc.VS)
def test_twin_equals_the_c_oracle_and_the_nbest_twin(V, tmp_path):
    """oracle.Oracle.modified_beam_search (float32 C, oracle/k2_oracle_beam.c): tokens and timestamps exact, scores within the bound --
    with the oracle's ONE chain of V additions in the sum of exponentials where the device has a lane's chain and a tree -- and the
    same, order included, for every alternative nbest_twin_search returns."""
    from oracle import Oracle
    m = model(V)
    p = str(tmp_path / f"ties_v{V}.k2w")
    m.write(p)
    ora = Oracle(p)
    e_u = bc.noise_terms(m.W, m.b, chain=V)[0]
    worst = [0.0, 0.0]
    try:
        for c in m.cases:
            T = c.enc.shape[1]
            for beam in bc.BEAMS:
                res, sc = ora.modified_beam_search(c.enc, beam, want_scores=True)
                for s in range(c.enc.shape[0]):
                    ref = reference(V, c.name, s, beam)
                    bound = bc.score_bound(m.W, m.b, ref, T, chain=V)
                    best = ref["alts"][0]
                    assert res[s] == (best["tokens"], best["timestamps"]), (c.name, s, beam)
                    assert abs(float(sc[s]) - best["score"]) <= bound, (c.name, s, beam, float(sc[s]), best["score"], bound)
                    if beam > 1:
                        tw = nbest_twin_search(ora, c.enc[s], beam)["alts"]
                        assert [(a["tokens"], a["timestamps"]) for a in tw] == [(a["tokens"], a["timestamps"]) for a in ref["alts"]], (c.name, s, beam)
                        for a, r in zip(tw, ref["alts"]):
                            worst[0] = max(worst[0], abs(a["score"] - r["score"]))
                            assert abs(a["score"] - r["score"]) <= bound, (c.name, s, beam, a["score"], r["score"], bound)
                            if len(a["tokens"]):
                                d = float(np.abs(a["token_log_probs"] - r["token_log_probs"]).max())
                                worst[1] = max(worst[1], d)
                                assert d <= e_u, (c.name, s, beam, d, e_u)
    finally:
        ora.close()
    print(f"V={V}: float32 twin on the oracle's operators, worst score diff {worst[0]:.3g}, worst token log-prob diff {worst[1]:.3g} (bound {e_u:.3g})")


@pytest.mark.parametrize("rule", bc.RULES)
@pytest.mark.parametrize("V", bc.VS)
def test_every_wrong_variant_is_caught_at_every_vocabulary(V, rule):
    """the twin run with one rule broken -- ties to the higher flat index, the last maximum of a lane's stride, the later path's
    timestamps at a merge, a merge into a merged-away entry, out-of-range columns in the log-sum-exp, the last entry on a final tie, the
    higher indexes kept at the beam cut -- differs from the reference (tokens, timestamps, order, or a score by more than the bound) on
    at least one committed case: the cases would catch the mistake."""
    m = model(V)
    caught = []
    for c, s, beam in runs(m):
        ref = reference(V, c.name, s, beam)
        if bc.different(bc.twin(m.W, m.b, c.enc[s], beam, rule=rule), ref, bc.score_bound(m.W, m.b, ref, c.enc.shape[1])):
            caught.append((c.name, s, beam))
    print(f"V={V} {rule}: told apart by {len(caught)} of {len(runs(m))} (case, stream, beam) runs")
    assert caught
