"""The half-precision rescoring without a GPU (tests/rnn_lm_rescore_half_cases.py): E16R re-measured, the half twin with its rounding
disabled against torch's own LSTM in float64, and the key gaps of the recognizer case test_rnn_lm_rescore_half_gpu.py rests on."""
import numpy as np
import pytest

import rnn_lm_cases as lmc
import rnn_lm_rescore_half_cases as cases
from rnn_lm_twin import Twin, rescored_order

from k2transducerasr_amd.synth import rnn_lm_state_dict


@pytest.fixture(scope="module")
def sds():
    return {name: rnn_lm_state_dict(V, E, H, L, seed) for name, (V, E, H, L, seed) in cases.LMS.items()}


def test_e16r_is_the_recorded_constant(sds):
    worst = 0.0
    for name, (V, _, _, L, _) in cases.LMS.items():
        t32, t64 = cases.HalfTwin(sds[name], L, np.float32), cases.HalfTwin(sds[name], L, np.float64)
        for hyps in lmc.hyp_sets(V).values():
            for eos, h in ((e, h) for e in (True, False) for h in hyps if len(h) + int(e)):
                worst = max(worst, float(np.abs(t32.score(h, eos)[1] - t64.score(h, eos)[1]).max()))
    print(f"E16R = {worst:.4g} (recorded {cases.E16R:.4g}), token bound {cases.token_bound():.4g}")
    # the recorded constant is this measurement (numpy's matrix product may sum in another order on another machine: a factor of two)
    assert worst <= 2 * cases.E16R and cases.E16R <= 4 * max(worst, 1e-9)


@pytest.mark.parametrize("name", list(cases.LMS))
def test_twin_without_rounding_is_the_float64_twin(sds, name):
    V, _, _, L, _ = cases.LMS[name]
    hyps = lmc.hyp_sets(V)["decreasing"]
    for eos in (True, False):
        wt, wl = Twin(sds[name], L).score_all(hyps, eos)
        gt, gl = cases.HalfTwin(sds[name], L, half=False).score_all(hyps, eos)
        assert np.abs(gt - wt).max() <= 1e-10 and all(np.abs(g - w).max() <= 1e-11 for g, w in zip(gl, wl) if len(w))
    assert np.abs(cases.HalfTwin(sds[name], L).score_all(hyps)[0] - wt).max() > 0   # ... and the rounding is not a no-op


def test_recognizer_case_gaps_under_the_half_twin(tmp_path, utts):
    """the rescoring recognizer case (LM A's shape, RECOGNIZER_SEED, scale 2) on the twins' own N-best lists: every adjacent pair of a
    stream's keys under the half twin is at least twice the key bound apart, so the device's order is decided"""
    from nbest_twin import nbest_twin_batch
    from oracle import Oracle
    from k2transducerasr_amd.synth import write_synthetic_model
    rc = lmc.RECOGNIZER["transducer"]
    assert cases.RECOGNIZER_SEED == rc["seed"]   # (the existing draw; another seed would be recorded in the cases)
    p = str(tmp_path / "m.k2w")
    write_synthetic_model(p, rc["preset"])
    ora = Oracle(p)
    enc = ora.encoder(ora.pad_sequence([ora.fbank(u) for u in utts]).reshape(len(utts), -1, 80))
    V, E, H, L, _ = cases.LMS["A"]
    tw = cases.HalfTwin(rnn_lm_state_dict(V, E, H, L, cases.RECOGNIZER_SEED), L)
    slack = np.inf
    for r in nbest_twin_batch(ora, enc, 4):
        alts = r["alts"][:4]
        n = [len(a["tokens"]) for a in alts]
        order, keys = rescored_order([a["score"] for a in alts], n, [tw.score(a["tokens"])[0] for a in alts], rc["scale"], False)
        for i, j in zip(order, order[1:]):
            slack = min(slack, (keys[i] - keys[j]) / max(cases.key_bound(n[i], rc["scale"]), cases.key_bound(n[j], rc["scale"])))
    print(f"smallest adjacent key gap under the half twin: {slack:.4g} key bounds")
    assert slack >= 2
