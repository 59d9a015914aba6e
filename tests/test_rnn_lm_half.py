"""The cases of the half-precision neural LM fusion tests on the CPU (tests/rnn_lm_half_cases.py): E16 re-measured, and every case
accepted under the half twin with a gap of at least twice the score bound the device is held to (test_rnn_lm_half_gpu.py asserts
nothing about acceptance that this test has not)."""
import pytest

import rnn_lm_fusion_cases as oc
import rnn_lm_half_cases as cases
from rnn_lm_fusion_twin import twin_batch


@pytest.mark.parametrize("name,beam", sorted(cases.SEEDS))
def test_half_cases_are_accepted(tmp_path, name, beam):
    base, seed, gap = cases.SEEDS[(name, beam)]
    _, ora = oc.make_oracle(tmp_path, oc.OPERATOR[name])
    enc = oc.encode(ora, oc.utterances(base))
    _, _, tw = oc.make_lm(tmp_path, name, seed)
    runs = twin_batch(ora, enc, beam, nlm=cases.HalfFusionLm(tw), nscale=cases.SCALE, nbest=cases.NBEST)[4]
    ok, g = oc.accepted(runs)
    e16, n_max = cases.case_views(tw, runs)
    bound = cases.score_bound(enc.shape[1], n_max)
    print(f"LM {name} beam {beam}: gap {g:.4g} (recorded {gap}), E16 here {e16:.3g} (constant {cases.E16}), score bound {bound:.3g}")
    assert len(runs) == oc.STREAMS and ok and abs(g - gap) <= 1e-5
    assert e16 <= cases.E16
    assert g >= 2 * bound
