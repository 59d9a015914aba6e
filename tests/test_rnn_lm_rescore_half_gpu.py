"""The half-precision LSTM step of the rescoring on the device (k2hip_set_rnn_lm_rescoring_precision; csrc/rnn_lm_f16.hip):
k_lm_lstm_step_f16 alone against float64 over f16-rounded operands, the scoring operator and the recognizer against the half twin
(tests/rnn_lm_rescore_half_cases.py), and the switch."""
import numpy as np
import pytest

import rnn_lm_cases as lmc
import rnn_lm_rescore_half_cases as cases
from rnn_lm_twin import rescored_order
from test_rnn_lm_gpu import decode, model, model165, run_op, step_f64   # noqa: F401 (fixtures)
from test_rnn_lm_half_gpu import relay_f16

pytestmark = pytest.mark.gpu
f32, f16 = np.float32, np.float16


@pytest.fixture(scope="module")
def lms(tmp_path_factory):
    """name -> (RnnLm, the float64 half twin)"""
    from k2transducerasr_amd import RnnLm
    from k2transducerasr_amd.synth import write_synthetic_rnn_lm
    d = tmp_path_factory.mktemp("rnn_lm_rescore_half")
    out = {}
    for name, (V, E, H, L, seed) in cases.LMS.items():
        sd = write_synthetic_rnn_lm(str(d / f"{name}.k2w"), V, E, H, L, seed)
        out[name] = (RnnLm(str(d / f"{name}.k2w")), cases.HalfTwin(sd, L))
    return out


@pytest.mark.parametrize("H", [32, 96])
def test_step_f16_kernel_one_step(model, H):
    """a = 1 (one strip), 5 (ragged), 33 (two strips), 130 (every wave finishes a strip; a second round), 300 (a second row block) x both
    `first`: c and h of the active rows against float64 over h_prev and W_hh rounded to f16 first -- f16 x f16 products are exact in
    float32, so the tolerance is test_step_kernel_one_step's, 4 K 2^-24 sqrt(K) + 2e-6 with K = H; the mirror is float16 of the device's
    own h_out bit for bit; rows >= a of the three outputs keep their sentinel; the operands nobody may read are NaN."""
    rng = np.random.default_rng(H)
    w_hh = rng.uniform(-1, 1, size=(4 * H, H)).astype(f32) / f32(np.sqrt(H))
    panels = relay_f16(np.zeros((4 * H, 0), f32), w_hh)   # (RnnLmDev::whh_h: the fused f16 panels with an input width of 0)
    tol, worst = 4 * H * 2.0 ** -24 * np.sqrt(H) + 2e-6, 0.0
    for a, first in ((a, first) for a in (1, 5, 33, 130, 300) for first in (0, 1)):
        rows = a + 3
        h = rng.uniform(-1, 1, size=(rows, H)).astype(f16)
        gx = rng.standard_normal((rows, 4 * H)).astype(f32)
        c = rng.uniform(-1, 1, size=(rows, H)).astype(f32)
        h[0 if first else a:] = np.nan
        gx[a:] = np.nan
        c_dev, h_out, mirror = c.copy(), np.full((rows, H), -7.0, f32), np.full((rows, H), -7.0, f16)
        run_op(model, "rnn_lm_step_f16", [a, H, first], [h, panels, gx, c_dev, h_out, mirror], (1 << 3) | (1 << 4) | (1 << 5))
        wc, wh = step_f64(h[:a], w_hh.astype(f16), gx[:a], c[:a].astype(np.float64), first)
        assert np.array_equal(c_dev[a:].view(np.uint32), c[a:].view(np.uint32)) and np.all(h_out[a:] == -7.0) and np.all(mirror[a:] == f16(-7.0)), (a, first)
        assert np.array_equal(mirror[:a].view(np.uint16), h_out[:a].astype(f16).view(np.uint16)), (a, first)
        err = float(max(np.abs(c_dev[:a] - wc).max(), np.abs(h_out[:a] - wh).max()))
        worst = max(worst, err)
        assert err <= tol, (a, first, err, tol)
    print(f"step_f16 kernel H = {H}: worst error {worst:.3g}, tolerance {tol:.3g}")


def check_against_twin(got, want, hyps, eos, what):
    (tot, tlp), (wt, wl) = got, want
    worst = max(float(np.abs(g - w).max()) for g, w in zip(tlp + [np.zeros(1)], wl + [np.zeros(1)]) if len(w))
    assert [len(t) for t in tlp] == [len(h) + int(eos) for h in hyps] and worst <= cases.token_bound(), (what, worst)
    assert all(abs(t - w) <= cases.total_bound(len(h) + int(eos)) for t, w, h in zip(tot, wt, hyps)), what
    return worst


@pytest.mark.parametrize("name", list(cases.LMS))
def test_operator_against_the_half_twin(model, model165, lms, name):
    from k2transducerasr_amd import set_switch
    lm, tw = lms[name]
    V, _, H, _, _ = cases.LMS[name]
    model = model165 if V == 165 else model
    model.set_rnn_lm(lm, 0.0)
    model.set_rnn_lm_rescoring_precision(True)
    try:
        worst = 0.0
        for sname, eos in ((s, e) for s in cases.SETS for e in (True, False)):
            hyps = lmc.hyp_sets(V)[sname]
            want = tw.score_all(hyps, eos)
            worst = max(worst, check_against_twin(model.rnn_lm_score(hyps, eos), want, hyps, eos, (name, sname, eos)))
            if (name, sname, eos) == ("A", "fall", True):   # the time-blocked route: 100 rows of GX at a time
                set_switch("K2HIP_RNN_LM_GX_CAP", 4 * H * 100)
                try:
                    worst = max(worst, check_against_twin(model.rnn_lm_score(hyps, eos), want, hyps, eos, (name, "blocked")))
                    assert model.rnn_lm_stats()["last_blocks"] > 10
                finally:
                    set_switch("K2HIP_RNN_LM_GX_CAP", 0)
        print(f"LM {name} in half precision: worst token error against the half twin {worst:.3g}, bound {cases.token_bound():.3g}")
    finally:
        model.set_rnn_lm_rescoring_precision(False)
        model.set_rnn_lm(None)


def test_switch(tiny_model_path, oracle_tiny, lms, tmp_path):
    import rnn_lm_fusion_cases as oc
    from k2transducerasr_amd import K2HipError, Model, RnnLm
    from k2transducerasr_amd.synth import rnn_lm_state_dict, write_rnn_lm
    hyps = lmc.hyp_sets(37)["drawn33"]
    bits = lambda r: (r[0].tobytes(), [t.tobytes() for t in r[1]])   # noqa: E731
    enc = oc.encode(oracle_tiny, oc.utterances(0))
    model = Model(tiny_model_path, 0)   # a model whose switch was never on
    fused = lambda: [[(a["tokens"], a["timestamps"], f32(a["score"]).tobytes()) for a in al] for al in model.beam_search(enc, 4, nbest=4)]   # noqa: E731
    try:
        model.set_rnn_lm(lms["A"][0], 0.5)
        never, calls = model.rnn_lm_score(hyps), model.rnn_lm_stats()["device_calls"]
        model.set_rnn_lm_fusion(True)
        fused_off = fused()
        model.set_rnn_lm_rescoring_precision(True)
        half = model.rnn_lm_score(hyps)
        assert model.rnn_lm_stats()["device_calls"] == calls + 1
        assert any(not np.array_equal(a, b) for a, b in zip(half[1], never[1]))   # on: another arithmetic
        assert fused() == fused_off                                                # the fused search does not read the switch
        model.set_rnn_lm_fusion(False)
        model.set_rnn_lm_rescoring_precision(False)
        assert bits(model.rnn_lm_score(hyps)) == bits(never) and model.rnn_lm_stats()["device_calls"] == calls + 2   # off after on
        # a W_hh weight that is not finite in f16: refused by the first half-precision scoring call, scored under float32
        V, E, H, L, _ = cases.LMS["A"]
        sd = rnn_lm_state_dict(V, E, H, L, 0, False)
        sd["rnn.weight_hh_l0"][3, 5] = 1e5
        write_rnn_lm(str(tmp_path / "big.k2w"), sd, L, 1, 1, False)
        model.set_rnn_lm_rescoring_precision(True)
        model.set_rnn_lm(RnnLm(str(tmp_path / "big.k2w")), 0.5)
        with pytest.raises(K2HipError) as e:
            model.rnn_lm_score(hyps)
        assert e.value.code == -1 and "half precision" in str(e.value)
        model.set_rnn_lm_rescoring_precision(False)
        assert len(model.rnn_lm_score(hyps)[0]) == len(hyps)
    finally:
        model.close()


def test_recognizer_rescoring_half(tmp_path, utts):
    """the existing rescoring recognizer case with rnn_lm_rescore_half=True: every stream's alternatives in the half twin's order (the
    gaps are test_rnn_lm_rescore_half.py's), lm_score within P token bounds of the half twin"""
    from k2transducerasr_amd import OfflineRecognizer, RnnLm
    from k2transducerasr_amd.synth import write_synthetic_model, write_synthetic_rnn_lm
    rc = lmc.RECOGNIZER["transducer"]
    mp, lp_ = str(tmp_path / "m.k2w"), str(tmp_path / "lm.k2w")
    write_synthetic_model(mp, rc["preset"])
    V, E, H, L, _ = cases.LMS["A"]
    tw = cases.HalfTwin(write_synthetic_rnn_lm(lp_, V, E, H, L, cases.RECOGNIZER_SEED), L)
    plain = OfflineRecognizer(mp, 0, rc["method"], 4, nbest=4)
    alts0 = decode(plain, utts)[1]
    plain.model.close()
    rec = OfflineRecognizer(mp, 0, rc["method"], 4, nbest=4, rnn_lm=RnnLm(lp_), rnn_lm_scale=rc["scale"], rnn_lm_rescore_half=True)
    try:
        worst = 0.0
        for b, (al, al0) in enumerate(zip(decode(rec, utts)[1], alts0)):
            twin_lm = [tw.score(a["tokens"])[0] for a in al0]
            order, _ = rescored_order([float(f32(a["score"])) for a in al0], [len(a["tokens"]) for a in al0], twin_lm, rc["scale"], False)
            assert [a["tokens"] for a in al] == [al0[i]["tokens"] for i in order], (b, order)
            worst = max([worst] + [abs(a["lm_score"] - twin_lm[i]) / cases.total_bound(len(a["tokens"]) + 1) for a, i in zip(al, order)])
        print(f"recognizer in half precision: worst lm_score error {worst:.3g} of its bound")
        assert worst <= 1
    finally:
        rec.model.close()
