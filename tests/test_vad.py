"""CPU tests of the voice activity detector: the float32 host reference (csrc/vad_ref.h, through k2hip_debug_vad_ref_*) and the float64
twin (tests/vad_twin.py) on the hand-written cases of tests/vad_cases.py, the reference against the twin on the fbank of synthetic
recordings within the float32 chain's own bound, the chunking rule, every refusal of the config, and the long entry's packing rule.
The stream rules that need a model (sample rates, life cycle) run on the CPU in tests/native/san_vad_driver.cpp and on the device in
tests/test_vad_gpu.py."""
import numpy as np
import pytest

import vad_cases
import vad_twin as vt


# ---- known answers for the machine ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(vad_cases.CASES))
def test_machine_known_answers(name):
    max_speech, runs, want, want_speech = vad_cases.CASES[name]
    cfg = vad_cases.config(max_speech)
    assert vt.check_config(cfg, vad_cases.NUM_BINS)[0] == 0
    d_star, x = vad_cases.decisions(runs), vad_cases.features(runs)
    ref = vt.ref_run(cfg, x)
    assert ref["d"].tolist() == d_star.tolist()            # the features give the decision string the case is written in
    tw = vt.Twin(cfg)
    tp = tw.taps(x)
    assert tp["d"].tolist() == d_star.astype(bool).tolist()
    assert tw.machine(tp["d"], tp["m"]) == (want, want_speech)
    assert (ref["segs"], ref["speech"]) == (want, want_speech)


# ---- the reference against the twin on synthetic recordings -----------------------------------------------------------------------
def recording(kind):
    """synth_utterance pieces of 2, 1.5, 1 and 6 s between stretches (0.6, 0.9, 0.3, 1.2, 0.7 s) of low noise or of exact zeros"""
    from k2transducerasr_amd.synth import synth_utterance
    rng = np.random.default_rng(5)
    parts = []
    for i, g in enumerate([0.6, 0.9, 0.3, 1.2, 0.7]):
        n = int(g * 16000)
        parts.append((1e-3 * rng.standard_normal(n)).astype(np.float32) if kind == "noise" else np.zeros(n, np.float32))
        if i < 4:
            parts.append(synth_utterance(10 + i, [2, 1.5, 1, 6][i]))
    return np.concatenate(parts)


@pytest.fixture(scope="module")
def fbanks(oracle_tiny):
    return {k: np.ascontiguousarray(oracle_tiny.fbank(recording(k)), np.float32) for k in ("noise", "zeros")}


@pytest.mark.parametrize("kind", ["noise", "zeros"])
@pytest.mark.parametrize("max_speech", [2000, 300])
def test_reference_against_the_twin(fbanks, kind, max_speech):
    x = fbanks[kind]
    cfg = vt.default_config(x.shape[1]).copy(max_speech=max_speech)
    tw = vt.Twin(cfg)
    tp, ref = tw.taps(x), vt.ref_run(cfg, x)
    for k in ("m", "n"):
        err, b = np.abs(ref[k].astype(np.float64) - tp[k]), tw.bound(tp[k + "_mag"])
        print(f"{kind} max_speech {max_speech}: max |{k}32 - {k}64| = {err.max():.3e}, largest error / bound = {(err / b).max():.3f}")
        assert np.all(err <= b)
    # decisions only where the twin is further from both thresholds than the bound; the twin alone shows that this leaves >= 99 %
    near = (np.abs(tp["m"] - tp["n"] - tw.margin) <= tw.bound(tp["m_mag"]) + tw.bound(tp["n_mag"])) | (np.abs(tp["m"] - tw.abs_floor) <= tw.bound(tp["m_mag"]))
    print(f"  frames excluded from the decision comparison: {near.sum()} of {len(near)}")
    assert near.mean() <= 0.01
    assert np.array_equal(ref["d"].astype(bool)[~near], tp["d"][~near])
    # the machine is exact arithmetic on (d, m): fed the reference's own taps the twin's machine gives the reference's segments
    assert tw.machine(ref["d"], ref["m"]) == (ref["segs"], ref["speech"])
    if not near.any():
        assert tw.machine(tp["d"], tp["m"])[0] == ref["segs"]
    # orientation (the issue's numpy prototype with an fbank of its own: (59, 263), (349, 633), (749, 1352); cuts at 523, 1011, 1209):
    # three segments at the defaults, the 0.3 s gap merged; at max_speech = 300 a cut inside that gap and two in the last utterance
    starts = [s for s, _, _ in ref["segs"]]
    forced = [e for _, e, f in ref["segs"] if f]
    if max_speech == 2000:
        assert len(ref["segs"]) == 3 and not forced and all(abs(a - b) <= 12 for a, b in zip(starts, (59, 349, 749)))
    else:
        assert len(forced) == 3 and 500 <= forced[0] < 530 and forced[1] > 749 and forced[2] > forced[1]


# ---- chunking ----------------------------------------------------------------------------------------------------------------------
def chunkings(T, forced_frames, seed):
    rng = np.random.default_rng(seed)

    def fixed(k):
        return [k] * (T // k) + ([T % k] if T % k else [])

    out = [fixed(1), fixed(3), fixed(64), fixed(65)]
    r, left = [], T
    while left:
        n = 0 if rng.random() < 0.2 else int(min(left, rng.integers(1, 130)))
        r.append(n)
        left -= n
    out.append(r + [0])
    for cut_after in (0, 1):   # a boundary in front of and behind every frame at which a forced cut happens
        edges = sorted({t + cut_after for t in forced_frames if 0 < t + cut_after < T})
        out.append(np.diff([0] + edges + [T]).tolist())
    return out


def _check_chunkings(cfg, x, min_forced):
    whole = vt.ref_run(cfg, x)
    tw = vt.Twin(cfg)
    forced_at = []
    tw.machine(whole["d"], whole["m"], forced_at=forced_at)
    assert len(forced_at) >= min_forced
    for sizes in chunkings(x.shape[0], forced_at, 3):
        got = vt.ref_run(cfg, x, chunks=sizes)
        assert vt.same_bits(got["m"], whole["m"]) and vt.same_bits(got["n"], whole["n"]) and np.array_equal(got["d"], whole["d"]), sizes[:4]
        assert (got["segs"], got["speech"]) == (whole["segs"], whole["speech"]), sizes[:4]
    # is_speech after every single frame equals the machine's trig at that frame
    st = vt.ref_stream(cfg, x.shape[1])
    for t in range(min(x.shape[0], 400)):
        st.ref_push(x[t:t + 1])
        assert st.is_speech == tw.machine(whole["d"][: t + 1], whole["m"][: t + 1], flush=False)[1], t


def test_chunking_on_a_recording(fbanks):
    x = fbanks["noise"]
    _check_chunkings(vt.default_config(x.shape[1]).copy(max_speech=300), x, 3)
    _check_chunkings(vt.default_config(x.shape[1]).copy(max_speech=300, floor_window=150, rise=0.01), x, 1)


@pytest.mark.parametrize("name", ["forced_cut_inside_a_pause", "forced_cut_te_is_max_of_te_and_cut", "silence_run_exact"])
def test_chunking_on_the_cases(name):
    max_speech, runs, _, _ = vad_cases.CASES[name]
    _check_chunkings(vad_cases.config(max_speech), vad_cases.features(runs), 1 if max_speech == 16 else 0)


# ---- rules and refusals ------------------------------------------------------------------------------------------------------------
def test_the_defaults():
    cfg = vt.default_config(80)
    assert cfg.as_dict() == dict(band_lo=cfg.band_lo, band_hi=cfg.band_hi, floor_window=1000, rise=np.float32(0.002), margin=2.0, abs_floor=-12.0,
                                 min_silence=50, min_speech=25, speech_pad=10, max_speech=2000)
    # the bins centred in [300, 3500] Hz of the 80-bin filterbank over [20, 8000] Hz, from the mel formula
    mel = lambda f: 1127.0 * np.log(1.0 + f / 700.0)
    centres = 700.0 * (np.exp((mel(20.0) + (np.arange(80) + 1) * (mel(8000.0) - mel(20.0)) / 81) / 1127.0) - 1.0)
    inside = np.nonzero((centres >= 300.0) & (centres <= 3500.0))[0]
    assert (cfg.band_lo, cfg.band_hi) == (inside[0], inside[-1] + 1) and cfg.band_hi - cfg.band_lo == 47
    assert vt.check_config(cfg, 80)[0] == 0


@pytest.mark.parametrize("change, code, field", [
    (dict(band_lo=20, band_hi=20), -1, "band_lo"), (dict(band_lo=30, band_hi=20), -1, "band_hi"), (dict(band_hi=81), -1, "band_hi"),
    (dict(band_lo=-1), -1, "band_lo"),
    (dict(floor_window=7, max_speech=50), -1, "floor_window"), (dict(floor_window=1025), -6, "floor_window"),
    (dict(min_silence=19), -1, "min_silence"), (dict(max_speech=49), -1, "max_speech"), (dict(floor_window=100, max_speech=202), -1, "max_speech"),
    (dict(floor_window=0), -1, "floor_window"), (dict(min_silence=0), -1, "min_silence"), (dict(min_speech=0), -1, "min_speech"),
    (dict(speech_pad=0), -1, "speech_pad"), (dict(max_speech=0), -1, "max_speech"), (dict(min_speech=-3), -1, "min_speech"),
    (dict(rise=np.inf), -1, "rise"), (dict(margin=np.nan), -1, "margin"), (dict(abs_floor=-np.inf), -1, "abs_floor"),
])
def test_refused_configs(change, code, field):
    rc, msg = vt.check_config(vt.default_config(80).copy(**change), 80)
    assert rc == code and field in msg, (rc, msg)


def test_config_limits_that_pass():
    base = vt.default_config(80)
    # the issue's defaults themselves (max_speech / 2 = floor_window = 1000: the cut's window is frame t and the W - 1 carried values),
    # the largest window, the smallest, min_silence = 2 * speech_pad, max_speech = 2 * min_speech, a one-bin band
    for change in (dict(), dict(floor_window=1024, max_speech=2048), dict(floor_window=8, max_speech=16, min_speech=8), dict(min_silence=20),
                   dict(max_speech=50), dict(band_lo=79, band_hi=80)):
        assert vt.check_config(base.copy(**change), 80) == (0, vt.check_config(base.copy(**change), 80)[1])
    from k2transducerasr_amd import K2HipError
    with pytest.raises(K2HipError) as e:
        vt.ref_stream(base.copy(speech_pad=26), 80)
    assert e.value.code == -1 and "min_silence" in str(e.value)


def test_batch_packing():
    # three fit (3 * 200 = 600 frames), the fourth closes the batch by count; 400 + 30 would need 2 * 400 > 600
    assert vt.lib_pack([100, 200, 50, 400, 30], 3, 600) == (0, [0, 0, 0, 1, 2])
    # a segment longer than max_batch_frames on its own is a batch of one
    assert vt.lib_pack([700, 10, 10], 8, 600) == (0, [0, 1, 1])
    assert vt.lib_pack([10, 700, 10], 8, 600) == (0, [0, 1, 2])
    assert vt.lib_pack([5] * 7, 2, 10 ** 9) == (0, [0, 0, 1, 1, 2, 2, 3])
    assert vt.lib_pack([], 4, 100) == (0, [])
    rng = np.random.default_rng(1)
    for _ in range(200):
        lens = rng.integers(1, 900, rng.integers(1, 30)).tolist()
        mb, mbf = int(rng.integers(1, 9)), int(rng.integers(1, 4000))
        got = vt.lib_pack(lens, mb, mbf)
        assert got == (0, vt.twin_pack(lens, mb, mbf))
        for b in set(got[1]):   # the rule's two promises, checked on the result itself
            mine = [n for n, bb in zip(lens, got[1]) if bb == b]
            assert len(mine) <= mb and (len(mine) == 1 or len(mine) * max(mine) <= mbf)
    assert vt.lib_pack([10], 0, 100)[0] == -1 and vt.lib_pack([10], 4, 0)[0] == -1 and vt.lib_pack([10, 0], 4, 100)[0] == -1
