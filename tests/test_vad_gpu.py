"""GPU tests of the voice activity detector (csrc/vad.hip) and of the long entry: the kernels against the float32 host reference
(csrc/vad_ref.h) bit for bit -- taps, segments, is_speech -- at the smallest shapes that can go wrong, chunked calls against one call,
the samples route against the features route, k2hip_offline_recognize_long against k2hip_offline_greedy_from_samples on the segments'
sample ranges, and the isolation of a model's other entries from VAD use.

A contracted multiply-add in the floor pass (m + rise * k in one rounding) changes n on a sizeable share of frames of the matrices
below (rise = 0.05 and 0.002 are not exact in binary, k runs to 1023): the bit comparison of n catches it."""
import numpy as np
import pytest

import vad_cases
import vad_twin as vt

pytestmark = pytest.mark.gpu

LOG_EPS = np.float32(np.log(np.float32(1.1920929e-07)))   # the fbank's floor: log(FLT_EPSILON)
TILE = 256                                                # kVadTile (csrc/kernels.h)


def small_cfg(lo=10, hi=57):
    """W = 8: the floor follows within 8 frames, so the decision is left to abs_floor (margin < 0); forced cuts every 16 frames of
    speech, windows of 8"""
    from k2transducerasr_amd import VadConfig
    return VadConfig(band_lo=lo, band_hi=hi, floor_window=8, rise=0.05, margin=-1.0, abs_floor=-6.0, min_silence=4, min_speech=4, speech_pad=2,
                     max_speech=16)


def big_cfg(lo=10, hi=57, max_speech=300):
    from k2transducerasr_amd import VadConfig
    return VadConfig(band_lo=lo, band_hi=hi, floor_window=1024, rise=0.002, margin=2.0, abs_floor=-12.0, min_silence=50, min_speech=25, speech_pad=10,
                     max_speech=max_speech)


def speechy(T, seed, block=37):
    """noise near -10 with blocks of speech near -2 of irregular lengths, a few rows at the fbank's floor"""
    rng = np.random.default_rng(seed)
    x = (-10.0 + 0.5 * rng.standard_normal((T, 80))).astype(np.float32)
    t = int(rng.integers(0, block))
    while t < T:
        n = int(rng.integers(block // 2, 6 * block))
        x[t:t + n] += np.float32(8.0) + rng.standard_normal((min(n, T - t), 1)).astype(np.float32)
        t += n + int(rng.integers(3, 3 * block))
    x[T // 3: T // 3 + 5] = LOG_EPS
    return x


def device_run(model, cfg, x, chunks=None, flush=True):
    """the kernels over x, fed whole or in chunks -> the dict of vad_twin.ref_run"""
    from k2transducerasr_amd import VadStream
    st = VadStream(model, cfg)
    taps, pos = [], 0
    for n in ([x.shape[0]] if chunks is None else chunks):
        st.accept_features(x[pos:pos + n])
        taps.append(model.vad_taps(0))
        assert len(taps[-1][0]) == n
        pos += n
    assert pos == x.shape[0] == st.num_frames
    speech = st.is_speech
    if flush:
        st.flush()
    segs = [(g["start"], g["end"], g["forced"]) for g in st.segments()]
    st.close()
    return dict(m=np.concatenate([t[0] for t in taps]), n=np.concatenate([t[1] for t in taps]), d=np.concatenate([t[2] for t in taps]), segs=segs,
                speech=speech)


def assert_same(got, want, what):
    assert vt.same_bits(got["m"], want["m"]), (what, "m", int(np.sum(got["m"].view(np.uint32) != want["m"].view(np.uint32))))
    assert vt.same_bits(got["n"], want["n"]), (what, "n", int(np.sum(got["n"].view(np.uint32) != want["n"].view(np.uint32))))
    assert np.array_equal(got["d"], want["d"]), (what, "d")
    assert (got["segs"], got["speech"]) == (want["segs"], want["speech"]), (what, got["segs"], want["segs"])


SMALL_T = (0, 1, 4, 5, 7, 8, 9, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1)
BIG_T = (0, 1, 5, 64, 65, TILE + 1, 1023, 1024, 1025, 1100)


@pytest.mark.parametrize("band", [(10, 57), (3, 4), (0, 80)], ids=lambda b: f"bins{b[1] - b[0]}")
@pytest.mark.parametrize("which", ["W8", "W1024"])
def test_kernels_against_the_reference(hip_tiny, which, band):
    cfg = small_cfg(*band) if which == "W8" else big_cfg(*band)
    x = speechy(1100, 11 + band[0], block=37 if which == "W8" else 90)   # (blocks of speech longer than max_speech = 300 among them)
    n_forced = 0
    for T in (SMALL_T if which == "W8" else BIG_T):
        want = vt.ref_run(cfg, x[:T])
        assert_same(device_run(hip_tiny, cfg, x[:T]), want, (which, band, T))
        n_forced += sum(f for _, _, f in want["segs"])
    assert n_forced > 0   # (the shapes above do reach the forced cut)


def test_forced_cut_window_straddles_the_carried_history(hip_tiny):
    """speech from frame 2 on, max_speech = 300: the cut at frame 301 looks at frames [152, 301]; the second call starts at 250 (the
    window is part history, part new) or at 301 (all history but the frame itself) or at 302 (the cut is the first call's last frame)"""
    cfg = big_cfg(max_speech=300)
    rng = np.random.default_rng(3)
    x = (-2.0 + 0.3 * rng.standard_normal((700, 80))).astype(np.float32)
    x[:2] = -10.0
    want = vt.ref_run(cfg, x)
    assert [f for _, _, f in want["segs"]].count(1) >= 2
    for first in (250, 301, 302, 160):
        assert_same(device_run(hip_tiny, cfg, x, chunks=[first, 700 - first]), want, first)


@pytest.mark.parametrize("kind", ["constant", "two_valued", "floor_rows"])
def test_exact_ties(hip_tiny, kind):
    """m constant (every window of the forced cut is one exact tie: the earliest frame), m from two values in blocks (ties between far
    frames), rows at the fbank's floor between speech"""
    T = 400
    if kind == "constant":
        x = np.full((T, 80), -3.0, np.float32)
    elif kind == "two_valued":
        x = np.where((np.arange(T) // 7 % 2 == 0)[:, None], np.float32(-3.0), np.float32(-4.5)) * np.ones((1, 80), np.float32)
    else:
        x = np.full((T, 80), LOG_EPS, np.float32)
        x[40:200] = -3.0
        x[230:390] = -3.0
    for cfg in (small_cfg(), big_cfg(max_speech=60).copy(margin=-1.0 if kind != "floor_rows" else 2.0)):
        want = vt.ref_run(cfg, x)
        assert [f for _, _, f in want["segs"]].count(1) >= 2
        if kind == "constant":   # every cut is the first frame of its window
            half = cfg.max_speech // 2
            ends = [e for _, e, f in want["segs"] if f]
            assert ends[0] == cfg.max_speech - half and all(b - a == cfg.max_speech - half for a, b in zip(ends, ends[1:]))
        assert_same(device_run(hip_tiny, cfg, x), want, (kind, cfg.floor_window))


@pytest.mark.parametrize("name", sorted(vad_cases.CASES))
def test_machine_cases_on_the_device(hip_tiny, name):
    """the hand-written decision strings (tests/vad_cases.py), on rows widened to the model's 80 bins"""
    max_speech, runs, want, want_speech = vad_cases.CASES[name]
    cfg = vad_cases.config(max_speech)
    x = np.full((len(vad_cases.decisions(runs)), 80), 7.0, np.float32)
    x[:, : vad_cases.NUM_BINS] = vad_cases.features(runs)
    got = device_run(hip_tiny, cfg, x)
    assert (got["segs"], got["speech"]) == (want, want_speech)
    assert got["d"].tolist() == vad_cases.decisions(runs).tolist()


def _batch_streams(model):
    from k2transducerasr_amd import VadStream
    cfgs = [big_cfg(), small_cfg(), big_cfg(3, 4), small_cfg(0, 80), big_cfg(max_speech=200)]
    xs = [speechy(1100, 40 + i)[:T] for i, T in enumerate((0, 1, 64, 300, 1100))]
    return cfgs, xs, [VadStream(model, c) for c in cfgs]


def test_a_batch_of_five_streams_in_one_call(hip_tiny):
    cfgs, xs, streams = _batch_streams(hip_tiny)
    hip_tiny.vad_accept_features(streams, xs)
    for b, (cfg, x, st) in enumerate(zip(cfgs, xs, streams)):
        want = vt.ref_run(cfg, x)
        m, n, d = hip_tiny.vad_taps(b)
        speech = st.is_speech
        assert st.num_frames == len(x)
        st.flush()
        got = dict(m=m, n=n, d=d, speech=speech, segs=[(g["start"], g["end"], g["forced"]) for g in st.segments()])
        assert_same(got, want, b)
        st.close()


def test_chunked_against_whole_on_the_device(hip_tiny):
    """three streams side by side in the same calls, in chunks of 1, of 64 and of random lengths (some empty): the bits of one call"""
    from k2transducerasr_amd import VadStream
    cfgs = [big_cfg(max_speech=100), small_cfg(), small_cfg(3, 4)]
    xs = [speechy(1100, 70 + i)[:T] for i, T in enumerate((330, 200, 130))]
    whole = [device_run(hip_tiny, c, x) for c, x in zip(cfgs, xs)]
    for b in range(3):
        assert_same(whole[b], vt.ref_run(cfgs[b], xs[b]), b)
    rng = np.random.default_rng(9)
    for plan in ("1", "64", "random"):
        streams = [VadStream(hip_tiny, c) for c in cfgs]
        pos, taps = [0, 0, 0], [[], [], []]
        while any(p < len(x) for p, x in zip(pos, xs)):
            take = [min(len(x) - p, 1 if plan == "1" else 64 if plan == "64" else int(rng.integers(0, 90)) * int(rng.random() > 0.2)) for p, x in zip(pos, xs)]
            hip_tiny.vad_accept_features(streams, [x[p:p + n] for x, p, n in zip(xs, pos, take)])
            for b in range(3):
                taps[b].append(hip_tiny.vad_taps(b))
                assert len(taps[b][-1][0]) == take[b]
                pos[b] += take[b]
        for b, st in enumerate(streams):
            speech = st.is_speech
            st.flush()
            got = dict(m=np.concatenate([t[0] for t in taps[b]]), n=np.concatenate([t[1] for t in taps[b]]), d=np.concatenate([t[2] for t in taps[b]]),
                       speech=speech, segs=[(g["start"], g["end"], g["forced"]) for g in st.segments()])
            assert_same(got, whole[b], (plan, b))
            st.close()


# ---- samples in ----------------------------------------------------------------------------------------------------------------------
def recording(seconds_speech, seconds_gap, seed=5, rate=16000):
    from k2transducerasr_amd.synth import synth_utterance
    rng = np.random.default_rng(seed)
    parts = [(1e-3 * rng.standard_normal(int(0.4 * rate))).astype(np.float32)]
    for i, s in enumerate(seconds_speech):
        parts.append(synth_utterance(20 + i, s, rate))
        parts.append((1e-3 * rng.standard_normal(int(seconds_gap[i] * rate))).astype(np.float32))
    return np.concatenate(parts)


def test_accept_samples_equals_the_features_route(hip_tiny):
    """two streams at 16 kHz and one at 8 kHz pushed in uneven pieces (so that every call leaves a remainder short of a frame shift, and
    some calls complete no frame): segments, is_speech and the taps equal those of the features route fed with k2hip_fbank of the same
    samples -- of the resampler's output for the 8 kHz stream"""
    from k2transducerasr_amd import K2HipError, VadStream
    m = hip_tiny
    cfg = m.vad_default_config().copy(max_speech=150)
    x16 = [recording([1.6, 1.2], [0.8, 0.5], 5), recording([0.9, 2.0], [0.7, 0.6], 6)]
    x8 = recording([1.4, 1.1], [0.9, 0.5], 7, rate=8000)
    want = []
    for x in x16 + [m.resample(x8, 8000)]:
        st = VadStream(m, cfg)
        st.accept_features(m.fbank(x))
        taps, speech, frames = m.vad_taps(0), st.is_speech, st.num_frames
        st.flush()
        want.append((taps, speech, frames, st.segments()))
        st.close()
    assert all(len(w[3]) >= 2 for w in want)
    rng = np.random.default_rng(2)
    for b, (x, rate) in enumerate(zip(x16 + [x8], (16000, 16000, 8000))):
        st = VadStream(m, cfg)
        pos, taps = 0, []
        while pos < len(x):
            n = int(min(len(x) - pos, rng.choice([37, 159, 160, 161, 399, 400, 401, 4000, 12345])))
            st.accept_waveform(rate, x[pos:pos + n])
            taps.append(m.vad_taps(0))
            pos += n
        got_taps = [np.concatenate([t[k] for t in taps]) for k in range(3)]
        assert st.num_frames == want[b][2] and st.is_speech == want[b][1]
        assert vt.same_bits(got_taps[0], want[b][0][0]) and vt.same_bits(got_taps[1], want[b][0][1]) and np.array_equal(got_taps[2], want[b][0][2])
        with pytest.raises(K2HipError) as e:   # the rate rule: a stream's rate is fixed by its first samples
            st.accept_waveform(44100 if rate != 44100 else 16000, x[:100])
        assert e.value.code == -1 and str(rate) in str(e.value) and "44100" in str(e.value)
        st.flush()
        assert st.segments() == want[b][3]
        st.accept_waveform(44100, np.zeros(500, np.float32))   # after a flush the rate is open again
        st.close()
    # a batch: the three streams in one call per round, the 8 kHz stream in calls of its own (one rate per call)
    streams = [VadStream(m, cfg) for _ in range(2)]
    for lo in range(0, max(len(x) for x in x16), 7001):
        m.vad_accept_samples(streams, 16000, [x[lo:lo + 7001] for x in x16])
    for b, st in enumerate(streams):
        assert st.num_frames == want[b][2]
        st.flush()
        assert st.segments() == want[b][3]
        st.close()
    with pytest.raises(K2HipError) as e:
        VadStream(m, cfg).accept_waveform(16001, x16[0][:1000])
    assert e.value.code == -6


# ---- long recordings -----------------------------------------------------------------------------------------------------------------
LONG_SPEECH, LONG_GAPS = [2.2, 1.8, 2.5, 1.6, 1.4], [0.8, 0.7, 0.9, 0.7, 0.4]   # 13 s, four pauses between five utterances


@pytest.fixture(scope="module")
def ctc_tiny(tmp_path_factory):
    from k2transducerasr_amd import Model
    from k2transducerasr_amd.synth import write_synthetic_model
    p = str(tmp_path_factory.mktemp("models") / "ctc_tiny.k2w")
    write_synthetic_model(p, "zipformer2-ctc-tiny-test")
    return Model(p, 0)


@pytest.mark.parametrize("which", ["zipformer2-tiny-test", "zipformer2-ctc-tiny-test"])
def test_recognize_long_equals_the_offline_path_on_the_segments(hip_tiny, ctc_tiny, oracle_tiny, which):
    model = hip_tiny if which == "zipformer2-tiny-test" else ctc_tiny
    x = recording(LONG_SPEECH, LONG_GAPS, 8)
    cfg = model.vad_default_config().copy(max_speech=150)
    # the CPU twin alone, on the oracle's fbank, already shows at least 4 segments and a forced cut
    tw = vt.Twin(cfg)
    tp = tw.taps(oracle_tiny.fbank(x))
    twin_segs = tw.machine(tp["d"], tp["m"])[0]
    assert len(twin_segs) >= 4 and sum(f for _, _, f in twin_segs) >= 1
    res = model.recognize_long(x, config=cfg, max_batch=3, max_batch_frames=700)
    assert len(res) >= 4 and sum(g["forced"] for g in res) >= 1
    # the segments are the detector's over the library's own features
    ref = vt.ref_run(cfg, model.fbank(x))
    assert [(g["start"], g["end"], g["forced"]) for g in res] == ref["segs"]
    assert vt.lib_pack([g["end"] - g["start"] for g in res], 3, 700) == (0, [g["batch"] for g in res])
    assert len({g["batch"] for g in res}) >= 2
    total = 0
    for b in sorted({g["batch"] for g in res}):
        mine = [g for g in res if g["batch"] == b]
        slices = [x[g["start"] * 160: (g["end"] - 1) * 160 + 400] for g in mine]
        want = model.offline_greedy_from_samples(slices)
        for g, (tok, ts) in zip(mine, want):
            assert (g["tokens"], g["timestamps"]) == (list(tok), list(ts)), (b, g["start"])
            total += len(tok)
    assert total > 0
    # at 8 kHz: the recording goes through the resampler first
    x8 = recording(LONG_SPEECH[:2], LONG_GAPS[:2], 8, rate=8000)
    res8 = model.recognize_long(x8, sample_rate=8000, config=cfg, max_batch=8)
    y = model.resample(x8, 8000)
    assert [(g["start"], g["end"], g["forced"]) for g in res8] == vt.ref_run(cfg, model.fbank(y))["segs"] and len(res8) >= 2
    want = model.offline_greedy_from_samples([y[g["start"] * 160: (g["end"] - 1) * 160 + 400] for g in res8])
    assert [(g["tokens"], g["timestamps"]) for g in res8] == [(list(a), list(b)) for a, b in want]


def test_long_entry_refusals(hip_tiny):
    from k2transducerasr_amd import K2HipError
    x = recording([1.0], [0.5], 1)
    for kw, code in ((dict(max_batch=0), -1), (dict(max_batch_frames=0), -1), (dict(config=hip_tiny.vad_default_config().copy(min_silence=5)), -1),
                     (dict(sample_rate=16001), -6)):
        with pytest.raises(K2HipError) as e:
            hip_tiny.recognize_long(x, **kw)
        assert e.value.code == code, kw
    assert hip_tiny.recognize_long(np.zeros(100, np.float32)) == []          # shorter than a frame
    assert hip_tiny.recognize_long(np.zeros(16000, np.float32)) == []        # silence: no segment


def test_isolation(hip_tiny, utts):
    """a decode before and after VAD use on the same model gives identical tokens"""
    from k2transducerasr_amd import VadStream
    before = hip_tiny.offline_greedy_from_samples(utts)
    st = VadStream(hip_tiny)
    st.accept_features(speechy(300, 1))
    st.accept_waveform(16000, utts[0])
    hip_tiny.recognize_long(recording([1.2, 1.0], [0.6, 0.5], 3))
    st.close()
    assert hip_tiny.offline_greedy_from_samples(utts) == before
