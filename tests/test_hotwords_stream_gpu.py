"""Per-stream hotword biasing of the STREAMING modified beam search on the GPU (k2hip_online_stream_set_hotwords,
k2hip_beam_stream_set_hotwords): after every step a stream holds what the offline biased search gives over all frames so far --
against the engine's own offline search (exactly), against the Python twin (tests/hotword_twin.py; no near-tie is excused here: the
streaming search has no per-frame tap to localise one with), on the hand-derived KAT case, through the fused chunk step, and the
lifecycle of the attached graphs."""
import contextlib
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import parity
from hotword_stream_cases import SCORE_TOL, STEPS, STREAM_BEAMS, STREAM_PRESET, stream_case, twin_prefix
from hotword_twin import (KAT_FLIP, SCORE, TINY_BEAMS, WIDE_BEAMS, WIDE_VOCAB, TwinGraph, draw_phrases, kat_flip_score, tiny_phrases,
                          twin_beam_search, wide_enc, wide_phrases)
from kat_model import frames, write_kat_model, write_wide_model
from test_online_beam_gpu import BLANK_BIAS, fused_score_ok, oracle_beam, oracle_frames


@contextlib.contextmanager
def launches(v):
    from k2transducerasr_amd import set_switch
    set_switch("K2HIP_BEAM_LAUNCHES", v)
    try:
        yield
    finally:
        set_switch("K2HIP_BEAM_LAUNCHES", 0)


def _lib():
    from k2transducerasr_amd import load_library
    L = load_library()
    L.k2hip_debug_stream_hotword_uploads.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.k2hip_debug_beam_launch_counts.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    return L


def launch_counts():
    a, b = C.c_int64(), C.c_int64()
    assert _lib().k2hip_debug_beam_launch_counts(C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def uploads(model):
    a, b = C.c_int32(), C.c_int32()
    assert _lib().k2hip_debug_stream_hotword_uploads(model.handle, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def _hw(model, phrases, score=SCORE):
    from k2transducerasr_amd import Hotwords
    return Hotwords(phrases, score, model.vocab_size)


@pytest.fixture(scope="module")
def tiny_stream(tmp_path_factory):
    from k2transducerasr_amd import Model
    from k2transducerasr_amd.synth import write_synthetic_model
    p = str(tmp_path_factory.mktemp("hw_stream") / "stream.k2w")
    write_synthetic_model(p, STREAM_PRESET, blank_bias=0.0)
    ora, enc, unbiased, phrases = stream_case(p)
    return Model(p, 0), ora, enc, unbiased, phrases


def offline_prefixes(model, enc, beam, hw, ends):
    """the engine's offline biased search over enc[:, :n] for every n in ends (enc [B, T, J]); the model-level list is cleared again"""
    out = {}
    model.set_hotwords(hw)
    try:
        for n in ends:
            out[n] = model.beam_search(enc[:, :n], beam, want_scores=True)
    finally:
        model.set_hotwords(None)
    return out


def feed(model, enc, beam, step, graphs, check):
    """enc [B, T, J] through B BeamStreams (graphs[b] or None attached) in chunks of `step`; check(n, streams) after every call"""
    from k2transducerasr_amd import BeamStream
    ss = [BeamStream(model, beam) for _ in range(enc.shape[0])]
    try:
        for s, g in zip(ss, graphs):
            if g is not None:
                s.set_hotwords(g)
        n, T = 0, enc.shape[1]
        while n < T:
            m = min(T, n + (step or T))
            BeamStream.search_chunk(ss, enc[:, n:m])
            n = m
            check(n, ss)
        return [(s.tokens, s.timestamps) for s in ss]
    finally:
        for s in ss:
            s.close()


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("beam", STREAM_BEAMS)
def test_operator_level_equals_the_offline_biased_search_and_the_twin(tiny_stream, beam, form):
    """items 4 and 5 on the streaming tiny model's oracle frames: every chunking, after every call"""
    model, ora, enc, unbiased, phrases = tiny_stream
    hw = _hw(model, phrases)
    N = enc.shape[0]
    want = offline_prefixes(model, enc[None], beam, hw, range(1, N + 1))
    checks = [0]

    def check(n, ss):
        (res,), sc = want[n]
        assert (ss[0].tokens, ss[0].timestamps) == (res[0], res[1]), (beam, form, n)
        assert abs(ss[0].score - float(sc[0])) <= SCORE_TOL, (beam, form, n, ss[0].score, float(sc[0]))
        tw = twin_prefix("stream", ora, enc, n, beam, phrases)
        parity.assert_beam_match([(ss[0].tokens, ss[0].timestamps)], [(tw["ys"], tw["ts"])], tw["margins"][None], tol=parity.LOGIT_TOL,
                                 what=f"stream beam={beam} form={form} n={n}", allow_tie=True)
        assert abs(ss[0].score - tw["lp"]) <= SCORE_TOL, (beam, form, n, ss[0].score, tw["lp"])
        checks[0] += 1

    with launches(form):
        got = [feed(model, enc[None], beam, step, [hw], check) for step in STEPS]
    hw.close()
    assert all(g == got[0] for g in got)
    if beam >= 2:
        assert got[0][0] != tuple(oracle_beam(ora, enc, beam)[:2]), "the phrases do not move the result: the case shows nothing"
    print(f"beam={beam} form={form}: {checks[0]} (stream, prefix) checks, all exact")


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("beam", TINY_BEAMS)
def test_tiny_batch_mixed_graphs(hip_tiny, oracle_tiny, utts, beam, form):
    """the offline tiny model over the utts batch in chunks of 8: streams with the graph and streams with none in ONE call, each held
    to the offline search (biased / unbiased) and, the biased ones, to the twin"""
    f = [oracle_tiny.fbank(u) for u in utts]
    enc = oracle_tiny.encoder(oracle_tiny.pad_sequence(f).reshape(len(utts), -1, 80))
    B, T = enc.shape[:2]
    phrases = tiny_phrases(oracle_tiny.modified_beam_search(enc, beam))
    hw = _hw(hip_tiny, phrases)
    ends = sorted(set(range(8, T, 8)) | {T})
    biased = offline_prefixes(hip_tiny, enc, beam, hw, ends)
    plain = {n: hip_tiny.beam_search(enc[:, :n], beam, want_scores=True) for n in ends}
    has = [b % 2 == 0 for b in range(B)]

    def check(n, ss):
        for b, s in enumerate(ss):
            res, sc = (biased if has[b] else plain)[n]
            assert (s.tokens, s.timestamps) == tuple(res[b]), (beam, form, n, b)
            assert abs(s.score - float(sc[b])) <= SCORE_TOL
            if has[b]:
                tw = twin_prefix(("tiny", beam, b), oracle_tiny, enc[b], n, beam, phrases)
                assert (s.tokens, s.timestamps) == (tw["ys"], tw["ts"]), (beam, form, n, b)
                assert abs(s.score - tw["lp"]) <= SCORE_TOL

    with launches(form):
        feed(hip_tiny, enc, beam, 8, [hw if h else None for h in has], check)
    hw.close()


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("beam", WIDE_BEAMS)
def test_wide_batch(tmp_path_factory, beam, form):
    """V = 400 (two 256-column chunks per frame), chunks of 13, against the offline biased search and the twin"""
    from k2transducerasr_amd import Model
    from oracle import Oracle
    p = str(tmp_path_factory.mktemp("hw_stream_wide") / "wide.k2w")
    write_wide_model(p, WIDE_VOCAB)
    m, ora = Model(p, 0), Oracle(p)
    enc = wide_enc()
    B, T = enc.shape[:2]
    phrases = wide_phrases(ora.modified_beam_search(enc, beam))
    hw = _hw(m, phrases)
    ends = sorted(set(range(13, T, 13)) | {T})
    want = offline_prefixes(m, enc, beam, hw, ends)

    def check(n, ss):
        res, sc = want[n]
        for b, s in enumerate(ss):
            assert (s.tokens, s.timestamps) == tuple(res[b]), (beam, form, n, b)
            assert abs(s.score - float(sc[b])) <= SCORE_TOL
            tw = twin_prefix(("wide", beam, b), ora, enc[b], n, beam, phrases)
            assert (s.tokens, s.timestamps) == (tw["ys"], tw["ts"]), (beam, form, n, b)

    with launches(form):
        got = feed(m, enc, beam, 13, [hw] * B, check)
    assert got != [tuple(r) for r in m.beam_search(enc, beam)]
    hw.close()
    m.close()


@pytest.mark.parametrize("form", [0, 1])
def test_kat_flip_frame_by_frame(tmp_path_factory, form):
    """hotword_twin.KAT_FLIP one frame per call: the unfinished [5] earns nothing at the step's pick, though its bonus is carried"""
    from k2transducerasr_amd import BeamStream, Model
    p = str(tmp_path_factory.mktemp("hw_stream_kat") / "kat.k2w")
    write_kat_model(p)
    kat = Model(p, 0)
    hw = _hw(kat, KAT_FLIP["phrases"])
    enc = frames(KAT_FLIP["rows"])[None]
    with launches(form):
        s = BeamStream(kat, KAT_FLIP["beam"])
        s.set_hotwords(hw)
        BeamStream.search_chunk([s], enc[:, 0:1])
        assert s.tokens == [6]
        BeamStream.search_chunk([s], enc[:, 1:2])
        assert s.tokens == [5, 7]
        BeamStream.search_chunk([s], enc[:, 2:3])
        assert (s.tokens, s.timestamps) == KAT_FLIP["biased"]
        assert abs(s.score - kat_flip_score()) < 1e-5, (s.score, kat_flip_score())
        s.reset()
        BeamStream.search_chunk([s], enc[:, 0:1])
        BeamStream.search_chunk([s], enc[:, 2:3])
        assert s.tokens == [6]
        s.close()
    hw.close()
    kat.close()


@pytest.mark.parametrize("preset", ["zipformer2-streaming-tiny-test", "zipformer-streaming-tiny-test", "lstm-tiny-test"])
def test_fused_step_with_two_graphs_and_none(tmp_path_factory, preset):
    """three ragged streams through OnlineRecognizer: graph A, graph B, none -- each checked after every get_results against the
    twin over its own concatenated oracle frames"""
    from k2transducerasr_amd import OnlineRecognizer
    from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model
    from oracle.online import OnlineOracle
    path = str(tmp_path_factory.mktemp("hw_fused") / f"{preset}.k2w")
    write_synthetic_model(path, preset, blank_bias=BLANK_BIAS.get(preset))
    beam = 4
    rec = OnlineRecognizer(path, decoding_method="modified_beam_search", beam=beam)
    ora = OnlineOracle(path)
    utts = [synth_utterance(20 + u, d) for u, d in enumerate([2.4, 1.3, 1.9])]
    feats = [ora.fbank(u) for u in utts]
    fr = [oracle_frames(ora, f) for f in feats]
    unbiased = [oracle_beam(ora, enc, beam) for enc, _ in fr]
    lists = [draw_phrases([unbiased[0][:2]], 5, np.random.default_rng(1)), draw_phrases([unbiased[1][:2]], 5, np.random.default_rng(2)), None]
    assert lists[0] and lists[1]
    hs = [rec.create_online_stream(hotwords=lists[0], hotwords_score=SCORE), rec.create_online_stream(hotwords=_hw(rec.model, lists[1])),
          rec.create_online_stream()]
    for h, f in zip(hs, feats):
        h.add_features(f)
    done, prev, ticks = [0] * 3, [2] * 3, 0
    moved = [False] * 3
    while True:
        dec, n_new = rec.get_results(hs)
        if not any(dec):
            break
        for b, h in enumerate(hs):
            if not dec[b]:
                continue
            done[b] += 1
            enc, cum = fr[b]
            n = cum[done[b] - 1]
            if lists[b] is None:
                tok, ts, sc = oracle_beam(ora, enc[:n], beam)
            else:
                tw = twin_beam_search(ora, enc[:n], beam, TwinGraph(lists[b], SCORE, ora.vocab_size))
                tok, ts, sc = tw["ys"], tw["ts"], tw["lp"]
                moved[b] = moved[b] or (tok, ts) != tuple(oracle_beam(ora, enc[:n], beam)[:2])
            want = [0, 0] + tok
            assert h.tokens == want and h.timestamps == ts, (preset, ticks, b)
            assert h.hyp == want[-2:]
            assert fused_score_ok(h.score, sc), (preset, ticks, b, h.score, sc)
            assert n_new[b] == len(want) - prev[b]
            prev[b] = len(want)
        ticks += 1
    assert done == [len(f[1]) for f in fr] and len(set(done)) > 1
    assert moved[0] or moved[1], "neither graph moved its stream: the case shows nothing"


def test_bit_equal_when_unused_and_the_plain_kernels_run(tiny_stream):
    from k2transducerasr_amd import BeamStream
    model, ora, enc, unbiased, phrases = tiny_stream
    for form in (0, 1):
        with launches(form):
            def run(graph):
                s = BeamStream(model, 4)
                if graph is not None:
                    s.set_hotwords(graph)
                    graph.close()
                out = []
                for n in range(0, enc.shape[0], 8):
                    BeamStream.search_chunk([s], enc[None, n:n + 8])
                    out.append((s.tokens, s.timestamps, np.float32(s.score).tobytes()))
                s.close()
                return out
            p0, h0 = launch_counts()
            want = run(None)
            p1, h1 = launch_counts()
            assert h1 == h0 and p1 - p0 == len(want), "a call without any graph must launch the HW = false kernels, and only those"
            assert run(_hw(model, [])) == want
            assert run(_hw(model, phrases, 0.0)) == want
            p2, h2 = launch_counts()
            assert h2 - h1 == 2 * len(want) and p2 == p1      # (attached graphs, even empty ones, run the HW = true kernels)
            assert run(_hw(model, phrases)) != want


def test_lifecycle(tiny_stream, tmp_path):
    from k2transducerasr_amd import BeamStream, Hotwords, K2HipError, OnlineRecognizer
    from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model
    model, ora, enc, unbiased, phrases = tiny_stream
    u0, r0 = uploads(model)
    hw = _hw(model, phrases)
    a, b = BeamStream(model, 4), BeamStream(model, 4)
    a.set_hotwords(hw)
    b.set_hotwords(hw)
    assert uploads(model) == (u0 + 1, r0 + 1), "two streams with the same Hotwords share one upload"
    hw.close()                                        # right after the attach: harmless
    BeamStream.search_chunk([a, b], np.stack([enc[:8], enc[:8]]))
    first = (a.tokens, a.timestamps, a.score)
    assert (b.tokens, b.timestamps, b.score) == first
    with pytest.raises(K2HipError) as e:              # not in the start state any more
        a.set_hotwords(None)
    assert e.value.code == -1 and "reset" in str(e.value)
    a.reset()                                         # keeps the graph, every hypothesis back at the root
    assert a.tokens == [] and a.score == 0.0
    BeamStream.search_chunk([a], enc[None, :8])
    assert (a.tokens, a.timestamps, a.score) == first
    a.reset()
    a.set_hotwords(None)                              # detach: the unbiased search
    BeamStream.search_chunk([a], enc[None, :8])
    assert (a.tokens, a.timestamps) == tuple(oracle_beam(ora, enc[:8], 4)[:2])
    assert uploads(model)[1] == r0 + 1                # b still holds it
    b.close()
    assert uploads(model)[1] == r0                    # the last stream let go: the tables are freed
    with pytest.raises(K2HipError) as e:
        a.reset()
        a.set_hotwords(Hotwords([[4, 5]], SCORE, model.vocab_size + 1))
    assert e.value.code == -1 and "vocab_size" in str(e.value)
    a.close()
    # the fused path: attach after the first chunk is refused, reset keeps the graph, greedy ignores it
    p = str(tmp_path / "s.k2w")
    write_synthetic_model(p, STREAM_PRESET, blank_bias=0.0)
    rec = OnlineRecognizer(p, decoding_method="modified_beam_search", beam=4)
    f = ora.fbank(synth_utterance(33, 2.0))

    def decode(s):
        s.add_features(f)
        while rec.get_results([s])[0][0]:
            pass
        return s.tokens, s.timestamps, s.score

    plain = decode(rec.create_online_stream())
    s = rec.create_online_stream(hotwords=phrases, hotwords_score=SCORE)
    s.add_features(f)
    rec.get_results([s])
    with pytest.raises(K2HipError) as e:
        s.set_hotwords(None)
    assert e.value.code == -1 and "reset" in str(e.value)
    s.reset()
    biased = decode(s)
    s.reset()
    assert decode(s) == biased
    fenc, _ = oracle_frames(ora, f)
    tw = twin_beam_search(ora, fenc, 4, TwinGraph(phrases, SCORE, ora.vocab_size))
    assert biased[:2] == ([0, 0] + tw["ys"], tw["ts"])
    rec.model.set_decoding_method("greedy_search")
    g0 = rec.create_online_stream()
    g1 = rec.create_online_stream(hotwords=phrases, hotwords_score=SCORE)
    for g in (g0, g1):
        g.add_features(f)
        while rec.get_results([g])[0][0]:
            pass
    assert (g1.tokens, g1.timestamps) == (g0.tokens, g0.timestamps)
    # stream destroyed after its model, as far as the graph is concerned (operator-level streams hold no device slot)
    from k2transducerasr_amd import Model
    m2 = Model(p, 0)
    late = BeamStream(m2, 4)
    late.set_hotwords(_hw(m2, phrases))
    m2.close()
    late.close()


def test_the_model_level_refusals_still_hold(tiny_stream):
    """with a model-level list set the streaming search is refused, graphs attached to the streams or not"""
    from k2transducerasr_amd import BeamStream, K2HipError
    model, ora, enc, unbiased, phrases = tiny_stream
    hw = _hw(model, phrases)
    s = BeamStream(model, 4)
    s.set_hotwords(hw)
    try:
        model.set_hotwords(hw)
        with pytest.raises(K2HipError) as e:
            BeamStream.search_chunk([s], enc[None, :8])
        assert e.value.code == -1 and "streaming" in str(e.value)
        assert s.tokens == []
    finally:
        model.set_hotwords(None)
    BeamStream.search_chunk([s], enc[None, :8])
    s.close()
    hw.close()


def test_large_vocabulary_launch_form_streaming_equals_offline(tmp_path_factory):
    """V = 2000 (zh streaming architecture): no decoder table, the k_beam_step form"""
    from k2transducerasr_amd import Model
    from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model
    from oracle.online import OnlineOracle
    path = str(tmp_path_factory.mktemp("hw_stream_zh") / "zh.k2w")
    write_synthetic_model(path, "zipformer2-streaming-zh")
    ora = OnlineOracle(path)
    enc, _ = oracle_frames(ora, ora.fbank(synth_utterance(61, 1.7)))
    model = Model(path)
    unb = model.beam_search(enc[None], 4)
    phrases = draw_phrases(unb, 6, np.random.default_rng(3))
    assert phrases
    hw = _hw(model, phrases)
    want = offline_prefixes(model, enc[None], 4, hw, range(1, enc.shape[0] + 1))
    assert tuple(want[enc.shape[0]][0][0]) != tuple(unb[0])

    def check(n, ss):
        (res,), sc = want[n]
        assert (ss[0].tokens, ss[0].timestamps) == tuple(res), n
        assert abs(ss[0].score - float(sc[0])) <= SCORE_TOL

    for step in (8, 5):
        feed(model, enc[None], 4, step, [hw], check)
    hw.close()
    model.close()
