"""N-gram LM shallow fusion in the STREAMING modified beam search on the GPU: after every step a stream holds what the offline LM
search gives over all frames so far -- against the engine's own offline search (exactly) and against the Python twin
(tests/ngram_twin.py), at operator level (BeamStream, ragged chunk lengths) and fused (OnlineStream), with and without per-stream
hotwords; a stream keeps the LM it started with; no LM, a cleared LM and scale = 0 are the plain steps bit for bit."""
import contextlib
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import parity
from hotword_twin import SCORE, TwinGraph, draw_phrases
from kat_model import frames, write_kat_model, write_wide_model
from ngram_twin import KAT_LM_FLIP, SCALE, WIDE_VOCAB, TwinLm, draw_lm, kat_lm_flip_score, tiny_lm, twin_beam_search, wide_enc, wide_lm
from test_online_beam_gpu import BLANK_BIAS, SCORE_TOL, fused_score_ok, oracle_beam, oracle_frames

RAGGED = (5, 1, 9, 3, 13, 2, 7)     # chunk lengths, repeated until the frames run out


@contextlib.contextmanager
def launches(v):
    from k2transducerasr_amd import set_switch
    set_switch("K2HIP_BEAM_LAUNCHES", v)
    try:
        yield
    finally:
        set_switch("K2HIP_BEAM_LAUNCHES", 0)


def launch_counts():
    from k2transducerasr_amd import load_library
    L = load_library()
    L.k2hip_debug_beam_launch_counts.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    a, b = C.c_int64(), C.c_int64()
    assert L.k2hip_debug_beam_launch_counts(C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def _lm(model, entries):
    from k2transducerasr_amd import NgramLm
    return NgramLm(entries, model.vocab_size)


def ragged_ends(T):
    ends, n, i = [], 0, 0
    while n < T:
        n = min(T, n + RAGGED[i % len(RAGGED)])
        ends.append(n)
        i += 1
    return ends


def feed(model, enc, beam, ends, graphs, check):
    """enc [B, T, J] through B BeamStreams (graphs[b] or None attached) in the chunks that end at `ends`; check(n, streams) after each"""
    from k2transducerasr_amd import BeamStream
    ss = [BeamStream(model, beam) for _ in range(enc.shape[0])]
    try:
        for s, g in zip(ss, graphs):
            if g is not None:
                s.set_hotwords(g)
        n = 0
        for m in ends:
            BeamStream.search_chunk(ss, enc[:, n:m])
            n = m
            check(n, ss)
        return [(s.tokens, s.timestamps) for s in ss]
    finally:
        for s in ss:
            s.close()


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    from k2transducerasr_amd import Model
    from oracle import Oracle
    p = str(tmp_path_factory.mktemp("lm_stream_wide") / "wide.k2w")
    write_wide_model(p, WIDE_VOCAB)
    return Model(p, 0), Oracle(p)


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("with_hotwords", [False, True])
@pytest.mark.parametrize("beam", [4, 8])
def test_operator_level_ragged_chunks_equal_the_offline_lm_search(wide, beam, with_hotwords, form):
    """V = 400, 8 streams, ragged chunks: after every call every stream equals the engine's offline search with the same LM (and
    hotwords) over the frames so far exactly, and the twin up to its own near-ties"""
    from k2transducerasr_amd import Hotwords
    m, ora = wide
    enc = wide_enc()
    B, T = enc.shape[:2]
    unbiased = ora.modified_beam_search(enc, beam)
    entries = wide_lm(unbiased, beam)
    phrases = draw_phrases(unbiased, 12, np.random.default_rng(5)) if with_hotwords else None
    ends = ragged_ends(T)
    lm = _lm(m, entries)
    m.set_ngram_lm(lm, SCALE)
    lm.close()
    hw = Hotwords(phrases, SCORE, m.vocab_size) if phrases else None
    try:
        m.set_hotwords(hw)          # (the model-level list is the offline batch's: cleared again before the streams run)
        want = {n: m.beam_search(enc[:, :n], beam, want_scores=True) for n in ends}
        m.set_hotwords(None)
        twin_lm, graph = TwinLm(entries, WIDE_VOCAB), TwinGraph(phrases, SCORE, WIDE_VOCAB) if phrases else None
        near = [0]

        def check(n, ss):
            res, sc = want[n]
            for b, s in enumerate(ss):
                assert (s.tokens, s.timestamps) == tuple(res[b]), (beam, form, n, b)
                assert abs(s.score - float(sc[b])) <= SCORE_TOL, (beam, form, n, b, s.score, float(sc[b]))
            if n in (ends[len(ends) // 2], T):      # the twin at two prefixes (it costs T' oracle steps per stream)
                for b, s in enumerate(ss):
                    tw = twin_beam_search(ora, enc[b, :n], beam, twin_lm, SCALE, graph)
                    exact = parity.assert_beam_match([(s.tokens, s.timestamps)], [(tw["ys"], tw["ts"])], tw["margins"][None], tol=parity.LOGIT_TOL,
                                                     what=f"stream LM beam={beam} hw={with_hotwords} form={form} n={n} b={b}", allow_tie=True)
                    near[0] += 1 - exact
                    if exact:
                        assert abs(s.score - tw["lp"]) <= SCORE_TOL, (n, b, s.score, tw["lp"])

        with launches(form):
            got = feed(m, enc, beam, ends, [hw] * B, check)
        assert 8 * near[0] <= 2 * B, f"{near[0]} of {2 * B} (stream, prefix) comparisons with the twin pass only as near-ties"
        m.set_ngram_lm(None)
        assert got != [tuple(r) for r in m.beam_search(enc, beam)], "the LM moves no stream: the case shows nothing"
    finally:
        m.set_ngram_lm(None)
        m.set_hotwords(None)
        if hw is not None:
            hw.close()


@pytest.mark.parametrize("form", [0, 1])
def test_kat_lm_flip_frame_by_frame(tmp_path_factory, form):
    """ngram_twin.KAT_LM_FLIP one frame per call: the LM state of [5] crosses the chunk boundary and earns the bigram at t1"""
    from k2transducerasr_amd import BeamStream, Model
    p = str(tmp_path_factory.mktemp("lm_stream_kat") / "kat.k2w")
    write_kat_model(p)
    kat = Model(p, 0)
    K = KAT_LM_FLIP
    kat.set_ngram_lm(_lm(kat, K["entries"]), K["scale"])
    enc = frames(K["rows"])[None]
    with launches(form):
        s = BeamStream(kat, K["beam"])
        for t in range(3):
            BeamStream.search_chunk([s], enc[:, t:t + 1])
        assert (s.tokens, s.timestamps) == K["fused"]
        assert abs(s.score - kat_lm_flip_score()) < 1e-5, (s.score, kat_lm_flip_score())
        s.reset()                       # every hypothesis back at the start state
        for t in range(3):
            BeamStream.search_chunk([s], enc[:, t:t + 1])
        assert (s.tokens, s.timestamps) == K["fused"]
        s.close()
    kat.close()


def test_a_stream_keeps_the_lm_it_started_with(wide):
    """changing or clearing the LM mid-stream is refused until the stream is reset, and the failed call changes no stream"""
    from k2transducerasr_amd import BeamStream, K2HipError
    m, ora = wide
    enc = wide_enc()
    entries = wide_lm(ora.modified_beam_search(enc, 4), 4)
    m.set_ngram_lm(_lm(m, entries), SCALE)
    a, b = BeamStream(m, 4), BeamStream(m, 4)
    try:
        BeamStream.search_chunk([a], enc[:1, :10])
        before = (a.tokens, a.timestamps, np.float32(a.score).tobytes())
        for setting in ((None, 0.0), (_lm(m, entries), SCALE), (_lm(m, entries), 0.25)):     # cleared, set again (a new upload), changed
            m.set_ngram_lm(*setting)
            with pytest.raises(K2HipError) as e:
                BeamStream.search_chunk([b, a], enc[[1, 0], 10:20])       # b is fresh and could run: the call fails as a whole
            assert e.value.code == -1 and "reset the stream first" in str(e.value)
            assert (a.tokens, a.timestamps, np.float32(a.score).tobytes()) == before
            assert (b.tokens, b.timestamps) == ([], [])
        a.reset()
        BeamStream.search_chunk([b, a], enc[[1, 0], :10])                 # after the reset a runs with the LM now set (scale 0.25)
        m.set_ngram_lm(_lm(m, entries), 0.25)
        a2 = BeamStream(m, 4)
        # (the upload above is a new setting again: a and b are held to it only after another reset)
        a.reset()
        BeamStream.search_chunk([a, a2], enc[[0, 0], :10])
        assert (a.tokens, a.timestamps) == (a2.tokens, a2.timestamps)
        a2.close()
    finally:
        m.set_ngram_lm(None)
        a.close()
        b.close()


def test_bit_equal_when_unused_and_the_plain_kernels_run(wide):
    from k2transducerasr_amd import BeamStream
    m, ora = wide
    enc = wide_enc()
    entries = wide_lm(ora.modified_beam_search(enc, 4), 4)
    for form in (0, 1):
        for beam in (1, 2, 4, 8):
            with launches(form):
                def run():
                    s = BeamStream(m, beam)
                    out = []
                    for n in range(0, enc.shape[1], 8):
                        BeamStream.search_chunk([s], enc[:1, n:n + 8])
                        out.append((s.tokens, s.timestamps, np.float32(s.score).tobytes()))
                    s.close()
                    return out
                m.set_ngram_lm(None)
                p0, h0 = launch_counts()
                want = run()
                m.set_ngram_lm(_lm(m, entries), SCALE)
                fused = run()
                m.set_ngram_lm(None)
                p1, h1 = launch_counts()
                assert (p1 - p0, h1 - h0) == (len(want), len(want))
                assert run() == want, "cleared"
                m.set_ngram_lm(_lm(m, entries), 0.0)
                assert run() == want, "scale = 0"
                m.set_ngram_lm(None)
                assert launch_counts() == (p1 + 2 * len(want), h1), "without an LM only the plain kernels may launch"
                if beam >= 2:
                    assert fused != want


@pytest.mark.parametrize("preset", ["zipformer2-streaming-tiny-test", "lstm-tiny-test"])
def test_fused_step_with_lm_and_per_stream_hotwords(tmp_path_factory, preset):
    """ragged streams through OnlineRecognizer(ngram_lm=...) to their end: two with hotword lists of their own, two without -- each
    checked after every get_results against the twin over its own concatenated oracle frames.  The streams finish at different
    ticks, so the ready set shrinks below the list (the LM side block is indexed by ready stream).  Then, on a second recognizer,
    the LM is cleared mid-stream: the step is refused and changes nothing until the streams are reset."""
    from k2transducerasr_amd import K2HipError, NgramLm, OnlineRecognizer
    from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model
    from oracle.online import OnlineOracle
    path = str(tmp_path_factory.mktemp("lm_fused") / f"{preset}.k2w")
    write_synthetic_model(path, preset, blank_bias=BLANK_BIAS.get(preset))
    beam = 4
    ora = OnlineOracle(path)
    utts = [synth_utterance(20 + u, d) for u, d in enumerate([2.4, 1.3, 1.9, 1.6])]
    feats = [ora.fbank(u) for u in utts]
    fr = [oracle_frames(ora, f) for f in feats]
    unbiased = [oracle_beam(ora, enc, beam) for enc, _ in fr]
    entries = draw_lm([u[:2] for u in unbiased], ora.vocab_size, np.random.default_rng(3))
    twin_lm = TwinLm(entries, ora.vocab_size)
    rec = OnlineRecognizer(path, decoding_method="modified_beam_search", beam=beam, ngram_lm=NgramLm(entries, ora.vocab_size), ngram_lm_scale=SCALE)
    lists = [draw_phrases([unbiased[0][:2]], 5, np.random.default_rng(1)), None, draw_phrases([unbiased[2][:2]], 5, np.random.default_rng(2)), None]
    assert lists[0] and lists[2]
    hs = [rec.create_online_stream(hotwords=l, hotwords_score=SCORE) if l else rec.create_online_stream() for l in lists]
    for h, f in zip(hs, feats):
        h.add_features(f)
    B = len(hs)
    done, prev, moved, ticks, near, compared, subset_ticks = [0] * B, [2] * B, False, 0, 0, 0, 0
    while True:
        dec, n_new = rec.get_results(hs)
        if not any(dec):
            break
        subset_ticks += 0 < sum(bool(d) for d in dec) < B
        for b, h in enumerate(hs):
            if not dec[b]:
                continue
            done[b] += 1
            enc, cum = fr[b]
            n = cum[done[b] - 1]
            tw = twin_beam_search(ora, enc[:n], beam, twin_lm, SCALE, TwinGraph(lists[b], SCORE, ora.vocab_size) if lists[b] else None)
            moved = moved or (tw["ys"], tw["ts"]) != tuple(oracle_beam(ora, enc[:n], beam)[:2])
            exact = parity.assert_beam_match([(h.tokens[2:], h.timestamps)], [(tw["ys"], tw["ts"])], tw["margins"][None], tol=parity.LOGIT_TOL,
                                             what=f"fused LM {preset} tick={ticks} b={b}", allow_tie=True)
            compared += 1
            near += 1 - exact
            if exact:
                assert h.hyp == ([0, 0] + tw["ys"])[-2:]
                assert fused_score_ok(h.score, tw["lp"]), (preset, ticks, b, h.score, tw["lp"])
            assert n_new[b] == len(h.tokens) - prev[b]
            prev[b] = len(h.tokens)
        ticks += 1
    assert done == [len(f[1]) for f in fr] and len(set(done)) > 1, "every stream must decode all its chunks, and they must not end together"
    assert subset_ticks >= 1, "the ready set was never a proper subset of the streams"
    assert 8 * near <= compared, f"{near} of {compared} (stream, tick) comparisons with the twin pass only as near-ties"
    assert moved, "the LM moved no stream: the case shows nothing"
    for h in hs:
        h.close()
    # a second recognizer, stopped after two ticks: clearing or changing the LM is refused for the streams that started with it
    rec2 = OnlineRecognizer(path, decoding_method="modified_beam_search", beam=beam, ngram_lm=NgramLm(entries, ora.vocab_size), ngram_lm_scale=SCALE)
    hs = [rec2.create_online_stream() for _ in range(2)]
    for h, f in zip(hs, feats):
        h.add_features(f)
    for _ in range(2):
        assert all(rec2.get_results(hs)[0])
    held = [(h.tokens, h.timestamps, np.float32(h.score).tobytes()) for h in hs]
    for setting in ((None, 0.0), (NgramLm(entries, ora.vocab_size), 0.25)):
        rec2.model.set_ngram_lm(*setting)
        with pytest.raises(K2HipError) as e:
            rec2.get_results(hs)
        assert e.value.code == -1 and "reset the stream first" in str(e.value)
        assert [(h.tokens, h.timestamps, np.float32(h.score).tobytes()) for h in hs] == held
    for h in hs:
        h.close()
