"""Hotword biasing of the offline modified beam search on the GPU: libk2hip.so through the C ABI against the Python twin
(tests/hotword_twin.py; its own agreement with the CPU oracle at c = 0 is checked without a GPU in test_hotwords.py)."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import parity
from hotword_twin import (KAT_FLIP, SCORE, TINY_BEAMS, WIDE_BEAMS, WIDE_VOCAB, TwinGraph, draw_phrases, kat_flip_score, tiny_phrases,
                          twin_batch, wide_enc, wide_phrases)
from kat_model import frames, write_kat_model, write_wide_model


@contextlib.contextmanager
def switches(**kw):
    import k2transducerasr_amd as pkg
    try:
        for k, v in kw.items():
            pkg.set_switch(k, v)
        yield
    finally:
        for k in kw:
            pkg.set_switch(k, 1024 if k == "K2HIP_DECODER_TABLE_MB" else 0)


# the forms of the search (the id says which one ran): the fused kernel as the shape selects it (two column slabs per stream for
# 256 < V <= 512 at beam <= 4, else one workgroup per stream), forced to one slab, with its hypotheses in device memory, and the
# per-frame k_beam_step path -- forced by the switch, and because no decoder table exists
FORMS = {
    "k_beam_loop": {},
    "k_beam_loop-one-slab": {"K2HIP_BEAM_PARTS": 1},
    "k_beam_loop-hyp-global": {"K2HIP_BEAM_HYP_GLOBAL": 1},
    "k_beam_step-launches": {"K2HIP_BEAM_LAUNCHES": 1},
}


@pytest.fixture(scope="module")
def enc_tiny(oracle_tiny, utts):
    f = [oracle_tiny.fbank(u) for u in utts]
    return oracle_tiny.encoder(oracle_tiny.pad_sequence(f).reshape(len(utts), -1, 80))


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    from k2transducerasr_amd import Model
    from oracle import Oracle
    p = str(tmp_path_factory.mktemp("hw_wide") / "wide.k2w")
    write_wide_model(p, WIDE_VOCAB)
    return p, Oracle(p)


@pytest.fixture(scope="module")
def kat(tmp_path_factory):
    from k2transducerasr_amd import Model
    p = str(tmp_path_factory.mktemp("hw_kat") / "kat.k2w")
    write_kat_model(p)
    return Model(p, 0)


def _hw(model, phrases, score=SCORE):
    from k2transducerasr_amd import Hotwords
    return Hotwords(phrases, score, model.vocab_size)


@pytest.mark.parametrize("beam", [1, 2, 4, 8])
def test_unbiased_results_are_bit_equal(hip_tiny, enc_tiny, beam):
    """no hotwords, cleared hotwords, an empty list and a list with c = 0: tokens, timestamps and scores as before any were set"""
    hip_tiny.set_hotwords(None)
    want, wsc = hip_tiny.beam_search(enc_tiny, beam, want_scores=True)
    phrases = tiny_phrases(want) or [[4, 5]]
    try:
        hip_tiny.set_hotwords(_hw(hip_tiny, phrases))
        biased = hip_tiny.beam_search(enc_tiny, beam)
        hip_tiny.set_hotwords(None)
        for what, graph in (("cleared", None), ("empty list", _hw(hip_tiny, [])), ("c = 0", _hw(hip_tiny, phrases, 0.0))):
            if graph is not None:
                hip_tiny.set_hotwords(graph)
                graph.close()        # the model keeps its own copy
            got, gsc = hip_tiny.beam_search(enc_tiny, beam, want_scores=True)
            assert got == want, what
            assert gsc.tobytes() == wsc.tobytes(), what
        if beam >= 2:
            assert biased != want      # (the list does bias: the comparisons above are not vacuous)
    finally:
        hip_tiny.set_hotwords(None)


def test_unbiased_get_results_and_greedy(tiny_model_path, utts):
    from k2transducerasr_amd import Hotwords, OfflineRecognizer
    rec = OfflineRecognizer(tiny_model_path, 0, "modified_beam_search", 4)

    def run():
        ss = [rec.create_offline_stream() for _ in utts]
        for s, u in zip(ss, utts):
            s.add_samples(u)
        return rec.get_results(ss), rec.model.last_scores(len(utts)).tobytes()

    want = run()
    phrases = tiny_phrases([(t[2 * len(utts):], ts) for t, ts in want[0]]) or [[4, 5]]
    rec.model.set_hotwords(Hotwords(phrases, SCORE, rec.model.vocab_size))
    biased = run()
    assert biased[0] != want[0]
    for graph in (None, Hotwords([], SCORE, rec.model.vocab_size), Hotwords(phrases, 0.0, rec.model.vocab_size)):
        rec.model.set_hotwords(graph)
        assert run() == want
    # the constructor's form, and greedy search ignores the hotwords
    rec2 = OfflineRecognizer(tiny_model_path, 0, "modified_beam_search", 4, hotwords=phrases, hotwords_score=SCORE)
    ss = [rec2.create_offline_stream() for _ in utts]
    for s, u in zip(ss, utts):
        s.add_samples(u)
    assert rec2.get_results(ss) == biased[0]
    m = rec.model
    m.set_decoding_method("greedy_search")
    m.set_hotwords(None)
    g = m.offline_greedy_from_samples(utts)
    m.set_hotwords(Hotwords(phrases, SCORE, m.vocab_size))
    assert m.offline_greedy_from_samples(utts) == g
    # a graph built for another vocabulary is refused
    from k2transducerasr_amd import K2HipError
    with pytest.raises(K2HipError) as e:
        m.set_hotwords(Hotwords([[4, 5]], SCORE, m.vocab_size + 1))
    assert e.value.code == -1 and "vocab_size" in str(e.value)


def test_kat_flip(kat):
    """hotword_twin.KAT_FLIP (derived by hand there): the phrase [5, 7] flips [6, 7] into [5, 7]"""
    enc = frames(KAT_FLIP["rows"])[None]
    kat.set_hotwords(None)
    assert kat.beam_search(enc, KAT_FLIP["beam"])[0] == KAT_FLIP["unbiased"]
    kat.set_hotwords(_hw(kat, KAT_FLIP["phrases"]))
    try:
        for form, sw in FORMS.items():
            with switches(**sw):
                got, sc = kat.beam_search(enc, KAT_FLIP["beam"], want_scores=True)
            assert got[0] == KAT_FLIP["biased"], form
            assert abs(float(sc[0]) - kat_flip_score()) < 1e-5, (form, float(sc[0]), kat_flip_score())
        cut = frames([KAT_FLIP["rows"][0], KAT_FLIP["rows"][2]])[None]     # an unfinished match earns nothing
        assert kat.beam_search(cut, KAT_FLIP["beam"])[0][0] == [6]
    finally:
        kat.set_hotwords(None)


def _against_twin(model, ora, enc, beam, phrases, sw, what):
    graph = TwinGraph(phrases, SCORE, ora.vocab_size)
    want, wsc, mg, wtr, ev = twin_batch(ora, enc, beam, graph)
    assert min(ev.values()) >= 1, f"{what}: bonuses, broken and committed matches must all occur on the twin: {ev}"
    model.set_hotwords(_hw(model, phrases))
    try:
        with switches(K2HIP_BEAM_TRACE=1, **sw):
            got, gsc = model.beam_search(enc, beam, want_scores=True)
            gtr = model.beam_trace()
    finally:
        model.set_hotwords(None)
    before = len(parity.NEAR_TIES)
    exact = parity.assert_beam_match(got, want, mg, tol=parity.LOGIT_TOL, what=what, allow_tie=True, trace_got=gtr, trace_want=wtr)
    print(f"{what}: {exact}/{len(want)} streams exact, events {ev}, near ties {parity.NEAR_TIES[before:]}")
    assert 8 * (len(want) - exact) <= len(want), f"{what}: {len(want) - exact} of {len(want)} streams pass only as localised near-ties"
    for b in range(len(want)):
        if got[b] == want[b]:
            assert abs(float(gsc[b]) - float(wsc[b])) < 2e-3, (what, b, float(gsc[b]), float(wsc[b]))
    return got


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("beam", TINY_BEAMS)
def test_tiny_against_twin(hip_tiny, oracle_tiny, enc_tiny, beam, form):
    unbiased = oracle_tiny.modified_beam_search(enc_tiny, beam)
    _against_twin(hip_tiny, oracle_tiny, enc_tiny, beam, tiny_phrases(unbiased), FORMS[form], f"tiny beam={beam} {form}")


@pytest.mark.parametrize("form", list(FORMS) + ["k_beam_step-no-decoder-table"])
@pytest.mark.parametrize("beam", WIDE_BEAMS)
def test_wide_against_twin(wide, beam, form):
    """V = 400: at beam 4 the fused kernel runs two column slabs per stream (both workgroups run the step and must stay identical)"""
    from k2transducerasr_amd import Model
    path, ora = wide
    enc = wide_enc()
    unbiased = ora.modified_beam_search(enc, beam)
    phrases = wide_phrases(unbiased)
    if form == "k_beam_step-no-decoder-table":
        with switches(K2HIP_DECODER_TABLE_MB=0):      # (read when the model builds its tables: a model of its own)
            m = Model(path, 0)
            got = _against_twin(m, ora, enc, beam, phrases, {}, f"wide beam={beam} {form}")
        m.close()
    else:
        m = Model(path, 0)
        got = _against_twin(m, ora, enc, beam, phrases, FORMS[form], f"wide beam={beam} {form}")
        m.close()
    assert got != unbiased


def test_slab_timeout_repeat_carries_the_tables(wide):
    """the simulated slab timeout marks the two-slab launch for a repeat with one slab: same result with hotwords set"""
    import ctypes as C
    from k2transducerasr_amd import Model, load_library
    path, ora = wide
    L = load_library()
    L.k2hip_debug_search_retries.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    m = Model(path, 0)

    def retries():
        n = C.c_int32(-1)
        assert L.k2hip_debug_search_retries(m.handle, C.byref(n)) == 0
        return n.value

    enc = wide_enc()
    phrases = wide_phrases(ora.modified_beam_search(enc, 4))
    m.set_hotwords(_hw(m, phrases))
    want, wsc = m.beam_search(enc, 4, want_scores=True)
    r0 = retries()
    with switches(K2HIP_TEST_GREEDY_TIMEOUT=1):
        got, gsc = m.beam_search(enc, 4, want_scores=True)
    assert retries() == r0 + 1, "the two-slab form did not run: the case shows nothing"
    assert got == want and gsc.tobytes() == wsc.tobytes()
    m.set_hotwords(None)
    assert m.beam_search(enc, 4) != want
    m.close()


def test_streaming_is_refused_with_hotwords(tiny_model_path, hip_tiny, enc_tiny):
    from k2transducerasr_amd import BeamStream, K2HipError, OnlineRecognizer
    from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model
    hw = _hw(hip_tiny, [[4, 5]])
    s = BeamStream(hip_tiny, 4)
    try:
        hip_tiny.set_hotwords(hw)
        with pytest.raises(K2HipError) as e:
            BeamStream.search_chunk([s], enc_tiny[:1, :8])
        assert e.value.code == -1 and "streaming" in str(e.value)
        hip_tiny.set_hotwords(None)
        BeamStream.search_chunk([s], enc_tiny[:1, :8])
    finally:
        hip_tiny.set_hotwords(None)
        s.close()


def test_online_step_is_refused_with_hotwords(tmp_path):
    from k2transducerasr_amd import Hotwords, K2HipError, OnlineRecognizer
    from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model
    p = str(tmp_path / "stream.k2w")
    write_synthetic_model(p, "zipformer2-streaming-tiny-test")
    rec = OnlineRecognizer(p, 0, "modified_beam_search", 4)
    st = rec.create_online_stream()
    st.add_samples(synth_utterance(3, 2.0))
    rec.model.set_hotwords(Hotwords([[4, 5]], SCORE, rec.model.vocab_size))
    with pytest.raises(K2HipError) as e:
        rec.get_results([st])
    assert e.value.code == -1 and "streaming" in str(e.value)
    rec.model.set_hotwords(None)
    rec.get_results([st])
    # streaming greedy is untouched by hotwords
    rec.model.set_decoding_method("greedy_search")
    rec.model.set_hotwords(Hotwords([[4, 5]], SCORE, rec.model.vocab_size))
    st2 = rec.create_online_stream()
    st2.add_samples(synth_utterance(3, 2.0))
    rec.get_results([st2])


def test_full_size_configs2_with_100_phrases(tmp_path_factory):
    """configs[2]'s shape (zipformer2-large-en, 32 x 10 s, beam 4) on the fixed batch with 100 phrases of 2 - 5 tokens drawn from the
    unbiased run's output: the engine against the twin on 4 of the 32 streams, and the bias must move at least one stream."""
    from k2transducerasr_amd import Hotwords, Model
    from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model
    from oracle import Oracle
    p = str(tmp_path_factory.mktemp("hw_large") / "large.k2w")
    write_synthetic_model(p, "zipformer2-large-en")
    m, ora = Model(p, 0), Oracle(p)
    B = 32
    feats = [m.fbank(synth_utterance(u, 10.0)) for u in range(B)]
    enc = m.encoder_proj(m.pad_sequence(feats).reshape(B, -1, 80))
    unbiased = m.beam_search(enc, 4)
    phrases = draw_phrases(unbiased, 100, np.random.default_rng(100), min_len=2, max_len=5)
    assert len(phrases) == 100
    graph = TwinGraph(phrases, SCORE, ora.vocab_size)
    m.set_hotwords(Hotwords(phrases, SCORE, m.vocab_size))
    with switches(K2HIP_BEAM_TRACE=1):
        got, gsc = m.beam_search(enc, 4, want_scores=True)
        gtr = m.beam_trace()
    assert sum(g != u for g, u in zip(got, unbiased)) >= 1, "100 phrases moved no stream: the case shows nothing"
    sub = [0, 9, 18, 27]
    want, wsc, mg, wtr, ev = twin_batch(ora, enc[sub], 4, graph)
    assert min(ev.values()) >= 1, ev
    gsub = dict(idx=gtr["idx"][sub], val=gtr["val"][sub], n=gtr["n"][sub], beam=4)
    exact = parity.assert_beam_match([got[b] for b in sub], want, mg, tol=parity.LOGIT_TOL, what="configs[2] shape, 100 phrases", allow_tie=True,
                                     trace_got=gsub, trace_want=wtr)
    print(f"full size: {exact}/4 exact, {sum(g != u for g, u in zip(got, unbiased))}/32 streams moved by the bias, events {ev}")
    assert exact >= 4 - 0, "at most one stream in eight may pass as a near-tie: none of four"
    m.close()
