"""N-gram LM shallow fusion of the offline modified beam search on the GPU: libk2hip.so through the C ABI against the Python twin
(tests/ngram_twin.py; its own agreement with the CPU oracle without an LM and at scale = 0 is checked without a GPU in test_ngram.py)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import parity
from hotword_twin import SCORE, TwinGraph, draw_phrases
from kat_model import frames, write_kat_model, write_wide_model
from ngram_twin import (EVENTS, KAT_LM_FLIP, SCALE, TINY_BEAMS, WIDE_BEAMS, WIDE_VOCAB, TwinLm, draw_lm, kat_lm_flip_score, tiny_lm,
                        twin_batch, twin_beam_search, wide_enc, wide_lm)


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


# the forms of the search, as test_hotwords_gpu.FORMS: the fused kernel as the shape selects it (two column slabs per stream for
# 256 < V <= 512 at beam <= 4, else one workgroup per stream), forced to one slab, with its hypotheses in device memory, and the
# per-frame k_beam_step path
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
    from oracle import Oracle
    p = str(tmp_path_factory.mktemp("lm_wide") / "wide.k2w")
    write_wide_model(p, WIDE_VOCAB)
    return p, Oracle(p)


@pytest.fixture(scope="module")
def kat(tmp_path_factory):
    from k2transducerasr_amd import Model
    p = str(tmp_path_factory.mktemp("lm_kat") / "kat.k2w")
    write_kat_model(p)
    return Model(p, 0)


def _lm(model, entries):
    from k2transducerasr_amd import NgramLm
    return NgramLm(entries, model.vocab_size)


def _launches():
    from k2transducerasr_amd import load_library
    L = load_library()
    L.k2hip_debug_beam_launch_counts.argtypes = [C.POINTER(C.c_int64)] * 2
    p, h = C.c_int64(-1), C.c_int64(-1)
    assert L.k2hip_debug_beam_launch_counts(C.byref(p), C.byref(h)) == 0
    return p.value, h.value


@pytest.mark.parametrize("beam", [1, 2, 4, 8])
def test_plain_results_are_bit_equal(hip_tiny, enc_tiny, beam):
    """no LM, a cleared LM and scale = 0: tokens, timestamps and scores as before any was set, from the plain launches only"""
    hip_tiny.set_ngram_lm(None)
    hip_tiny.set_hotwords(None)
    want, wsc = hip_tiny.beam_search(enc_tiny, beam, want_scores=True)
    entries = tiny_lm(want, hip_tiny.vocab_size)
    try:
        lm = _lm(hip_tiny, entries)
        hip_tiny.set_ngram_lm(lm, SCALE)
        p0, h0 = _launches()
        fused = hip_tiny.beam_search(enc_tiny, beam)
        assert _launches() == (p0, h0 + 1)           # (the LM runs in the biased instantiation)
        hip_tiny.set_ngram_lm(None)
        for what in ("cleared", "scale = 0"):
            if what == "scale = 0":
                hip_tiny.set_ngram_lm(lm, 0.0)
                lm.close()                           # the model keeps its own copy
            p0, h0 = _launches()
            got, gsc = hip_tiny.beam_search(enc_tiny, beam, want_scores=True)
            assert _launches() == (p0 + 1, h0), what
            assert got == want, what
            assert gsc.tobytes() == wsc.tobytes(), what
        if beam >= 2:
            assert fused != want       # (the LM does move results: the comparisons above are not vacuous)
    finally:
        hip_tiny.set_ngram_lm(None)


def test_plain_get_results_and_greedy(tiny_model_path, utts):
    from k2transducerasr_amd import K2HipError, NgramLm, OfflineRecognizer
    rec = OfflineRecognizer(tiny_model_path, 0, "modified_beam_search", 4)

    def run(r=rec):
        ss = [r.create_offline_stream() for _ in utts]
        for s, u in zip(ss, utts):
            s.add_samples(u)
        return r.get_results(ss), r.model.last_scores(len(utts)).tobytes()

    want = run()
    V = rec.model.vocab_size
    entries = tiny_lm([(t[2 * len(utts):], ts) for t, ts in want[0]], V)
    rec.model.set_ngram_lm(NgramLm(entries, V), SCALE)
    fused = run()
    assert fused[0] != want[0]
    rec.model.set_ngram_lm(None)
    assert run() == want
    rec.model.set_ngram_lm(NgramLm(entries, V), 0.0)
    assert run() == want
    # the constructor's form, and greedy search ignores the LM
    rec2 = OfflineRecognizer(tiny_model_path, 0, "modified_beam_search", 4, ngram_lm=NgramLm(entries, V), ngram_lm_scale=SCALE)
    assert run(rec2)[0] == fused[0]
    m = rec.model
    m.set_decoding_method("greedy_search")
    m.set_ngram_lm(None)
    g = m.offline_greedy_from_samples(utts)
    m.set_ngram_lm(NgramLm(entries, V), SCALE)
    assert m.offline_greedy_from_samples(utts) == g
    # an LM built for another vocabulary and a bad scale are refused
    for lm, scale, named in ((NgramLm([((3,), -1.0, 0.0), ((-3,), -2.0, 0.0)], V + 1), SCALE, "vocab_size"), (NgramLm(entries, V), -0.5, "scale"),
                             (NgramLm(entries, V), float("nan"), "scale")):
        with pytest.raises(K2HipError) as e:
            m.set_ngram_lm(lm, scale)
        assert e.value.code == -1 and named in str(e.value)


def test_kat_lm_flip(kat):
    """ngram_twin.KAT_LM_FLIP (derived by hand there): the bigram (5, 7) flips [6, 7] into [5, 7]"""
    K = KAT_LM_FLIP
    enc = frames(K["rows"])[None]
    kat.set_ngram_lm(None)
    assert kat.beam_search(enc, K["beam"])[0] == K["plain"]
    kat.set_ngram_lm(_lm(kat, K["entries"]), K["scale"])
    try:
        for form, sw in FORMS.items():
            with switches(**sw):
                got, sc = kat.beam_search(enc, K["beam"], want_scores=True)
            assert got[0] == K["fused"], form
            assert abs(float(sc[0]) - kat_lm_flip_score()) < 1e-5, (form, float(sc[0]), kat_lm_flip_score())
    finally:
        kat.set_ngram_lm(None)


def _against_twin(model, ora, enc, beam, entries, sw, what, phrases=None, need_events=True):
    lm = TwinLm(entries, ora.vocab_size)
    graph = TwinGraph(phrases, SCORE, ora.vocab_size) if phrases else None
    want, wsc, mg, wtr, ev = twin_batch(ora, enc, beam, lm=lm, scale=SCALE, graph=graph)
    if need_events:
        assert min(ev[k] for k in EVENTS) >= 1, f"{what}: every LM event class must occur on the twin: {ev}"
    model.set_ngram_lm(_lm(model, entries), SCALE)
    if phrases:
        from k2transducerasr_amd import Hotwords
        model.set_hotwords(Hotwords(phrases, SCORE, model.vocab_size))
    try:
        with switches(K2HIP_BEAM_TRACE=1, **sw):
            got, gsc = model.beam_search(enc, beam, want_scores=True)
            gtr = model.beam_trace()
    finally:
        model.set_ngram_lm(None)
        model.set_hotwords(None)
    before = len(parity.NEAR_TIES)
    exact = parity.assert_beam_match(got, want, mg, tol=parity.LOGIT_TOL, what=what, allow_tie=True, trace_got=gtr, trace_want=wtr)
    print(f"{what}: {exact}/{len(want)} streams exact, events {ev}, near ties {parity.NEAR_TIES[before:]}")
    assert 8 * (len(want) - exact) <= len(want), f"{what}: {len(want) - exact} of {len(want)} streams pass only as localised near-ties"
    for b in range(len(want)):
        if got[b] == want[b]:
            print(f"{what}: stream {b} score {float(gsc[b]):.6f} twin {float(wsc[b]):.6f}")
            assert abs(float(gsc[b]) - float(wsc[b])) < 2e-3, (what, b, float(gsc[b]), float(wsc[b]))
    return got


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("beam", TINY_BEAMS)
def test_tiny_against_twin(hip_tiny, oracle_tiny, enc_tiny, beam, form):
    unbiased = oracle_tiny.modified_beam_search(enc_tiny, beam)
    _against_twin(hip_tiny, oracle_tiny, enc_tiny, beam, tiny_lm(unbiased, oracle_tiny.vocab_size, beam), FORMS[form], f"tiny beam={beam} {form}")


@pytest.mark.parametrize("form", list(FORMS) + ["k_beam_step-no-decoder-table"])
@pytest.mark.parametrize("beam", WIDE_BEAMS)
def test_wide_against_twin(wide, beam, form):
    """V = 400: at beam 4 the fused kernel runs two column slabs per stream (both workgroups run the walks and must stay identical)"""
    from k2transducerasr_amd import Model
    path, ora = wide
    enc = wide_enc()
    unbiased = ora.modified_beam_search(enc, beam)
    entries = wide_lm(unbiased, beam)
    if form == "k_beam_step-no-decoder-table":
        with switches(K2HIP_DECODER_TABLE_MB=0):      # (read when the model builds its tables: a model of its own)
            m = Model(path, 0)
            got = _against_twin(m, ora, enc, beam, entries, {}, f"wide beam={beam} {form}")
        m.close()
    else:
        m = Model(path, 0)
        got = _against_twin(m, ora, enc, beam, entries, FORMS[form], f"wide beam={beam} {form}")
        m.close()
    assert got != unbiased


@pytest.mark.parametrize("form", ["k_beam_loop", "k_beam_step-launches"])
def test_hotwords_and_lm_together(wide, form):
    """(sum + hotword bonus) + LM term, both states carried; the pending hotword bonus is still taken back at the end"""
    from k2transducerasr_amd import Model
    path, ora = wide
    enc = wide_enc()
    unbiased = ora.modified_beam_search(enc, 4)
    phrases = draw_phrases(unbiased, 12, np.random.default_rng(5))
    m = Model(path, 0)
    _against_twin(m, ora, enc, 4, wide_lm(unbiased, 4), FORMS[form], f"hotwords + LM {form}", phrases=phrases)
    m.close()


def test_large_vocabulary_sparse_bigram(tmp_path):
    """V = 5537 (the size of conformer-zh's table): a bigram over it has states whose dense form (states x V) would not fit the
    hotword tables' cap; here one state has more than 64 arcs, so the 64-ary narrowing of the walk runs"""
    from k2transducerasr_amd import Model
    from oracle import Oracle
    V = 5537
    p = str(tmp_path / "zh.k2w")
    write_wide_model(p, V)
    ora = Oracle(p)
    enc = np.random.default_rng(77).standard_normal((4, 24, 64)).astype(np.float32)
    unbiased = ora.modified_beam_search(enc, 4)
    rng = np.random.default_rng(78)
    entries = draw_lm(unbiased, V, rng, order=2, n_cut=40, n_random=3000, n_no_unigram=4)
    # a state with thousands of arcs: the most emitted token followed by every third token
    emitted = [int(t) for toks, _ in unbiased for t in toks]
    hub = max(set(emitted), key=emitted.count)
    have = {e[0] for e in entries}
    assert (hub,) in have
    entries += [((hub, v), np.float32(rng.uniform(-2.0, -0.1)), np.float32(0)) for v in range(3, V, 3) if (v,) in have and (hub, v) not in have]
    lm = TwinLm(entries, V)
    assert lm.num_states * V > (1 << 23) and sum(1 for k in lm.lp if k[:-1] == (hub,)) > 1000
    # on the twin, selected candidates do walk from the hub state (> 64 arcs: the narrowing loop runs), with hits and with misses
    visits = {"hit": 0, "miss": 0}
    step = TwinLm.step

    def counting(self, s, w):
        if self.hist[s] == (hub,) and w not in (0, 2):
            visits["hit" if (hub, w) in self.lp else "miss"] += 1
        return step(self, s, w)

    TwinLm.step = counting
    try:
        for b in range(enc.shape[0]):
            twin_beam_search(ora, enc[b], 4, lm, SCALE)
    finally:
        TwinLm.step = step
    assert visits["hit"] >= 1 and visits["miss"] >= 1, visits
    m = Model(p, 0)
    for form in ("k_beam_step-launches",):      # (no decoder table at this vocabulary: the per-frame path is the one that runs)
        got = _against_twin(m, ora, enc, 4, entries, FORMS[form], f"V=5537 bigram {form}", need_events=False)
        assert got != unbiased, "the bigram moved no stream: the case shows nothing"
    m.close()


def test_nbest_with_lm(wide):
    """entry 0 equals the result, scores include the LM, token log-probs stay the unbiased acoustic terms"""
    from k2transducerasr_amd import Model
    path, ora = wide
    enc = wide_enc()
    m = Model(path, 0)
    plain = m.beam_search(enc, 4, nbest=4)
    unbiased = [(a[0]["tokens"], a[0]["timestamps"]) for a in plain]
    m.set_ngram_lm(_lm(m, wide_lm(ora.modified_beam_search(enc, 4), 4)), SCALE)
    got, gsc = m.beam_search(enc, 4, want_scores=True)
    alts = m.beam_search(enc, 4, nbest=4)
    moved = 0
    for b in range(len(got)):
        assert (list(alts[b][0]["tokens"]), list(alts[b][0]["timestamps"])) == (list(got[b][0]), list(got[b][1]))
        assert np.float32(alts[b][0]["score"]).tobytes() == gsc[b].tobytes()
        norm = [a["score"] / (len(a["tokens"]) + 2) for a in alts[b]]
        assert norm == sorted(norm, reverse=True)
        for a in alts[b]:       # the same token sequence emitted at the same frames without the LM: the same acoustic terms
            for q in plain[b]:
                if list(q["tokens"]) == list(a["tokens"]) and list(q["timestamps"]) == list(a["timestamps"]):
                    np.testing.assert_allclose(a["token_log_probs"], q["token_log_probs"], atol=2e-5, rtol=0)
        moved += (list(got[b][0]), list(got[b][1])) != (list(unbiased[b][0]), list(unbiased[b][1]))
    assert moved >= 1
    m.close()


def test_slab_timeout_repeat_carries_the_tables(wide):
    """the simulated slab timeout marks the two-slab launch for a repeat with one slab: same result with an LM set"""
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
    m.set_ngram_lm(_lm(m, wide_lm(ora.modified_beam_search(enc, 4), 4)), SCALE)
    want, wsc = m.beam_search(enc, 4, want_scores=True)
    r0 = retries()
    with switches(K2HIP_TEST_GREEDY_TIMEOUT=1):
        got, gsc = m.beam_search(enc, 4, want_scores=True)
    assert retries() == r0 + 1, "the two-slab form did not run: the case shows nothing"
    assert got == want and gsc.tobytes() == wsc.tobytes()
    m.set_ngram_lm(None)
    assert m.beam_search(enc, 4) != want
    m.close()


def test_full_size_configs2_with_a_trigram(tmp_path_factory):
    """configs[2]'s shape (zipformer2-large-en, 32 x 10 s, beam 4) on the fixed batch with a seeded trigram cut from the plain run's
    output: the engine against the twin on 8 of the 32 streams, under the same cap, and the LM must move at least one stream."""
    from k2transducerasr_amd import Model
    from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model
    from oracle import Oracle
    p = str(tmp_path_factory.mktemp("lm_large") / "large.k2w")
    write_synthetic_model(p, "zipformer2-large-en")
    m, ora = Model(p, 0), Oracle(p)
    B = 32
    feats = [m.fbank(synth_utterance(u, 10.0)) for u in range(B)]
    enc = m.encoder_proj(m.pad_sequence(feats).reshape(B, -1, 80))
    plain = m.beam_search(enc, 4)
    entries = draw_lm(plain, ora.vocab_size, np.random.default_rng(100), n_cut=300, n_random=2000, n_no_unigram=5)
    m.set_ngram_lm(_lm(m, entries), SCALE)
    with switches(K2HIP_BEAM_TRACE=1):
        got, gsc = m.beam_search(enc, 4, want_scores=True)
        gtr = m.beam_trace()
    assert sum(g != u for g, u in zip(got, plain)) >= 1, "the LM moved no stream: the case shows nothing"
    sub = [0, 4, 9, 13, 18, 22, 27, 31]
    want, wsc, mg, wtr, ev = twin_batch(ora, enc[sub], 4, lm=TwinLm(entries, ora.vocab_size), scale=SCALE)
    assert min(ev[k] for k in EVENTS) >= 1, ev
    gsub = dict(idx=gtr["idx"][sub], val=gtr["val"][sub], n=gtr["n"][sub], beam=4)
    exact = parity.assert_beam_match([got[b] for b in sub], want, mg, tol=parity.LOGIT_TOL, what="configs[2] shape, trigram", allow_tie=True,
                                     trace_got=gsub, trace_want=wtr)
    print(f"full size: {exact}/8 exact, {sum(g != u for g, u in zip(got, plain))}/32 streams moved by the LM, events {ev}")
    assert 8 * (8 - exact) <= 8, "at most one stream in eight may pass as a near-tie"
    for i, b in enumerate(sub):
        if got[b] == want[i]:
            assert abs(float(gsc[b]) - float(wsc[i])) < 2e-3, (b, float(gsc[b]), float(wsc[i]))
    m.close()
