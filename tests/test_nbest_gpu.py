"""N-best hypotheses and token log-probs of the modified beam search on the GPU, against the Python twin (tests/nbest_twin.py).

Bounds (none of them taken from what the engine gives): the number of alternatives, their order, tokens and timestamps are exact;
scores within 2e-3, the bound tests/test_beam_gpu.py holds beam scores to; token log-probs within 2 * LOGIT_TOL / 10 = 2e-4, twice the
joiner-logit bound of test_parity_gpu.py::test_joiner_proj_logits (a log-softmax value moves by at most the logit's own error plus
the error of the log-sum-exp).  A stream may be excused from the ORDER check only when the twin's own smallest adjacent gap of
normalised scores is below parity.LOGIT_TOL (its alternatives must then still match as a set).  The committed cases DO have such gaps
(with up to 8 alternatives over 35 frames nearly every list has two entries closer than 1e-3; the smallest is 1.0e-4, a hundred
times float32's rounding of these sums), so the excuse is available to them -- and every test asserts that it was not used: zero
excused streams.  (The order on EXACT ties -- planted duplicates, tied hypotheses, tied final scores, with no excuse available -- is
held by tests/test_beam_ties_gpu.py on the cases of tests/beam_cases.py.)

The fused streaming step scores the DEVICE encoder's frames, not the oracle's: its token log-probs are held to the same 2e-4
(measured 2.4e-6), its scores -- sums over every frame so far -- to the relative bound tests/test_online_beam_gpu.py already uses for
the fused step."""
import contextlib

import numpy as np
import pytest

import parity
from hotword_twin import SCORE, tiny_phrases
from nbest_twin import KAT_MERGE, TwinGraph, kat_merge_logp, nbest_twin_batch, nbest_twin_search

pytestmark = pytest.mark.gpu

SCORE_TOL = 2e-3
YP_TOL = 2 * parity.LOGIT_TOL / 10
FORMS = ("loop", "hyp_global", "launches")   # one kernel with the hypotheses in LDS / in device memory, four launches per frame


@contextlib.contextmanager
def form(name):
    import k2transducerasr_amd as pkg
    sw = {"loop": None, "hyp_global": "K2HIP_BEAM_HYP_GLOBAL", "launches": "K2HIP_BEAM_LAUNCHES"}[name]
    if sw:
        pkg.set_switch(sw, 1)
    try:
        yield
    finally:
        if sw:
            pkg.set_switch(sw, 0)


@pytest.fixture(scope="module")
def enc_tiny(oracle_tiny, utts):
    f = [oracle_tiny.fbank(u) for u in utts]
    return oracle_tiny.encoder(oracle_tiny.pad_sequence(f).reshape(len(utts), -1, 80))


def compare(got, twin, n, what, worst):
    """one stream: got = the engine's alternatives, twin = nbest_twin_search's result, n = the nbest asked for.  Returns 1 if the
    stream had to be excused from the order check (a near-tie of the twin's own), else 0."""
    want = twin["alts"][:n]
    assert len(got) == len(want), (what, len(got), len(want))
    excused = 0
    if [(a["tokens"], a["timestamps"]) for a in got] != [(a["tokens"], a["timestamps"]) for a in want]:
        assert twin["min_gap"] < parity.LOGIT_TOL and n >= len(twin["alts"]), (what, "order / content differs", got, want, twin["min_gap"])
        excused = 1
        key = lambda a: (a["tokens"], a["timestamps"])   # noqa: E731
        got, want = sorted(got, key=key), sorted(want, key=key)
        assert [key(a) for a in got] == [key(a) for a in want], (what, "not even the same set")
    for g, w in zip(got, want):
        worst[0] = max(worst[0], abs(g["score"] - w["score"]))
        assert abs(g["score"] - w["score"]) <= SCORE_TOL, (what, g["score"], w["score"])
        assert len(g["token_log_probs"]) == len(g["tokens"])
        if len(g["tokens"]):
            d = float(np.abs(g["token_log_probs"] - w["token_log_probs"]).max())
            worst[1] = max(worst[1], d)
            assert d <= YP_TOL, (what, d)
            assert (g["token_log_probs"] <= 0).all()
    return excused


@pytest.mark.parametrize("hotwords", [False, True])
@pytest.mark.parametrize("beam", [1, 2, 4, 8])
def test_offline_operator_level_against_the_twin(hip_tiny, oracle_tiny, enc_tiny, beam, hotwords):
    from k2transducerasr_amd import Hotwords
    graph = hw = None
    if hotwords:
        phrases = tiny_phrases(oracle_tiny.modified_beam_search(enc_tiny, max(beam, 2)))
        graph = TwinGraph(phrases, SCORE, oracle_tiny.vocab_size)
        hw = Hotwords(phrases, SCORE, hip_tiny.vocab_size)
    twins = nbest_twin_batch(oracle_tiny, enc_tiny, beam, graph)
    excused, worst = 0, [0.0, 0.0]
    hip_tiny.set_hotwords(hw)
    try:
        for f in FORMS:
            with form(f):
                plain, psc = hip_tiny.beam_search(enc_tiny, beam, want_scores=True)
                for n in sorted({1, 2, beam, 8}):
                    got = hip_tiny.beam_search(enc_tiny, beam, nbest=n)
                    for b in range(len(got)):
                        excused += compare(got[b], twins[b], n, f"{f} beam={beam} nbest={n} hw={hotwords} stream {b}", worst)
                        # entry 0 is the unchanged call's result, bit for bit
                        assert (got[b][0]["tokens"], got[b][0]["timestamps"]) == plain[b]
                        assert np.float32(got[b][0]["score"]) == psc[b]
                # and the unchanged call is unchanged by the calls in between
                again, asc = hip_tiny.beam_search(enc_tiny, beam, want_scores=True)
                assert again == plain and np.array_equal(asc, psc)
                best = hip_tiny.beam_search(enc_tiny, beam, want_token_log_probs=True)
                assert [(a["tokens"], a["timestamps"]) for a in best] == plain
    finally:
        hip_tiny.set_hotwords(None)
        if hw:
            hw.close()
    print(f"beam={beam} hw={hotwords}: worst score diff {worst[0]:.3g} (bound {SCORE_TOL}), worst token log-prob diff {worst[1]:.3g} (bound {YP_TOL})")
    assert excused == 0
    if beam > 1:
        assert max(len(t["alts"]) for t in twins) > 1


def test_kat_merge_on_the_device(tmp_path):
    """nbest_twin.KAT_MERGE: the merged [5] keeps the first-inserted path's timestamp and token log-prob; the bonus of the phrase [5] is in
    the score and not in the token log-probs"""
    from kat_model import frames, write_kat_model
    from k2transducerasr_amd import Hotwords, Model
    p = str(tmp_path / "kat.k2w")
    write_kat_model(p)
    m = Model(p, 0)
    enc = frames(KAT_MERGE["rows"])[None]
    kept = kat_merge_logp(0, 5, 0.1)
    for f in FORMS:
        with form(f):
            plain = {tuple(a["tokens"]): a for a in m.beam_search(enc, KAT_MERGE["beam"], nbest=8)[0]}
            assert set(plain) == {(), (5,), (5, 5)}
            assert plain[(5,)]["timestamps"] == [0] and abs(float(plain[(5,)]["token_log_probs"][0]) - kept) < 1e-5
            hw = Hotwords(KAT_MERGE["phrases"], SCORE, 8)
            m.set_hotwords(hw)
            try:
                biased = {tuple(a["tokens"]): a for a in m.beam_search(enc, KAT_MERGE["beam"], nbest=8)[0]}
            finally:
                m.set_hotwords(None)
                hw.close()
            assert biased[(5,)]["timestamps"] == [0]
            assert abs(biased[(5,)]["score"] - (plain[(5,)]["score"] + SCORE)) < 1e-5
            assert np.array_equal(biased[(5,)]["token_log_probs"], plain[(5,)]["token_log_probs"])
    m.close()


def test_argument_checks_and_routes(tiny_model_path, enc_tiny):
    from k2transducerasr_amd import K2HipError, Model
    m = Model(tiny_model_path, 0)
    for bad in (0, 9, -1):
        with pytest.raises(K2HipError) as e:
            m.beam_search(enc_tiny, 4, nbest=bad)
        assert e.value.code == -1
        with pytest.raises(K2HipError):
            m.set_nbest(bad)
    with pytest.raises(K2HipError) as e:      # greedy_search has no alternatives
        m.set_nbest(4)
    assert e.value.code == -1 and "modified_beam_search" in str(e.value)
    m.set_decoding_method("modified_beam_search", 4)
    m.set_nbest(4)
    samples = np.zeros((2, 16000), np.float32)
    with pytest.raises(K2HipError) as e:      # the pipelined route has one result per stream: refused, not silently one result
        m.offline_submit_samples(samples)
    assert e.value.code == -1 and "set_nbest" in str(e.value)
    m.set_nbest(1)
    assert len(m.offline_wait(m.offline_submit_samples(samples))) == 2
    m.close()


def test_offline_recognizer_streams_carry_the_alternatives(tiny_model_path, oracle_tiny, utts):
    from k2transducerasr_amd import OfflineRecognizer
    plain = OfflineRecognizer(tiny_model_path, 0, "modified_beam_search", 4)
    ps = [plain.create_offline_stream() for _ in utts]
    for s, u in zip(ps, utts):
        s.add_samples(u)
        assert [a["tokens"] for a in s.alternatives()] == [[]] and s.alternatives()[0]["score"] == 0.0   # the start state
    want = plain.get_results(ps)
    assert all(len(s.alternatives()) == 1 and not s.alternatives()[0]["tokens"] for s in ps)   # n = 1: nothing is kept
    psc = plain.model.last_scores(len(utts))
    rec = OfflineRecognizer(tiny_model_path, 0, "modified_beam_search", 4, nbest=4)
    ss = [rec.create_offline_stream() for _ in utts]
    for s, u in zip(ss, utts):
        s.add_samples(u)
    got = rec.get_results(ss)
    assert got == want                                                   # the result itself is what it is without the feature
    B = len(utts)
    multi = 0
    for b, s in enumerate(ss):
        alts = s.alternatives()
        assert 1 <= len(alts) <= 4
        assert alts[0]["tokens"] == got[b][0][2 * B:] and alts[0]["timestamps"] == got[b][1][2 * B:]
        assert np.float32(alts[0]["score"]) == psc[b]
        assert np.array_equal(s.token_log_probs(), alts[0]["token_log_probs"])
        assert len({tuple(a["tokens"]) for a in alts}) == len(alts)
        multi += len(alts) > 1
    assert multi > 0
    # against the twin, on the oracle's encoder output of the same batch (the engine's own encoder differs by float rounding only)
    f = [oracle_tiny.fbank(u) for u in utts]
    enc = oracle_tiny.encoder(oracle_tiny.pad_sequence(f).reshape(B, -1, 80))
    excused, worst = 0, [0.0, 0.0]
    for b, tw in enumerate(nbest_twin_batch(oracle_tiny, enc, 4)):
        excused += compare(ss[b].alternatives(), tw, 4, f"recognizer stream {b}", worst)
    assert excused == 0


def same_alternatives(got, want):
    """two N-best lists of a batch ([stream][alternative] dicts), bit for bit"""
    assert [len(a) for a in got] == [len(a) for a in want]
    for ga, wa in zip(got, want):
        for g, w in zip(ga, wa):
            assert (g["tokens"], g["timestamps"]) == (w["tokens"], w["timestamps"])
            assert np.float32(g["score"]) == np.float32(w["score"])
            assert np.array_equal(g["token_log_probs"], w["token_log_probs"])


def test_by_products_do_not_outlive_their_call(tiny_model_path, utts):
    """One handle, three synchronous calls in a row: beam 4 with nbest = 3 on B = 3, the same on B = 2 with another max_tokens (a shorter
    longest utterance), then greedy search.  Each call's N-best is what a fresh handle returns for that batch alone -- nothing of an
    earlier search's device by-products (another batch size, another max_tokens, an arena since rebuilt) is fetched -- and the greedy
    call leaves the streams with no alternatives; a beam call after it has its own again."""
    from k2transducerasr_amd import OfflineRecognizer
    batches = [utts[:3], [utts[4], utts[1]]]

    def decode(rec, batch):
        ss = [rec.create_offline_stream() for _ in batch]
        for s, u in zip(ss, batch):
            s.add_samples(u)
        res = rec.get_results(ss)
        return res, [s.alternatives() for s in ss], [s.token_log_probs() for s in ss]

    fresh = []
    for batch in batches:
        rec = OfflineRecognizer(tiny_model_path, 0, "modified_beam_search", 4, nbest=3)
        fresh.append(decode(rec, batch))
        rec.model.close()
    assert max(len(a) for a in fresh[0][1]) > 1 and max(len(a) for a in fresh[1][1]) > 1   # there are alternatives to mix up
    rec = OfflineRecognizer(tiny_model_path, 0, "modified_beam_search", 4, nbest=3)
    for batch, (wres, walts, _) in zip(batches, fresh):
        res, alts, _ = decode(rec, batch)
        assert res == wres
        same_alternatives(alts, walts)
    rec.model.set_nbest(1)
    rec.model.set_decoding_method("greedy_search")
    res, alts, yps = decode(rec, batches[0])
    assert all(len(a) == 1 and a[0]["tokens"] == [] and a[0]["score"] == 0.0 for a in alts) and all(len(y) == 0 for y in yps)
    greedy = OfflineRecognizer(tiny_model_path, 0)
    assert res == decode(greedy, batches[0])[0]
    greedy.model.close()
    rec.model.set_decoding_method("modified_beam_search", 4)
    rec.model.set_nbest(3)
    res, alts, _ = decode(rec, batches[0])
    assert res == fresh[0][0]
    same_alternatives(alts, fresh[0][1])
    rec.model.close()


def test_slab_timeout_repeat_returns_its_own_by_products(tmp_path):
    """Beam 4, nbest = 2, B = 2 on the V = 400 model (Vp / 4 = 100 column groups: in (64, 128], beam <= 4, 2 B <= a quarter of the CUs --
    beam_search's two-slab form).  The simulated slab timeout makes the engine repeat the search with one slab: tokens, scores and the
    N-best the call returns are the REPEAT's, equal to the run without the switch -- and the retry counter shows that the repeat ran."""
    import ctypes as C
    from hotword_twin import WIDE_VOCAB, wide_enc
    from kat_model import write_wide_model
    from k2transducerasr_amd import Model, load_library, set_switch
    p = str(tmp_path / "wide.k2w")
    write_wide_model(p, WIDE_VOCAB)
    m = Model(p, 0)
    L = load_library()
    L.k2hip_debug_search_retries.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]

    def retries():
        n = C.c_int32(-1)
        assert L.k2hip_debug_search_retries(m.handle, C.byref(n)) == 0
        return n.value

    enc = wide_enc()[:2]
    want, wsc = m.beam_search(enc, 4, want_scores=True)
    want_alts = m.beam_search(enc, 4, nbest=2)
    assert max(len(a) for a in want_alts) == 2
    r0 = retries()
    set_switch("K2HIP_TEST_GREEDY_TIMEOUT", 1)
    try:
        got, gsc = m.beam_search(enc, 4, want_scores=True)
        got_alts = m.beam_search(enc, 4, nbest=2)
    finally:
        set_switch("K2HIP_TEST_GREEDY_TIMEOUT", 0)
    assert retries() == r0 + 2, "the two-slab form did not run: the case shows nothing"
    assert got == want and gsc.tobytes() == wsc.tobytes()
    same_alternatives(got_alts, want_alts)
    m.close()


@pytest.mark.parametrize("hotwords", [False, True])
@pytest.mark.parametrize("beam", [2, 4])
def test_beam_stream_alternatives_after_every_step(hip_tiny, oracle_tiny, enc_tiny, beam, hotwords):
    """operator level of the streaming search: after every call a stream's alternatives and its best result's token log-probs are the
    offline twin's over all frames so far -- chunkings of 1 frame, 7 frames and everything at once, a reset mid-stream"""
    from k2transducerasr_amd import BeamStream, Hotwords
    enc = enc_tiny[:2]
    T = enc.shape[1]
    graph = hw = None
    if hotwords:
        phrases = tiny_phrases(oracle_tiny.modified_beam_search(enc_tiny, max(beam, 2)))
        graph = TwinGraph(phrases, SCORE, oracle_tiny.vocab_size)
        hw = Hotwords(phrases, SCORE, hip_tiny.vocab_size)
    twin = {}

    def tw(b, n):
        if (b, n) not in twin:
            twin[(b, n)] = nbest_twin_search(oracle_tiny, enc[b, :n], beam, graph)
        return twin[(b, n)]

    excused, worst, checks = 0, [0.0, 0.0], 0
    hip_tiny.set_decoding_method("modified_beam_search", beam)
    hip_tiny.set_nbest(8)
    try:
        for f in ("loop", "launches"):
            with form(f):
                for step in (1, 7, T):
                    ss = [BeamStream(hip_tiny, beam) for _ in range(2)]
                    for s in ss:
                        assert [a["tokens"] for a in s.alternatives()] == [[]] and len(s.token_log_probs()) == 0
                        if hw:
                            s.set_hotwords(hw)
                    n, did_reset = 0, False
                    while n < T:
                        m = min(T, n + step)
                        BeamStream.search_chunk(ss, enc[:, n:m])
                        n = m
                        for b, s in enumerate(ss):
                            alts = s.alternatives()
                            excused += compare(alts, tw(b, n), 8, f"{f} beam={beam} hw={hotwords} step={step} stream {b} n={n}", worst)
                            assert alts[0]["tokens"] == s.tokens and alts[0]["timestamps"] == s.timestamps
                            assert np.float32(alts[0]["score"]) == np.float32(s.score)
                            assert np.array_equal(s.token_log_probs(), alts[0]["token_log_probs"])
                            checks += 1
                        if step == 7 and not did_reset and n >= 14:      # reset mid-stream: the start state, then the same again
                            for s in ss:
                                s.reset()
                                assert [a["tokens"] for a in s.alternatives()] == [[]] and s.alternatives()[0]["score"] == 0.0
                                assert len(s.token_log_probs()) == 0
                            n, did_reset = 0, True
                    for s in ss:
                        s.close()
    finally:
        hip_tiny.set_nbest(1)
        hip_tiny.set_decoding_method("greedy_search")
        if hw:
            hw.close()
    print(f"beam={beam} hw={hotwords}: {checks} (stream, prefix) checks; worst score diff {worst[0]:.3g}, worst token log-prob diff {worst[1]:.3g}")
    assert excused == 0


# ---- full size: configs[2]'s shape (zipformer2-large-en, 32 x 10 s, beam 4) on the fixed batch tests/test_large_gpu.py uses ---------
def test_full_size_beam4_nbest(tmp_path_factory):
    """T' = 253, V = 500: the one-kernel search with two column slabs per stream and 6 K cap floats of hypotheses in LDS, then the
    device-memory form and the four-launch form.  Entry 0 of all 32 streams against the oracle (tokens, timestamps, score) and bit for
    bit against the plain call; every alternative of the first streams against the twin, token log-probs included."""
    import k2transducerasr_amd as pkg
    from k2transducerasr_amd import Model
    from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model
    from oracle import Oracle
    p = str(tmp_path_factory.mktemp("nbest_large") / "large.k2w")
    write_synthetic_model(p, "zipformer2-large-en")
    hip, ora = Model(p, 0), Oracle(p)
    B, TWINS = 32, 3
    utts = np.stack([synth_utterance(u, 10.0) for u in range(B)])
    feats = [ora.fbank(utts[b]) for b in range(B)]
    enc = ora.encoder(ora.pad_sequence(feats).reshape(B, -1, 80))
    want, mg, sc = ora.modified_beam_search(enc, 4, want_margins=True, want_scores=True)
    twins = nbest_twin_batch(ora, enc[:TWINS], 4)
    excused, worst = 0, [0.0, 0.0]
    for f in FORMS:
        with form(f):
            plain, psc = hip.beam_search(enc, 4, want_scores=True)
            got = hip.beam_search(enc, 4, nbest=4)
            parity.assert_beam_match([(g[0]["tokens"], g[0]["timestamps"]) for g in got], want, mg, what=f"full size nbest entry 0, {f}")
            np.testing.assert_allclose([g[0]["score"] for g in got], sc, atol=SCORE_TOL, rtol=0)
            for b in range(B):
                assert (got[b][0]["tokens"], got[b][0]["timestamps"]) == plain[b] and np.float32(got[b][0]["score"]) == psc[b]
                assert 1 <= len(got[b]) <= 4 and len({tuple(a["tokens"]) for a in got[b]}) == len(got[b])
                for a in got[b]:
                    assert len(a["token_log_probs"]) == len(a["tokens"]) and (a["token_log_probs"] <= 0).all()
            for b in range(TWINS):
                excused += compare(got[b], twins[b], 4, f"full size {f} stream {b}", worst)
    # the fused entry under set_nbest: the batch from samples, the lists on the engine's own encoder output
    print(f"full size: worst score diff {worst[0]:.3g} (bound {SCORE_TOL}), worst token log-prob diff {worst[1]:.3g} (bound {YP_TOL})")
    assert excused == 0
    hip.close()


# ---- the fused streaming step: OnlineStream under modified_beam_search ------------------------------------------------------------
FUSED_YP_TOL = YP_TOL


def compare_fused(got, twin, what, worst):
    from test_online_beam_gpu import fused_score_ok
    want = twin["alts"]
    assert len(got) == len(want), (what, len(got), len(want))
    excused = 0
    key = lambda a: (a["tokens"], a["timestamps"])   # noqa: E731
    if [key(a) for a in got] != [key(a) for a in want]:
        assert twin["min_gap"] < parity.LOGIT_TOL, (what, "order / content differs", got, want, twin["min_gap"])
        excused = 1
        got, want = sorted(got, key=key), sorted(want, key=key)
        assert [key(a) for a in got] == [key(a) for a in want], (what, "not even the same set")
    for g, w in zip(got, want):
        assert fused_score_ok(g["score"], w["score"]), (what, g["score"], w["score"])
        if len(g["tokens"]):
            d = float(np.abs(g["token_log_probs"] - w["token_log_probs"]).max())
            worst[0] = max(worst[0], d)
            assert d <= FUSED_YP_TOL, (what, d)
            assert (g["token_log_probs"] <= 0).all()
    return excused


@pytest.mark.parametrize("hotwords", [False, True])
def test_online_stream_alternatives_after_every_tick(tmp_path_factory, hotwords):
    """three ragged streams through OnlineRecognizer (k2hip_online_step) with Model.set_nbest(4): after every tick a stream's
    alternatives and its best result's token log-probs are the offline twin's over all of its oracle frames so far; with per-stream
    hotword graphs (two different lists and a stream with none); a reset mid-stream returns the start state and the stream then
    decodes the same again"""
    from hotword_twin import draw_phrases
    from k2transducerasr_amd import OnlineRecognizer
    from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model
    from oracle.online import OnlineOracle
    from test_online_beam_gpu import BLANK_BIAS, oracle_beam, oracle_frames
    preset, beam = "zipformer2-streaming-tiny-test", 4
    path = str(tmp_path_factory.mktemp("nbest_fused") / f"{preset}.k2w")
    write_synthetic_model(path, preset, blank_bias=BLANK_BIAS.get(preset))
    rec = OnlineRecognizer(path, decoding_method="modified_beam_search", beam=beam)
    rec.model.set_nbest(4)
    ora = OnlineOracle(path)
    utts = [synth_utterance(20 + u, d) for u, d in enumerate([2.4, 1.3, 1.9])]
    feats = [ora.fbank(u) for u in utts]
    fr = [oracle_frames(ora, f) for f in feats]
    lists = [None] * 3
    if hotwords:
        unb = [oracle_beam(ora, e, beam) for e, _ in fr]
        lists = [draw_phrases([unb[0][:2]], 5, np.random.default_rng(1)), draw_phrases([unb[1][:2]], 5, np.random.default_rng(2)), None]
        assert lists[0] and lists[1]
    graphs = [TwinGraph(x, SCORE, ora.vocab_size) if x else None for x in lists]
    hs = [rec.create_online_stream(hotwords=x, hotwords_score=SCORE) if x else rec.create_online_stream() for x in lists]
    excused, worst, checks, multi = 0, [0.0], 0, 0

    def start(h):
        alts = h.alternatives()
        assert len(alts) == 1 and alts[0]["tokens"] == [] and alts[0]["score"] == 0.0 and len(h.token_log_probs()) == 0

    def decode(which):
        nonlocal excused, checks, multi
        for b in which:
            start(hs[b])
            hs[b].add_features(feats[b])
        done = {b: 0 for b in which}
        while True:
            dec, _ = rec.get_results([hs[b] for b in which])
            if not any(dec):
                break
            for i, b in enumerate(which):
                if not dec[i]:
                    continue
                done[b] += 1
                enc, cum = fr[b]
                tw = nbest_twin_search(ora, enc[: cum[done[b] - 1]], beam, graphs[b])
                alts = hs[b].alternatives()
                excused += compare_fused(alts, tw, f"fused hw={hotwords} stream {b} tick {done[b]}", worst)
                assert [0, 0] + alts[0]["tokens"] == hs[b].tokens and alts[0]["timestamps"] == hs[b].timestamps
                assert np.float32(alts[0]["score"]) == np.float32(hs[b].score)
                assert np.array_equal(hs[b].token_log_probs(), alts[0]["token_log_probs"])
                multi += len(alts) > 1
                checks += 1
        assert all(done[b] == len(fr[b][1]) for b in which)

    decode([0, 1, 2])
    hs[1].reset()                       # mid-stream for the recognizer: the other streams keep their hypotheses
    start(hs[1])
    decode([1])
    print(f"fused hw={hotwords}: {checks} (stream, tick) checks, {multi} with more than one alternative; worst token log-prob diff {worst[0]:.3g} "
          f"(bound {FUSED_YP_TOL})")
    assert excused == 0 and multi > 0
    for h in hs:
        h.close()


def test_small_cap_writes_nothing(hip_tiny, enc_tiny):
    """the getters' cap rule on alternatives that hold tokens: K2HIP_ERR_CAPACITY, and not one word is written"""
    import ctypes as C
    from k2transducerasr_amd import BeamStream
    L = hip_tiny._L
    hip_tiny.set_decoding_method("modified_beam_search", 4)
    hip_tiny.set_nbest(4)
    try:
        s = BeamStream(hip_tiny, 4)
        BeamStream.search_chunk([s], enc_tiny[:1])
        alts = s.alternatives()
        n_tok = len(alts[0]["tokens"])
        assert n_tok >= 2
        L.k2hip_beam_stream_get_alternative.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 3 + [C.c_int32, C.c_void_p, C.c_void_p]
        L.k2hip_beam_stream_get_token_log_probs.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        tok, ts, lp = np.full(n_tok, -7, np.int64), np.full(n_tok, -7, np.int32), np.full(n_tok, -7, np.float32)
        n, sc = C.c_int32(-7), C.c_float(-7)
        rc = L.k2hip_beam_stream_get_alternative(s._h, 0, tok.ctypes.data, ts.ctypes.data, lp.ctypes.data, n_tok - 1, C.byref(n), C.byref(sc))
        assert rc == -5 and n.value == -7 and sc.value == -7 and (tok == -7).all() and (ts == -7).all() and (lp == -7).all()
        assert L.k2hip_beam_stream_get_token_log_probs(s._h, lp.ctypes.data, n_tok - 1) == -5 and (lp == -7).all()
        assert L.k2hip_beam_stream_get_token_log_probs(s._h, lp.ctypes.data, n_tok) == n_tok
        assert np.array_equal(lp, alts[0]["token_log_probs"])
        rc = L.k2hip_beam_stream_get_alternative(s._h, 0, tok.ctypes.data, ts.ctypes.data, None, n_tok, C.byref(n), C.byref(sc))
        assert rc == 0 and n.value == n_tok and tok.tolist() == alts[0]["tokens"] and ts.tolist() == alts[0]["timestamps"]
        s.close()
    finally:
        hip_tiny.set_nbest(1)
        hip_tiny.set_decoding_method("greedy_search")
