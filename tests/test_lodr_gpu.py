"""LODR on the device (k2hip_set_lodr_lm; the second automaton of the NLM instantiation of k_beam_step and its carried states): the
fused offline search against the Python twin (tests/lodr_twin.py) on the accepted cases of tests/lodr_cases.py, together with hotwords
and with a positive-weight tri-gram LM, the paths that ignore the setting, the streaming search after every call of every chunking
against the engine's own offline fused-plus-LODR search, the setting changes, the rescoring and the refusals."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import lodr_cases as cases
import parity
import rnn_lm_cases as lmc
import rnn_lm_fusion_cases as fc
from lodr_twin import lodr_total, rescored_order, twin_batch
from ngram_twin import TwinLm, draw_lm
from rnn_lm_fusion_twin import FusionLm
from rnn_lm_twin import Twin

pytestmark = pytest.mark.gpu
f32 = np.float32
CHUNKINGS = (1, 3, 7, 0)     # frames per call; 0: the whole utterance


def launches():
    from k2transducerasr_amd import load_library
    L = load_library()
    L.k2hip_debug_beam_launch_counts.argtypes = [C.POINTER(C.c_int64)] * 2
    p, h = C.c_int64(-1), C.c_int64(-1)
    assert L.k2hip_debug_beam_launch_counts(C.byref(p), C.byref(h)) == 0
    return p.value, h.value


@pytest.fixture(scope="module")
def lms(tmp_path_factory):
    """(LM name, seed) -> (RnnLm, FusionLm), made on first use"""
    from k2transducerasr_amd import RnnLm
    from k2transducerasr_amd.synth import write_synthetic_rnn_lm
    d = tmp_path_factory.mktemp("lodr_lms")
    made = {}

    def get(name, seed):
        if (name, seed) not in made:
            V, E, H, L, _ = lmc.LMS[name]
            p = str(d / f"{name}_{seed}.k2w")
            tw = Twin(write_synthetic_rnn_lm(p, V, E, H, L, seed), L)
            made[(name, seed)] = (RnnLm(p), FusionLm(tw))
        return made[(name, seed)]
    return get


def _world(model, ora):
    made = {}

    def enc(base):
        if base not in made:
            e = fc.encode(ora, fc.utterances(base))
            made[base] = (e,) + cases.lodr_lm(ora, e)      # (encoder output, TwinLm, entries)
        return made[base]
    return model, ora, enc


@pytest.fixture(scope="module")
def tiny(tiny_model_path, oracle_tiny):
    from k2transducerasr_amd import Model
    m = Model(tiny_model_path, 0)
    yield _world(m, oracle_tiny)
    m.close()


@pytest.fixture(scope="module")
def tiny165(tmp_path_factory):
    from k2transducerasr_amd import Model
    from k2transducerasr_amd.synth import write_synthetic_model
    from oracle import Oracle
    p = str(tmp_path_factory.mktemp("lodr165") / "tiny165.k2w")
    write_synthetic_model(p, "zipformer2-tiny-test", meta_overrides={"vocab_size": str(lmc.LMS["C"][0])})
    m = Model(p, 0)
    yield _world(m, Oracle(p))
    m.close()


class Fused:
    """the neural LM attached with both switches on, and (entries given) the LODR LM beside it"""

    def __init__(self, model, rlm, entries=None, lscale=0.0, scale=cases.SCALE, offline=True, streaming=True):
        self.m, self.rlm, self.entries, self.ls, self.scale, self.off, self.st = model, rlm, entries, lscale, scale, offline, streaming

    def __enter__(self):
        from k2transducerasr_amd import NgramLm
        self.m.set_rnn_lm(self.rlm, self.scale)
        self.m.set_rnn_lm_fusion(self.off)
        self.m.set_rnn_lm_stream_fusion(self.st)
        if self.entries is not None:
            self.m.set_lodr_lm(NgramLm(self.entries, self.m.vocab_size), self.ls)      # (the handle goes at once: the model keeps a copy)
        return self

    def __exit__(self, *a):
        self.m.set_lodr_lm(None)
        self.m.set_rnn_lm_fusion(False)
        self.m.set_rnn_lm_stream_fusion(False)
        self.m.set_rnn_lm(None)


@contextlib.contextmanager
def keep_alternatives(model, beam, n):
    model.set_decoding_method("modified_beam_search", beam)
    model.set_nbest(n)
    try:
        yield
    finally:
        model.set_nbest(1)
        model.set_decoding_method("greedy_search")


def bits(x):
    return f32(x).tobytes()


def alt_key(al):
    return [(a["tokens"], a["timestamps"], bits(a["score"]), np.asarray(a["token_log_probs"], f32).tobytes()) for a in al]


# ---- 1. the offline operator against the twin -----------------------------------------------------------------------------------------
def check_case(model, ora, enc, beam, rlm, nlm, lodr, entries, ls, what, **twin_kw):
    """the device equals the twin in tokens, timestamps and the number and order of alternatives with nothing excused; scores within
    lodr_cases.score_bound, token log-probs within YP_TOL.  Returns (device lists with LODR, device lists without)."""
    want, wsc, mg, _, runs = twin_batch(ora, enc, beam, nlm=nlm, nscale=cases.SCALE, nbest=cases.NBEST, lodr=lodr, lscale=ls, **twin_kw)
    ok, g = fc.accepted(runs)
    assert ok, f"{what}: not an accepted case (gap {g:.3g})"
    S, T = cases.case_smax(runs), enc.shape[1]
    with Fused(model, rlm):
        without = model.beam_search(enc, beam, nbest=cases.NBEST)
    with Fused(model, rlm, entries, ls):
        got, gsc = model.beam_search(enc, beam, want_scores=True)
        alts = model.beam_search(enc, beam, nbest=cases.NBEST)
    assert parity.assert_beam_match(got, want, mg, what=what, allow_tie=False) == len(want)
    worst, worst_yp = 0.0, 0.0
    for b, r in enumerate(runs):
        d = abs(float(gsc[b]) - r["lp"])
        worst = max(worst, d)
        print(f"{what} stream {b}: score {float(gsc[b]):.6f} twin {r['lp']:.6f} difference {d:.3g} bound {cases.score_bound(T, len(r['ys']), S):.3g}")
        assert d <= cases.score_bound(T, len(r["ys"]), S), (what, b, float(gsc[b]), r["lp"])
        assert len(alts[b]) == len(r["alts"]), (what, b, len(alts[b]), len(r["alts"]))
        assert bits(alts[b][0]["score"]) == gsc[b].tobytes()
        for a, w in zip(alts[b], r["alts"]):
            assert (list(a["tokens"]), list(a["timestamps"])) == (list(w["tokens"]), list(w["timestamps"])), (what, b)
            d = abs(a["score"] - w["score"])
            worst = max(worst, d)
            assert d <= cases.score_bound(T, len(w["tokens"]), S), (what, b, a["score"], w["score"])
            assert len(a["token_log_probs"]) == len(w["token_log_probs"])
            if len(w["tokens"]):
                e = float(np.abs(np.asarray(a["token_log_probs"], np.float64) - w["token_log_probs"]).max())
                worst_yp = max(worst_yp, e)
                assert e <= cases.YP_TOL, (what, b, e)
    print(f"{what}: {len(want)} streams equal the twin, worst score difference {worst:.3g} (bound {cases.score_bound(T, 1, S):.3g} and up, S = {S:.3g}), "
          f"worst token log-prob difference {worst_yp:.3g} (bound {cases.YP_TOL}), smallest twin gap {g:.3g}")
    return alts, without


def moved(alts, without):
    return sum([a["tokens"] for a in x] != [a["tokens"] for a in y] for x, y in zip(alts, without))


@pytest.mark.parametrize("name,beam", sorted(cases.SEEDS))
def test_operator_against_the_twin(tiny, tiny165, lms, name, beam):
    model, ora, enc_of = tiny165 if cases.OPERATOR[name] == "tiny165" else tiny
    base, seed, ls, _, rec_moved = cases.SEEDS[(name, beam)]
    enc, lodr, entries = enc_of(base)
    rlm, nlm = lms(name, seed)
    alts, without = check_case(model, ora, enc, beam, rlm, nlm, lodr, entries, ls, f"LM {name} beam {beam} LODR {ls}")
    assert moved(alts, without) == rec_moved, "the device's fused search without LODR differs from the twin's in what LODR moves"


@pytest.mark.parametrize("what", sorted(cases.TOGETHER))
def test_together_with_hotwords_and_an_ngram_lm(tiny, lms, what):
    from k2transducerasr_amd import Hotwords, NgramLm
    model, ora, enc_of = tiny
    base, seed, ls, _, rec_moved = cases.TOGETHER[what]
    enc, lodr, entries = enc_of(base)
    rlm, nlm = lms("A", seed)
    ex = fc.together_extras(ora, enc, what)
    try:
        if what == "hotwords":
            model.set_hotwords(Hotwords(ex["phrases"], ex["score"], model.vocab_size))
        else:      # two automata walked at once, of different sizes
            tri = NgramLm(ex["entries"], model.vocab_size)
            assert tri.num_states != lodr.num_states
            model.set_ngram_lm(tri, ex["scale"])
        alts, without = check_case(model, ora, enc, 4, rlm, nlm, lodr, entries, ls, f"LODR + neural LM + {what}", lm=ex.get("lm"),
                                   scale=ex.get("scale", 0.0), graph=ex.get("graph"))
        assert moved(alts, without) == rec_moved
    finally:
        model.set_hotwords(None)
        model.set_ngram_lm(None)


# ---- 2. the paths that ignore the setting ---------------------------------------------------------------------------------------------
def test_off_paths(tiny, lms, tiny_model_path, utts):
    from k2transducerasr_amd import NgramLm, OfflineRecognizer
    model, ora, enc_of = tiny
    base, seed, ls, _, _ = cases.SEEDS[("A", 4)]
    enc, lodr, entries = enc_of(base)
    rlm, _ = lms("A", seed)
    want, wsc = model.beam_search(enc, 4, want_scores=True)

    def plain_again(what):
        p0, h0 = launches()
        s0 = model.rnn_lm_fusion_stats()
        got, gsc = model.beam_search(enc, 4, want_scores=True)
        assert launches() == (p0 + 1, h0) and model.rnn_lm_fusion_stats() == s0, what
        assert got == want and gsc.tobytes() == wsc.tobytes(), what

    try:
        plain_again("nothing set")
        model.set_lodr_lm(NgramLm(entries, model.vocab_size), ls)
        plain_again("LODR set, no neural LM")
        model.set_rnn_lm(rlm, cases.SCALE)
        plain_again("LODR set, neural LM attached, fusion off")
        model.set_rnn_lm_fusion(True)
        model.set_rnn_lm(rlm, 0.0)
        plain_again("LODR set, fusion on, neural scale 0")
        # under active fusion: scale 0 and a cleared LODR LM give the fused search's bits
        model.set_rnn_lm(rlm, cases.SCALE)
        model.set_lodr_lm(None)
        fused, fsc = model.beam_search(enc, 4, want_scores=True)
        falts = model.beam_search(enc, 4, nbest=cases.NBEST)
        model.set_lodr_lm(NgramLm(entries, model.vocab_size), ls)
        moved_sc = model.beam_search(enc, 4, want_scores=True)[1]
        assert moved_sc.tobytes() != fsc.tobytes(), "LODR moves no score"
        for step in ("scale 0", "cleared"):
            if step == "scale 0":
                model.set_lodr_lm(NgramLm(entries, model.vocab_size), 0.0)
            else:
                model.set_lodr_lm(None)
            s0 = model.rnn_lm_fusion_stats()
            got, gsc = model.beam_search(enc, 4, want_scores=True)
            assert model.rnn_lm_fusion_stats()["searches"] == s0["searches"] + 1
            assert got == fused and gsc.tobytes() == fsc.tobytes(), step
            assert [alt_key(al) for al in model.beam_search(enc, 4, nbest=cases.NBEST)] == [alt_key(al) for al in falts], step
    finally:
        model.set_lodr_lm(None)
        model.set_rnn_lm_fusion(False)
        model.set_rnn_lm(None)

    # the batch entry: a recognizer with the LODR LM set, fusion inactive, N-best 1 -- the results and the counters of one without it
    def decode(rec):
        ss = [rec.create_offline_stream() for _ in utts]
        for s, u in zip(ss, utts):
            s.add_samples(u)
        p0, h0 = launches()
        s0 = rec.model.rnn_lm_fusion_stats()["searches"]
        res = rec.get_results(ss)
        p1, h1 = launches()
        return res, (p1 - p0, h1 - h0, rec.model.rnn_lm_fusion_stats()["searches"] - s0)

    ref = OfflineRecognizer(tiny_model_path, 0, "modified_beam_search", 4)
    rec = OfflineRecognizer(tiny_model_path, 0, "modified_beam_search", 4, rnn_lm=rlm, rnn_lm_scale=cases.SCALE,
                            lodr_lm=NgramLm(entries, model.vocab_size), lodr_scale=ls)
    try:
        r0, c0 = decode(ref)
        r1, c1 = decode(rec)
        assert r0 == r1 and c0 == c1 and c0[2] == 0 and c0[0] + c0[1] == 1, (c0, c1)
        rec.model.set_decoding_method("greedy_search")
        ref.model.set_decoding_method("greedy_search")
        assert rec.model.offline_greedy_from_samples(utts) == ref.model.offline_greedy_from_samples(utts)
    finally:
        rec.model.close()
        ref.model.close()


# ---- 3. streaming --------------------------------------------------------------------------------------------------------------------
def snapshot(s):
    return (s.tokens, s.timestamps, bits(s.score), alt_key(s.alternatives()))


def feed(model, enc, beam, step, check=None, graphs=None):
    from k2transducerasr_amd import BeamStream
    ss = [BeamStream(model, beam) for _ in range(enc.shape[0])]
    try:
        for s, g in zip(ss, graphs or []):
            if g is not None:
                s.set_hotwords(g)
        n, T = 0, enc.shape[1]
        while n < T:
            m = min(T, n + (step or T))
            BeamStream.search_chunk(ss, enc[:, n:m])
            n = m
            if check:
                check(n, ss)
        return [snapshot(s) for s in ss]
    finally:
        for s in ss:
            s.close()


def check_streaming_case(model, ora, enc, beam, rlm, nlm, lodr, entries, ls, what, **twin_kw):
    """every chunking, after every call: the engine's own offline fused-plus-LODR search over enc[:, :n] -- tokens, timestamps, the number
    and order of alternatives, nothing excused, score difference 0; at the full length the twin, which the acceptance rule covers"""
    B, T = enc.shape[0], enc.shape[1]
    want, _, mg, _, runs = twin_batch(ora, enc, beam, nlm=nlm, nscale=cases.SCALE, nbest=cases.NBEST, lodr=lodr, lscale=ls, **twin_kw)
    assert fc.accepted(runs)[0]
    S = cases.case_smax(runs)
    worst = dict(off=0.0, twin=0.0, checks=0)
    with Fused(model, rlm, entries, ls):
        ends = sorted({min(T, n) for step in CHUNKINGS for n in (range(step, T + step, step) if step else [T])})
        off = {n: (model.beam_search(enc[:, :n], beam, want_scores=True), model.beam_search(enc[:, :n], beam, nbest=cases.NBEST)) for n in ends}

        def check(n, ss):
            (res, sc), alts = off[n]
            for b, s in enumerate(ss):
                tag = (what, b, n)
                ga = s.alternatives()
                assert (s.tokens, s.timestamps) == (res[b][0], res[b][1]), tag
                assert [(a["tokens"], a["timestamps"]) for a in ga] == [(a["tokens"], a["timestamps"]) for a in alts[b]], tag
                for a, w in zip(ga, alts[b]):
                    worst["off"] = max(worst["off"], abs(a["score"] - w["score"]))
                    np.testing.assert_allclose(a["token_log_probs"], w["token_log_probs"], atol=cases.YP_TOL, rtol=0)
                worst["off"] = max(worst["off"], abs(s.score - float(sc[b])))
                if n == T:
                    tw = runs[b]
                    assert parity.assert_beam_match([(s.tokens, s.timestamps)], [(tw["ys"], tw["ts"])], tw["margins"][None], what=str(tag), allow_tie=False) == 1
                    assert [(a["tokens"], a["timestamps"]) for a in ga] == [(list(a["tokens"]), list(a["timestamps"])) for a in tw["alts"]], tag
                    for a, w in zip(ga, tw["alts"]):
                        worst["twin"] = max(worst["twin"], abs(a["score"] - w["score"]))
                        assert abs(a["score"] - w["score"]) <= cases.score_bound(T, len(w["tokens"]), S), (tag, a["score"], w["score"])
                worst["checks"] += 1

        with keep_alternatives(model, beam, cases.NBEST):
            finals = [feed(model, enc, beam, step, check) for step in CHUNKINGS]
    print(f"{what}: {worst['checks']} (stream, call) checks over chunkings {CHUNKINGS}; largest score difference against the offline search "
          f"{worst['off']:.3g} (must be 0), against the twin at the full length {worst['twin']:.3g}")
    assert worst["off"] == 0.0, worst
    assert all(f == finals[0] for f in finals), f"{what}: the chunkings disagree"


@pytest.mark.parametrize("name", cases.LMS)
def test_streaming_operator_every_chunking(tiny, tiny165, lms, name):
    model, ora, enc_of = tiny165 if cases.OPERATOR[name] == "tiny165" else tiny
    base, seed, ls, _, _ = cases.SEEDS[(name, 4)]
    enc, lodr, entries = enc_of(base)
    rlm, nlm = lms(name, seed)
    check_streaming_case(model, ora, enc, 4, rlm, nlm, lodr, entries, ls, f"streaming LM {name} beam 4 LODR {ls}")


def test_streaming_together_with_an_ngram_lm(tiny, lms):
    from k2transducerasr_amd import NgramLm
    model, ora, enc_of = tiny
    base, seed, ls, _, _ = cases.TOGETHER["ngram"]
    enc, lodr, entries = enc_of(base)
    rlm, nlm = lms("A", seed)
    ex = fc.together_extras(ora, enc, "ngram")
    try:
        model.set_ngram_lm(NgramLm(ex["entries"], model.vocab_size), ex["scale"])
        check_streaming_case(model, ora, enc, 4, rlm, nlm, lodr, entries, ls, "streaming LODR + neural LM + ngram", lm=ex["lm"], scale=ex["scale"])
    finally:
        model.set_ngram_lm(None)


def synthetic_bigram(V, seed=3):
    """a bi-gram over V tokens for the cases that have no plain search to draw from"""
    rng = np.random.default_rng(seed)
    real = [v for v in range(V) if v not in (0, 2)]
    results = [([int(x) for x in rng.choice(real, size=8)], []) for _ in range(6)]
    return draw_lm(results, V, np.random.default_rng(seed + 1), order=2)


REC = dict(seconds=(2.0, 1.2, 1.6), seeds=(67, 86, 78), join=(0, 0, 1), beam=4, lm="A", lm_seed=0, scale=0.5, lscale=-0.5)


def test_recognizer_equals_beam_streams(tmp_path, lms):
    """zipformer2-streaming-tiny-test, 3 ragged streams (one joins a tick later, all end at different ticks), stream 1 with hotwords,
    N-best 4, OnlineRecognizer(rnn_lm_fusion=True, lodr_lm=...).  Route B feeds the same features through the online encoder operator in the
    same batch composition and a BeamStream per stream: after every step each recognizer stream equals its BeamStream -- tokens,
    timestamps, alternatives, scores to the bit.  At the end every stream equals the offline fused-plus-LODR search over route B's frames,
    and differs from the same streams run without LODR somewhere."""
    from k2transducerasr_amd import BeamStream, Hotwords, NgramLm, OnlineProj, OnlineRecognizer
    from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model
    from hotword_twin import SCORE
    sp = str(tmp_path / "s.k2w")
    write_synthetic_model(sp, "zipformer2-streaming-tiny-test", blank_bias=0.0)
    rlm, _ = lms(REC["lm"], REC["lm_seed"])
    entries = synthetic_bigram(lmc.LMS[REC["lm"]][0])
    rec = OnlineRecognizer(sp, 0, "modified_beam_search", REC["beam"], rnn_lm=rlm, rnn_lm_scale=REC["scale"], rnn_lm_fusion=True, nbest=cases.NBEST,
                           lodr_lm=NgramLm(entries, lmc.LMS[REC["lm"]][0]), lodr_scale=REC["lscale"])
    proj = OnlineProj(sp)
    hw = None
    try:
        m = rec.model
        hw = Hotwords([[5, 9], [12, 3, 7]], SCORE, m.vocab_size)
        Tch, shift = rec.chunk_length, rec.shift_length
        feats = [np.ascontiguousarray(m.fbank(synth_utterance(s, sec)), np.float32) for s, sec in zip(REC["seeds"], REC["seconds"])]
        hs = [rec.create_online_stream(hotwords=hw if i == 1 else None) for i in range(3)]
        bs = [BeamStream(m, REC["beam"]) for _ in range(3)]
        bs[1].set_hotwords(hw)
        states = [proj.get_encoder_init_states() for _ in range(3)]
        pos, frames, fed, ticks, checks = [0, 0, 0], [[], [], []], [False] * 3, 0, 0
        while True:
            for i in range(3):
                if not fed[i] and REC["join"][i] <= ticks:
                    hs[i].add_features(feats[i])
                    fed[i] = True
            ready = [i for i in range(3) if fed[i] and feats[i].shape[0] - pos[i] >= Tch]
            if not ready:
                break
            dec, _ = rec.get_results(hs)
            assert [i for i in range(3) if dec[i]] == ready, (ticks, dec, ready)
            out = proj.encoder_proj(np.stack([feats[i][pos[i]: pos[i] + Tch] for i in ready]), [states[i] for i in ready])
            BeamStream.search_chunk([bs[i] for i in ready], out)
            for b, i in enumerate(ready):
                frames[i].append(out[b])
                pos[i] += shift
                assert hs[i].tokens == [0, 0] + bs[i].tokens and hs[i].timestamps == bs[i].timestamps, (ticks, i)
                assert alt_key(hs[i].alternatives()) == alt_key(bs[i].alternatives()), (ticks, i)
                checks += 1
            ticks += 1
        assert len({len(f) for f in frames}) == 3 and checks > 6      # ragged
        m.set_rnn_lm_fusion(True)      # (the offline switch, for the reference searches)
        with_lodr = []
        for i in range(3):
            enc = np.concatenate(frames[i])[None]
            m.set_hotwords(hw if i == 1 else None)
            off = m.beam_search(enc, REC["beam"], nbest=cases.NBEST)[0]
            m.set_hotwords(None)
            assert alt_key(bs[i].alternatives()) == alt_key(off), i
            with_lodr.append([a["tokens"] for a in off])
        m.set_lodr_lm(None)
        without = [[a["tokens"] for a in m.beam_search(np.concatenate(frames[i])[None], REC["beam"], nbest=cases.NBEST)[0]] for i in (0, 2)]
        assert without != [with_lodr[0], with_lodr[2]], "LODR moves nothing in the recognizer case"
    finally:
        rec.model.close()
        proj.model.close()
        if hw:
            hw.close()


def test_one_wide_tick(tiny, lms):
    """32 streams at beam 4 in 3 chunks of 8 frames against the offline search of the same batch over the same 24 frames: score difference 0"""
    model, ora, _ = tiny
    w = fc.WIDE
    enc = np.ascontiguousarray(fc.encode(ora, fc.wide_utterances())[:, :24])
    rlm, _ = lms(w["lm"], w["seed"])
    entries = cases.lodr_lm(ora, enc[:4])[1]
    with Fused(model, rlm, entries, -0.5):
        want, wsc = model.beam_search(enc, w["beam"], want_scores=True)
        walts = model.beam_search(enc, w["beam"], nbest=cases.NBEST)
        with keep_alternatives(model, w["beam"], cases.NBEST):
            got = feed(model, enc, w["beam"], 8)
    with Fused(model, rlm):
        plain = model.beam_search(enc, w["beam"], nbest=cases.NBEST)
    worst = 0.0
    for b in range(w["B"]):
        assert got[b][:2] == (want[b][0], want[b][1]), b
        assert [(a[0], a[1]) for a in got[b][3]] == [(a["tokens"], a["timestamps"]) for a in walts[b]], b
        for a, q in zip(got[b][3], walts[b]):
            worst = max(worst, abs(float(np.frombuffer(a[2], f32)[0]) - q["score"]))
        worst = max(worst, abs(float(np.frombuffer(got[b][2], f32)[0]) - float(wsc[b])))
    print(f"wide tick: 32 streams x beam 4 over 3 chunks of 8 frames against the offline search: largest score difference {worst:.3g} (must be 0); "
          f"{moved(walts, plain)} of 32 streams moved by LODR")
    assert worst == 0.0
    assert moved(walts, plain) > 0


# ---- 4. setting changes ---------------------------------------------------------------------------------------------------------------
def test_setting_changes(tiny, lms):
    from k2transducerasr_amd import BeamStream, K2HipError, NgramLm
    model, ora, enc_of = tiny
    base, seed, ls, _, _ = cases.SEEDS[("A", 4)]
    enc, lodr, entries = enc_of(base)
    rlm, _ = lms("A", seed)
    other = synthetic_bigram(model.vocab_size)
    with Fused(model, rlm, entries, ls):
        with keep_alternatives(model, 4, cases.NBEST):
            want7, want14, want = feed(model, enc[:1, :7], 4, 7), feed(model, enc[:1, :14], 4, 7), feed(model, enc[:1], 4, 7)
            a = BeamStream(model, 4)
            try:
                BeamStream.search_chunk([a], enc[:1, :7])
                assert snapshot(a) == want7[0]
                for change in (lambda: model.set_lodr_lm(NgramLm(entries, model.vocab_size), 2 * ls),       # another scale
                               lambda: model.set_lodr_lm(NgramLm(other, model.vocab_size), ls),             # another LM
                               lambda: model.set_lodr_lm(NgramLm(entries, model.vocab_size), ls),           # the same again: a new setting
                               lambda: model.set_lodr_lm(None)):                                            # cleared
                    change()
                    with pytest.raises(K2HipError) as e:
                        BeamStream.search_chunk([a], enc[:1, 7:14])
                    assert e.value.code == -1 and "reset the stream first" in str(e.value)
                    assert snapshot(a) == want7[0]
                    # a fresh stream beside it: decided for all streams of the call before anything changes
                    b = BeamStream(model, 4)
                    with pytest.raises(K2HipError):
                        BeamStream.search_chunk([b, a], enc[:2, :7])
                    assert b.tokens == [] and snapshot(a) == want7[0]
                    b.close()
                # reset: the stream starts over under the setting then set (none) and equals a new stream's run
                a.reset()
                BeamStream.search_chunk([a], enc[:1, :7])
                fresh = feed(model, enc[:1, :7], 4, 7)
                assert snapshot(a) == fresh[0] and fresh[0] != want7[0]
                # ... and under the restored LODR LM, from the start, the undisturbed run
                model.set_lodr_lm(NgramLm(entries, model.vocab_size), ls)
                a.reset()
                for n in (0, 7, 14):
                    BeamStream.search_chunk([a], enc[:1, n: n + 7])
                    if n == 7:
                        assert snapshot(a) == want14[0]
                assert snapshot(a) == want[0]
            finally:
                a.close()


# ---- 5. rescoring ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["transducer", "ctc"])
def test_recognizer_rescoring(kind, tmp_path, utts):
    from k2transducerasr_amd import NgramLm, OfflineRecognizer, RnnLm
    from k2transducerasr_amd.synth import write_synthetic_model, write_synthetic_rnn_lm
    from test_rnn_lm_gpu import decode
    rc = lmc.RECOGNIZER[kind]
    ctc = kind == "ctc"
    mp, lp_ = str(tmp_path / "m.k2w"), str(tmp_path / "lm.k2w")
    write_synthetic_model(mp, rc["preset"])
    V, E, H, L, _ = lmc.LMS["A"]
    write_synthetic_rnn_lm(lp_, V, E, H, L, rc["seed"])
    plain = OfflineRecognizer(mp, 0, rc["method"], 4, nbest=4)
    res0, alts0, _ = decode(plain, utts)
    plain.model.close()
    entries = draw_lm([(a["tokens"], a["timestamps"]) for al in alts0 for a in al[:1]], V, np.random.default_rng(cases.LODR_LM_SEED), order=2)
    lodr, ls = TwinLm(entries, V), -1.0
    only = OfflineRecognizer(mp, 0, rc["method"], 4, nbest=4, rnn_lm=RnnLm(lp_), rnn_lm_scale=rc["scale"])
    rec = OfflineRecognizer(mp, 0, rc["method"], 4, nbest=4, rnn_lm=RnnLm(lp_), rnn_lm_scale=rc["scale"], lodr_lm=NgramLm(entries, V), lodr_scale=ls)
    try:
        _, alts1, _ = decode(only, utts)
        assert all(a["lodr_score"] == 0.0 for al in alts1 for a in al)
        assert rec.create_offline_stream().alternative_lodr_score(0) == 0.0      # (nothing rescored yet)
        res, alts, _ = decode(rec, utts)
        gap, changed, B = np.inf, 0, len(utts)
        for b, (al, al1, al0) in enumerate(zip(alts, alts1, alts0)):
            lm_of = {(tuple(a["tokens"]), tuple(a["timestamps"])): a["lm_score"] for a in al1}      # the neural totals, checked elsewhere
            tot = [lodr_total(lodr, ls, a["tokens"]) for a in al0]
            order, keys = rescored_order([float(f32(a["score"])) for a in al0], [len(a["tokens"]) for a in al0],
                                         [lm_of[(tuple(a["tokens"]), tuple(a["timestamps"]))] for a in al0], rc["scale"], [float(t) for t in tot], ctc)
            ks = sorted(keys, reverse=True)
            gap = min([gap] + [x - y for x, y in zip(ks, ks[1:])])
            changed += [(a["tokens"], a["timestamps"]) for a in al] != [(a["tokens"], a["timestamps"]) for a in al1]
            assert len(al) == len(al0)
            for i, (a, j) in enumerate(zip(al, order)):
                w = al0[j]
                assert (a["tokens"], a["timestamps"]) == (w["tokens"], w["timestamps"]), (b, order)
                assert bits(a["score"]) == bits(w["score"])                      # reported scores stay the search's own
                assert bits(a["lodr_score"]) == bits(tot[j]), (b, i)             # lodr_i: the host walk, to the bit
                assert bits(a["lm_score"]) == bits(lm_of[(tuple(a["tokens"]), tuple(a["timestamps"]))])
            n = len(al[0]["tokens"])
            assert list(res[b][0])[len(res[b][0]) - n:] == al[0]["tokens"]
        print(f"{kind}: LODR changes the rescored order of {changed} of {B} lists, smallest adjacent key gap {gap:.4g}")
        assert gap >= 1e-5 and changed >= 1                                       # conditions of the chosen inputs
        if not ctc:      # both getters give 0 under active fusion
            rec.model.set_rnn_lm_fusion(True)
            _, falts, _ = decode(rec, utts)
            assert all(a["lodr_score"] == 0.0 and a["lm_score"] == 0.0 for al in falts for a in al)
    finally:
        rec.model.close()
        only.model.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(tiny, tiny_model_path, utts):
    from k2transducerasr_amd import K2HipError, Model, NgramLm
    model, ora, enc_of = tiny
    entries = synthetic_bigram(model.vocab_size)
    lm = NgramLm(entries, model.vocab_size)
    with pytest.raises(K2HipError) as e:
        model.set_lodr_lm(lm, 0.25)
    assert e.value.code == -1 and "k2hip_set_ngram_lm" in str(e.value)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(K2HipError) as e:
            model.set_lodr_lm(lm, bad)
        assert e.value.code == -1
    with pytest.raises(K2HipError) as e:
        model.set_lodr_lm(NgramLm(synthetic_bigram(model.vocab_size + 3), model.vocab_size + 3), -0.5)
    assert e.value.code == -1 and "vocab_size" in str(e.value)
    model.set_lodr_lm(lm, 0.0)      # "none"
    model.set_lodr_lm(None, 0.7)    # clearing takes any scale
    # while submitted batches are in flight
    m = Model(tiny_model_path, 0)
    try:
        t = m.offline_submit_samples(np.zeros((2, 16000), np.float32))
        with pytest.raises(K2HipError) as e:
            m.set_lodr_lm(lm, -0.5)
        assert e.value.code == -1 and "in flight" in str(e.value)
        m.offline_wait(t)
        m.set_lodr_lm(lm, -0.5)
    finally:
        m.close()
