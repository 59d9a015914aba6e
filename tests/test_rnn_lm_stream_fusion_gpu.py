"""Neural LM shallow fusion in the STREAMING modified beam search on the device (k2hip_set_rnn_lm_stream_fusion; csrc/rnn_lm_fuse.hip
k_nlm_load_streams / k_nlm_store_streams, the resumed form of beam.hip with the LM launches behind every frame): the two movers alone
bit for bit against numpy, the operator after every call of every chunking against the engine's own offline fused search (nothing
excused) and against the Python twin of the prefix (tests/rnn_lm_stream_fusion_cases.py), the carried state on the recorded "dropped
hypothesis" case, the recognizer against BeamStreams fed the same encoder frames, the switch, and one wide tick."""
import contextlib

import numpy as np
import pytest

import parity
import rnn_lm_cases as lmc
import rnn_lm_fusion_cases as oc
import rnn_lm_stream_fusion_cases as cases
from rnn_lm_fusion_twin import FusionLm, twin_beam_search
from rnn_lm_twin import Twin
from test_rnn_lm_fusion_gpu import launches, run_op

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def model(tiny_model_path):
    from k2transducerasr_amd import Model
    m = Model(tiny_model_path, 0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def lms(tmp_path_factory):
    """(LM name, seed) -> (RnnLm, FusionLm), made on first use"""
    from k2transducerasr_amd import RnnLm
    from k2transducerasr_amd.synth import write_synthetic_rnn_lm
    d = tmp_path_factory.mktemp("rnn_lm_stream_fusion")
    made = {}

    def get(name, seed):
        if (name, seed) not in made:
            V, E, H, L, _ = lmc.LMS[name]
            p = str(d / f"{name}_{seed}.k2w")
            tw = Twin(write_synthetic_rnn_lm(p, V, E, H, L, seed), L)
            made[(name, seed)] = (RnnLm(p), FusionLm(tw))
        return made[(name, seed)]
    return get


@pytest.fixture(scope="module")
def tiny(model, oracle_tiny):
    made = {}

    def enc(base):
        if base not in made:
            made[base] = oc.encode(oracle_tiny, oc.utterances(base))
        return made[base]
    return model, oracle_tiny, enc


@pytest.fixture(scope="module")
def tiny165(tmp_path_factory):
    from k2transducerasr_amd import Model
    from k2transducerasr_amd.synth import write_synthetic_model
    from oracle import Oracle
    p = str(tmp_path_factory.mktemp("models165s") / "tiny165.k2w")
    write_synthetic_model(p, "zipformer2-tiny-test", meta_overrides={"vocab_size": str(lmc.LMS["C"][0])})
    ora = Oracle(p)
    m = Model(p, 0)
    made = {}

    def enc(base):
        if base not in made:
            made[base] = oc.encode(ora, oc.utterances(base))
        return made[base]
    yield m, ora, enc
    m.close()


# ---- 1. the two movers alone -----------------------------------------------------------------------------------------------------------
def layout(K, L, H, V):
    """csrc/rnn_lm_stream_pool.h NlmStreamLayout restated: floats of a half, and a half's views (state [K][L][2][H], rows [K][V])"""
    ns = K * L * 2 * H
    return (ns + K * V + 3) // 4 * 4, ns


@pytest.mark.parametrize("B", [1, 5, 40])
@pytest.mark.parametrize("L,H,V", [(1, 32, 37), (2, 64, 37), (3, 96, 165)])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_movers_bit_for_bit(model, K, L, H, V, B):
    """load: every stream's current half into the parity-0 slot arrays, the start state for fresh streams (no block half) and for dead
    slots (k >= nh); store: the slot arrays into every block's OTHER half.  Destinations are NaN-filled (a missed element shows), the half
    a call must not touch comes back bit for bit, and so does the padding behind a half's rows.  V = 37 puts every row after the first
    off 16 bytes; B = 40 at K = 8 is 320 rows."""
    rng = np.random.default_rng(1000 * K + 10 * L + B + V)
    half, ns = layout(K, L, H, V)
    M = B * K
    blocks = rng.standard_normal((B, 2, half)).astype(f32)
    cur = rng.integers(-1, 2, size=B).astype(np.int32)        # -1: a fresh stream
    if B >= 5:
        cur[:3] = (-1, 0, 1)
    nh = rng.integers(1, K + 1, size=B).astype(np.int32)
    nh[0] = K if B == 1 else nh[0]
    if B >= 5:
        nh[1], nh[2] = 1, K
    h0, c0, q0 = (rng.standard_normal((L, H)).astype(f32), rng.standard_normal((L, H)).astype(f32), rng.standard_normal(V).astype(f32))
    nan = f32(np.nan)
    # load
    h, c, q = np.full((L, M, H), nan, f32), np.full((L, M, H), nan, f32), np.full((M, V), nan, f32)
    before = blocks.copy()
    io = np.zeros(4 * B, np.int32)
    run_op(model, "nlm_load_streams", [B, K, L, H, V], [blocks, cur, nh, h0, c0, q0, h, c, q, io], (1 << 0) | (1 << 6) | (1 << 7) | (1 << 8))
    assert np.array_equal(blocks.view(np.uint32), before.view(np.uint32)), "the load wrote into a block"
    wh, wc, wq = np.empty_like(h), np.empty_like(c), np.empty_like(q)
    for b in range(B):
        for k in range(K):
            m = b * K + k
            if cur[b] < 0 or k >= nh[b]:
                wh[:, m], wc[:, m], wq[m] = h0, c0, q0
            else:
                st = blocks[b, cur[b], :ns].reshape(K, L, 2, H)
                wh[:, m], wc[:, m] = st[k, :, 0], st[k, :, 1]
                wq[m] = blocks[b, cur[b], ns: ns + K * V].reshape(K, V)[k]
    for got, want, what in ((h, wh, "h"), (c, wc, "c"), (q, wq, "q")):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (what, K, L, H, V, B)
    # store
    h, c, q = (rng.standard_normal((L, M, H)).astype(f32), rng.standard_normal((L, M, H)).astype(f32), rng.standard_normal((M, V)).astype(f32))
    hb, cb, qb = h.copy(), c.copy(), q.copy()
    want = blocks.copy()
    for b in range(B):
        w = 0 if cur[b] < 0 else cur[b] ^ 1
        st = want[b, w, :ns].reshape(K, L, 2, H)
        st[:, :, 0] = h[:, b * K: (b + 1) * K].transpose(1, 0, 2)
        st[:, :, 1] = c[:, b * K: (b + 1) * K].transpose(1, 0, 2)
        want[b, w, ns: ns + K * V] = q[b * K: (b + 1) * K].reshape(-1)
        blocks[b, w, : ns + K * V] = nan          # the written half's payload: NaN until the store fills it
    run_op(model, "nlm_store_streams", [B, K, L, H, V], [blocks, cur, h, c, q, io], (1 << 0) | (1 << 2) | (1 << 3) | (1 << 4))
    assert np.array_equal(blocks.view(np.uint32), want.view(np.uint32)), ("store", K, L, H, V, B)
    assert np.array_equal(h.view(np.uint32), hb.view(np.uint32)) and np.array_equal(c.view(np.uint32), cb.view(np.uint32)) and \
        np.array_equal(q.view(np.uint32), qb.view(np.uint32)), "the store wrote into the slot arrays"


# ---- 2. the operator ---------------------------------------------------------------------------------------------------------------------
class Fused:
    """the LM attached with both switches on (the offline one for the reference searches, the streaming one for the streams)"""

    def __init__(self, model, lm, scale=cases.SCALE, offline=True, streaming=True):
        self.m, self.lm, self.scale, self.off, self.st = model, lm, scale, offline, streaming

    def __enter__(self):
        self.m.set_rnn_lm(self.lm, self.scale)
        self.m.set_rnn_lm_fusion(self.off)
        self.m.set_rnn_lm_stream_fusion(self.st)
        return self

    def __exit__(self, *a):
        self.m.set_rnn_lm_fusion(False)
        self.m.set_rnn_lm_stream_fusion(False)
        self.m.set_rnn_lm(None)


@contextlib.contextmanager
def keep_alternatives(model, beam, n):
    """the streams keep n alternatives and their token log-probs (k2hip_set_nbest wants the model under modified_beam_search)"""
    model.set_decoding_method("modified_beam_search", beam)
    model.set_nbest(n)
    try:
        yield
    finally:
        model.set_nbest(1)
        model.set_decoding_method("greedy_search")


def feed(model, enc, beam, step, check=None, graphs=None):
    """enc [B, T, J] through B BeamStreams in chunks of `step` (0: whole); check(n, streams) after every call.  Returns per stream
    (tokens, timestamps, score bits, alternatives as (tokens, timestamps, score bits, token log-prob bytes))"""
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


def snapshot(s):
    return (s.tokens, s.timestamps, f32(s.score).tobytes(),
            [(a["tokens"], a["timestamps"], f32(a["score"]).tobytes(), np.asarray(a["token_log_probs"], f32).tobytes()) for a in s.alternatives()])


def check_streaming_case(model, ora, enc, beam, rlm, nlm, what, near, graphs=None, offline_setup=None, **twin_kw):
    """every chunking, after every call: against the engine's offline fused search over the prefix (exact, scores within the bound and
    their largest difference printed) and against the twin of the prefix (order and pick excused only at the recorded near-tied ends)"""
    B, T = enc.shape[0], enc.shape[1]
    near = set(map(tuple, near))
    assert len(near) <= cases.CAP
    twins = [[twin_beam_search(ora, enc[b, :n], beam, nlm=nlm, nscale=cases.SCALE, nbest=cases.NBEST, **twin_kw) for n in range(1, T + 1)] for b in range(B)]
    worst = dict(off=0.0, twin=0.0, yp=0.0, excused=0, checks=0)
    with Fused(model, rlm):
        if offline_setup:
            offline_setup(True)
        try:
            off = {n: (model.beam_search(enc[:, :n], beam, want_scores=True), model.beam_search(enc[:, :n], beam, nbest=cases.NBEST)) for n in range(1, T + 1)}
        finally:
            if offline_setup:
                offline_setup(False)

        def check(n, ss):
            (res, sc), alts = off[n]
            for b, s in enumerate(ss):
                tag = (what, b, n)
                got_alts = s.alternatives()
                # the engine's own offline fused search over the same frames: nothing excused
                assert (s.tokens, s.timestamps) == (res[b][0], res[b][1]), tag
                assert len(got_alts) == len(alts[b]), tag
                assert [(a["tokens"], a["timestamps"]) for a in got_alts] == [(a["tokens"], a["timestamps"]) for a in alts[b]], tag
                for a, w in zip(got_alts, alts[b]):
                    d = abs(a["score"] - w["score"])
                    worst["off"] = max(worst["off"], d)
                    assert d <= cases.score_bound(n, len(w["tokens"])), (tag, a["score"], w["score"])
                    np.testing.assert_allclose(a["token_log_probs"], w["token_log_probs"], atol=cases.YP_TOL, rtol=0)
                worst["off"] = max(worst["off"], abs(s.score - float(sc[b])))
                assert abs(s.score - float(sc[b])) <= cases.score_bound(n, len(s.tokens)), tag
                # the twin of the prefix
                tw = twins[b][n - 1]
                talts = tw["alts"]
                assert len(got_alts) == len(talts), tag
                if (b, n) in near:
                    worst["excused"] += 1
                    # order and pick excused: the same alternatives as a set, the pick among the twin's entries within tolerance of its best
                    key = lambda a: (tuple(a["tokens"]), tuple(a["timestamps"]))   # noqa: E731
                    assert sorted(map(key, got_alts)) == sorted(map(key, talts)), tag
                    close = [key(a) for a in talts if talts[0]["norm"] - a["norm"] < parity.LOGIT_TOL]
                    assert (tuple(s.tokens), tuple(s.timestamps)) in close, tag
                    pairs = [(a, next(w for w in talts if key(w) == key(a))) for a in got_alts]
                else:
                    assert parity.assert_beam_match([(s.tokens, s.timestamps)], [(tw["ys"], tw["ts"])], tw["margins"][None], what=str(tag), allow_tie=False) == 1
                    assert [(a["tokens"], a["timestamps"]) for a in got_alts] == [(list(a["tokens"]), list(a["timestamps"])) for a in talts], tag
                    pairs = list(zip(got_alts, talts))
                    assert abs(s.score - tw["lp"]) <= cases.score_bound(n, len(tw["ys"])), (tag, s.score, tw["lp"])
                for a, w in pairs:
                    d = abs(a["score"] - w["score"])
                    worst["twin"] = max(worst["twin"], d)
                    assert d <= cases.score_bound(n, len(w["tokens"])), (tag, a["score"], w["score"])
                    if len(w["tokens"]):
                        e = float(np.abs(np.asarray(a["token_log_probs"], np.float64) - w["token_log_probs"]).max())
                        worst["yp"] = max(worst["yp"], e)
                        assert e <= cases.YP_TOL, (tag, e)
                worst["checks"] += 1

        with keep_alternatives(model, beam, cases.NBEST):
            finals = [feed(model, enc, beam, step, check, graphs) for step in cases.CHUNKINGS]
    assert all(f == finals[0] for f in finals), f"{what}: the chunkings disagree"
    print(f"{what}: {worst['checks']} (stream, call) checks over chunkings {cases.CHUNKINGS}; largest score difference against the offline fused search "
          f"{worst['off']:.3g}, against the twin {worst['twin']:.3g} (bound {cases.score_bound(T, 1):.3g} and up at n = {T}), token log-probs {worst['yp']:.3g}; "
          f"{worst['excused']} checks at the {len(near)} recorded near-tied prefix ends")
    return finals[0]


@pytest.mark.parametrize("name,beam", sorted(oc.SEEDS))
def test_operator_every_chunking(tiny, tiny165, lms, name, beam):
    model, ora, enc_of = tiny165 if oc.OPERATOR[name] == "tiny165" else tiny
    base, seed, _ = oc.SEEDS[(name, beam)]
    lm, nlm = lms(name, seed)
    check_streaming_case(model, ora, enc_of(base), beam, lm, nlm, f"LM {name} beam {beam}", cases.NEAR_TIED[(name, beam)])


@pytest.mark.parametrize("what", sorted(oc.TOGETHER))
def test_together_with_hotwords_and_an_ngram_lm(tiny, lms, what):
    from k2transducerasr_amd import Hotwords, NgramLm
    model, ora, enc_of = tiny
    base, seed, _ = oc.TOGETHER[what]
    enc = enc_of(base)
    lm, nlm = lms("A", seed)
    ex = oc.together_extras(ora, enc, what)
    hw = Hotwords(ex["phrases"], ex["score"], model.vocab_size) if what == "hotwords" else None
    try:
        if what == "ngram":
            model.set_ngram_lm(NgramLm(ex["entries"], model.vocab_size), ex["scale"])
        # (the offline reference takes its hotwords from the model, the streams each their own graph)
        check_streaming_case(model, ora, enc, 4, lm, nlm, f"neural LM + {what}", cases.NEAR_TIED_TOGETHER[what],
                             graphs=[hw] * enc.shape[0] if hw else None, offline_setup=(lambda on: model.set_hotwords(hw if on else None)) if hw else None,
                             lm=ex.get("lm"), scale=ex.get("scale", 0.0), graph=ex.get("graph"))
    finally:
        model.set_hotwords(None)
        model.set_ngram_lm(None)
        if hw:
            hw.close()


# ---- 3. the state is really carried ------------------------------------------------------------------------------------------------------
def test_carry_really_happens(tiny, tiny165, lms):
    """THE TEST THAT FAILS WITHOUT THE FEATURE.  On the recorded case the unfused search drops a hypothesis the fused one keeps: the fused
    streaming result differs from the unfused streaming one, equals the offline fused one, and with one frame per call differs from a
    search that starts from the start LM state at the last chunk (a fresh stream fed only the last chunk)."""
    d = cases.DROPPED
    model, ora, enc_of = tiny165 if oc.OPERATOR[d["name"]] == "tiny165" else tiny
    base, seed, _ = oc.SEEDS[(d["name"], d["beam"])]
    enc = enc_of(base)
    lm, _ = lms(d["name"], seed)
    b, n, beam = d["stream"], d["n"], d["beam"]
    with keep_alternatives(model, beam, 8):
        plain = feed(model, enc, beam, 1)
        plain_n = feed(model, enc[:, :n], beam, 1)
    with Fused(model, lm):
        off, off_sc = model.beam_search(enc, beam, want_scores=True)
        off_n = model.beam_search(enc[:, :n], beam, nbest=8)
        with keep_alternatives(model, beam, 8):
            c0 = model.rnn_lm_stream_fusion_stats()
            fused = feed(model, enc, beam, 1)
            c1 = model.rnn_lm_stream_fusion_stats()
            fused_n = feed(model, enc[:, :n], beam, 1)
            last = feed(model, enc[:, -1:], beam, 1)
    assert c1["chunk_calls"] - c0["chunk_calls"] == enc.shape[1] and c1["live_blocks"] == 0
    assert fused[b][:2] != plain[b][:2], "fusion moves nothing on the recorded case"
    assert [f[:2] for f in fused] == [(r[0], r[1]) for r in off]
    assert all(abs(float(np.frombuffer(f[2], f32)[0]) - float(s)) <= cases.score_bound(enc.shape[1], len(f[0])) for f, s in zip(fused, off_sc))
    # the dropped hypothesis: in the fused beam after n frames (streaming and offline), not in the unfused one
    assert d["tokens"] in [a[0] for a in fused_n[b][3]] and d["tokens"] in [a["tokens"] for a in off_n[b]]
    assert d["tokens"] not in [a[0] for a in plain_n[b][3]]
    assert fused[b][:2] != last[b][:2]


# ---- 4. the recognizer ------------------------------------------------------------------------------------------------------------------
# The recognizer draw: per stream the first utterance seed (in the order 61, 64, 67 .. for stream 0, one and two further for streams 1 and
# 2) whose fused twin run over the CPU oracle's chunk frames is accepted by rnn_lm_fusion_cases.accepted (gaps 0.0019, 0.011, 0.0038); the
# test re-checks acceptance on the frames it collects
REC = dict(seconds=(2.0, 1.2, 1.6), seeds=(67, 86, 78), join=(0, 0, 1), beam=4, lm="A", lm_seed=0, scale=0.5, chunks=[5, 3, 4])


def test_recognizer_equals_beam_streams(tmp_path, lms):
    """zipformer2-streaming-tiny-test, 3 streams of unequal length, one joining a tick later and all finishing at different ticks, stream
    1 with hotwords, N-best 4, OnlineRecognizer(rnn_lm_fusion=True).  Route B feeds the same features through the online encoder
    operator in the same batch composition and a BeamStream per stream: after every step each recognizer stream equals its BeamStream --
    tokens, timestamps and alternatives exactly, scores within the bound.  At the final end the twin over route B's frames, where the
    draw is accepted by the rule of rnn_lm_fusion_cases on those frames."""
    from k2transducerasr_amd import BeamStream, Hotwords, OnlineProj, OnlineRecognizer
    from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model
    from hotword_twin import SCORE, TwinGraph
    from oracle.online import OnlineOracle
    sp = str(tmp_path / "s.k2w")
    write_synthetic_model(sp, "zipformer2-streaming-tiny-test", blank_bias=0.0)
    lm, nlm = lms(REC["lm"], REC["lm_seed"])
    rec = OnlineRecognizer(sp, 0, "modified_beam_search", REC["beam"], rnn_lm=lm, rnn_lm_scale=REC["scale"], rnn_lm_fusion=True, nbest=cases.NBEST)
    proj = OnlineProj(sp)
    hw = None
    try:
        m = rec.model
        assert m.vocab_size == lmc.LMS[REC["lm"]][0]
        phrases = [[5, 9], [12, 3, 7]]
        hw = Hotwords(phrases, SCORE, m.vocab_size)
        Tch, shift, Tp = rec.chunk_length, rec.shift_length, rec.frames_per_chunk
        feats = [np.ascontiguousarray(m.fbank(synth_utterance(s, sec)), np.float32) for s, sec in zip(REC["seeds"], REC["seconds"])]
        hs = [rec.create_online_stream(hotwords=hw if i == 1 else None) for i in range(3)]
        bs = [BeamStream(m, REC["beam"]) for _ in range(3)]
        bs[1].set_hotwords(hw)
        states = [proj.get_encoder_init_states() for _ in range(3)]
        pos, frames, fed, done = [0, 0, 0], [[], [], []], [False] * 3, [0, 0, 0]
        c0 = m.rnn_lm_stream_fusion_stats()["chunk_calls"]
        worst, checks, ticks = 0.0, 0, 0
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
                done[i] += 1
                assert hs[i].tokens == [0, 0] + bs[i].tokens and hs[i].timestamps == bs[i].timestamps, (ticks, i)
                ga, wa = hs[i].alternatives(), bs[i].alternatives()
                assert [(a["tokens"], a["timestamps"]) for a in ga] == [(a["tokens"], a["timestamps"]) for a in wa], (ticks, i)
                for a, w in zip(ga, wa):
                    worst = max(worst, abs(a["score"] - w["score"]))
                    assert abs(a["score"] - w["score"]) <= cases.score_bound(done[i] * Tp, len(w["tokens"]), REC["scale"]), (ticks, i)
                checks += 1
            ticks += 1
        assert done == REC["chunks"], done
        assert m.rnn_lm_stream_fusion_stats()["chunk_calls"] - c0 == 2 * ticks      # (the recognizer's tick and route B's call)
        # the twin at the final end, on the streams whose run over route B's frames the acceptance rule admits
        ora = OnlineOracle(sp)
        accepted = 0
        for i in range(3):
            enc = np.concatenate(frames[i])
            tw = twin_beam_search(ora, enc, REC["beam"], nlm=nlm, nscale=REC["scale"], nbest=cases.NBEST,
                                  graph=TwinGraph(phrases, SCORE, ora.vocab_size) if i == 1 else None)
            ok, g = oc.accepted([tw])
            print(f"recognizer stream {i}: {done[i]} chunks, twin gap {g:.3g}, {'accepted' if ok else 'NOT accepted'}")
            assert ok, (i, g)
            accepted += 1
            assert (bs[i].tokens, bs[i].timestamps) == (tw["ys"], tw["ts"]), i
            for a, w in zip(bs[i].alternatives(), tw["alts"]):
                assert (a["tokens"], a["timestamps"]) == (list(w["tokens"]), list(w["timestamps"])), i
                assert abs(a["score"] - w["score"]) <= cases.score_bound(enc.shape[0], len(w["tokens"]), REC["scale"]), (i, a["score"], w["score"])
        assert accepted == 3
        print(f"recognizer: {checks} (stream, tick) checks over {ticks} ticks, chunks per stream {done}, largest score difference against the BeamStreams {worst:.3g}")
    finally:
        rec.model.close()
        proj.model.close()
        if hw:
            hw.close()


# ---- 5. the switch -----------------------------------------------------------------------------------------------------------------------
def test_switch_behaviour(tiny, lms):
    """switch off, scale 0, LM cleared, only the offline switch on: the results and k2hip_debug_beam_launch_counts of the plain streaming
    search, the new stats unmoved; on: a counter of its own.  A refused call on streams that hold blocks leaves blocks and streams as they
    were and the next good call continues an uninterrupted run (the device offers no refusal AFTER staging: that path -- no flip, the
    call's blocks given back -- runs over the stand-in engine in tests/native/san_rnn_lm_stream_fusion_driver.cpp); the mid-stream
    refusals; reset and re-use."""
    from k2transducerasr_amd import BeamStream, K2HipError
    model, ora, enc_of = tiny
    base, seed, _ = oc.SEEDS[("A", 4)]
    enc = enc_of(base)
    lm, _ = lms("A", seed)
    lm2, _ = lms("B", seed)
    model.set_decoding_method("modified_beam_search", 4)
    model.set_nbest(cases.NBEST)
    try:
        want = feed(model, enc, 4, 7)

        def plain_again(what):
            p0, h0 = launches()
            s0, f0 = model.rnn_lm_stream_fusion_stats(), model.rnn_lm_fusion_stats()
            got = feed(model, enc, 4, 7)
            assert launches() == (p0 + 3, h0), what            # (20 frames in chunks of 7: three calls of the plain kernels)
            assert model.rnn_lm_stream_fusion_stats() == s0 and model.rnn_lm_fusion_stats() == f0, what
            assert got == want, what

        plain_again("nothing attached")
        model.set_rnn_lm(lm, cases.SCALE)
        plain_again("LM attached, both switches off")
        model.set_rnn_lm_fusion(True)
        plain_again("only the offline switch on")
        model.set_rnn_lm_fusion(False)
        model.set_rnn_lm_stream_fusion(True)
        model.set_rnn_lm(lm, 0.0)
        plain_again("streaming switch on, scale 0")
        model.set_rnn_lm(None)
        plain_again("streaming switch on, LM cleared")
        model.set_rnn_lm(lm, cases.SCALE)
        p0, h0 = launches()
        s0, f0 = model.rnn_lm_stream_fusion_stats(), model.rnn_lm_fusion_stats()
        fused = feed(model, enc, 4, 7)
        s1 = model.rnn_lm_stream_fusion_stats()
        assert launches() == (p0, h0) and model.rnn_lm_fusion_stats() == f0
        assert s1["chunk_calls"] == s0["chunk_calls"] + 3 and s1["live_blocks"] == 0 and s1["pool_bytes"] > 0
        assert [f[:2] for f in fused] != [w[:2] for w in want]

        # a failed call on streams that hold blocks (an argument refusal) leaves blocks and streams as they were
        ss = [BeamStream(model, 4) for _ in range(3)]
        BeamStream.search_chunk(ss, enc[:, :7])
        live = model.rnn_lm_stream_fusion_stats()
        assert live["live_blocks"] == 3
        before = [snapshot(s) for s in ss]
        with pytest.raises(K2HipError):
            BeamStream.search_chunk(ss + [ss[0]], np.concatenate([enc[:, 7:14], enc[:1, 7:14]]))      # the same stream twice
        assert [snapshot(s) for s in ss] == before and model.rnn_lm_stream_fusion_stats()["live_blocks"] == 3
        BeamStream.search_chunk(ss, enc[:, 7:14])
        BeamStream.search_chunk(ss, enc[:, 14:])
        assert [snapshot(s) for s in ss] == fused, "the call after a failed one does not continue an uninterrupted run"

        # the mid-stream refusals: the switch, the scale, the LM -- each INVALID, the stream as it was; back under its own setting it goes on
        a = BeamStream(model, 4)
        BeamStream.search_chunk([a], enc[:1, :7])
        snap = snapshot(a)
        for change, undo in ((lambda: model.set_rnn_lm_stream_fusion(False), lambda: model.set_rnn_lm_stream_fusion(True)),
                             (lambda: model.set_rnn_lm(lm, 0.25), None), (lambda: model.set_rnn_lm(lm2, cases.SCALE), None),
                             (lambda: model.set_rnn_lm(lm, cases.SCALE), None)):      # (the same LM set again is a new setting)
            change()
            with pytest.raises(K2HipError) as e:
                BeamStream.search_chunk([a], enc[:1, 7:14])
            assert e.value.code == -1 and "reset the stream first" in str(e.value)
            assert snapshot(a) == snap
            if undo:
                undo()
                BeamStream.search_chunk([a], enc[:1, 7:14])
                snap = snapshot(a)
        # a fresh stream beside it: one call cannot mix settings
        b = BeamStream(model, 4)
        with pytest.raises(K2HipError):
            BeamStream.search_chunk([b, a], enc[:2, :7])
        assert b.tokens == [] and model.rnn_lm_stream_fusion_stats()["live_blocks"] == 4
        # reset and re-use: the block goes back, the stream starts over under the current setting and equals a new stream
        a.reset()
        assert model.rnn_lm_stream_fusion_stats()["live_blocks"] == 3
        n = 0
        while n < enc.shape[1]:
            BeamStream.search_chunk([a, b], enc[:2, n: n + 7])
            n += 7
        fresh = feed(model, enc[:2], 4, 7)
        assert [snapshot(a), snapshot(b)] == fresh
        for s in ss + [a, b]:
            s.close()
        assert model.rnn_lm_stream_fusion_stats()["live_blocks"] == 0
    finally:
        model.set_rnn_lm_fusion(False)
        model.set_rnn_lm_stream_fusion(False)
        model.set_rnn_lm(None)
        model.set_nbest(1)
        model.set_decoding_method("greedy_search")


def test_stream_outlives_its_model(tiny_model_path, tiny, lms):
    """model destroy frees the pool; a stream reset or destroyed afterwards must not touch freed memory (it only forgets its block)"""
    import k2transducerasr_amd as pkg
    _, _, enc_of = tiny
    enc = enc_of(oc.SEEDS[("A", 4)][0])
    lm, _ = lms("A", 0)
    m = pkg.Model(tiny_model_path, 0)
    m.set_rnn_lm(lm, cases.SCALE)
    m.set_rnn_lm_stream_fusion(True)
    a, b = pkg.BeamStream(m, 4), pkg.BeamStream(m, 4)
    pkg.BeamStream.search_chunk([a, b], enc[:2, :5])
    assert m.rnn_lm_stream_fusion_stats()["live_blocks"] == 2
    m._children.discard(a)
    m._children.discard(b)
    m.close()
    assert a._L.k2hip_beam_stream_reset(a._h) == 0
    a.close()
    b.close()


# ---- 6. one wide tick --------------------------------------------------------------------------------------------------------------------
def test_one_wide_tick(model, oracle_tiny, lms):
    """32 streams, beam 4 (128 slots: four row strips per LM launch), LM A, 3 chunks of 8 frames of the wide case's utterances: every
    stream equals the offline fused search of the same batch over the same 24 frames exactly"""
    w = oc.WIDE
    enc = np.ascontiguousarray(oc.encode(oracle_tiny, oc.wide_utterances())[:, :24])
    lm, _ = lms(w["lm"], w["seed"])
    with Fused(model, lm):
        want, wsc = model.beam_search(enc, w["beam"], want_scores=True)
        walts = model.beam_search(enc, w["beam"], nbest=cases.NBEST)
        with keep_alternatives(model, w["beam"], cases.NBEST):
            got = feed(model, enc, w["beam"], 8)
    worst = 0.0
    for b in range(w["B"]):
        assert got[b][:2] == (want[b][0], want[b][1]), b
        assert [(a[0], a[1]) for a in got[b][3]] == [(a["tokens"], a["timestamps"]) for a in walts[b]], b
        for a, q in zip(got[b][3], walts[b]):
            d = abs(float(np.frombuffer(a[2], f32)[0]) - q["score"])
            worst = max(worst, d)
            assert d <= cases.score_bound(24, len(q["tokens"])), (b, d)
    print(f"wide tick: 32 streams x beam 4 over 3 chunks of 8 frames equal the offline fused search; largest score difference {worst:.3g}")
