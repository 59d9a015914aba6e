"""Neural LM shallow fusion on the device (csrc/rnn_lm_fuse.hip, the NLM instantiation of k_beam_step): the two LM launches alone through
k2hip_debug_op_run against float64, the fused search against the Python twin (tests/rnn_lm_fusion_twin.py) on the accepted cases of
tests/rnn_lm_fusion_cases.py, together with hotwords and an n-gram LM, the switch, the idle frames and one wide batch."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import parity
import rnn_lm_cases as lmc
import rnn_lm_fusion_cases as cases
from rnn_lm_fusion_twin import FusionLm, twin_batch
from rnn_lm_twin import Twin

pytestmark = pytest.mark.gpu
f32 = np.float32


@contextlib.contextmanager
def switches(**kw):
    import k2transducerasr_amd as pkg
    try:
        for k, v in kw.items():
            pkg.set_switch(k, v)
        yield
    finally:
        for k in kw:
            pkg.set_switch(k, 0)


def run_op(model, op, ints, bufs, out_mask):
    L = model._L
    L.k2hip_debug_op_run.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                     C.c_int32, C.c_uint32]
    ia = (C.c_int64 * len(ints))(*ints)
    ptrs = (C.c_void_p * len(bufs))(*[b.ctypes.data for b in bufs])
    sizes = (C.c_int64 * len(bufs))(*[b.nbytes for b in bufs])
    rc = L.k2hip_debug_op_run(model.handle, op.encode(), ia, len(ints), ptrs, sizes, len(bufs), out_mask)
    assert rc == 0, L.k2hip_last_error()


def launches():
    from k2transducerasr_amd import load_library
    L = load_library()
    L.k2hip_debug_beam_launch_counts.argtypes = [C.POINTER(C.c_int64)] * 2
    p, h = C.c_int64(-1), C.c_int64(-1)
    assert L.k2hip_debug_beam_launch_counts(C.byref(p), C.byref(h)) == 0
    return p.value, h.value


@pytest.fixture(scope="module")
def model(tiny_model_path):
    from k2transducerasr_amd import Model
    m = Model(tiny_model_path, 0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def lms(tmp_path_factory):
    """(LM name, seed) -> (RnnLm, FusionLm, Twin), made on first use"""
    from k2transducerasr_amd import RnnLm
    from k2transducerasr_amd.synth import write_synthetic_rnn_lm
    d = tmp_path_factory.mktemp("rnn_lm_fusion")
    made = {}

    def get(name, seed):
        if (name, seed) not in made:
            V, E, H, L, _ = lmc.LMS[name]
            p = str(d / f"{name}_{seed}.k2w")
            tw = Twin(write_synthetic_rnn_lm(p, V, E, H, L, seed), L)
            made[(name, seed)] = (RnnLm(p), FusionLm(tw), tw)
        return made[(name, seed)]
    return get


@pytest.fixture(scope="module")
def tiny(model, oracle_tiny):
    """(Model, Oracle, base -> encoder output of the case's three utterances) of the V = 37 model"""
    made = {}

    def enc(base):
        if base not in made:
            made[base] = cases.encode(oracle_tiny, cases.utterances(base))
        return made[base]
    return model, oracle_tiny, enc


@pytest.fixture(scope="module")
def tiny165(tmp_path_factory):
    from k2transducerasr_amd import Model
    from k2transducerasr_amd.synth import write_synthetic_model
    from oracle import Oracle
    p = str(tmp_path_factory.mktemp("models165") / "tiny165.k2w")
    write_synthetic_model(p, "zipformer2-tiny-test", meta_overrides={"vocab_size": str(lmc.LMS["C"][0])})
    ora = Oracle(p)
    m = Model(p, 0)
    yield m, ora, lambda base: cases.encode(ora, cases.utterances(base))
    m.close()


# ---- 1. the LM launches alone ---------------------------------------------------------------------------------------------------------
def relay(w_ih, w_hh):
    """kernels.h RnnLmDev::wcat restated: [W_ih | zeros up to a multiple of 32 | W_hh] along k; panel jb = [Kc / 4][32][4], its column c the
    gate c // 8 of hidden column 8 jb + c % 8"""
    H, I = w_hh.shape[1], w_ih.shape[1]
    Ip = (I + 31) // 32 * 32
    cat = np.zeros((4 * H, Ip + H), f32)
    cat[:, :I] = w_ih
    cat[:, Ip:] = w_hh
    p = cat.reshape(4, H // 8, 8, (Ip + H) // 4, 4)   # gate, block, column of the block, k / 4, k % 4
    return np.ascontiguousarray(p.transpose(1, 3, 0, 2, 4)).reshape(-1)


def parent_maps(M, rng):
    """name -> (par, appended mask)"""
    ident = np.arange(M, dtype=np.int32)
    mix = rng.integers(0, M, size=M).astype(np.int32)
    keep = np.ones(M, bool)
    keep[::3] = False       # rows 0, 3, 6 .. keep their parent's state
    return {"identity": (ident, np.ones(M, bool)), "reversed": (ident[::-1].copy(), np.ones(M, bool)),
            "one parent": (np.full(M, M // 2, np.int32), np.ones(M, bool)), "keep and append": (mix, keep)}


@pytest.mark.parametrize("E,H", [(32, 32), (64, 64), (32, 96), (20, 32)])   # (20: input columns padded up to 32)
def test_nlm_advance_against_float64(model, E, H):
    """rows in {1, 5, 33, 100, 130, 300} under every parent map, x from an embedding (layer 0) and from rows (the layers above): the rows that
    appended against float64, the others bit-equal to their parent's state.  The operands nobody may read are NaN: x of rows that
    appended nothing, embedding rows no token names, h and c of slots that are nobody's parent.  Tolerance: test_step_kernel_one_step's
    derivation over the K = E + H products a gate sums here (|x|, |h| <= 1, |w| <= 1 / sqrt(K)): 4 K 2^-24 sqrt(K) + 2e-6."""
    rng = np.random.default_rng(100 * E + H)
    K, V = E + H, 9
    w_ih = rng.uniform(-1, 1, size=(4 * H, E)).astype(f32) / f32(np.sqrt(K))
    w_hh = rng.uniform(-1, 1, size=(4 * H, H)).astype(f32) / f32(np.sqrt(K))
    bias = rng.uniform(-1, 1, size=4 * H).astype(f32)
    wcat = relay(w_ih, w_hh)
    tol = 4 * K * 2.0 ** -24 * np.sqrt(K) + 2e-6
    sig = lambda v: 1 / (1 + np.exp(-v))   # noqa: E731
    worst = 0.0
    for M in (1, 5, 33, 100, 130, 300):   # (100: four strips, one per wave; 300: a second block of rows, blockIdx.y = 1)
        for name, (par, app) in parent_maps(M, rng).items():
            for use_emb in (1, 0):
                hp = rng.uniform(-1, 1, size=(M, H)).astype(f32)
                cp = rng.uniform(-1, 1, size=(M, H)).astype(f32)
                unread = np.setdiff1d(np.arange(M), par)
                hp[unread] = np.nan
                cp[unread] = np.nan
                if use_emb:
                    x = rng.uniform(-1, 1, size=(V, E)).astype(f32)
                    tok = np.where(app, rng.integers(0, V - 1, size=M), -1).astype(np.int32)
                    x[V - 1] = np.nan          # (no row names the last token)
                    xin = np.where(app[:, None], x[np.maximum(tok, 0)], 0)
                else:
                    x = rng.uniform(-1, 1, size=(M, E)).astype(f32)
                    tok = np.where(app, 3, -1).astype(np.int32)
                    x[~app] = np.nan
                    xin = np.where(app[:, None], x, 0)
                for live in ((-1, 1, 0) if M == 33 else (-1,)):
                    ho, co = np.full((M, H), -7.0, f32), np.full((M, H), -7.0, f32)
                    flag, work = np.zeros(1, np.int32), np.zeros(2, np.int64)
                    run_op(model, "nlm_advance", [M, E, H, use_emb, V, live], [wcat, bias, x, hp, cp, ho, co, par, tok, flag, work],
                           (1 << 5) | (1 << 6) | (1 << 10))
                    what = (M, name, use_emb, live)
                    assert work.tolist() == ([0, 1] if live == 0 else [1, 0]), what
                    on = app & (live != 0)
                    g = xin.astype(np.float64) @ w_ih.astype(np.float64).T + bias + hp[par].astype(np.float64) @ w_hh.astype(np.float64).T
                    wc = sig(g[:, H: 2 * H]) * cp[par] + sig(g[:, :H]) * np.tanh(g[:, 2 * H: 3 * H])
                    wh = sig(g[:, 3 * H:]) * np.tanh(wc)
                    if on.any():
                        err = max(np.abs(co[on] - wc[on]).max(), np.abs(ho[on] - wh[on]).max())
                        worst = max(worst, float(err))
                        assert err <= tol, (what, err, tol)
                    assert np.array_equal(ho[~on].view(np.uint32), hp[par][~on].view(np.uint32)), what
                    assert np.array_equal(co[~on].view(np.uint32), cp[par][~on].view(np.uint32)), what
    print(f"nlm_advance E = {E}, H = {H}: worst error {worst:.3g}, tolerance {tol:.3g}")


@pytest.mark.parametrize("M,H,V", [(1, 32, 37), (33, 64, 165), (130, 96, 37)])
def test_nlm_rows_against_float64(model, M, H, V):
    """q of the rows that appended against float64 within rnn_lm_cases.token_bound() (operands in the LMs' range: |h| <= 1, the output
    layer as synth draws it); the other rows bit-equal to their parent's row.  Rows are V floats: there is no column >= V to enter the
    sum, and the guard bands of the operator's buffers hold NaN patterns."""
    rng = np.random.default_rng(M + H + V)
    h = rng.uniform(-1, 1, size=(M, H)).astype(f32)
    w = (rng.uniform(-1, 1, size=(V, H)) / np.sqrt(H)).astype(f32)
    b = rng.uniform(-1, 1, size=V).astype(f32) * f32(0.1)
    qp = rng.standard_normal((M, V)).astype(f32)
    par = rng.integers(0, M, size=M).astype(np.int32)
    app = np.ones(M, bool)
    app[1::4] = False
    tok = np.where(app, 5, -1).astype(np.int32)
    h[~app] = np.nan
    z = np.where(app[:, None], h, 0).astype(np.float64) @ w.astype(np.float64).T + b
    mx = z.max(1, keepdims=True)
    want = z - (mx + np.log(np.exp(z - mx).sum(1, keepdims=True)))
    for live in (-1, 1, 0):
        qo = np.full((M, V), -7.0, f32)
        run_op(model, "nlm_rows", [M, H, V, live], [h, w, b, qp, qo, par, tok, np.zeros(1, np.int32)], 1 << 4)
        on = app & (live != 0)
        if on.any():
            err = float(np.abs(qo[on] - want[on]).max())
            print(f"nlm_rows M = {M}, H = {H}, V = {V}, live {live}: error {err:.3g}, bound {lmc.token_bound():.3g}")
            assert err <= lmc.token_bound(), (live, err)
        assert np.array_equal(qo[~on].view(np.uint32), qp[par][~on].view(np.uint32)), live


# ---- 2. the operator against the twin ---------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def fusion(model, lm, scale):
    model.set_rnn_lm(lm, scale)
    model.set_rnn_lm_fusion(True)
    try:
        yield
    finally:
        model.set_rnn_lm_fusion(False)
        model.set_rnn_lm(None)


def check_case(model, ora, enc, beam, rlm, nlm, nscale, what, plain_alts, **twin_kw):
    """the device against the twin on an accepted case: the result and (N-best 4) the list, with nothing excused"""
    want, wsc, mg, wtr, runs = twin_batch(ora, enc, beam, nlm=nlm, nscale=nscale, nbest=cases.NBEST, **twin_kw)
    ok, g = cases.accepted(runs)
    assert ok, f"{what}: not an accepted case (gap {g:.3g})"
    with fusion(model, rlm, nscale):
        got, gsc = model.beam_search(enc, beam, want_scores=True)
        alts = model.beam_search(enc, beam, nbest=cases.NBEST)
    assert parity.assert_beam_match(got, want, mg, what=what, allow_tie=False) == len(want)
    worst, worst_yp, T = 0.0, 0.0, enc.shape[1]
    for b, r in enumerate(runs):
        tol = cases.score_bound(T, len(r["ys"]), nscale)
        worst = max(worst, abs(float(gsc[b]) - r["lp"]))
        assert abs(float(gsc[b]) - r["lp"]) <= tol, (what, b, float(gsc[b]), r["lp"], tol)
        assert len(alts[b]) == len(r["alts"]), (what, b, len(alts[b]), len(r["alts"]))
        assert np.float32(alts[b][0]["score"]).tobytes() == gsc[b].tobytes()
        for a, w in zip(alts[b], r["alts"]):
            assert (list(a["tokens"]), list(a["timestamps"])) == (list(w["tokens"]), list(w["timestamps"])), (what, b)
            worst = max(worst, abs(a["score"] - w["score"]))
            assert abs(a["score"] - w["score"]) <= cases.score_bound(T, len(w["tokens"]), nscale), (what, b, a["score"], w["score"])
            # token log-probs stay acoustic: every alternative's against the twin's log-softmax terms, which carry no LM
            assert len(a["token_log_probs"]) == len(w["token_log_probs"])
            if len(w["tokens"]):
                e = float(np.abs(np.asarray(a["token_log_probs"], np.float64) - w["token_log_probs"]).max())
                worst_yp = max(worst_yp, e)
                assert e <= cases.YP_TOL, (what, b, e)
            # ... and the same tokens at the same frames in the unfused search carry the same terms
            for q in plain_alts[b]:
                if (list(q["tokens"]), list(q["timestamps"])) == (list(a["tokens"]), list(a["timestamps"])):
                    np.testing.assert_allclose(a["token_log_probs"], q["token_log_probs"], atol=cases.YP_TOL, rtol=0)
    print(f"{what}: {len(want)} streams equal the twin, worst score difference {worst:.3g} (bound {cases.score_bound(T, 1, nscale):.3g} and up), "
          f"worst token log-prob difference {worst_yp:.3g} (bound {cases.YP_TOL}), smallest twin gap {g:.3g}")
    return got


@pytest.mark.parametrize("name,beam", sorted(cases.SEEDS))
def test_operator_against_the_twin(tiny, tiny165, lms, name, beam):
    model, ora, enc_of = tiny165 if cases.OPERATOR[name] == "tiny165" else tiny
    base, seed, _ = cases.SEEDS[(name, beam)]
    enc = enc_of(base)
    lm, nlm, _ = lms(name, seed)
    plain = model.beam_search(enc, beam, nbest=8)
    got = check_case(model, ora, enc, beam, lm, nlm, cases.SCALE, f"LM {name} beam {beam}", plain)
    if beam >= 2:
        with fusion(model, lm, cases.SCALE):
            fused = model.beam_search(enc, beam, nbest=cases.NBEST)
        assert [[a["tokens"] for a in al] for al in fused] != [[a["tokens"] for a in al[:cases.NBEST]] for al in plain], "the LM moves nothing"
    assert len(got) == cases.STREAMS


@pytest.mark.parametrize("what", sorted(cases.TOGETHER))
def test_together_with_hotwords_and_an_ngram_lm(tiny, lms, what):
    from k2transducerasr_amd import Hotwords, NgramLm
    model, ora, enc_of = tiny
    base, seed, _ = cases.TOGETHER[what]
    enc = enc_of(base)
    lm, nlm, _ = lms("A", seed)
    ex = cases.together_extras(ora, enc, what)
    plain = model.beam_search(enc, 4, nbest=8)
    try:
        if what == "hotwords":
            model.set_hotwords(Hotwords(ex["phrases"], ex["score"], model.vocab_size))
        else:
            model.set_ngram_lm(NgramLm(ex["entries"], model.vocab_size), ex["scale"])
        check_case(model, ora, enc, 4, lm, nlm, cases.SCALE, f"neural LM + {what}", plain, lm=ex.get("lm"), scale=ex.get("scale", 0.0), graph=ex.get("graph"))
    finally:
        model.set_hotwords(None)
        model.set_ngram_lm(None)


# ---- 3. the switch -------------------------------------------------------------------------------------------------------------------------
def test_switch_behaviour(tiny, lms, tiny_model_path, utts, tmp_path):
    from k2transducerasr_amd import OfflineRecognizer, OnlineRecognizer
    from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model
    model, ora, enc_of = tiny
    enc = enc_of(cases.SEEDS[("A", 4)][0])
    lm, _, _ = lms("A", cases.SEEDS[("A", 4)][1])
    want, wsc = model.beam_search(enc, 4, want_scores=True)
    walts = model.beam_search(enc, 4, nbest=4)

    def plain_again(what):
        p0, h0 = launches()
        s0 = model.rnn_lm_fusion_stats()
        got, gsc = model.beam_search(enc, 4, want_scores=True)
        assert launches() == (p0 + 1, h0) and model.rnn_lm_fusion_stats()["searches"] == s0["searches"], what
        assert got == want and gsc.tobytes() == wsc.tobytes(), what
        alts = model.beam_search(enc, 4, nbest=4)
        for al, wl in zip(alts, walts):
            assert [(a["tokens"], a["timestamps"], np.float32(a["score"]).tobytes(), a["token_log_probs"].tobytes()) for a in al] == \
                   [(a["tokens"], a["timestamps"], np.float32(a["score"]).tobytes(), a["token_log_probs"].tobytes()) for a in wl], what

    try:
        model.set_rnn_lm(lm, cases.SCALE)
        plain_again("LM attached, fusion off")
        model.set_rnn_lm_fusion(True)
        model.set_rnn_lm(lm, 0.0)
        plain_again("fusion on, scale 0")
        model.set_rnn_lm(None)
        plain_again("fusion on, LM cleared")
        model.set_rnn_lm(lm, cases.SCALE)
        p0, h0 = launches()
        s0, c0 = model.rnn_lm_fusion_stats(), model.rnn_lm_stats()["device_calls"]
        fused = model.beam_search(enc, 4)
        s1 = model.rnn_lm_fusion_stats()
        assert launches() == (p0, h0) and s1["searches"] == s0["searches"] + 1 and s1["swept"] > s0["swept"]
        assert model.rnn_lm_stats()["device_calls"] == c0 and fused != want
        model.set_rnn_lm_fusion(False)
        plain_again("fusion switched off again")
    finally:
        model.set_rnn_lm_fusion(False)
        model.set_rnn_lm(None)

    # the recognizer: fused lists are not rescored as well; greedy search and get_result ignore the switch
    def decode(rec):
        ss = [rec.create_offline_stream() for _ in utts]
        for s, u in zip(ss, utts):
            s.add_samples(u)
        res = rec.get_results(ss)
        return res, [s.alternatives() for s in ss]

    rec = OfflineRecognizer(tiny_model_path, 0, "modified_beam_search", 4, nbest=4, rnn_lm=lm, rnn_lm_scale=cases.SCALE, rnn_lm_fusion=True)
    ref = OfflineRecognizer(tiny_model_path, 0, "modified_beam_search", 4, nbest=4)
    try:
        c0 = rec.model.rnn_lm_stats()["device_calls"]
        res, alts = decode(rec)
        res0, alts0 = decode(ref)
        assert rec.model.rnn_lm_stats()["device_calls"] == c0 and all(a["lm_score"] == 0.0 for al in alts for a in al)
        assert res != res0
        B = len(utts)
        for b in range(B):
            assert res[b][0][2 * B:] == alts[b][0]["tokens"] and res[b][1][2 * B:] == alts[b][0]["timestamps"]
        rec.model.set_nbest(1)      # (the single-stream entry refuses a model that keeps alternatives)
        ref.model.set_nbest(1)
        s = rec.create_offline_stream()
        s.add_samples(utts[0])
        s0 = ref.create_offline_stream()
        s0.add_samples(utts[0])
        assert rec.get_result(s) == ref.get_result(s0)
        rec.model.set_decoding_method("greedy_search")
        ref.model.set_decoding_method("greedy_search")
        assert rec.model.offline_greedy_from_samples(utts) == ref.model.offline_greedy_from_samples(utts)
    finally:
        rec.model.close()
        ref.model.close()
    # a streaming model with fusion on runs the unfused search
    sp = str(tmp_path / "s.k2w")
    write_synthetic_model(sp, "zipformer2-streaming-tiny-test")
    outs = []
    for on in (False, True):
        orec = OnlineRecognizer(sp, 0, "modified_beam_search", 4)
        try:
            if on:
                orec.model.set_rnn_lm(lm, 2.0)
                orec.model.set_rnn_lm_fusion(True)
            n0 = orec.model.rnn_lm_fusion_stats()["searches"]
            hs = [orec.create_online_stream() for _ in range(2)]
            for u, h in enumerate(hs):
                h.add_samples(synth_utterance(40 + u, 1.5))
            for _ in range(64):
                dec, _ = orec.get_results(hs)
                if not any(dec):
                    break
            outs.append([(h.tokens, h.timestamps) for h in hs])
            assert orec.model.rnn_lm_fusion_stats()["searches"] == n0
        finally:
            orec.model.close()
    assert outs[0] == outs[1] and sum(len(t) for t, _ in outs[0]) > 0


# ---- 4. idle frames -----------------------------------------------------------------------------------------------------------------------
def test_idle_frames_read_no_weights(tmp_path):
    """the hand-made model of kat_model.py at beam 1: ten frames of blank, token 5, ten frames of blank.  Of the 20 frames that have LM
    launches behind them (the last has none) one appends: its L = 2 layer launches sweep their weights, the other 38 only move state."""
    from k2transducerasr_amd import Model, RnnLm
    from k2transducerasr_amd.synth import write_synthetic_rnn_lm
    from kat_model import frames, write_kat_model
    mp, lp_ = str(tmp_path / "kat.k2w"), str(tmp_path / "lm8.k2w")
    write_kat_model(mp)
    write_synthetic_rnn_lm(lp_, 8, 8, 32, 2, 3)
    m = Model(mp, 0)
    try:
        enc = frames([{0: 3.0}] * 10 + [{5: 3.0}] + [{0: 3.0}] * 10)[None]
        plain = m.beam_search(enc, 1)
        assert plain == [([5], [10])]
        with fusion(m, RnnLm(lp_), 0.5):
            s0 = m.rnn_lm_fusion_stats()
            assert m.beam_search(enc, 1) == plain
            s1 = m.rnn_lm_fusion_stats()
        assert (s1["searches"] - s0["searches"], s1["swept"] - s0["swept"], s1["idle"] - s0["idle"]) == (1, 2, 38)
    finally:
        m.close()


# ---- 5. one wide batch --------------------------------------------------------------------------------------------------------------------
def test_wide_batch(model, oracle_tiny, lms):
    """B = 32 streams of 4 s, beam 4 (128 slots: four row strips per LM launch): localised near-ties are tolerated, at most 4 of 32"""
    w = cases.WIDE
    enc = cases.encode(oracle_tiny, cases.wide_utterances())
    lm, nlm, _ = lms(w["lm"], w["seed"])
    want, wsc, mg, wtr, runs = twin_batch(oracle_tiny, enc, w["beam"], nlm=nlm, nscale=cases.SCALE)
    with fusion(model, lm, cases.SCALE):
        with switches(K2HIP_BEAM_TRACE=1):
            got, gsc = model.beam_search(enc, w["beam"], want_scores=True)
            gtr = model.beam_trace()
    exact = parity.assert_beam_match(got, want, mg, tol=parity.LOGIT_TOL, what="wide fused batch", allow_tie=True, trace_got=gtr, trace_want=wtr)
    worst = max(abs(float(gsc[b]) - runs[b]["lp"]) for b in range(w["B"]) if got[b] == want[b])
    print(f"wide: {exact}/{w['B']} streams exact, worst score difference of the exact ones {worst:.3g}")
    assert w["B"] - exact <= 4
    for b in range(w["B"]):
        if got[b] == want[b]:
            assert abs(float(gsc[b]) - runs[b]["lp"]) <= cases.score_bound(enc.shape[1], len(want[b][0])), (b, float(gsc[b]), runs[b]["lp"])
