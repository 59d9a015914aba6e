"""Half-precision LM weights in the fused searches on the device (k2hip_set_rnn_lm_fusion_precision; csrc/rnn_lm_fuse_f16.hip):
k_nlm_advance_f16 alone against float64 over f16-rounded operands, the offline fused search against the half twin
(tests/rnn_lm_half_cases.py), the streaming search against the engine's own offline search bit for bit, and the switch."""
import contextlib

import numpy as np
import pytest

import parity
import rnn_lm_cases as lmc
import rnn_lm_fusion_cases as oc
import rnn_lm_half_cases as cases
from rnn_lm_fusion_twin import twin_batch
from test_rnn_lm_fusion_gpu import lms, model, parent_maps, run_op, tiny, tiny165   # noqa: F401 (fixtures)
from test_rnn_lm_stream_fusion_gpu import snapshot

pytestmark = pytest.mark.gpu
f32, f16 = np.float32, np.float16


def relay_f16(w_ih, w_hh):
    """kernels.h RnnLmDev::wcat_h restated: [W_ih | zeros up to a multiple of 32 | W_hh] along k, rounded to f16; panel jb =
    [Kc / 32][j][hh][32 columns][e] with k = 32 q + 16 hh + 8 j + e, its column c the gate c // 8 of hidden column 8 jb + c % 8"""
    H, I = w_hh.shape[1], w_ih.shape[1]
    Ip = (I + 31) // 32 * 32
    cat = np.zeros((4 * H, Ip + H), f16)
    cat[:, :I] = w_ih.astype(f16)
    cat[:, Ip:] = w_hh.astype(f16)
    p = cat.reshape(4, H // 8, 8, (Ip + H) // 32, 2, 2, 8)   # gate, block, column of the block, q, hh, j, e
    return np.ascontiguousarray(p.transpose(1, 3, 5, 4, 0, 2, 6)).reshape(-1)


@contextlib.contextmanager
def half_fusion(model, lm, scale, half=True, streaming=False):
    model.set_rnn_lm_fusion_precision(half)
    model.set_rnn_lm(lm, scale)
    model.set_rnn_lm_fusion(True)
    model.set_rnn_lm_stream_fusion(streaming)
    try:
        yield
    finally:
        model.set_rnn_lm_fusion(False)
        model.set_rnn_lm_stream_fusion(False)
        model.set_rnn_lm(None)
        model.set_rnn_lm_fusion_precision(False)


@pytest.mark.parametrize("E,H", [(32, 32), (20, 32), (64, 96)])   # (20: input columns padded up to 32)
def test_nlm_advance_f16_against_float64(model, E, H):
    """rows 1 (one strip), 5 (ragged), 33 (two strips), 130 (every wave finishes a strip; a second round), 300 (a second row block) under
    three parent maps, x from an embedding and from rows, live in {-1, 0} at 33 rows.  Reference: float64 over w, x and h rounded to f16
    first; bias, c and the cell in float64.  f16 x f16 products are exact in float32, so only the accumulation differs and the tolerance is
    test_nlm_advance_against_float64's, 4 K 2^-24 sqrt(K) + 2e-6 with K = E + H.  The operands nobody may read are NaN.  Rows that did
    not append, and every row under live == 0, are bit-equal to the parent's state."""
    rng = np.random.default_rng(100 * E + H)
    K, V = E + H, 9
    w_ih = rng.uniform(-1, 1, size=(4 * H, E)).astype(f32) / f32(np.sqrt(K))
    w_hh = rng.uniform(-1, 1, size=(4 * H, H)).astype(f32) / f32(np.sqrt(K))
    bias = rng.uniform(-1, 1, size=4 * H).astype(f32)
    panels = relay_f16(w_ih, w_hh)
    r64 = lambda a: a.astype(f16).astype(np.float64)   # noqa: E731
    tol = 4 * K * 2.0 ** -24 * np.sqrt(K) + 2e-6
    sig = lambda v: 1 / (1 + np.exp(-v))   # noqa: E731
    worst = 0.0
    for M in (1, 5, 33, 130, 300):
        maps = parent_maps(M, rng)
        for name in ("identity", "one parent", "keep and append"):
            par, app = maps[name]
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
                for live in ((-1, 0) if M == 33 else (-1,)):
                    ho, co = np.full((M, H), -7.0, f32), np.full((M, H), -7.0, f32)
                    flag, work = np.zeros(1, np.int32), np.zeros(2, np.int64)
                    run_op(model, "nlm_advance_f16", [M, E, H, use_emb, V, live], [panels, bias, x, hp, cp, ho, co, par, tok, flag, work],
                           (1 << 5) | (1 << 6) | (1 << 10))
                    what = (M, name, use_emb, live)
                    assert work.tolist() == ([0, 1] if live == 0 else [1, 0]), what
                    on = app & (live != 0)
                    g = r64(xin.astype(f32)) @ r64(w_ih).T + bias + r64(hp[par]) @ r64(w_hh).T
                    wc = sig(g[:, H: 2 * H]) * cp[par] + sig(g[:, :H]) * np.tanh(g[:, 2 * H: 3 * H])
                    wh = sig(g[:, 3 * H:]) * np.tanh(wc)
                    if on.any():
                        err = max(np.abs(co[on] - wc[on]).max(), np.abs(ho[on] - wh[on]).max())
                        worst = max(worst, float(err))
                        assert err <= tol, (what, err, tol)
                    assert np.array_equal(ho[~on].view(np.uint32), hp[par][~on].view(np.uint32)), what
                    assert np.array_equal(co[~on].view(np.uint32), cp[par][~on].view(np.uint32)), what
    print(f"nlm_advance_f16 E = {E}, H = {H}: worst error {worst:.3g}, tolerance {tol:.3g}")


@pytest.mark.parametrize("name,beam", sorted(cases.SEEDS))
def test_operator_against_the_half_twin(tiny, tiny165, lms, name, beam):
    """tokens, timestamps and the number and order of alternatives equal the half twin's with nothing excused; scores within
    rnn_lm_half_cases.score_bound (acceptance and the gap are test_rnn_lm_half.py's, on the CPU)"""
    model, ora, enc_of = tiny165 if oc.OPERATOR[name] == "tiny165" else tiny
    base, seed, _ = cases.SEEDS[(name, beam)]
    enc = enc_of(base)
    lm, _, tw = lms(name, seed)
    want, _, mg, _, runs = twin_batch(ora, enc, beam, nlm=cases.HalfFusionLm(tw), nscale=cases.SCALE, nbest=cases.NBEST)
    with half_fusion(model, lm, cases.SCALE):
        got, gsc = model.beam_search(enc, beam, want_scores=True)
        alts = model.beam_search(enc, beam, nbest=cases.NBEST)
    what = f"half LM {name} beam {beam}"
    assert len(got) == oc.STREAMS and parity.assert_beam_match(got, want, mg, what=what, allow_tie=False) == len(want)
    worst, T = 0.0, enc.shape[1]
    for b, r in enumerate(runs):
        assert len(alts[b]) == len(r["alts"]), (what, b)
        pairs = [(float(gsc[b]), r["lp"], len(r["ys"]))]
        for a, w in zip(alts[b], r["alts"]):
            assert (list(a["tokens"]), list(a["timestamps"])) == (list(w["tokens"]), list(w["timestamps"])), (what, b)
            pairs.append((a["score"], w["score"], len(w["tokens"])))
        for g, w, n in pairs:
            worst = max(worst, abs(g - w))
            assert abs(g - w) <= cases.score_bound(T, n), (what, b, g, w, cases.score_bound(T, n))
    print(f"{what}: worst score difference {worst:.3g} (bound {cases.score_bound(T, 1):.3g} and up)")


def test_streaming_equals_offline_half(tiny, lms):
    """chunkings 1, 3 and whole: after every call tokens, timestamps, alternatives and the bits of every score equal the engine's own
    offline fused f16 search over the same prefix"""
    from k2transducerasr_amd import BeamStream
    model, _, enc_of = tiny
    name, beam = cases.STREAMING
    base, seed, _ = cases.SEEDS[(name, beam)]
    enc = enc_of(base)
    lm = lms(name, seed)[0]
    B, T = enc.shape[0], enc.shape[1]
    model.set_decoding_method("modified_beam_search", beam)
    model.set_nbest(cases.NBEST)
    try:
        with half_fusion(model, lm, cases.SCALE, streaming=True):
            off = {n: (model.beam_search(enc[:, :n], beam, want_scores=True), model.beam_search(enc[:, :n], beam, nbest=cases.NBEST)) for n in range(1, T + 1)}
            for step in (1, 3, T):
                ss = [BeamStream(model, beam) for _ in range(B)]
                try:
                    for n in range(0, T, step):
                        m = min(T, n + step)
                        BeamStream.search_chunk(ss, enc[:, n:m])
                        (res, sc), alts = off[m]
                        for b, s in enumerate(ss):
                            tokens, ts, score, got = snapshot(s)
                            assert (tokens, ts) == (res[b][0], res[b][1]) and score == f32(sc[b]).tobytes(), (step, m, b)
                            assert [a[:3] for a in got] == [(a["tokens"], a["timestamps"], f32(a["score"]).tobytes()) for a in alts[b]], (step, m, b)
                finally:
                    for s in ss:
                        s.close()
    finally:
        model.set_nbest(1)
        model.set_decoding_method("greedy_search")


def test_precision_switch(tiny, lms, tmp_path):
    from k2transducerasr_amd import BeamStream, K2HipError, RnnLm
    from k2transducerasr_amd.synth import rnn_lm_state_dict, write_rnn_lm
    model, _, enc_of = tiny
    base, seed, _ = cases.SEEDS[("A", 4)]
    enc = enc_of(base)
    lm = lms("A", seed)[0]

    def fused(half):
        """the fused search's results with the switch set to `half` (None: never touched)"""
        if half is not None:
            model.set_rnn_lm_fusion_precision(half)
        model.set_rnn_lm(lm, cases.SCALE)
        model.set_rnn_lm_fusion(True)
        try:
            alts = model.beam_search(enc, 4, nbest=cases.NBEST)
            return [[(a["tokens"], a["timestamps"], f32(a["score"]).tobytes()) for a in al] for al in alts]
        finally:
            model.set_rnn_lm_fusion(False)
            model.set_rnn_lm(None)

    try:
        # (a) the switch at 0 gives the bits of a model whose switch was never touched; f16 moves at least one score
        untouched = fused(None)
        h16 = fused(True)
        assert fused(False) == untouched
        assert [[a[2] for a in al] for al in h16] != [[a[2] for a in al] for al in untouched]
        # (b) a stream keeps the precision of its first chunk
        model.set_rnn_lm(lm, cases.SCALE)
        model.set_rnn_lm_stream_fusion(True)
        s = BeamStream(model, 4)
        try:
            BeamStream.search_chunk([s], enc[:1, :7])
            snap = snapshot(s)
            model.set_rnn_lm_fusion_precision(True)
            with pytest.raises(K2HipError) as e:
                BeamStream.search_chunk([s], enc[:1, 7:14])
            assert e.value.code == -1 and "reset the stream first" in str(e.value) and snapshot(s) == snap
            s.reset()
            BeamStream.search_chunk([s], enc[:1, :7])
            assert len(s.tokens) == len(snap[0])
        finally:
            s.close()
            model.set_rnn_lm_stream_fusion(False)
        # (c) a weight that is not finite in f16: refused by the first fused search under f16, decoded under float32
        V, E, H, L, _ = lmc.LMS["A"]
        sd = rnn_lm_state_dict(V, E, H, L, 0, False)
        sd["rnn.weight_hh_l0"][3, 5] = 1e6
        p = str(tmp_path / "big.k2w")
        write_rnn_lm(p, sd, L, 1, 1, False)
        model.set_rnn_lm(RnnLm(p), cases.SCALE)
        model.set_rnn_lm_fusion(True)
        with pytest.raises(K2HipError) as e:
            model.beam_search(enc, 4)
        assert e.value.code == -1 and "half precision" in str(e.value)
        model.set_rnn_lm_fusion_precision(False)
        assert len(model.beam_search(enc, 4)) == oc.STREAMS
    finally:
        model.set_rnn_lm_fusion(False)
        model.set_rnn_lm_stream_fusion(False)
        model.set_rnn_lm(None)
        model.set_rnn_lm_fusion_precision(False)
