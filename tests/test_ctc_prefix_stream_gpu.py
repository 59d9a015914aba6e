"""The streaming CTC prefix beam search on the GPU: prefixes carried across chunks (csrc/ctc_prefix.hip's resume form through the debug op
"ctc_prefix_resume", k2hip_ctc_prefix_beam_search_chunk, and k2hip_online_step on streams set with
k2hip_online_stream_set_ctc_prefix_beam).

The property: after any sequence of chunk calls a stream's live prefixes are those of the offline kernel run once over all frames it has
been given -- BIT FOR BIT: tokens, absolute timestamps, token log-probs, float32 scores, the number of prefixes and their order.  Both
forms run one per-frame source, so nothing here has a tolerance but the comparison with the float64 twin, which keeps the rule of
tests/test_ctc_prefix_gpu.py (exact lists on inputs whose twin gaps clear G = 8 E; scores within 1e-5 relative to max(1, |value|)).
The small-vocabulary rows are required: the V = 37 seeded cases have no fold relation crossing a 16-frame boundary and would pass a carry
that forgets them (tests/test_ctc_prefix_stream.py counts this on the CPU).  Outputs are pre-filled with -7."""
import ctypes as C

import numpy as np
import pytest

import ctc_prefix_cases as cases
import ctc_prefix_stream_cases as scases
from ctc_prefix_stream_twin import HostCarry, Layout
from ctc_prefix_twin import min_gap, prefix_beam_search

pytestmark = pytest.mark.gpu

REL = 1e-5


def rel(got, want):
    return abs(float(got) - want) / max(1.0, abs(want))


@pytest.fixture(scope="module")
def ctc_path(tmp_path_factory):
    from k2transducerasr_amd.synth import write_synthetic_model
    p = str(tmp_path_factory.mktemp("ctcprefixstream") / "ctc_tiny.k2w")
    write_synthetic_model(p, "zipformer2-ctc-tiny-test")
    return p


@pytest.fixture(scope="module")
def hip_ctc(ctc_path):
    from k2transducerasr_amd import Model
    m = Model(ctc_path, 0)
    assert m.vocab_size == 37
    return m


def _debug_op(model, name, ints, bufs, out_from):
    from k2transducerasr_amd import load_library
    L = load_library()
    L.k2hip_debug_op_run.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                     C.c_int32, C.c_uint32]
    n = len(bufs)
    ptrs = (C.c_void_p * n)(*[b.ctypes.data if b is not None else None for b in bufs])
    sizes = (C.c_int64 * n)(*[b.nbytes if b is not None else 0 for b in bufs])
    ia = (C.c_int64 * len(ints))(*ints)
    rc = L.k2hip_debug_op_run(model.handle, name, ia, len(ints), ptrs, sizes, n, sum(1 << k for k in range(out_from, n)))
    assert rc == 0, (rc, L.k2hip_last_error())


def run_offline(model, lp, n_frames, beam, max_tokens):
    """the offline kernel alone through "ctc_prefix_beam", nbest = beam, every output pre-filled with -7"""
    lp = np.ascontiguousarray(lp, np.float32)
    R, Tp, V = lp.shape
    tok = np.full((R, beam, max_tokens), -7, np.int64)
    ts = np.full((R, beam, max_tokens), -7, np.int32)
    yp = np.full((R, beam, max_tokens), -7, np.float32)
    n = np.full((R, beam), -7, np.int32)
    nh = np.full(R, -7, np.int32)
    sc = np.full((R, beam), -7, np.float32)
    flag = np.full(1, -7, np.int32)
    _debug_op(model, b"ctc_prefix_beam", (R, Tp, V, beam, beam, max_tokens), [lp, np.ascontiguousarray(n_frames, np.int32), tok, ts, yp, n, nh, sc, flag], 2)
    assert flag[0] == 0
    return dict(tokens=tok, timestamps=ts, token_log_probs=yp, n_tokens=n, n_hyps=nh, scores=sc)


def run_resume(model, lp, n_frames, beam, in_blocks):
    """the resume form alone through "ctc_prefix_resume": out blocks [B][out_ints] pre-filled with -7, and the status word"""
    lp = np.ascontiguousarray(lp, np.float32)
    B, Tc, V = lp.shape
    L = Layout(beam, Tc)
    inb = np.ascontiguousarray(in_blocks, np.int32)
    assert inb.shape == (B, L.in_ints)
    out = np.full((B, L.out_ints), -7, np.int32)
    status = np.full(1, -7, np.int32)
    _debug_op(model, b"ctc_prefix_resume", (B, Tc, V, beam), [lp, np.ascontiguousarray(n_frames, np.int32), inb, out, status], 3)
    assert status[0] == 0
    return out


def same_as_offline(carry, off, r):
    """a carried stream's slots against row r of an offline result: everything bit for bit"""
    n = len(carry.slots)
    assert off["n_hyps"][r] == n, (r, off["n_hyps"][r], n)
    for i, s in enumerate(carry.slots):
        Ln = len(s["tokens"])
        assert off["n_tokens"][r, i] == Ln, (r, i, off["n_tokens"][r, i], Ln)
        assert off["tokens"][r, i, :Ln].tolist() == list(s["tokens"]), (r, i, off["tokens"][r, i, :Ln].tolist(), s["tokens"])
        assert off["timestamps"][r, i, :Ln].tolist() == list(s["timestamps"]), (r, i, off["timestamps"][r, i, :Ln].tolist(), s["timestamps"])
        assert off["token_log_probs"][r, i, :Ln].view(np.int32).tolist() == list(s["token_log_probs"]), (r, i)
        assert int(off["scores"][r, i].view(np.int32)) == s["tot"], (r, i, off["scores"][r, i], np.int32(s["tot"]).view(np.float32))


def against_twin(carry, want, lp_row):
    """the existing rule: lists exact, token log-probs copies of the input, scores within REL; returns the worst relative difference"""
    hyps = want["hyps"]
    assert len(carry.slots) == len(hyps)
    worst = 0.0
    for s, h in zip(carry.slots, hyps):
        assert list(s["tokens"]) == h["tokens"] and list(s["timestamps"]) == h["timestamps"]
        assert [np.int32(b).view(np.float32) for b in s["token_log_probs"]] == [lp_row[t, v] for t, v in zip(h["timestamps"], h["tokens"])]
        got = float(np.int32(s["tot"]).view(np.float32))
        if h["score"] == -np.inf:
            assert got == -np.inf
        else:
            worst = max(worst, rel(got, h["score"]))
            assert rel(got, h["score"]) <= REL, (got, h["score"])
    return worst


def stream_rows(model, rows, beam, Tc, after_chunk=None):
    """rows: [(lp [T][V], chunk lengths)], one V.  Every row is a stream carried by a HostCarry through the resume kernel, all streams that
    still have frames in one call per step (rows leave the batch as they end), per-row n_frames.  After EVERY step each stream that moved
    equals the offline kernel over its frames so far (one batched offline call per step).  Frames behind n_frames hold ordinary values
    that must not be read.  after_chunk(row index, carry): a hook for further checks."""
    V = rows[0][0].shape[1]
    Tmax = max(lp.shape[0] for lp, _ in rows)
    whole = np.full((len(rows), Tmax, V), 0.25, np.float32)
    for r, (lp, ch) in enumerate(rows):
        assert sum(ch) == lp.shape[0] and max(ch) <= Tc and min(ch) >= 1
        whole[r, : lp.shape[0]] = lp
    carries = [HostCarry(beam) for _ in rows]
    step = 0
    while True:
        active = [r for r, (_, ch) in enumerate(rows) if step < len(ch)]
        if not active:
            break
        lp = np.full((len(active), Tc, V), 0.25, np.float32)
        nf = np.zeros(len(active), np.int32)
        for b, r in enumerate(active):
            n = rows[r][1][step]
            t0 = carries[r].frames
            lp[b, :n] = rows[r][0][t0: t0 + n]
            nf[b] = n
        out = run_resume(model, lp, nf, beam, np.stack([carries[r].fill_in(Tc) for r in active]))
        for b, r in enumerate(active):
            carries[r].apply_out(out[b], Tc, int(nf[b]))
            L = Layout(beam, Tc)
            n = len(carries[r].slots)
            assert np.all(out[b, L.out_org + n: L.out_org + beam] == -7) and np.all(out[b, L.out_ys + n * Tc: L.out_ys + beam * Tc] == -7), (r, step)
        done = np.array([carries[r].frames for r in active], np.int32)
        off = run_offline(model, whole[active], done, beam, Tmax)
        for b, r in enumerate(active):
            same_as_offline(carries[r], off, b)
            if after_chunk:
                after_chunk(r, carries[r])
        step += 1
    for r, (lp, _) in enumerate(rows):
        assert carries[r].frames == lp.shape[0]
    return carries


_twin_cache = {}


def twin(key, lp, beam):
    if (key, beam) not in _twin_cache:
        _twin_cache[(key, beam)] = prefix_beam_search(np.asarray(lp, np.float64), beam)
    return _twin_cache[(key, beam)]


# ---- 1. the kernel alone -------------------------------------------------------------------------------------------------------------
def test_kernel_respelled_row_at_every_split(hip_ctc):
    """V = 3, T = 10, beam 4: the nine two-chunk splits and chunks of 1, 2, 3 as twelve streams of one batch (Tc = 9)"""
    row = cases.respelled_row()
    chunkings = [ch for ch in scases.respelled_chunkings() if max(ch) != 4 or len(ch) == 2]
    assert len(chunkings) == 12
    carries = stream_rows(hip_ctc, [(row, ch) for ch in chunkings], cases.RESPELLED_BEAM, 9)
    want = twin("respelled", row, cases.RESPELLED_BEAM)
    assert want["respelled_folds"] >= 1 and min_gap(want) >= cases.G_SMALL
    for c in carries:
        against_twin(c, want, row)
        toks = [s["tokens"] for s in c.slots]
        assert len(set(toks)) == len(toks) == cases.RESPELLED_BEAM        # prefix identity is sequence identity


@pytest.mark.parametrize("beam", scases.SMALL4_BEAMS)
def test_kernel_small_vocabulary_case(hip_ctc, beam):
    """V = 4, T = 48 in chunks of 16, and in chunks of 7 with a ragged last chunk of 6; at the chunk ends 16 / 32 / 48 also the float64 twin"""
    lp = scases.small4_row()
    worst = [0.0]

    def at_end(r, carry):
        if carry.frames in (16, 32, 48):
            want = twin(("small4", carry.frames), lp[: carry.frames], beam)
            assert min_gap(want) >= 8 * scases.SMALL4_E[beam]
            worst[0] = max(worst[0], against_twin(carry, want, lp))

    stream_rows(hip_ctc, [(lp, [16, 16, 16])], beam, 16, at_end)
    carries = stream_rows(hip_ctc, [(lp, [7] * 6 + [6])], beam, 7)
    against_twin(carries[0], twin(("small4", 48), lp, beam), lp)
    print(f"small4 beam {beam}: worst relative score difference against the float64 twin {worst[0]:.3g} (bound {REL:g})")


@pytest.mark.parametrize("beam", cases.RAGGED_BEAMS)
def test_kernel_ragged_rows_leave_the_batch_as_they_end(hip_ctc, beam):
    """V = 37, frames 1, 2, 7, 70, 70, 70 (a row with -inf cells, a row that is -inf everywhere) in chunks of 16 with per-row n_frames"""
    lp, nf = cases.ragged_rows()
    rows = [(lp[r, : nf[r]], scases.uniform(int(nf[r]), scases.CHUNK)) for r in range(len(nf))]
    carries = stream_rows(hip_ctc, rows, beam, scases.CHUNK)
    worst = 0.0
    for r in range(len(cases.RAGGED_SEEDS)):
        want = twin(("ragged", r), lp[r, : nf[r]], beam)
        assert min_gap(want) >= cases.G_RAGGED
        worst = max(worst, against_twin(carries[r], want, lp[r]))
    c = carries[cases.RAGGED_ALL_INF_ROW]                       # -inf everywhere: the empty prefix, score -inf, carried through every chunk
    assert len(c.slots) == 1 and c.slots[0]["tokens"] == () and np.int32(c.slots[0]["tot"]).view(np.float32) == -np.inf
    print(f"ragged beam {beam}: worst relative score difference against the float64 twin {worst:.3g} (bound {REL:g})")


def test_kernel_wide_and_long_rows(hip_ctc):
    """V = 600 (several columns per thread) and T = 300 (long histories: 19 chunks), beam 4, chunks of 16"""
    for name, lp, G in (("wide", cases.wide_row(), cases.G_WIDE), ("long", cases.long_row(), cases.G_LONG)):
        carries = stream_rows(hip_ctc, [(lp, scases.uniform(lp.shape[0], scases.CHUNK))], 4, scases.CHUNK)
        want = twin(name, lp, 4)
        assert min_gap(want) >= G
        print(f"{name}: worst relative score difference against the float64 twin {against_twin(carries[0], want, lp):.3g} (bound {REL:g})")


# ---- 2. the operator entry -------------------------------------------------------------------------------------------------------------
def same_alternatives(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert g["tokens"] == w["tokens"] and g["timestamps"] == w["timestamps"], (g, w)
        assert np.array_equal(np.asarray(g["token_log_probs"], np.float32).view(np.int32), np.asarray(w["token_log_probs"], np.float32).view(np.int32))
        assert np.float32(g["score"]).view(np.int32) == np.float32(w["score"]).view(np.int32), (g["score"], w["score"])


def chunk_streams(model, streams, rows, Tc):
    """rows [B][T][V] (one T) through Model.ctc_prefix_beam_search_chunk in chunks of Tc, the last one ragged"""
    T = rows.shape[1]
    for t0 in range(0, T, Tc):
        n = min(Tc, T - t0)
        lp = np.full((rows.shape[0], Tc, rows.shape[2]), 0.25, np.float32)
        lp[:, :n] = rows[:, t0: t0 + n]
        model.ctc_prefix_beam_search_chunk(streams, lp, None if n == Tc else np.full(rows.shape[0], n, np.int32))


def test_operator_entry_small_vocabularies_embedded(hip_ctc):
    """the V = 3 and V = 4 rows inside the model's V = 37 (columns above at -inf), nbest = beam = 8, against Model.ctc_prefix_beam_search"""
    for row, Tc in ((cases.respelled_row(), 3), (scases.small4_row(), 16)):
        lp = scases.embed(row, 37)[None]
        s = hip_ctc.create_ctc_prefix_stream(8, 8)
        try:
            assert s.num_frames == 0 and s.tokens == [] and s.score == 0.0 and len(s.alternatives()) == 1
            chunk_streams(hip_ctc, [s], lp, Tc)
            want = hip_ctc.ctc_prefix_beam_search(lp, beam=8, nbest=8)[0]
            assert s.num_frames == row.shape[0] and len(want) > 1
            same_alternatives(s.alternatives(), want)
            assert s.tokens == want[0]["tokens"] and s.timestamps == want[0]["timestamps"]
            assert np.array_equal(s.token_log_probs(), want[0]["token_log_probs"])
            s.reset()
            assert s.num_frames == 0 and s.tokens == [] and s.score == 0.0
        finally:
            s.close()


def test_operator_entry_fixture_batch(hip_ctc, utts):
    """the tiny CTC model's own log_probs of the fixture batch (T' = 35) cut into chunks of 16, every stream in every call"""
    feats = [hip_ctc.fbank(u) for u in utts]
    lp = hip_ctc.encoder_proj(hip_ctc.pad_sequence(feats).reshape(len(utts), -1, 80))
    streams = [hip_ctc.create_ctc_prefix_stream(8, 8) for _ in utts]
    try:
        chunk_streams(hip_ctc, streams, lp, scases.CHUNK)
        want = hip_ctc.ctc_prefix_beam_search(lp, beam=8, nbest=8)
        for s, w in zip(streams, want):
            same_alternatives(s.alternatives(), w)
            assert s.num_frames == lp.shape[1]
    finally:
        for s in streams:
            s.close()


# ---- 3. the argument rules -------------------------------------------------------------------------------------------------------------
def test_argument_rules_leave_every_stream_as_it_was(hip_ctc, ctc_path, hip_tiny):
    from k2transducerasr_amd import K2HipError, Model
    for bad in ((0, 1), (9, 1), (4, 0), (4, 5)):
        with pytest.raises(K2HipError) as e:
            hip_ctc.create_ctc_prefix_stream(*bad)
        assert e.value.code == -1, (bad, e.value.code, str(e.value))
    with pytest.raises(K2HipError) as e:
        hip_tiny.create_ctc_prefix_stream(4, 1)
    assert e.value.code == -6, (e.value.code, str(e.value))
    other_model = Model(ctc_path, 0)
    a, b, wide, foreign = (hip_ctc.create_ctc_prefix_stream(4, 4), hip_ctc.create_ctc_prefix_stream(4, 2), hip_ctc.create_ctc_prefix_stream(8, 8),
                           other_model.create_ctc_prefix_stream(4, 4))
    try:
        lp, _ = cases.ragged_rows()
        chunk = np.ascontiguousarray(lp[2:4, :16])
        hip_ctc.ctc_prefix_beam_search_chunk([a, b], chunk)
        snap = lambda s: (s.tokens, s.timestamps, s.num_frames, np.float32(s.score).view(np.int32), [x["tokens"] for x in s.alternatives()])
        before = [snap(s) for s in (a, b, wide, foreign)]
        assert before[0][2] == 16 and before[2][2] == 0
        refused = [([a, wide], chunk, None), ([a, a], chunk, None), ([a, foreign], chunk, None), ([a, b], chunk, [16, 0]), ([a, b], chunk, [17, 16]),
                   ([a, b], chunk, [16, -1])]
        for streams, x, nf in refused:
            with pytest.raises(K2HipError) as e:
                hip_ctc.ctc_prefix_beam_search_chunk(streams, x, nf)
            assert e.value.code == -1, (nf, e.value.code, str(e.value))
            assert [snap(s) for s in (a, b, wide, foreign)] == before
        with pytest.raises(K2HipError) as e:                      # a transducer model: UNSUPPORTED
            hip_tiny._chk(hip_tiny._L.k2hip_ctc_prefix_beam_search_chunk(hip_tiny.handle, (C.c_void_p * 2)(a._h.value, b._h.value), 2,
                                                                         chunk.ctypes.data_as(C.POINTER(C.c_float)), 16, None))
        assert e.value.code == -6, (e.value.code, str(e.value))
        assert [snap(s) for s in (a, b, wide, foreign)] == before
        hip_ctc.ctc_prefix_beam_search_chunk([a, b], np.ascontiguousarray(lp[2:4, 16:32]))      # and the streams go on as if nothing had happened
        want = hip_ctc.ctc_prefix_beam_search(np.ascontiguousarray(lp[2:4, :32]), beam=4, nbest=4)
        same_alternatives(a.alternatives(), want[0])
        same_alternatives(b.alternatives(), want[1][:2])
    finally:
        for s in (a, b, wide, foreign):
            s.close()
        other_model.close()


# ---- 4. the recognizer level -------------------------------------------------------------------------------------------------------------
def test_recognizer_level_against_the_search_over_all_frames_so_far(tmp_path):
    """zipformer2-ctc-streaming-tiny-test, three streams of 2 s (one joins a tick later) with ctc_prefix_beam = 4, nbest = 2, fed with
    features.  Route B feeds the same features through the online encoder entry in the same batch composition and collects each stream's
    log-probs; after every tick each stream equals Model.ctc_prefix_beam_search over route B's frames so far, bit for bit (the token
    log-probs are copies of the inputs: the exact comparison is the detector for a difference between the routes).  A stream without the
    setting decodes as before; a list mixing settings fails with INVALID, streams unchanged."""
    from k2transducerasr_amd import K2HipError, OnlineProj, OnlineRecognizer
    from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model
    p = str(tmp_path / "ctc_streaming.k2w")
    write_synthetic_model(p, "zipformer2-ctc-streaming-tiny-test")
    rec, plain, proj = OnlineRecognizer(p), OnlineRecognizer(p), OnlineProj(p)
    streams, states, others = [], [], []
    try:
        Tch, shift, Tp = rec.chunk_length, rec.shift_length, rec.frames_per_chunk
        feats = [np.ascontiguousarray(rec.model.fbank(synth_utterance(u, 2.0)), np.float32) for u in range(3)]
        streams = [rec.create_online_stream(ctc_prefix_beam=4, nbest=2) for _ in range(3)]
        greedy, greedy_ref = rec.create_online_stream(), plain.create_online_stream()
        others = [greedy, greedy_ref]
        states = [proj.get_encoder_init_states() for _ in range(3)]
        pos, lps, fed = [0, 0, 0], [[], [], []], [False, False, False]
        assert streams[0].score == 0.0 and len(streams[0].alternatives()) == 1 and streams[0].tokens == [0, 0]
        with pytest.raises(K2HipError) as e:
            greedy_ref.set_ctc_prefix_beam(4, 5)
        assert e.value.code == -1
        greedy.add_features(feats[0])
        greedy_ref.add_features(feats[0])
        ticks = 0
        while True:
            for i in range(3):
                if not fed[i] and (i < 2 or ticks >= 1):             # stream 2 joins a tick later
                    streams[i].add_features(feats[i])
                    fed[i] = True
            ready = [i for i in range(3) if fed[i] and feats[i].shape[0] - pos[i] >= Tch]
            if not ready:
                break
            if ticks == 0:                                           # a list mixing settings: INVALID, nothing moves
                before = (streams[0].speech_length, streams[0].tokens, greedy.speech_length, greedy.tokens)
                with pytest.raises(K2HipError) as e:
                    rec.get_results([streams[0], greedy])
                assert e.value.code == -1 and "ctc_prefix_beam" in str(e.value)
                assert (streams[0].speech_length, streams[0].tokens, greedy.speech_length, greedy.tokens) == before
            lens_before = [len(s.tokens) for s in streams]
            dec, nnew = rec.get_results(streams)
            assert [i for i in range(3) if dec[i]] == ready, (ticks, dec, ready)
            out = proj.encoder_proj(np.stack([feats[i][pos[i]: pos[i] + Tch] for i in ready]), [states[i] for i in ready])
            assert out.shape == (len(ready), Tp, rec.model.vocab_size)
            for b, i in enumerate(ready):
                lps[i].append(out[b])
                pos[i] += shift
                sofar = np.concatenate(lps[i])[None]
                want = rec.model.ctc_prefix_beam_search(sofar, beam=4, nbest=2)[0]
                s = streams[i]
                assert s.tokens == [0, 0] + want[0]["tokens"] and s.timestamps == want[0]["timestamps"], (ticks, i)
                assert nnew[i] == len(s.tokens) - lens_before[i]
                assert np.array_equal(s.token_log_probs().view(np.int32), np.asarray(want[0]["token_log_probs"], np.float32).view(np.int32)), (ticks, i)
                same_alternatives(s.alternatives(), want)
                assert np.float32(s.score).view(np.int32) == np.float32(want[0]["score"]).view(np.int32)
            # the stream without the setting, in the same recogniser, against the same features in a recogniser that has no set stream
            d1, n1 = rec.get_results([greedy])
            d2, n2 = plain.get_results([greedy_ref])
            assert (d1, n1, greedy.tokens, greedy.timestamps) == (d2, n2, greedy_ref.tokens, greedy_ref.timestamps)
            ticks += 1
        assert ticks >= 3 and all(len(x) >= 2 for x in lps)
        with pytest.raises(K2HipError) as e:                         # the setting is fixed once the stream has searched
            streams[0].set_ctc_prefix_beam(8, 1)
        assert e.value.code == -1 and "reset" in str(e.value)
        streams[0].reset()
        assert streams[0].tokens == [0, 0] and streams[0].score == 0.0
        streams[0].set_ctc_prefix_beam(0)
    finally:
        for st in states:                                            # (streams and states go before the models they belong to)
            proj.free_states(st)
        for s in streams + others:
            s.close()
        rec.model.close()
        plain.model.close()
        proj.model.close()


def test_a_transducer_stream_refuses_the_setting(tmp_path):
    from k2transducerasr_amd import K2HipError, OnlineRecognizer
    from k2transducerasr_amd.synth import write_synthetic_model
    p = str(tmp_path / "streaming.k2w")
    write_synthetic_model(p, "zipformer2-streaming-tiny-test")
    rec = OnlineRecognizer(p)
    s = rec.create_online_stream()
    try:
        with pytest.raises(K2HipError) as e:
            s.set_ctc_prefix_beam(4, 1)
        assert e.value.code == -6, (e.value.code, str(e.value))
        with pytest.raises(K2HipError) as e:
            rec.create_online_stream(ctc_prefix_beam=4)
        assert e.value.code == -6
    finally:
        s.close()
        rec.model.close()
