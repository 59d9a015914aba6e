"""CTC prefix beam search with N-best on the GPU (csrc/ctc_prefix.hip through the debug op "ctc_prefix_beam",
k2hip_ctc_prefix_beam_search and the batch entries under k2hip_set_decoding_method("ctc_prefix_beam_search")), against the float64 twin
(tests/ctc_prefix_twin.py).

Bounds (none of them taken from what the engine gives):
  * tokens, timestamps, n_hyps and the order of the entries are exact on inputs whose every twin gap is >= G; G = 8 E with E the measured
    float32-against-float64 difference of the twin's gaps, per group of like shapes (tests/ctc_prefix_cases.py has the table: E from
    5.1e-7 to 7.53e-5, G from 4.1e-6 to 6.1e-4; tests/test_ctc_prefix.py re-measures E and checks every input on the CPU);
  * token log-probs are exact: they are copies of inputs;
  * scores are within 1e-5 relative to max(1, |value|), the bound tests/test_ctc_align_gpu.py uses for the same kind of sum.
Outputs are pre-filled with -7, so what the kernel does not write shows.

Worst differences seen on an MI355X are recorded in DESIGN.md "CTC prefix beam search"."""
import ctypes as C

import numpy as np
import pytest

import ctc_prefix_cases as cases
from ctc_prefix_twin import brute_force, min_gap, prefix_beam_search

pytestmark = pytest.mark.gpu

REL = 1e-5


def rel(got, want):
    return abs(float(got) - want) / max(1.0, abs(want))


@pytest.fixture(scope="module")
def ctc_path(tmp_path_factory):
    from k2transducerasr_amd.synth import write_synthetic_model
    p = str(tmp_path_factory.mktemp("ctcprefix") / "ctc_tiny.k2w")
    write_synthetic_model(p, "zipformer2-ctc-tiny-test")
    return p


@pytest.fixture(scope="module")
def hip_ctc(ctc_path):
    from k2transducerasr_amd import Model
    m = Model(ctc_path, 0)
    assert m.vocab_size == 37
    return m


@pytest.fixture(scope="module")
def device_log_probs(hip_ctc, utts):
    """log_probs [B, T', V] of the padded fixture batch from the existing encoder entry, on the engine's own features"""
    feats = [hip_ctc.fbank(u) for u in utts]
    return hip_ctc.encoder_proj(hip_ctc.pad_sequence(feats).reshape(len(utts), -1, 80))


def run_op(model, lp, n_frames, beam, nbest, max_tokens):
    """the kernel alone through "ctc_prefix_beam", every output pre-filled with -7"""
    from k2transducerasr_amd import load_library
    L = load_library()
    L.k2hip_debug_op_run.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                     C.c_int32, C.c_uint32]
    lp = np.ascontiguousarray(lp, np.float32)
    R, Tp, V = lp.shape
    tok = np.full((R, nbest, max_tokens), -7, np.int64)
    ts = np.full((R, nbest, max_tokens), -7, np.int32)
    yp = np.full((R, nbest, max_tokens), -7, np.float32)
    n = np.full((R, nbest), -7, np.int32)
    nh = np.full(R, -7, np.int32)
    sc = np.full((R, nbest), -7, np.float32)
    flag = np.full(1, -7, np.int32)
    nf = None if n_frames is None else np.ascontiguousarray(n_frames, np.int32)
    bufs = [lp, nf, tok, ts, yp, n, nh, sc, flag]
    ptrs = (C.c_void_p * 9)(*[b.ctypes.data if b is not None else None for b in bufs])
    sizes = (C.c_int64 * 9)(*[b.nbytes if b is not None else 0 for b in bufs])
    ia = (C.c_int64 * 6)(R, Tp, V, beam, nbest, max_tokens)
    rc = L.k2hip_debug_op_run(model.handle, b"ctc_prefix_beam", ia, 6, ptrs, sizes, 9, sum(1 << k for k in range(2, 9)))
    assert rc == 0, (rc, L.k2hip_last_error())
    return dict(tokens=tok, timestamps=ts, token_log_probs=yp, n_tokens=n, n_hyps=nh, scores=sc, flag=int(flag[0]))


_twin_cache = {}


def twin(key, lp, beam):
    """the float64 twin, computed once per (case, beam) and shared"""
    if (key, beam) not in _twin_cache:
        _twin_cache[(key, beam)] = prefix_beam_search(np.asarray(lp, np.float64), beam)
    return _twin_cache[(key, beam)]


def check_row(out, r, lp_row, want, nbest):
    """row r of a kernel result against a twin run: everything exact but the scores; returns the worst relative score difference"""
    hyps = want["hyps"]
    nh = min(nbest, len(hyps))
    assert out["n_hyps"][r] == nh, (r, out["n_hyps"][r], nh)
    worst = 0.0
    for i in range(nbest):
        if i >= nh:
            assert out["n_tokens"][r, i] == -7 and out["scores"][r, i] == -7 and np.all(out["tokens"][r, i] == -7), (r, i)
            continue
        h = hyps[i]
        L = len(h["tokens"])
        assert out["n_tokens"][r, i] == L, (r, i, out["n_tokens"][r, i], L)
        assert out["tokens"][r, i, :L].tolist() == h["tokens"], (r, i, out["tokens"][r, i, :L].tolist(), h["tokens"])
        assert out["timestamps"][r, i, :L].tolist() == h["timestamps"], (r, i)
        assert np.array_equal(out["token_log_probs"][r, i, :L], np.asarray([lp_row[t, v] for t, v in zip(h["timestamps"], h["tokens"])], np.float32)), (r, i)
        assert np.all(out["tokens"][r, i, L:] == -7) and np.all(out["timestamps"][r, i, L:] == -7) and np.all(out["token_log_probs"][r, i, L:] == -7)
        if h["score"] == -np.inf:
            assert out["scores"][r, i] == -np.inf
        else:
            worst = max(worst, rel(out["scores"][r, i], h["score"]))
            assert rel(out["scores"][r, i], h["score"]) <= REL, (r, i, out["scores"][r, i], h["score"])
    return worst


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------
def test_kernel_exhaustive_small_vocabulary(hip_ctc):
    """V = 3, beam 8, nbest 8, rows T = 1 and T = 2: nothing is pruned, T = 2 has its 5 prefixes, every score is the brute-force sum"""
    lp, nf = cases.exhaustive_rows()
    out = run_op(hip_ctc, lp, nf, 8, 8, 2)
    assert out["flag"] == 0
    for r, T in enumerate(nf):
        check_row(out, r, lp[r], twin(("ex", r), lp[r, :T], 8), 8)
        bf = brute_force(lp[r, :T])
        assert out["n_hyps"][r] == len(bf) == (3, 5)[r]
        for i in range(len(bf)):
            key = tuple(out["tokens"][r, i, : out["n_tokens"][r, i]].tolist())
            assert rel(out["scores"][r, i], bf[key][0]) <= REL, (r, i, key)


def test_kernel_hand_built_rows(hip_ctc):
    """the tie rows, the `a a` rows and the re-spelled row at its own beam, as in the CPU tests"""
    lp, beam = cases.TIE_LOWER_ID
    out = run_op(hip_ctc, lp[None], None, beam, beam, 1)
    assert out["tokens"][0, :, 0].tolist() == [1, 2] and out["scores"][0].tolist() == [-0.5, -0.5]
    lp, beam = cases.TIE_STAY
    out = run_op(hip_ctc, lp[None], None, beam, beam, 1)
    assert out["n_hyps"][0] == 1 and out["n_tokens"][0, 0] == 0 and out["scores"][0, 0] == -0.5 and out["tokens"][0, 0, 0] == -7
    lp, beam = cases.TIE_LOWER_SLOT
    out = run_op(hip_ctc, lp[None], None, beam, beam, 2)
    assert out["n_tokens"][0].tolist() == [1, 2] and out["tokens"][0, 0, 0] == 2 and out["tokens"][0, 1].tolist() == [1, 2]
    assert out["timestamps"][0, 0, 0] == 1 and out["timestamps"][0, 1].tolist() == [0, 1] and out["scores"][0].tolist() == [-1.25, -1.25]
    out = run_op(hip_ctc, cases.PEAKY_A_BLANK_A[None], None, 4, 1, 3)
    assert out["n_tokens"][0, 0] == 2 and out["tokens"][0, 0, :2].tolist() == [1, 1] and out["timestamps"][0, 0, :2].tolist() == [0, 2]
    out = run_op(hip_ctc, cases.PEAKY_A_A_A[None], None, 4, 1, 3)
    assert out["n_tokens"][0, 0] == 1 and out["tokens"][0, 0, 0] == 1 and out["timestamps"][0, 0, 0] == 0 and out["token_log_probs"][0, 0, 0] == 0
    lp, beam = cases.respelled_row(), cases.RESPELLED_BEAM
    want = twin("respelled", lp, beam)
    assert want["respelled_folds"] >= 1
    out = run_op(hip_ctc, lp[None], None, beam, beam, cases.RESPELLED_T)
    check_row(out, 0, lp, want, beam)
    got = [tuple(out["tokens"][0, i, : out["n_tokens"][0, i]].tolist()) for i in range(out["n_hyps"][0])]
    assert len(set(got)) == len(got) == beam, got       # prefix identity is sequence identity: no two equal prefixes


@pytest.mark.parametrize("beam", cases.RAGGED_BEAMS)
def test_kernel_ragged(hip_ctc, beam):
    """V = 37, one call with n_frames = 1, 2, 7, 70, a row with 2 % -inf cells and a row that is -inf everywhere; nbest = beam"""
    lp, nf = cases.ragged_rows()
    out = run_op(hip_ctc, lp, nf, beam, beam, int(nf.max()))
    assert out["flag"] == 0
    worst = 0.0
    for r in range(len(cases.RAGGED_SEEDS)):
        want = twin(("ragged", r), lp[r, : nf[r]], beam)
        assert min_gap(want) >= cases.G_RAGGED
        worst = max(worst, check_row(out, r, lp[r], want, beam))
    r = cases.RAGGED_ALL_INF_ROW       # -inf everywhere: the empty prefix, score -inf, nothing out of range
    assert out["n_hyps"][r] == 1 and out["n_tokens"][r, 0] == 0 and out["scores"][r, 0] == -np.inf
    assert np.all(out["tokens"][r] == -7) and np.all(out["timestamps"][r] == -7) and np.all(out["n_tokens"][r, 1:] == -7)
    print(f"ragged beam {beam}: worst relative score difference {worst:.3g} (bound {REL:g})")


@pytest.mark.parametrize("beam", cases.WIDE_BEAMS)
def test_kernel_wide_vocabulary(hip_ctc, beam):
    """V = 600: columns above 256 and above 512, several per thread"""
    lp = cases.wide_row()
    want = twin("wide", lp, beam)
    assert min_gap(want) >= cases.G_WIDE
    assert any(v > 512 for h in want["hyps"] for v in h["tokens"]) and any(256 < v <= 512 for h in want["hyps"] for v in h["tokens"])
    out = run_op(hip_ctc, lp[None], None, beam, beam, cases.WIDE_T)
    print(f"wide beam {beam}: worst relative score difference {check_row(out, 0, lp, want, beam):.3g} (bound {REL:g})")


def test_kernel_long_histories(hip_ctc):
    """V = 37, T = 300, beam 4, nbest 4, max_tokens = 300"""
    lp = cases.long_row()
    want = twin("long", lp, cases.LONG_BEAM)
    assert min_gap(want) >= cases.G_LONG and len(want["hyps"][0]["tokens"]) > 100
    out = run_op(hip_ctc, lp[None], None, cases.LONG_BEAM, 4, cases.LONG_T)
    assert out["flag"] == 0
    print(f"long: worst relative score difference {check_row(out, 0, lp, want, 4):.3g} (bound {REL:g})")


# ---- 2. independence ---------------------------------------------------------------------------------------------------------------
def test_a_rows_result_does_not_depend_on_the_other_rows(hip_ctc):
    lp, nf = cases.ragged_rows()
    batch = run_op(hip_ctc, lp, nf, 4, 4, 70)
    for r in (2, 3):
        alone = run_op(hip_ctc, lp[r: r + 1], nf[r: r + 1], 4, 4, 70)
        for k in ("tokens", "timestamps", "token_log_probs", "n_tokens", "n_hyps", "scores"):
            assert np.array_equal(alone[k][0], batch[k][r]), (r, k)
    other = lp.copy()
    other[[0, 1, 2, 4, 5]] = other[[0, 1, 2, 4, 5]][:, ::-1]          # every other row changes
    again = run_op(hip_ctc, other, nf, 4, 4, 70)
    for k in ("tokens", "timestamps", "token_log_probs", "n_tokens", "scores"):
        assert np.array_equal(again[k][3], batch[k][3]), k


# ---- 3. against the alignment on the device ------------------------------------------------------------------------------------------
def test_scores_against_the_alignment_on_the_device(hip_ctc):
    """every alternative of the ragged case (beam 8) back through k2hip_ctc_align with stream_of, in one call: score <= total_logp; the
    exhaustive T = 2 row (its three columns inside V = 37, the rest -inf) is not pruned, so there the two are equal"""
    lp, nf = cases.ragged_rows()
    ex, _ = cases.exhaustive_rows()
    row = np.full((1, lp.shape[1], 37), -np.inf, np.float32)
    row[0, :2, :3] = ex[1]
    lp = np.concatenate([lp, row])
    nf = np.concatenate([nf, [2]]).astype(np.int32)
    ex_row = lp.shape[0] - 1
    alts = hip_ctc.ctc_prefix_beam_search(lp, beam=8, n_frames=nf, nbest=8)
    assert len(alts[ex_row]) == 5
    targets, stream_of, scores = [], [], []
    for r, lst in enumerate(alts):
        for a in lst:
            targets.append(np.asarray(a["tokens"], np.int64))
            stream_of.append(r)
            scores.append(a["score"])
    got = hip_ctc.ctc_align(lp, targets, n_frames=nf, stream_of=stream_of)
    worst = 0.0
    for h, (r, s) in enumerate(zip(stream_of, scores)):
        total = got[h]["total_logp"]
        if total == -np.inf:
            assert s == -np.inf, (h, r)
            continue
        assert s <= total + REL * max(1.0, abs(total)), (h, r, s, total)
        if r == ex_row:
            worst = max(worst, rel(s, total))
            assert rel(s, total) <= REL, (h, s, total)
    print(f"exhaustive row, score against k2hip_ctc_align's total: worst relative difference {worst:.3g} (bound {REL:g})")


# ---- 4. capacity ---------------------------------------------------------------------------------------------------------------------
def test_capacity(hip_ctc):
    from k2transducerasr_amd import K2HipError
    lp, nf = cases.ragged_rows()
    best = hip_ctc.ctc_prefix_beam_search(lp, beam=4, n_frames=nf)
    longest = max(len(tok) for tok, _ in best)
    assert longest >= 2
    with pytest.raises(K2HipError) as e:
        hip_ctc.ctc_prefix_beam_search(lp, beam=4, n_frames=nf, max_tokens=longest - 1)
    assert e.value.code == -5, (e.value.code, str(e.value))
    assert hip_ctc.ctc_prefix_beam_search(lp, beam=4, n_frames=nf, max_tokens=longest) == best
    for bad in (dict(beam=0), dict(beam=9), dict(beam=4, nbest=5), dict(beam=4, n_frames=[1, 2, 7, 70, 70, 71])):
        with pytest.raises(K2HipError) as e:
            hip_ctc.ctc_prefix_beam_search(lp, **bad)
        assert e.value.code == -1, (bad, e.value.code, str(e.value))


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------
def test_end_to_end_against_the_twin(hip_ctc, ctc_path, utts, device_log_probs):
    from k2transducerasr_amd import OfflineRecognizer
    B, Tp, V = device_log_probs.shape
    hip_ctc.set_decoding_method("ctc_prefix_beam_search", 4)
    try:
        got = hip_ctc.offline_greedy_from_samples(utts)
        scores = hip_ctc.last_scores(B)
    finally:
        hip_ctc.set_decoding_method("greedy_search")
    want = [twin(("e2e", b), device_log_probs[b], 4) for b in range(B)]
    strict = [b for b in range(B) if min_gap(want[b]) >= cases.G_FIXTURE]
    assert 4 * (B - len(strict)) <= B, strict
    worst = 0.0
    for b in strict:
        h = want[b]["hyps"][0]
        assert (list(got[b][0]), list(got[b][1])) == (h["tokens"], h["timestamps"]), b
        worst = max(worst, rel(scores[b], h["score"]))
        assert rel(scores[b], h["score"]) <= REL, (b, scores[b], h["score"])
    print(f"end to end: {len(strict)} of {B} streams strict, worst relative score difference {worst:.3g} (bound {REL:g})")
    op = hip_ctc.ctc_prefix_beam_search(device_log_probs, beam=4, nbest=4)
    rec = OfflineRecognizer(ctc_path, decoding_method="ctc_prefix_beam_search", beam=4, nbest=4)
    try:
        streams = [rec.create_offline_stream() for _ in utts]
        for s, u in zip(streams, utts):
            s.add_samples(u)
        res = rec.get_results(streams)
        for b in strict:
            alts = streams[b].alternatives()
            assert len(alts) == len(op[b]) == 4, b
            for a, o in zip(alts, op[b]):
                assert a["tokens"] == o["tokens"] and a["timestamps"] == o["timestamps"], b       # (frame indexes, no FrameOffset)
                assert rel(a["score"], o["score"]) <= REL and np.allclose(a["token_log_probs"], o["token_log_probs"], rtol=0, atol=1e-4)
            assert list(res[b][0])[-len(alts[0]["tokens"]):] == alts[0]["tokens"] or not alts[0]["tokens"]
            assert np.array_equal(streams[b].token_log_probs(), alts[0]["token_log_probs"])
    finally:
        rec.model.close()


# ---- 6. peaky input ------------------------------------------------------------------------------------------------------------------
def test_peaky_input_gives_the_greedy_result(hip_ctc):
    """log_probs whose row maximum leads by 20: at beam 1 the prefix search returns k2hip_ctc_greedy's tokens and timestamps.  At beam 4
    and 8 the tokens are the same, but a timestamp may lie EARLIER than the collapse's: the 36 extensions of a frame tie 20 below its
    maximum, the lowest ids fill the spare slots, and when such a prefix becomes the best one a frame later (the peak's extension folds
    into it) it keeps its own timestamp -- the first-inserted rule of the semantics (the float64 twin shows it on rows 0 and 2 of this
    input).  Which of the tied prefixes sits in a spare slot depends on the last bit of sums near -20 k, so this input has no gap G and
    the beams above 1 are not held to the twin: their tokens are the collapse's and no timestamp is later than the collapse's."""
    rng = np.random.default_rng(5)
    R, T, V = 3, 40, 37
    lab = rng.integers(0, 6, size=(R, T))          # blanks, repeats and a few tokens
    lp = np.full((R, T, V), -20 - np.log1p((V - 1) * np.exp(-20.0)), np.float32)
    np.put_along_axis(lp, lab[:, :, None], np.float32(-np.log1p((V - 1) * np.exp(-20.0))), axis=2)
    greedy, _ = hip_ctc.ctc_greedy(lp)
    greedy = [(list(a), list(b)) for a, b in greedy]
    assert any(len(t) > 3 for t, _ in greedy)
    assert [(list(a), list(b)) for a, b in hip_ctc.ctc_prefix_beam_search(lp, beam=1)] == greedy
    for beam in (4, 8):
        got = hip_ctc.ctc_prefix_beam_search(lp, beam=beam)
        for r in range(R):
            assert list(got[r][0]) == greedy[r][0] and all(a <= b for a, b in zip(got[r][1], greedy[r][1])), (beam, r)
            assert all(a < b for a, b in zip(got[r][1], got[r][1][1:]))


# ---- 7. nothing else moved -------------------------------------------------------------------------------------------------------------
def test_the_other_methods_of_a_ctc_model_are_untouched(hip_ctc, utts):
    from k2transducerasr_amd import K2HipError
    before = hip_ctc.offline_greedy_from_samples(utts)
    hip_ctc.set_decoding_method("ctc_prefix_beam_search", 4)
    hip_ctc.set_nbest(2)
    under = hip_ctc.offline_greedy_from_samples(utts)
    assert len(under) == len(before)
    hip_ctc.set_decoding_method("greedy_search")
    after = hip_ctc.offline_greedy_from_samples(utts)
    with pytest.raises(K2HipError) as e:               # leaving the method reset the list to 1; asking again fails as before
        hip_ctc.set_nbest(2)
    assert e.value.code == -6
    hip_ctc.set_decoding_method("modified_beam_search", 4)
    try:
        mbs = hip_ctc.offline_greedy_from_samples(utts)
        with pytest.raises(K2HipError) as e:
            hip_ctc.set_nbest(2)
        assert e.value.code == -6
    finally:
        hip_ctc.set_decoding_method("greedy_search")
    assert before == after == mbs


def test_a_transducer_handle_refuses_both_entries(hip_tiny):
    from k2transducerasr_amd import K2HipError
    with pytest.raises(K2HipError) as e:
        hip_tiny.ctc_prefix_beam_search(np.zeros((1, 4, hip_tiny.vocab_size), np.float32))
    assert e.value.code == -6, (e.value.code, str(e.value))
    with pytest.raises(K2HipError) as e:
        hip_tiny.set_decoding_method("ctc_prefix_beam_search", 4)
    assert e.value.code == -6, (e.value.code, str(e.value))


def test_streaming_step_refuses_the_method_without_changing_a_stream(tmp_path):
    from k2transducerasr_amd import K2HipError, OnlineRecognizer
    from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model
    p = str(tmp_path / "ctc_streaming.k2w")
    write_synthetic_model(p, "zipformer2-ctc-streaming-tiny-test")
    rec = OnlineRecognizer(p)
    try:
        s = rec.create_online_stream()
        s.add_samples(synth_utterance(0, 2.0))
        rec.model.set_decoding_method("ctc_prefix_beam_search", 4)
        before = (s.speech_length, list(s.tokens), list(s.timestamps), s.processed_len)
        assert before[0] > 0
        with pytest.raises(K2HipError) as e:
            rec.get_results([s])
        assert e.value.code == -1 and "ctc_prefix_beam_search" in str(e.value), (e.value.code, str(e.value))
        assert (s.speech_length, list(s.tokens), list(s.timestamps), s.processed_len) == before
        rec.model.set_decoding_method("greedy_search")
        dec, _ = rec.get_results([s])                   # and the stream decodes as if nothing had happened
        assert dec == [1] and s.speech_length < before[0]
    finally:
        rec.model.close()
