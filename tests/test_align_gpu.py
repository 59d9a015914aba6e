"""Forced alignment and full-sum scoring on the GPU (csrc/align.hip through k2hip_transducer_align, k2hip_offline_align_from_samples
and the two debug ops), against the float64 twin (tests/align_twin.py).

Bounds (none of them taken from what the engine gives):
  * a cell (stay / emit, a log-softmax value): CELL_TOL = 2 * LOGIT_TOL / 10 = 2e-4, the bound tests/test_nbest_gpu.py derives for a
    token log-prob (the logit's own error plus that of the log-sum-exp);
  * total_logp / best_logp: T' * CELL_TOL -- a path's sum moves by at most T' cell errors, and a logsumexp or a maximum over paths moves
    by at most what every path moves;
  * the DP on planes whose values are multiples of 0.25: sums along a path are exact in float32, so best, the timestamps and the token
    log-probs are exact; total is held to 1e-5 relative (float32 rounding of exp / log1p in the forward sums);
  * the beam search's score is a pruned sum of alignments of its tokens, so score <= total_logp + SCORE_TOL (2e-3, the bound
    tests/test_beam_gpu.py holds beam scores to);
  * the fused route scores the DEVICE encoder's frames: against Model.align on the engine's own encoder_proj output the timestamps are
    equal and the scores agree within the relative bound tests/test_online_beam_gpu.py uses for the fused step.

Worst differences seen on an MI355X are recorded in DESIGN.md "Forced alignment and full-sum scoring"."""
import ctypes as C

import numpy as np
import pytest

import parity
from align_twin import align_twin, lattice_dp, path_score

pytestmark = pytest.mark.gpu

CELL_TOL = 2 * parity.LOGIT_TOL / 10
SCORE_TOL = 2e-3


def fused_score_ok(got, want):   # tests/test_online_beam_gpu.py
    return abs(got - want) <= SCORE_TOL + 1e-2 * abs(want)


def targets_for(V, lens, seed):
    """fixed seeded sequences over [3, V), plus id 1 once (in the first non-empty one)"""
    rng = np.random.default_rng(seed)
    tg = [rng.integers(3, V, size=n).astype(np.int64) for n in lens]
    for t in tg:
        if t.size:
            t[t.size // 2] = 1
            break
    return tg


def debug_op(model, name, iargs, bufs, outs):
    from k2transducerasr_amd import load_library
    L = load_library()
    L.k2hip_debug_op_run.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                     C.c_int32, C.c_uint32]
    n = len(bufs)
    ptrs = (C.c_void_p * n)(*[b.ctypes.data if b is not None and b.size else None for b in bufs])
    sizes = (C.c_int64 * n)(*[b.nbytes if b is not None else 0 for b in bufs])
    ia = (C.c_int64 * len(iargs))(*[int(v) for v in iargs])
    rc = L.k2hip_debug_op_run(model.handle, name.encode(), ia, len(iargs), ptrs, sizes, n, sum(1 << k for k in outs))
    assert rc == 0, (name, rc, L.k2hip_last_error())


def plane_offsets(n_frames, lens):
    off, o = [], 0
    for T, U in zip(n_frames, lens):
        off.append(o)
        o += int(T) * (int(U) + 1)
    return off, o


def band_mask(T, U):
    t, u = np.meshgrid(np.arange(T), np.arange(U + 1), indexing="ij")
    return (u <= t) & (U - u <= T - t)


@pytest.fixture(scope="module")
def enc_tiny(oracle_tiny, utts):
    f = [oracle_tiny.fbank(u) for u in utts]
    return oracle_tiny.encoder(oracle_tiny.pad_sequence(f).reshape(len(utts), -1, 80))


@pytest.fixture(scope="module")
def wide_pair(tmp_path_factory):
    """the tiny preset with a vocabulary of 3000: several column slabs, no all-contexts decoder table (as test_parity_gpu.py)"""
    from k2transducerasr_amd import Model
    from k2transducerasr_amd.synth import write_synthetic_model
    from oracle import Oracle
    p = str(tmp_path_factory.mktemp("align") / "wide.k2w")
    write_synthetic_model(p, "zipformer2-tiny-test", blank_bias=2.4, meta_overrides={"vocab_size": "3000"})
    return Model(p, 0), Oracle(p)


# (T, U) of the three streams of one call: strip edges (1, 33, 35, 70 frames against strips of 32), the single-path lattice (U = T),
# U = 0, and U + 1 past one wave (66)
CELL_CALLS = ([(1, 0), (33, 5), (70, 65)], [(1, 1), (35, 0), (35, 35)])


@pytest.mark.parametrize("which", ["tiny", "conformer", "wide"])
def test_cells_against_the_twin(which, request):
    if which == "tiny":
        hip, ora = request.getfixturevalue("hip_tiny"), request.getfixturevalue("oracle_tiny")
        assert hip.vocab_size == 37
    elif which == "conformer":
        hip, ora = request.getfixturevalue("hip_conformer"), request.getfixturevalue("oracle_conformer")
        assert hip.vocab_size == 41
    else:
        hip, ora = request.getfixturevalue("wide_pair")
        assert hip.vocab_size == 3000
    V, J = hip.vocab_size, hip.joiner_dim
    worst = 0.0
    for call, shapes in enumerate(CELL_CALLS):
        B, Tp = len(shapes), max(T for T, _ in shapes)
        nf = np.array([T for T, _ in shapes], np.int32)
        lens = np.array([U for _, U in shapes], np.int32)
        tg = targets_for(V, lens, 11 + call)
        enc = np.random.default_rng(5 + call).standard_normal((B, Tp, J)).astype(np.float32)
        off, total = plane_offsets(nf, lens)
        stay = np.full(total, np.nan, np.float32)
        emit = np.full(total, np.nan, np.float32)
        ids = np.concatenate(tg).astype(np.int64)
        debug_op(hip, "lattice_logprobs", [B, Tp], [enc, nf, ids, lens, stay, emit], outs=(4, 5))
        twin = align_twin(ora, enc, tg, nf)
        for b, (T, U) in enumerate(shapes):
            band = band_mask(T, U)
            gs = stay[off[b]: off[b] + T * (U + 1)].reshape(T, U + 1)
            ge = emit[off[b]: off[b] + T * (U + 1)].reshape(T, U + 1)
            ds = np.abs(gs[band] - twin[b]["stay"][band]).max()
            eb = band & (np.arange(U + 1)[None, :] < U)
            de = np.abs(ge[eb] - twin[b]["emit"][eb]).max() if eb.any() else 0.0
            assert np.all(ge[band & ~eb] == -np.inf)
            worst = max(worst, float(ds), float(de))
            assert ds <= CELL_TOL and de <= CELL_TOL, (which, call, b, T, U, float(ds), float(de))
    print(f"lattice_logprobs {which}: worst cell difference {worst:.3g} (bound {CELL_TOL:g})")


def quarter_planes(rng, T, U, inf_share=0.0):
    stay = -0.25 * rng.integers(0, 13, size=(T, U + 1)).astype(np.float32)
    emit = -0.25 * rng.integers(0, 13, size=(T, U + 1)).astype(np.float32)
    if inf_share:
        stay[rng.random(stay.shape) < inf_share] = -np.inf
        emit[rng.random(emit.shape) < inf_share] = -np.inf
    emit[:, U] = -np.inf
    return stay, emit


def test_dp_known_answers(hip_tiny):
    """lattice_dp on hand-built planes of multiples of 0.25: the tie case decided by the emit-wins rule by hand, the rest against the
    float64 twin (exact on such values) -- U = 0, U = T, T = 1, -inf cells, U + 1 past one wave and past the workgroup"""
    rng = np.random.default_rng(3)
    # T = 2, U = 1: stay(0,0) + emit(1,0) = -0.5 - 0.5 and emit(0,0) + stay(1,1) = -0.75 - 0.25 tie at -1.0 exactly; the emit
    # predecessor wins at (2,1): the token sits on frame 1 with log-prob -0.5; total = -1 + log 2
    tie = (np.array([[-0.5, -0.75], [-0.25, -0.25]], np.float32), np.array([[-0.75, -np.inf], [-0.5, -np.inf]], np.float32))
    cases = [tie, quarter_planes(rng, 1, 0), quarter_planes(rng, 1, 1), quarter_planes(rng, 9, 0), quarter_planes(rng, 7, 7),
             quarter_planes(rng, 40, 12, 0.1), quarter_planes(rng, 90, 70), quarter_planes(rng, 300, 280), quarter_planes(rng, 300, 260, 0.02)]
    B = len(cases)
    nf = np.array([s.shape[0] for s, _ in cases], np.int32)
    lens = np.array([s.shape[1] - 1 for s, _ in cases], np.int32)
    Tp, mt = int(nf.max()), int(lens.max())
    stay = np.concatenate([s.reshape(-1) for s, _ in cases]).astype(np.float32)
    emit = np.concatenate([e.reshape(-1) for _, e in cases]).astype(np.float32)
    ts = np.full((B, mt), -7, np.int32)
    lp = np.full((B, mt), -7, np.float32)
    sc = np.full((B, 2), -7, np.float32)
    debug_op(hip_tiny, "lattice_dp", [B, Tp, mt], [nf, lens, stay, emit, ts, lp, sc], outs=(4, 5, 6))
    assert sc[0, 1] == -1.0 and ts[0, 0] == 1 and lp[0, 0] == -0.5 and abs(sc[0, 0] - (-1.0 + np.log(2.0))) <= 1e-5
    worst = 0.0
    for b, (s, e) in enumerate(cases):
        want = lattice_dp(s.astype(np.float64), e.astype(np.float64))
        U = int(lens[b])
        assert sc[b, 1] == np.float32(want["best"]), (b, sc[b, 1], want["best"])
        assert ts[b, :U].tolist() == want["timestamps"], b
        assert np.array_equal(lp[b, :U], want["token_log_probs"].astype(np.float32)), b
        if want["total"] == -np.inf:
            assert sc[b, 0] == -np.inf
        else:
            rel = abs(float(sc[b, 0]) - want["total"]) / max(1.0, abs(want["total"]))
            worst = max(worst, rel)
            assert rel <= 1e-5, (b, sc[b, 0], want["total"])
        if U == int(nf[b]):
            assert sc[b, 0] == sc[b, 1]
    print(f"lattice_dp: worst relative difference of total {worst:.3g} (bound 1e-5)")


def test_end_to_end_against_the_twin(hip_tiny, oracle_tiny, enc_tiny):
    B, Tp, _ = enc_tiny.shape
    nf = np.array([Tp, Tp - 3, 17, Tp, 9][:B], np.int32)
    lens = [12, 5, 17, 0, 3][:B]
    tg = targets_for(hip_tiny.vocab_size, lens, 21)
    got = hip_tiny.align(enc_tiny, tg, nf)
    twin = align_twin(oracle_tiny, enc_tiny, tg, nf)
    bound = Tp * CELL_TOL
    worst = dict(total=0.0, best=0.0, path=0.0, token=0.0)
    for b in range(B):
        g, w = got[b], twin[b]
        T, U = int(nf[b]), lens[b]
        worst["total"] = max(worst["total"], abs(g["total_logp"] - w["total"]))
        worst["best"] = max(worst["best"], abs(g["best_logp"] - w["best"]))
        assert abs(g["total_logp"] - w["total"]) <= bound and abs(g["best_logp"] - w["best"]) <= bound, (b, g, w["total"], w["best"])
        ts = g["timestamps"]
        assert len(ts) == U and all(y > x for x, y in zip(ts, ts[1:])) and all(0 <= t < T for t in ts), (b, ts)
        rescored = path_score(w["stay"], w["emit"], ts)     # the engine's path under the twin's float64 cells: no stream is excused
        worst["path"] = max(worst["path"], abs(rescored - w["best"]))
        assert abs(rescored - w["best"]) <= bound, (b, rescored, w["best"])
        yp = g["token_log_probs"]
        assert np.all(yp <= 0)
        if U:
            d = float(np.abs(yp - w["emit"][ts, np.arange(U)]).max())
            worst["token"] = max(worst["token"], d)
            assert d <= CELL_TOL, (b, d)
        assert g["best_logp"] <= g["total_logp"]
        if U == T:
            assert g["best_logp"] == g["total_logp"] and ts == list(range(T))
    print("Model.align against the twin, worst differences: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) +
          f" (bounds {bound:.3g}, token {CELL_TOL:g})")


@pytest.mark.parametrize("beam", [1, 4, 8])
def test_beam_score_is_below_the_full_sum(hip_tiny, enc_tiny, beam):
    """the modified beam search's score is the pruned sum of the alignments of its tokens that the beam kept"""
    res, sc = hip_tiny.beam_search(enc_tiny, beam, want_scores=True)
    tg = [np.array(t, np.int64) for t, _ in res]
    assert sum(t.size for t in tg) > 0
    got = hip_tiny.align(enc_tiny, tg)
    for b, g in enumerate(got):
        assert sc[b] <= g["total_logp"] + SCORE_TOL, (beam, b, sc[b], g["total_logp"])
        assert g["best_logp"] <= g["total_logp"]
    # U = T: one path, best == total bit for bit
    T = 6
    one = hip_tiny.align(enc_tiny[:, :T], targets_for(hip_tiny.vocab_size, [T] * enc_tiny.shape[0], 31))
    for g in one:
        assert np.float32(g["best_logp"]).tobytes() == np.float32(g["total_logp"]).tobytes() and g["timestamps"] == list(range(T))


def test_fused_route_equals_align_on_the_engines_frames(hip_tiny, utts):
    feats = [hip_tiny.fbank(u) for u in utts]
    enc = hip_tiny.encoder_proj(hip_tiny.pad_sequence(feats).reshape(len(utts), -1, 80))
    tg = targets_for(hip_tiny.vocab_size, [7, 4, 0, 11, 2][: len(utts)], 41)
    want = hip_tiny.align(enc, tg)
    got = hip_tiny.align_samples(utts, tg)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g["timestamps"] == w["timestamps"], b
        assert fused_score_ok(g["total_logp"], w["total_logp"]) and fused_score_ok(g["best_logp"], w["best_logp"]), (b, g, w)
        assert np.all(np.abs(g["token_log_probs"] - w["token_log_probs"]) <= SCORE_TOL + 1e-2 * np.abs(w["token_log_probs"]))
    from k2transducerasr_amd import OfflineRecognizer   # the recognizer's method is the same call
    assert OfflineRecognizer.align is not None


def test_errors_leave_the_handle_usable(hip_tiny, enc_tiny, utts, tmp_path):
    from k2transducerasr_amd import K2HipError, Model
    from k2transducerasr_amd.synth import write_synthetic_model
    B, Tp, _ = enc_tiny.shape
    V = hip_tiny.vocab_size
    good = targets_for(V, [3] * B, 51)
    ref = hip_tiny.align(enc_tiny, good)

    def still_fine():
        again = hip_tiny.align(enc_tiny, good)
        assert [(a["timestamps"], a["total_logp"], a["best_logp"]) for a in again] == [(a["timestamps"], a["total_logp"], a["best_logp"]) for a in ref]

    def refused(code, fn, word):
        with pytest.raises(K2HipError) as e:
            fn()
        assert e.value.code == code and word in str(e.value), (e.value.code, str(e.value))
        still_fine()

    long = [np.full(Tp + 1, 5, np.int64)] + good[1:]
    refused(-1, lambda: hip_tiny.align(enc_tiny, long), "stream 0")                       # U > T
    refused(-1, lambda: hip_tiny.align(enc_tiny, good, np.array([2] + [Tp] * (B - 1), np.int32)), "stream 0")
    for bad, word in ((0, "blank"), (2, "unk"), (V, "vocabulary"), (-1, "vocabulary")):
        tg = [t.copy() for t in good]
        tg[1][1] = bad
        refused(-1, lambda tg=tg: hip_tiny.align(enc_tiny, tg), word)
        refused(-1, lambda tg=tg: hip_tiny.align_samples(utts, tg), word)
    refused(-5, lambda: hip_tiny.align(enc_tiny, good, max_tokens=2), "max_tokens")      # lens[b] > max_tokens
    refused(-5, lambda: hip_tiny.align_samples(utts, good, max_tokens=2), "max_tokens")
    p = str(tmp_path / "ctc.k2w")
    write_synthetic_model(p, "zipformer2-ctc-tiny-test")
    ctc = Model(p, 0)
    try:
        with pytest.raises(K2HipError) as e:
            ctc.align(np.zeros((1, 4, ctc.vocab_size), np.float32), [np.array([3], np.int64)])
        assert e.value.code == -6 and "CTC" in str(e.value)
        with pytest.raises(K2HipError) as e:
            ctc.align_samples(utts[:1], [np.array([3], np.int64)])
        assert e.value.code == -6 and "CTC" in str(e.value)
    finally:
        ctc.close()
    still_fine()


def test_align_changes_no_search(hip_tiny, enc_tiny):
    """a greedy call and a beam-4 call give identical tokens, timestamps and scores before and after an align call on the same handle"""
    greedy0 = hip_tiny.greedy_batch(enc_tiny)
    beam0, sc0 = hip_tiny.beam_search(enc_tiny, 4, want_scores=True)
    hip_tiny.align(enc_tiny, targets_for(hip_tiny.vocab_size, [4] * enc_tiny.shape[0], 61))
    assert hip_tiny.greedy_batch(enc_tiny) == greedy0
    beam1, sc1 = hip_tiny.beam_search(enc_tiny, 4, want_scores=True)
    assert beam1 == beam0 and np.array_equal(sc0, sc1)


def test_fused_align_changes_no_fused_search(hip_tiny, utts):
    """the fused greedy and beam-4 results (tokens, timestamps, scores) are identical before and after fused align calls on the same handle,
    one that runs and one that is refused: what the fused route runs behind the encoder is named by the call, not left behind by one"""
    from k2transducerasr_amd import K2HipError

    def fused():
        greedy = hip_tiny.offline_greedy_from_samples(utts)
        hip_tiny.set_decoding_method("modified_beam_search", 4)
        try:
            beam = hip_tiny.offline_greedy_from_samples(utts)
            sc = hip_tiny.last_scores(len(utts)).copy()
        finally:
            hip_tiny.set_decoding_method("greedy_search")
        return greedy, beam, sc

    greedy0, beam0, sc0 = fused()
    assert sum(len(t) for t, _ in greedy0) > 0 and sum(len(t) for t, _ in beam0) > 0
    tg = targets_for(hip_tiny.vocab_size, [7, 4, 0, 11, 2][: len(utts)], 71)
    got = hip_tiny.align_samples(utts, tg)
    assert [len(g["timestamps"]) for g in got] == [len(t) for t in tg]
    with pytest.raises(K2HipError) as e:
        hip_tiny.align_samples(utts, tg, max_tokens=2)
    assert e.value.code == -5 and "max_tokens" in str(e.value), (e.value.code, str(e.value))
    greedy1, beam1, sc1 = fused()
    assert greedy1 == greedy0 and beam1 == beam0 and np.array_equal(sc0, sc1)
