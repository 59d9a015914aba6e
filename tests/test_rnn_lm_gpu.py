"""Neural LM rescoring on the device (csrc/rnn_lm.hip, rnn_lm_engine.cpp): the kernels alone through k2hip_debug_op_run, the scoring
operator against torch's own LSTM in float64 (tests/rnn_lm_twin.py) within the measured bound (tests/rnn_lm_cases.py), the recognizer's
re-ordered N-best lists, and the paths that must not notice the LM."""
import ctypes as C

import numpy as np
import pytest

import rnn_lm_cases as cases
from rnn_lm_twin import Twin, rescored_order

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lms(tmp_path_factory):
    """name -> (RnnLm, Twin)"""
    from k2transducerasr_amd import RnnLm
    from k2transducerasr_amd.synth import write_synthetic_rnn_lm
    d = tmp_path_factory.mktemp("rnn_lm")
    out = {}
    for name, (V, E, H, L, seed) in cases.LMS.items():
        p = str(d / f"{name}.k2w")
        sd = write_synthetic_rnn_lm(p, V, E, H, L, seed)
        out[name] = (RnnLm(p), Twin(sd, L))
    return out


@pytest.fixture(scope="module")
def model(tiny_model_path):
    from k2transducerasr_amd import Model
    m = Model(tiny_model_path, 0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def model165(tmp_path_factory):
    """the tiny model with LM C's vocabulary (k2hip_set_rnn_lm checks vocab_size against the model)"""
    from k2transducerasr_amd import Model
    from k2transducerasr_amd.synth import write_synthetic_model
    p = str(tmp_path_factory.mktemp("models") / "tiny165.k2w")
    write_synthetic_model(p, "zipformer2-tiny-test", meta_overrides={"vocab_size": str(cases.LMS["C"][0])})
    m = Model(p, 0)
    yield m
    m.close()


def run_op(model, op, ints, bufs, out_mask):
    L = model._L
    L.k2hip_debug_op_run.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                     C.c_int32, C.c_uint32]
    ia = (C.c_int64 * len(ints))(*ints)
    ptrs = (C.c_void_p * len(bufs))(*[b.ctypes.data for b in bufs])
    sizes = (C.c_int64 * len(bufs))(*[b.nbytes for b in bufs])
    rc = L.k2hip_debug_op_run(model.handle, op.encode(), ia, len(ints), ptrs, sizes, len(bufs), out_mask)
    assert rc == 0, L.k2hip_last_error()


# ---- 1. the kernels alone --------------------------------------------------------------------------------------------------------------
def test_embed_kernel_bit_for_bit(model):
    rng = np.random.default_rng(1)
    for R, V, E in ((1, 5, 4), (70, 37, 64), (257, 165, 36)):
        emb = rng.standard_normal((V, E)).astype(np.float32)
        ids = rng.integers(0, V, size=R).astype(np.int32)
        ids[-1] = V - 1
        x0 = np.full((R, E), np.nan, np.float32)
        run_op(model, "rnn_lm_embed", [R, E], [emb, ids, x0], 1 << 2)
        assert np.array_equal(x0.view(np.uint32), emb[ids].view(np.uint32)), (R, V, E)


def step_f64(h, w_hh, gx, c, first):
    H = c.shape[1]
    g = gx.astype(np.float64) + (0 if first else h.astype(np.float64) @ w_hh.astype(np.float64).T)
    sig = lambda v: 1 / (1 + np.exp(-v))   # noqa: E731
    cn = sig(g[:, H: 2 * H]) * c + sig(g[:, :H]) * np.tanh(g[:, 2 * H: 3 * H])
    return cn, sig(g[:, 3 * H:]) * np.tanh(cn)


@pytest.mark.parametrize("H", [32, 96, 288])   # one column slice; three; more than one LDS chunk of k (256) with a ragged second chunk
def test_step_kernel_one_step(model, H):
    """one step from random h, c, GX at a in {1, 31, 32, 33, 70}: the a active rows against float64, rows beyond a and the c of inactive
    rows untouched; the operands of inactive rows are NaN.  Tolerance: the recurrent product sums H float32 products, so its error is at
    most H 2^-24 sum |h| |w| <= H 2^-24 sqrt(H) here (|h| <= 1, |w| <= 1 / sqrt(H)); sigmoid and tanh have slope <= 1 and |c| <= 2, so a
    gate error d moves c and h by less than 4 d; + 2e-6 for a few ulp of expf / tanhf on values <= 2."""
    rng = np.random.default_rng(H)
    w_hh = rng.uniform(-1, 1, size=(4 * H, H)).astype(np.float32) / np.float32(np.sqrt(H))
    whh_kn = np.ascontiguousarray(w_hh.T)
    tol = 4 * H * 2.0 ** -24 * np.sqrt(H) + 2e-6
    worst = 0.0
    for a in (1, 31, 32, 33, 70):
        for first in (0, 1):
            rows = a + 3
            h = rng.uniform(-1, 1, size=(rows, H)).astype(np.float32)
            gx = rng.standard_normal((rows, 4 * H)).astype(np.float32)
            c = rng.uniform(-1, 1, size=(rows, H)).astype(np.float32)
            h[a:] = np.nan
            gx[a:] = np.nan
            if first:
                h[:] = np.nan   # (not read at all)
            c_dev, h_out = c.copy(), np.full((rows, H), -7.0, np.float32)
            run_op(model, "rnn_lm_step", [a, H, first], [h, whh_kn, gx, c_dev, h_out], (1 << 3) | (1 << 4))
            wc, wh = step_f64(h[:a], w_hh, gx[:a], c[:a].astype(np.float64), first)
            assert np.array_equal(c_dev[a:].view(np.uint32), c[a:].view(np.uint32)) and np.all(h_out[a:] == -7.0), (a, first)
            err = max(np.abs(c_dev[:a] - wc).max(), np.abs(h_out[:a] - wh).max())
            worst = max(worst, float(err))
            assert err <= tol, (a, first, err, tol)
    print(f"step kernel H = {H}: worst error {worst:.3g}, tolerance {tol:.3g}")


@pytest.mark.parametrize("R,H,V", [(1, 32, 37), (33, 96, 165), (70, 288, 165), (64, 64, 5)])
def test_score_kernel_against_float64(model, R, H, V):
    """lp of R rows against float64 numpy; the padded columns V .. Vp-1 of out_kn hold NaN: they never enter the sum.  Tolerance: a logit
    sums H float32 products (error <= H 2^-24 max sum |y| |w|) and the log-sum-exp is a convex combination of such errors, so lp is
    within twice that, + 8 ulp at the largest |logit| for expf / logf and the online rescaling."""
    rng = np.random.default_rng(R + H + V)
    Vp = (V + 31) // 32 * 32
    y = rng.uniform(-1, 1, size=(R, H)).astype(np.float32)
    w = (rng.standard_normal((V, H)) / np.sqrt(H) * 2).astype(np.float32)
    b = rng.uniform(-1, 1, size=V).astype(np.float32)
    tgt = rng.integers(0, V, size=R).astype(np.int32)
    tgt[0], tgt[-1] = V - 1, 0
    out_kn = np.full((H, Vp), np.nan, np.float32)
    out_kn[:, :V] = w.T
    lp = np.full(R, np.nan, np.float32)
    run_op(model, "rnn_lm_score", [R, H, V, Vp], [y, out_kn, b, tgt, lp], 1 << 4)
    z = y.astype(np.float64) @ w.astype(np.float64).T + b
    m = z.max(1, keepdims=True)
    want = (z - (m + np.log(np.exp(z - m).sum(1, keepdims=True))))[np.arange(R), tgt]
    tol = 2 * H * 2.0 ** -24 * float((np.abs(y) @ np.abs(w.T)).max()) + 8 * 2.0 ** -23 * max(float(np.abs(z).max()), 1.0)
    err = float(np.abs(lp - want).max())
    print(f"score kernel R = {R}, H = {H}, V = {V}: error {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol


# ---- 2. the operator ----------------------------------------------------------------------------------------------------------------------
def check_against_twin(got, tw, hyps, eos, what):
    tot, tlp = got
    wt, wl = tw.score_all(hyps, eos)
    worst = 0.0
    for i, h in enumerate(hyps):
        P = len(h) + int(eos)
        assert len(tlp[i]) == P, (what, i)
        if P:
            e = float(np.abs(tlp[i] - wl[i]).max())
            worst = max(worst, e)
            assert e <= cases.token_bound(), (what, i, e)
        else:
            assert tot[i] == 0.0
        assert abs(tot[i] - wt[i]) <= cases.total_bound(P), (what, i, tot[i], wt[i])
    return worst


@pytest.mark.parametrize("name", list(cases.LMS))
def test_operator_against_the_twin(model, model165, lms, name):
    lm, tw = lms[name]
    V = cases.LMS[name][0]
    model = model165 if V == 165 else model
    model.set_rnn_lm(lm, 0.0)   # (the operator runs the attached LM whatever its scale)
    try:
        worst = 0.0
        for sname, hyps in cases.hyp_sets(V).items():
            for eos in (True, False):
                worst = max(worst, check_against_twin(model.rnn_lm_score(hyps, eos), tw, hyps, eos, (name, sname, eos)))
        print(f"LM {name}: worst token error against the twin {worst:.3g}, bound {cases.token_bound():.3g}")
        # the caller's order under a permuted input
        hyps = cases.hyp_sets(V)["fall"]
        perm = np.random.default_rng(3).permutation(len(hyps))
        check_against_twin(model.rnn_lm_score([hyps[i] for i in perm]), tw, [hyps[i] for i in perm], True, (name, "permuted"))
    finally:
        model.set_rnn_lm(None)


def test_operator_edges(model, lms):
    from k2transducerasr_amd import K2HipError, set_switch
    lm, tw = lms["A"]
    with pytest.raises(K2HipError) as e:   # no LM attached
        model.rnn_lm_score([[1, 2]])
    assert e.value.code == -1 and "no LM" in str(e.value)
    model.set_rnn_lm(lm, 0.5)
    try:
        # an empty hypothesis alone without eos: 0, and nothing reaches the device
        before = model.rnn_lm_stats()["device_calls"]
        tot, tlp = model.rnn_lm_score([[]], with_eos=False)
        assert tot.tolist() == [0.0] and len(tlp[0]) == 0 and model.rnn_lm_stats()["device_calls"] == before
        tot, _ = model.rnn_lm_score([[], []], with_eos=False)
        assert tot.tolist() == [0.0, 0.0] and model.rnn_lm_stats()["device_calls"] == before
        tot, tlp = model.rnn_lm_score([[]], with_eos=True)   # with eos it is one position
        assert model.rnn_lm_stats()["device_calls"] == before + 1 and abs(tot[0] - tw.score([])[0]) <= cases.total_bound(1)
        for hyps, word in (([[1], [2, 37]], "hypothesis 1"), ([[-3]], "hypothesis 0")):
            with pytest.raises(K2HipError) as e:
                model.rnn_lm_score(hyps)
            assert e.value.code == -1 and word in str(e.value)
        # over the arena cap: the time-blocked route agrees with the unblocked one
        hyps = cases.hyp_sets(37)["fall"]
        plain = model.rnn_lm_score(hyps)
        assert model.rnn_lm_stats()["last_blocks"] == 1
        set_switch("K2HIP_RNN_LM_GX_CAP", 4 * 64 * 100)   # 100 rows of GX: the 70-row steps go one by one, the later ones in groups
        try:
            blocked = model.rnn_lm_score(hyps)
            assert model.rnn_lm_stats()["last_blocks"] > 10
        finally:
            set_switch("K2HIP_RNN_LM_GX_CAP", 0)
        check_against_twin(blocked, tw, hyps, True, "blocked")
        for i, h in enumerate(hyps):
            assert abs(blocked[0][i] - plain[0][i]) <= cases.total_bound(len(h) + 1)
            assert np.abs(blocked[1][i] - plain[1][i]).max() <= cases.token_bound()
        # a wrong vocabulary is refused
        with pytest.raises(K2HipError) as e:
            model.set_rnn_lm(lms["C"][0], 0.5)
        assert "vocab_size" in str(e.value)
        for bad in (-0.5, float("nan"), float("inf")):
            with pytest.raises(K2HipError):
                model.set_rnn_lm(lm, bad)
    finally:
        model.set_rnn_lm(None)


# ---- 3. the recognizer -------------------------------------------------------------------------------------------------------------------
def decode(rec, utts):
    ss = [rec.create_offline_stream() for _ in utts]
    for s, u in zip(ss, utts):
        s.add_samples(u)
    res = rec.get_results(ss)
    return res, [s.alternatives() for s in ss], [s.token_log_probs() for s in ss]


def same_lists(got, want):
    assert [len(a) for a in got] == [len(a) for a in want]
    for ga, wa in zip(got, want):
        for g, w in zip(ga, wa):
            assert (g["tokens"], g["timestamps"]) == (w["tokens"], w["timestamps"])
            assert np.float32(g["score"]) == np.float32(w["score"]) and g["lm_score"] == w["lm_score"]
            assert np.array_equal(g["token_log_probs"], w["token_log_probs"])


@pytest.mark.parametrize("kind", ["transducer", "ctc"])
def test_recognizer_rescoring(kind, tmp_path, utts):
    from k2transducerasr_amd import OfflineRecognizer, RnnLm
    from k2transducerasr_amd.synth import write_synthetic_model, write_synthetic_rnn_lm
    rc = cases.RECOGNIZER[kind]
    ctc = kind == "ctc"
    mp, lp_ = str(tmp_path / "m.k2w"), str(tmp_path / "lm.k2w")
    write_synthetic_model(mp, rc["preset"])
    V, E, H, L, _ = cases.LMS["A"]
    tw = Twin(write_synthetic_rnn_lm(lp_, V, E, H, L, rc["seed"]), L)
    lm = RnnLm(lp_)
    plain = OfflineRecognizer(mp, 0, rc["method"], 4, nbest=4)      # a model that never saw an LM
    res0, alts0, yp0 = decode(plain, utts)
    plain.model.close()
    assert all(a["lm_score"] == 0.0 for al in alts0 for a in al)
    rec = OfflineRecognizer(mp, 0, rc["method"], 4, nbest=4, rnn_lm=lm, rnn_lm_scale=0.0)
    lm.close()                                                       # (the model keeps its own copy)
    try:
        # scale = 0, and an LM set and cleared: bit for bit the plain results
        for step in ("scale 0", "cleared"):
            res, alts, yp = decode(rec, utts)
            assert res == res0, step
            same_lists(alts, alts0)
            assert all(np.array_equal(a, b) for a, b in zip(yp, yp0))
            lm2 = RnnLm(lp_)
            rec.model.set_rnn_lm(lm2, rc["scale"])
            rec.model.set_rnn_lm(None)
        rec.model.set_rnn_lm(lm2, rc["scale"])
        res, alts, yp = decode(rec, utts)
        # the operator on the same call: every alternative of every stream in the plain order
        flat = [a["tokens"] for al in alts0 for a in al]
        op_tot, _ = rec.model.rnn_lm_score(flat, True)
        op = {(b, tuple(a["tokens"])): op_tot[i] for i, (b, a) in enumerate((b, a) for b, al in enumerate(alts0) for a in al)}
        changed, gap, B = 0, np.inf, len(utts)
        for b, (al, al0) in enumerate(zip(alts, alts0)):
            key0 = [tuple(a["tokens"]) for a in al0]
            assert len(set(key0)) == len(key0) and sorted(tuple(a["tokens"]) for a in al) == sorted(key0)   # the plain list re-ordered
            twin_lm = [tw.score(a["tokens"])[0] for a in al0]
            order, keys = rescored_order([float(np.float32(a["score"])) for a in al0], [len(a["tokens"]) for a in al0], twin_lm, rc["scale"], ctc)
            ks = sorted(keys, reverse=True)
            gap = min([gap] + [x - y for x, y in zip(ks, ks[1:])])
            changed += order[0] != 0
            for a, i in zip(al, order):      # the twin's order (every adjacent pair of keys is KEY_GAP apart: asserted below)
                w = al0[i]
                assert (a["tokens"], a["timestamps"]) == (w["tokens"], w["timestamps"]), (b, order)
                assert np.float32(a["score"]) == np.float32(w["score"]) and np.array_equal(a["token_log_probs"], w["token_log_probs"])
                assert abs(a["lm_score"] - twin_lm[i]) <= cases.total_bound(len(w["tokens"]) + 1)
                assert np.float32(a["lm_score"]) == np.float32(op[(b, tuple(a["tokens"]))])
            # entry 0 is the stream's result
            n = len(al[0]["tokens"])
            assert list(res[b][0])[len(res[b][0]) - n:] == al[0]["tokens"] and np.array_equal(yp[b], al[0]["token_log_probs"])
            if not ctc:
                assert res[b][0][2 * B:] == al[0]["tokens"] and res[b][1][2 * B:] == al[0]["timestamps"]
        print(f"{kind}: {changed} of {B} tops change, smallest adjacent key gap {gap:.4g}")
        assert gap >= cases.KEY_GAP and changed >= 2                 # conditions of the chosen inputs, not measurements
        assert sum(r != r0 for r, r0 in zip(res, res0)) >= 2
    finally:
        rec.model.close()


# ---- 4. unchanged paths ------------------------------------------------------------------------------------------------------------------
def test_paths_that_ignore_the_lm(tmp_path, tiny_model_path, utts):
    from k2transducerasr_amd import OfflineRecognizer, OnlineRecognizer, RnnLm
    from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model, write_synthetic_rnn_lm
    V, E, H, L, _ = cases.LMS["A"]
    lp_ = str(tmp_path / "lm.k2w")
    write_synthetic_rnn_lm(lp_, V, E, H, L, 1)
    lm = RnnLm(lp_)
    long_x = np.concatenate([np.concatenate([u, np.zeros(6400, np.float32)]) for u in utts[:3]])

    def offline(with_lm, method, nbest):
        rec = OfflineRecognizer(tiny_model_path, 0, method, 4, nbest=nbest, rnn_lm=lm if with_lm else None, rnn_lm_scale=2.0)
        try:
            batch = decode(rec, utts)
            s = rec.create_offline_stream()
            s.add_samples(utts[0])
            single = rec.get_result(s) if nbest == 1 else None
            return batch, single, rec.model.recognize_long(long_x), rec.model.rnn_lm_stats()["device_calls"]
        finally:
            rec.model.close()

    # greedy, get_result and recognize_long; beam search with n = 1 (nothing to rescore): no scoring call is ever issued
    for method, nbest in (("greedy_search", 1), ("modified_beam_search", 1)):
        a, b = offline(False, method, nbest), offline(True, method, nbest)
        assert a[0][0] == b[0][0] and a[1] == b[1] and a[2] == b[2] and b[3] == 0, method
        same_lists(a[0][1], b[0][1])
    # recognize_long under beam search with a list kept and the LM on: the batch is rescored, the long entry is not
    a, b = offline(False, "modified_beam_search", 4), offline(True, "modified_beam_search", 4)
    assert a[2] == b[2] and b[3] == 1 and len(b[2]) >= 1
    # the streaming step
    sp = str(tmp_path / "s.k2w")
    write_synthetic_model(sp, "zipformer2-streaming-tiny-test")
    outs = []
    for with_lm in (False, True):
        rec = OnlineRecognizer(sp, 0, "modified_beam_search", 4)
        try:
            if with_lm:
                rec.model.set_rnn_lm(lm, 2.0)
            hs = [rec.create_online_stream() for _ in range(2)]
            for u, h in enumerate(hs):
                h.add_samples(synth_utterance(40 + u, 1.5))
            for _ in range(64):
                dec, _ = rec.get_results(hs)
                if not any(dec):
                    break
            outs.append([(h.tokens, h.timestamps) for h in hs])
            assert rec.model.rnn_lm_stats()["device_calls"] == 0
        finally:
            rec.model.close()
    assert outs[0] == outs[1] and sum(len(t) for t, _ in outs[0]) > 0
