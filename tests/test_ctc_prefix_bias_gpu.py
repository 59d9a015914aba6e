"""Hotword and n-gram LM biasing of the CTC prefix beam search on the GPU (csrc/ctc_prefix.hip k_ctc_prefix<false, true> through the debug
op "ctc_prefix_beam_bias", k2hip_set_ctc_prefix_biasing with k2hip_ctc_prefix_beam_search and the batch entries under
"ctc_prefix_beam_search"), against the float64 twin (tests/ctc_prefix_bias_twin.py).

Bounds, those of tests/test_ctc_prefix_gpu.py (none of them taken from what the engine gives):
  * tokens, timestamps, n_hyps and the order of the entries are exact; every case clears its G = 8 E on the twin alone
    (tests/ctc_prefix_bias_cases.py has the table, tests/test_ctc_prefix_bias.py re-measures E and checks every gap on the CPU);
  * token log-probs are exact: they are copies of inputs;
  * final is within 1e-5 relative to max(1, |value|).
Outputs are pre-filled with -7, so what the kernel does not write shows.

Worst differences seen on an MI355X are recorded in DESIGN.md "Hotword and n-gram LM biasing of the CTC prefix beam search"."""
import ctypes as C

import numpy as np
import pytest

import ctc_prefix_bias_cases as bc
import ctc_prefix_cases as base
from ctc_prefix_bias_twin import biased_prefix_beam_search, dense_graph, lm_tables, min_gap
from hotword_twin import TwinGraph

pytestmark = pytest.mark.gpu

REL = 1e-5
KEYS = ("tokens", "timestamps", "token_log_probs", "n_tokens", "n_hyps", "scores")


def rel(got, want):
    return abs(float(got) - want) / max(1.0, abs(want))


def lists(op):
    """what Model.ctc_prefix_beam_search returned, as comparable tuples (scores by their float32 bits)"""
    return [[(a["tokens"], a["timestamps"], np.float32(a["score"]).tobytes(), np.asarray(a["token_log_probs"], np.float32).tobytes()) for a in row]
            for row in op]


@pytest.fixture(scope="module")
def ctc_path(tmp_path_factory):
    from k2transducerasr_amd.synth import write_synthetic_model
    p = str(tmp_path_factory.mktemp("ctcprefixbias") / "ctc_tiny.k2w")
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
    feats = [hip_ctc.fbank(u) for u in utts]
    return hip_ctc.encoder_proj(hip_ctc.pad_sequence(feats).reshape(len(utts), -1, 80))


def _lib():
    from k2transducerasr_amd import load_library
    L = load_library()
    L.k2hip_debug_op_run.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                     C.c_int32, C.c_uint32]
    return L


def _outputs(R, nbest, max_tokens):
    return [np.full((R, nbest, max_tokens), -7, np.int64), np.full((R, nbest, max_tokens), -7, np.int32),
            np.full((R, nbest, max_tokens), -7, np.float32), np.full((R, nbest), -7, np.int32), np.full(R, -7, np.int32),
            np.full((R, nbest), -7, np.float32), np.full(1, -7, np.int32)]


def _result(outs):
    tok, ts, yp, n, nh, sc, flag = outs
    return dict(tokens=tok, timestamps=ts, token_log_probs=yp, n_tokens=n, n_hyps=nh, scores=sc, flag=int(flag[0]))


def run_plain(model, lp, n_frames, beam, nbest, max_tokens):
    """the unbiased kernel through "ctc_prefix_beam\""""
    L = _lib()
    lp = np.ascontiguousarray(lp, np.float32)
    R, Tp, V = lp.shape
    nf = None if n_frames is None else np.ascontiguousarray(n_frames, np.int32)
    bufs = [lp, nf] + _outputs(R, nbest, max_tokens)
    ptrs = (C.c_void_p * 9)(*[b.ctypes.data if b is not None else None for b in bufs])
    sizes = (C.c_int64 * 9)(*[b.nbytes if b is not None else 0 for b in bufs])
    ia = (C.c_int64 * 6)(R, Tp, V, beam, nbest, max_tokens)
    rc = L.k2hip_debug_op_run(model.handle, b"ctc_prefix_beam", ia, 6, ptrs, sizes, 9, sum(1 << k for k in range(2, 9)))
    assert rc == 0, (rc, L.k2hip_last_error())
    return _result(bufs[2:])


def tables_of(graph, lm):
    """the nine table buffers of "ctc_prefix_beam_bias" and (S, S_lm, A, start); a missing half is None"""
    hw = [None, None, None]
    S = S_lm = A = start = 0
    if graph is not None:
        hw = [np.ascontiguousarray(x) for x in dense_graph(graph)]
        S = hw[0].shape[0]
    lmb = [None] * 6
    if lm is not None:
        t = lm_tables(lm)
        lmb = [t["states"], t["arc_tok"] if len(t["arc_tok"]) else None, t["arc_lp"] if len(t["arc_lp"]) else None,
               t["arc_next"] if len(t["arc_next"]) else None, t["uni_lp"], t["uni_next"]]
        S_lm, A, start = t["states"].shape[0], len(t["arc_tok"]), t["start"]
    return hw + lmb, (S, S_lm, A, start)


def run_raw(model, lp, n_frames, beam, nbest, max_tokens, tabs, dims):
    """the biased kernel alone through "ctc_prefix_beam_bias", every output pre-filled with -7; returns (rc, result)"""
    L = _lib()
    lp = np.ascontiguousarray(lp, np.float32)
    R, Tp, V = lp.shape
    nf = None if n_frames is None else np.ascontiguousarray(n_frames, np.int32)
    bufs = [lp, nf] + _outputs(R, nbest, max_tokens) + [None if b is None else np.ascontiguousarray(b) for b in tabs]
    ptrs = (C.c_void_p * 18)(*[b.ctypes.data if b is not None else None for b in bufs])
    sizes = (C.c_int64 * 18)(*[b.nbytes if b is not None else 0 for b in bufs])
    ia = (C.c_int64 * 10)(R, Tp, V, beam, nbest, max_tokens, *dims)
    rc = L.k2hip_debug_op_run(model.handle, b"ctc_prefix_beam_bias", ia, 10, ptrs, sizes, 18, sum(1 << k for k in range(2, 9)))
    return rc, _result(bufs[2:9])


def run_op(model, lp, n_frames, beam, nbest, max_tokens, graph, lm):
    from k2transducerasr_amd import load_library
    tabs, dims = tables_of(graph, lm)
    rc, out = run_raw(model, lp, n_frames, beam, nbest, max_tokens, tabs, dims)
    assert rc == 0, (rc, load_library().k2hip_last_error())
    return out


_twin_cache = {}


def twin(key, lp, beam, graph, lm):
    """the float64 twin, computed once per (case, beam) and shared"""
    if (key, beam) not in _twin_cache:
        _twin_cache[(key, beam)] = biased_prefix_beam_search(np.asarray(lp, np.float64), beam, graph, lm)
    return _twin_cache[(key, beam)]


def check_row(out, r, lp_row, want, nbest):
    """row r of a kernel result against a twin run: everything exact but final; returns the worst relative difference of final"""
    hyps = want["hyps"]
    nh = min(nbest, len(hyps))
    assert out["n_hyps"][r] == nh, (r, out["n_hyps"][r], nh)
    worst = 0.0
    for i in range(nbest):
        if i >= nh:
            assert out["n_tokens"][r, i] == -7 and out["scores"][r, i] == -7 and np.all(out["tokens"][r, i] == -7), (r, i)
            continue
        h = hyps[i]
        n = len(h["tokens"])
        assert out["n_tokens"][r, i] == n, (r, i, out["n_tokens"][r, i], n)
        assert out["tokens"][r, i, :n].tolist() == h["tokens"], (r, i, out["tokens"][r, i, :n].tolist(), h["tokens"])
        assert out["timestamps"][r, i, :n].tolist() == h["timestamps"], (r, i)
        assert np.array_equal(out["token_log_probs"][r, i, :n], np.asarray([lp_row[t, v] for t, v in zip(h["timestamps"], h["tokens"])], np.float32)), (r, i)
        assert np.all(out["tokens"][r, i, n:] == -7) and np.all(out["timestamps"][r, i, n:] == -7) and np.all(out["token_log_probs"][r, i, n:] == -7)
        if h["score"] == -np.inf:
            assert out["scores"][r, i] == -np.inf
        else:
            worst = max(worst, rel(out["scores"][r, i], h["score"]))
            assert rel(out["scores"][r, i], h["score"]) <= REL, (r, i, out["scores"][r, i], h["score"])
    return worst


# ---- 1. null and empty tables: the plain kernel, bit for bit ----------------------------------------------------------------------------
@pytest.mark.parametrize("beam", base.RAGGED_BEAMS)
def test_null_and_empty_tables_are_the_plain_kernel(hip_ctc, beam):
    lp, nf = base.ragged_rows()
    want = run_plain(hip_ctc, lp, nf, beam, beam, 70)
    empty_lm = bc.TwinLm([((-1,), -99.0, 0.0), ((-3,), -7.5, 0.0)], 37).scaled(0.0)      # <s> and <unk> only, every weight +0.0
    for graph, lm in ((None, None), (TwinGraph([], bc.SCORE, 37), None), (TwinGraph([[5, 7], [9]], 0.0, 37), None), (TwinGraph([], bc.SCORE, 37), empty_lm)):
        got = run_op(hip_ctc, lp, nf, beam, beam, 70, graph, lm)
        assert got["flag"] == want["flag"] == 0
        for k in KEYS:
            assert got[k].tobytes() == want[k].tobytes(), (beam, k, graph is not None, lm is not None)


# ---- 2. against the twin ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", bc.KINDS)
def test_kernel_small_vocabulary(hip_ctc, kind):
    """V = 3 exhaustive at beam 8 (nothing pruned), the re-spelled row at beam 4 with a graph over its tokens"""
    lp, nf = base.exhaustive_rows()
    graph, lm = bc.pick(kind, bc.small_graph(bc.EXHAUSTIVE_PHRASES), bc.small_lm())
    out = run_op(hip_ctc, lp, nf, 8, 8, 2, graph, lm)
    assert out["flag"] == 0
    for r, T in enumerate(nf):
        want = twin(("ex", kind, r), lp[r, :T], 8, graph, lm)
        assert min_gap(want) >= bc.G_SMALL and len(want["hyps"]) == (3, 5)[r]
        check_row(out, r, lp[r], want, 8)
    graph, lm = bc.pick(kind, bc.small_graph(bc.RESPELLED_PHRASES), bc.small_lm())
    lp, beam = base.respelled_row(), base.RESPELLED_BEAM
    want = twin(("respelled", kind), lp, beam, graph, lm)
    assert min_gap(want) >= bc.G_SMALL and (kind == "lm" or want["respelled_folds"] >= 1)
    out = run_op(hip_ctc, lp[None], None, beam, beam, base.RESPELLED_T, graph, lm)
    check_row(out, 0, lp, want, beam)
    got = [tuple(out["tokens"][0, i, : out["n_tokens"][0, i]].tolist()) for i in range(out["n_hyps"][0])]
    assert len(set(got)) == len(got), got


def test_kernel_hand_built_flip(hip_ctc):
    """the derivation in ctc_prefix_bias_cases.py: [b] without the phrase, [a, b] @ 0, 1 with it, final exactly 0.75"""
    lp = bc.FLIP_ROWS
    plain = run_plain(hip_ctc, lp[None], None, bc.FLIP_BEAM, bc.FLIP_BEAM, 3)
    assert plain["tokens"][0, 0, : plain["n_tokens"][0, 0]].tolist() == bc.FLIP_UNBIASED[0]
    out = run_op(hip_ctc, lp[None], None, bc.FLIP_BEAM, bc.FLIP_BEAM, 3, bc.flip_graph(), None)
    check_row(out, 0, lp, twin("flip", lp, bc.FLIP_BEAM, bc.flip_graph(), None), bc.FLIP_BEAM)
    assert out["tokens"][0, 0, :2].tolist() == bc.FLIP_BIASED[0] and out["timestamps"][0, 0, :2].tolist() == bc.FLIP_BIASED[1]
    assert out["scores"][0, 0] == bc.FLIP_BIASED[2]


@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("beam", base.RAGGED_BEAMS)
def test_kernel_ragged(hip_ctc, beam, kind):
    """V = 37, one call with n_frames = 1, 2, 7, 70, a row with 2 % -inf cells and a row that is -inf everywhere; nbest = beam"""
    lp, nf = base.ragged_rows()
    graph, lm = bc.pick(kind, *bc.ragged_tables())
    out = run_op(hip_ctc, lp, nf, beam, beam, int(nf.max()), graph, lm)
    assert out["flag"] == 0
    worst = 0.0
    for r in range(len(base.RAGGED_SEEDS)):
        want = twin(("ragged", kind, r), lp[r, : nf[r]], beam, graph, lm)
        assert min_gap(want) >= bc.G_RAGGED
        worst = max(worst, check_row(out, r, lp[r], want, beam))
    r = base.RAGGED_ALL_INF_ROW       # -inf everywhere: the empty prefix, final -inf, nothing out of range
    assert out["n_hyps"][r] == 1 and out["n_tokens"][r, 0] == 0 and out["scores"][r, 0] == -np.inf
    assert np.all(out["tokens"][r] == -7) and np.all(out["timestamps"][r] == -7) and np.all(out["n_tokens"][r, 1:] == -7)
    print(f"ragged {kind} beam {beam}: worst relative difference of final {worst:.3g} (bound {REL:g})")


@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("beam", base.WIDE_BEAMS)
def test_kernel_wide_vocabulary(hip_ctc, beam, kind):
    """V = 600: columns above 256 and above 512; the LM's hub state has more than 64 arcs, so the walk's narrowing runs"""
    lp = base.wide_row()
    graph, lm = bc.pick(kind, *bc.wide_tables())
    want = twin(("wide", kind), lp, beam, graph, lm)
    assert min_gap(want) >= bc.G_WIDE
    assert any(v > 512 for h in want["hyps"] for v in h["tokens"]) and any(256 < v <= 512 for h in want["hyps"] for v in h["tokens"])
    if lm is not None:
        st = lm_tables(lm)["states"]
        assert (st[:, 1] - st[:, 0]).max() > 64
    out = run_op(hip_ctc, lp[None], None, beam, beam, base.WIDE_T, graph, lm)
    print(f"wide {kind} beam {beam}: worst relative difference of final {check_row(out, 0, lp, want, beam):.3g} (bound {REL:g})")


@pytest.mark.parametrize("kind", bc.KINDS)
def test_kernel_long_histories(hip_ctc, kind):
    """V = 37, T = 300, beam 4, nbest 4, max_tokens = 300"""
    lp = base.long_row()
    graph, lm = bc.pick(kind, *bc.long_tables())
    want = twin(("long", kind), lp, base.LONG_BEAM, graph, lm)
    assert min_gap(want) >= bc.G_LONG and len(want["hyps"][0]["tokens"]) > 100
    out = run_op(hip_ctc, lp[None], None, base.LONG_BEAM, 4, base.LONG_T, graph, lm)
    assert out["flag"] == 0
    print(f"long {kind}: worst relative difference of final {check_row(out, 0, lp, want, 4):.3g} (bound {REL:g})")


# ---- 3. independence, overflow, table checks ------------------------------------------------------------------------------------------------
def test_a_rows_result_does_not_depend_on_the_other_rows(hip_ctc):
    lp, nf = base.ragged_rows()
    graph, lm = bc.ragged_tables()
    batch = run_op(hip_ctc, lp, nf, 4, 4, 70, graph, lm)
    for r in (2, 3):
        alone = run_op(hip_ctc, lp[r: r + 1], nf[r: r + 1], 4, 4, 70, graph, lm)
        for k in KEYS:
            assert np.array_equal(alone[k][0], batch[k][r]), (r, k)
    other = lp.copy()
    other[[0, 1, 2, 4, 5]] = other[[0, 1, 2, 4, 5]][:, ::-1]          # every other row changes
    again = run_op(hip_ctc, other, nf, 4, 4, 70, graph, lm)
    for k in ("tokens", "timestamps", "token_log_probs", "n_tokens", "scores"):
        assert np.array_equal(again[k][3], batch[k][3]), k


def test_overflow_rule_per_entry(hip_ctc):
    """max_tokens below the longest entry: that entry is not written (n_tokens 0, its row keeps the fill), the flag is raised, the other
    entries and every final are as without the limit"""
    lp, nf = base.ragged_rows()
    graph, lm = bc.ragged_tables()
    full = run_op(hip_ctc, lp, nf, 4, 4, 70, graph, lm)
    lens = full["n_tokens"][3]
    cap = int(lens.max()) - 1
    assert full["flag"] == 0 and cap >= 1 and (lens <= cap).any()
    cut = run_op(hip_ctc, lp, nf, 4, 4, cap, graph, lm)
    assert cut["flag"] == 1
    for r in range(lp.shape[0]):
        for i in range(full["n_hyps"][r]):
            n = full["n_tokens"][r, i]
            assert cut["scores"][r, i] == full["scores"][r, i]
            if n > cap:
                assert cut["n_tokens"][r, i] == 0 and np.all(cut["tokens"][r, i] == -7) and np.all(cut["timestamps"][r, i] == -7)
            else:
                assert cut["n_tokens"][r, i] == n and np.array_equal(cut["tokens"][r, i, :n], full["tokens"][r, i, :n])


def test_bad_tables_are_refused_before_any_launch(hip_ctc):
    """a next entry and an arc range that point outside their tables: K2HIP_ERR_INVALID from the host-side check, nothing written"""
    lp, nf = base.ragged_rows()
    graph, lm = bc.ragged_tables()
    tabs, dims = tables_of(graph, lm)
    S, S_lm, A, start = dims

    def refused(tabs, dims):
        rc, out = run_raw(hip_ctc, lp, nf, 4, 4, 70, tabs, dims)
        assert rc == -1, rc
        assert all(np.all(out[k] == -7) for k in KEYS) and out["flag"] == -7

    bad = [None if t is None else t.copy() for t in tabs]
    bad[0][1, 5] = S                                   # next out of range
    refused(bad, dims)
    bad = [None if t is None else t.copy() for t in tabs]
    bad[3][S_lm - 1, 1] = A + 1                        # an arc range past A
    refused(bad, dims)
    bad = [None if t is None else t.copy() for t in tabs]
    bad[3][S_lm - 1, 0] = bad[3][S_lm - 1, 1] + 1      # begin behind end
    refused(bad, dims)
    bad = [None if t is None else t.copy() for t in tabs]
    bad[3][1, 2] = S_lm                                # a back-off state out of range
    refused(bad, dims)
    bad = [None if t is None else t.copy() for t in tabs]
    bad[6][0] = -1                                     # arc_next
    refused(bad, dims)
    bad = [None if t is None else t.copy() for t in tabs]
    bad[8][7] = S_lm                                   # uni_next
    refused(bad, dims)
    refused(tabs, (S, S_lm, A, S_lm))                  # the start state
    refused(tabs[:2] + [None] + tabs[3:], dims)        # an incomplete hotword group
    rc, _ = run_raw(hip_ctc, lp, nf, 4, 4, 70, tabs, dims)
    assert rc == 0


# ---- 4. end to end ------------------------------------------------------------------------------------------------------------------------
def test_end_to_end(hip_ctc, ctc_path, utts, device_log_probs, hip_tiny):
    from k2transducerasr_amd import Hotwords, K2HipError, NgramLm, OfflineRecognizer
    lp = device_log_probs
    B, Tp, V = lp.shape
    beam = bc.FIXTURE_BEAM
    phrases, entries = bc.fixture_entries(lp)
    graph, lm = bc.fixture_tables(lp)
    assert len(phrases) >= 3

    def batch():
        hip_ctc.set_decoding_method("ctc_prefix_beam_search", beam)
        try:
            got = hip_ctc.offline_greedy_from_samples(utts)
            return [(list(a), list(b)) for a, b in got], np.array(hip_ctc.last_scores(B), np.float32)
        finally:
            hip_ctc.set_decoding_method("greedy_search")

    nothing = batch()
    op_nothing = hip_ctc.ctc_prefix_beam_search(lp, beam=beam, nbest=4)
    assert all(len(row) == 4 for row in op_nothing)
    hw, ng = Hotwords(phrases, bc.SCORE, V), NgramLm(entries, V)
    try:
        hip_ctc.set_hotwords(hw)
        hip_ctc.set_ngram_lm(ng, bc.LM_SCALE)
        # switch off, both set: bit for bit the results with nothing set
        off = batch()
        assert off[0] == nothing[0] and off[1].tobytes() == nothing[1].tobytes()
        assert lists(hip_ctc.ctc_prefix_beam_search(lp, beam=beam, nbest=4)) == lists(op_nothing)
        hip_ctc.set_ctc_prefix_biasing(True)
        try:
            worst, moved = 0.0, 0
            for kind in ("both", "hw", "lm"):
                hip_ctc.set_hotwords(hw if kind != "lm" else None)
                hip_ctc.set_ngram_lm(ng if kind != "hw" else None, bc.LM_SCALE)
                g, m = bc.pick(kind, graph, lm)
                got, scores = batch()
                op = hip_ctc.ctc_prefix_beam_search(lp, beam=beam, nbest=4)
                for b in range(B):
                    want = twin(("e2e", kind, b), lp[b], beam, g, m)
                    assert min_gap(want) >= bc.G_FIXTURE, (kind, b, min_gap(want))
                    h = want["hyps"][0]
                    assert got[b] == (h["tokens"], h["timestamps"]), (kind, b)
                    assert rel(scores[b], h["score"]) <= REL, (kind, b, scores[b], h["score"])
                    worst = max(worst, rel(scores[b], h["score"]))
                    moved += got[b][0] != nothing[0][b][0]
                    assert len(op[b]) == min(4, len(want["hyps"]))
                    for a, w in zip(op[b], want["hyps"]):          # the operator entry: the same lists
                        assert (a["tokens"], a["timestamps"]) == (w["tokens"], w["timestamps"]) and rel(a["score"], w["score"]) <= REL, (kind, b)
                    assert (op[b][0]["tokens"], op[b][0]["timestamps"]) == got[b] and np.float32(op[b][0]["score"]) == scores[b]
            assert moved > 0
            print(f"end to end: worst relative difference of final {worst:.3g} (bound {REL:g})")
            hip_ctc.set_hotwords(hw)
            hip_ctc.set_ngram_lm(ng, bc.LM_SCALE)
            op = hip_ctc.ctc_prefix_beam_search(lp, beam=beam, nbest=4)
            # with neither table set the plain instantiation runs, switch still on
            hip_ctc.set_hotwords(None)
            hip_ctc.set_ngram_lm(None)
            on_nothing = batch()
            assert on_nothing[0] == nothing[0] and on_nothing[1].tobytes() == nothing[1].tobytes()
        finally:
            hip_ctc.set_ctc_prefix_biasing(False)
    finally:
        hip_ctc.set_hotwords(None)
        hip_ctc.set_ngram_lm(None)
    after = batch()
    assert after[0] == nothing[0] and after[1].tobytes() == nothing[1].tobytes()
    # the recognizer: the same lists
    rec = OfflineRecognizer(ctc_path, decoding_method="ctc_prefix_beam_search", beam=beam, hotwords=phrases, hotwords_score=bc.SCORE, nbest=4,
                            ngram_lm=ng, ngram_lm_scale=bc.LM_SCALE, ctc_prefix_biasing=True)
    try:
        streams = [rec.create_offline_stream() for _ in utts]
        for s, u in zip(streams, utts):
            s.add_samples(u)
        rec.get_results(streams)
        for b in range(B):
            alts = streams[b].alternatives()
            assert len(alts) == len(op[b])
            for a, o in zip(alts, op[b]):
                assert a["tokens"] == o["tokens"] and a["timestamps"] == o["timestamps"] and rel(a["score"], o["score"]) <= REL, b
    finally:
        rec.model.close()
    plain = OfflineRecognizer(ctc_path, decoding_method="ctc_prefix_beam_search", beam=beam, hotwords=phrases, hotwords_score=bc.SCORE, nbest=4,
                              ngram_lm=ng, ngram_lm_scale=bc.LM_SCALE)       # without the keyword: as before
    try:
        streams = [plain.create_offline_stream() for _ in utts]
        for s, u in zip(streams, utts):
            s.add_samples(u)
        plain.get_results(streams)
        for b in range(B):
            assert [(a["tokens"], a["timestamps"]) for a in streams[b].alternatives()] == [(a["tokens"], a["timestamps"]) for a in op_nothing[b]]
    finally:
        plain.model.close()
    with pytest.raises(K2HipError) as e:               # a transducer handle refuses the switch
        hip_tiny.set_ctc_prefix_biasing(True)
    assert e.value.code == -6, (e.value.code, str(e.value))


def test_streaming_search_is_unaffected_by_the_switch(tmp_path):
    """a streaming CTC stream under set_ctc_prefix_beam: the same result with the switch on (hotwords and an LM set) as with it off"""
    from k2transducerasr_amd import Hotwords, NgramLm, OnlineRecognizer
    from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model
    p = str(tmp_path / "ctc_streaming.k2w")
    write_synthetic_model(p, "zipformer2-ctc-streaming-tiny-test")
    results = []
    for on in (False, True):
        rec = OnlineRecognizer(p)
        try:
            V = rec.model.vocab_size
            if on:
                rec.model.set_hotwords(Hotwords([[5, 7], [9, 11, 4]], bc.SCORE, V))
                rec.model.set_ngram_lm(NgramLm([((-1,), -99.0, -0.5), ((-3,), -7.5, 0.0)] + [((v,), -3.0 - 0.01 * v, -0.25) for v in range(3, V)] +
                                               [((5, 7), -0.5, 0.0)], V), bc.LM_SCALE)
                rec.model.set_ctc_prefix_biasing(True)
            s = rec.create_online_stream(ctc_prefix_beam=4, nbest=2)
            s.add_samples(synth_utterance(0, 2.0))
            while True:
                dec, _ = rec.get_results([s])
                if not dec[0]:
                    break
            results.append((list(s.tokens), list(s.timestamps), s.score, [(a["tokens"], a["timestamps"], a["score"]) for a in s.alternatives()]))
        finally:
            rec.model.close()
    assert results[0] == results[1] and results[0][3] and results[0][2] != 0.0        # (and the carried search did run)
