"""CTC keyword spotting on the GPU (csrc/ctc_kws.hip through the k2hip_ctc_kws_* entries, k2hip_offline_ctc_spot_keywords_from_samples
and the debug op "ctc_trie_dp"), against the float32 host reference (csrc/ctc_kws_ref.h) and the float64 twin (tests/ctc_kws_twin.py).

Bounds (none of them taken from what the engine gives):
  * the kernel's float32 operations and their order are the host reference's, adds and compares only: events, sum_logp, counts and the
    whole carried block equal it BIT FOR BIT, on planes of multiples of 0.25 and on the engine's own log-probs alike;
  * against the float64 twin on the engine's log-probs: tests/test_ctc_kws.py's bound (every comparison's gap at least 4 x the float32
    error of a cell) is asserted on the array itself, so every (keyword, start, end) equals the twin's;
  * chunking: bit-identical events and carried blocks, whatever the chunk list;
  * the fused route scores the DEVICE encoder's frames, which encoder_proj returns: the events are equal."""
import numpy as np
import pytest

from ctc_kws_cases import GPU_S, GPU_T, GPU_V, KEYWORDS, THRESHOLDS, hand_cases, random_plane, random_trie, tables
from ctc_kws_twin import fresh_state
from test_align_gpu import debug_op
from test_ctc_kws import F32_BOUND, MAX_SUM, MIN_RATIO, fixture_run, ref_dp

pytestmark = pytest.mark.gpu

TABLE_KEYS = ("parent", "tok", "depth", "kw", "bar", "rc")


@pytest.fixture(scope="module")
def hip_ctc(tmp_path_factory):
    from k2transducerasr_amd import Model
    from k2transducerasr_amd.synth import write_synthetic_model
    p = str(tmp_path_factory.mktemp("ctckwsgpu") / "ctc_tiny.k2w")
    write_synthetic_model(p, "zipformer2-ctc-tiny-test")
    return Model(p, 0)


@pytest.fixture(scope="module")
def device_log_probs(hip_ctc, utts):
    """log_probs [5, 35, 37] of the padded fixture batch from the existing encoder entry, on the engine's own features"""
    feats = [hip_ctc.fbank(u) for u in utts]
    lp = hip_ctc.encoder_proj(hip_ctc.pad_sequence(feats).reshape(len(utts), -1, 80))
    assert lp.shape == (5, 35, 37)
    return lp


@pytest.fixture(scope="module")
def keywords24(hip_ctc):
    from k2transducerasr_amd import Keywords
    return Keywords(KEYWORDS, THRESHOLDS, hip_ctc.vocab_size)


@pytest.fixture(scope="module")
def graph24(keywords24):
    """the fixture graph's tables as the library built them, with rc restated"""
    from ctc_kws_twin import root_children
    t = keywords24.tables()
    t["rc"] = root_children(t).astype(np.int32)
    return t


def as_tuples(events):
    return [(e["keyword"], e["start"], e["end"], float(e["sum_logp"])) for e in events]


def run_dp(hip, graphs, graph_of, planes, blocks=None, n_frames=None):
    """"ctc_trie_dp": stream b walks graphs[graph_of[b]] over the first n_frames[b] frames of planes[b] [T_b][V] from blocks[b] (or a fresh
    block) -> (events per stream, v per stream, st per stream).  The output buffers are NaN / -7 prefilled: what comes back was written."""
    B, V = len(planes), planes[0].shape[1]
    nf = np.array([p.shape[0] for p in planes] if n_frames is None else n_frames, np.int32)
    Tp = max(int(max(p.shape[0] for p in planes)), 1)
    lp = np.full((B, Tp, V), np.nan, np.float32)   # the frames beyond a stream's own are never read
    for b, p in enumerate(planes):
        lp[b, : p.shape[0]] = p
    tab = np.concatenate([np.concatenate([g[k].view(np.int32) for k in TABLE_KEYS]) for g in graphs])
    ns = np.array([len(g["parent"]) for g in graphs], np.int32)
    vs, sts = [], []
    for b in range(B):
        blk = None if blocks is None else blocks[b]
        if blk is None:
            v64, s64 = fresh_state(int(ns[graph_of[b]]))
            blk = (v64.astype(np.float32), s64.astype(np.int32))
        vs.append(np.ascontiguousarray(blk[0], np.float32).reshape(-1))
        sts.append(np.ascontiguousarray(blk[1], np.int32).reshape(-1))
    v, st = np.concatenate(vs), np.concatenate(sts)
    ek = np.full((B, Tp), -7, np.int64)
    es, ee = np.full((B, Tp), -7, np.int32), np.full((B, Tp), -7, np.int32)
    em = np.full((B, Tp), np.nan, np.float32)
    n = np.full(B, -7, np.int32)
    debug_op(hip, "ctc_trie_dp", [B, Tp, len(graphs), V], [lp, nf, np.asarray(graph_of, np.int32), tab, ns, v, st, ek, es, ee, em, n],
             outs=(5, 6, 7, 8, 9, 10, 11))
    assert np.all((n >= 0) & (n <= nf)), n
    events = [[(int(ek[b, i]), int(es[b, i]), int(ee[b, i]), float(em[b, i])) for i in range(n[b])] for b in range(B)]
    out_v, out_st, o = [], [], 0
    for b in range(B):
        S = int(ns[graph_of[b]])
        out_v.append(v[o: o + 2 * S].reshape(2, S))
        out_st.append(st[o: o + 2 * S].reshape(2, S))
        o += 2 * S
    return events, out_v, out_st


def check_against_ref(graph, plane, block, got, what):
    ev, v, st = got
    wev, wv, ws = ref_dp(graph, plane, *(block if block is not None else (None, None)))
    assert ev == wev, (what, ev[:3], wev[:3])
    assert v.tobytes() == wv.tobytes() and st.tobytes() == ws.tobytes(), what
    return len(wev)


@pytest.mark.parametrize("V", GPU_V)
@pytest.mark.parametrize("S", GPU_S)
def test_dp_equals_the_host_reference_bit_for_bit(hip_ctc, S, V):
    """"ctc_trie_dp" on planes of multiples of 0.25 with -inf cells against csrc/ctc_kws_ref.h: events, sum_logp, counts and the whole
    carried block, S in {1, 2, 65, 257, 1024} x T in {1, 2, 15, 16, 17, 33, 64} (both sides of the 16-frame block) x V in {5, 37, 3000};
    the seven T of one (S, V) are seven streams of one call, each with a plane of its own; then every stream is resumed over its plane
    again from the block it ended with (frame counts, live cells and holds carried in)"""
    rng = np.random.default_rng(50 * S + V)
    graph = tables(random_trie(rng, S, V))
    planes = [random_plane(rng, T, V, graph["tok"]) for T in GPU_T]
    B = len(planes)
    ev, v, st = run_dp(hip_ctc, [graph], [0] * B, planes)
    fired = sum(check_against_ref(graph, planes[b], None, (ev[b], v[b], st[b]), (S, V, GPU_T[b])) for b in range(B))
    blocks = list(zip(v, st))
    ev2, v2, st2 = run_dp(hip_ctc, [graph], [0] * B, planes, blocks)
    fired += sum(check_against_ref(graph, planes[b], blocks[b], (ev2[b], v2[b], st2[b]), (S, V, GPU_T[b], "resumed")) for b in range(B))
    assert all(s[0, 0] == 2 * T for s, T in zip(st2, GPU_T))
    if S > 1:
        assert fired > 0


def test_hand_built_cases_on_the_device(hip_ctc):
    """the hand-built cases of tests/ctc_kws_cases.py (every tie, n == bar, several terminals in one frame, the reset, the hold and its
    release, rc = -1, a repeated token through b): their written-down events and cells, and the host reference bit for bit"""
    for case in hand_cases():
        B = len(case["streams"])
        blocks = case.get("blocks", [None] * B)
        ev, v, st = run_dp(hip_ctc, [case], [0] * B, case["streams"], blocks)
        for b in range(B):
            check_against_ref(case, case["streams"][b], blocks[b], (ev[b], v[b], st[b]), (case["name"], b))
            assert ev[b] == case["expect"][b], (case["name"], b, ev[b])
            for (pl, c), (x, s) in case.get("states", [{}] * (b + 1))[b].items():
                assert v[b][pl, c] == x and st[b][pl, c] == s, (case["name"], b, pl, c)


def test_mixed_streams_graphs_and_a_held_block(hip_ctc):
    """one call with three streams of different T, one of them with n_frames = 0, over two different graphs; and a resumed block whose
    hold is set: the one-token keyword's run goes on in the next call and stays silent, then a blank frame releases it"""
    rng = np.random.default_rng(77)
    g0, g1 = tables(random_trie(rng, 65, 37)), tables(random_trie(rng, 300, 37))
    planes = [random_plane(rng, T, 37, None) for T in (33, 20, 7)]
    v1, s1 = fresh_state(300)
    blocks = [None, (v1.astype(np.float32), s1.astype(np.int32)), None]
    blocks[1][0][0, 5], blocks[1][1][0, 5], blocks[1][1][0, 0] = -1.25, 3, 9    # some history for the stream that sits the call out
    ev, v, st = run_dp(hip_ctc, [g0, g1], [0, 1, 1], planes, blocks, n_frames=[33, 0, 7])
    assert ev[1] == [] and v[1].tobytes() == blocks[1][0].tobytes() and st[1].tobytes() == blocks[1][1].tobytes()
    check_against_ref(g0, planes[0], None, (ev[0], v[0], st[0]), "graph 0")
    check_against_ref(g1, planes[2], None, (ev[2], v[2], st[2]), "graph 1")
    assert len(ev[0]) + len(ev[2]) > 0
    # the hold across calls
    hold = next(c for c in hand_cases() if c["name"] == "hold")
    run = hold["streams"][1]   # A A blank A
    ev_a, v_a, st_a = run_dp(hip_ctc, [hold], [0], [run[:1]])
    assert ev_a[0] == [(0, 0, 0, -0.25)] and st_a[0][1, 0] == 1
    ev_b, v_b, st_b = run_dp(hip_ctc, [hold], [0], [run[1:]], [(v_a[0], st_a[0])])
    assert ev_b[0] == [(0, 3, 3, -0.25)]
    check_against_ref(hold, run[1:], (v_a[0], st_a[0]), (ev_b[0], v_b[0], st_b[0]), "held block")


def stream_view(s):
    v, st = s.state()
    return as_tuples(s.events()), v.tobytes(), st.tobytes(), s.num_frames()


CHUNKINGS = ([35], [16, 16, 3], [1] * 35, [7, 28])


def test_chunking_is_bit_identical(hip_ctc, device_log_probs, keywords24):
    """the engine's own log-probs of the fixture batch as chunk lists [35], [16,16,3], [1]*35 and [7,28]: events and carried blocks are
    bit-identical; also with streams joining and leaving between calls"""
    from k2transducerasr_amd import CtcKeywordStream
    lp = device_log_probs
    B, Tp, _ = lp.shape
    results = []
    for chunks in CHUNKINGS:
        assert sum(chunks) == Tp
        streams = [CtcKeywordStream(hip_ctc, keywords24) for _ in range(B)]
        t = 0
        for n in chunks:
            CtcKeywordStream.search_chunk(streams, lp[:, t: t + n])
            t += n
        results.append([stream_view(s) for s in streams])
        for s in streams:
            s.close()
    assert sum(len(r[0]) for r in results[0]) > 10 and all(r[3] == Tp for r in results[0])
    for r in results[1:]:
        assert r == results[0]
    # joining and leaving: stream 0 alone for 7 frames; 0, 1, 2 together for 9 (1 and 2 from their frame 0); 0 leaves, 1 and 2 go on with 3
    # joining; everyone finishes alone
    streams = [CtcKeywordStream(hip_ctc, keywords24) for _ in range(4)]
    CtcKeywordStream.search_chunk(streams[:1], lp[:1, :7])
    CtcKeywordStream.search_chunk(streams[:3], np.stack([lp[0, 7:16], lp[1, :9], lp[2, :9]]))
    CtcKeywordStream.search_chunk(streams[1:], np.stack([lp[1, 9:20], lp[2, 9:20], lp[3, :11]]))
    for b, done in enumerate((16, 20, 20, 11)):
        CtcKeywordStream.search_chunk([streams[b]], lp[b: b + 1, done:])
        assert stream_view(streams[b]) == results[0][b], b
        streams[b].close()


def test_end_to_end_against_the_reference_and_the_twin(hip_ctc, device_log_probs, keywords24, graph24):
    """Model.ctc_spot_keywords on the engine's log-probs = csrc/ctc_kws_ref.h on the same array bit for bit (events, sum_logp, score); the
    array clears the decision bound of tests/test_ctc_kws.py, so (keyword, start, end) also equal the float64 twin's"""
    lp = device_log_probs
    got = hip_ctc.ctc_spot_keywords(lp, keywords24)
    twin, gaps, held, top = fixture_run(lp)
    ratio = min(gaps) / F32_BOUND
    print(f"engine log-probs: {sum(len(e) for e in twin)} events, {held} frames closed by the hold, smallest gap {min(gaps):.3g} = {ratio:.1f} x the bound")
    assert top <= MAX_SUM and ratio >= MIN_RATIO
    assert sum(len(e) for e in twin) > 10 and held > 0
    for b in range(lp.shape[0]):
        wev, _, _ = ref_dp(graph24, lp[b])
        assert as_tuples(got[b]) == wev, b
        assert [e[:3] for e in wev] == [e[:3] for e in twin[b]], b
        for e in got[b]:
            assert e["score"] == np.float32(e["sum_logp"]) / np.float32(len(KEYWORDS[e["keyword"]]))


def test_fused_route_equals_ctc_spot_keywords_on_the_engines_frames(hip_ctc, utts, device_log_probs, keywords24, tmp_path):
    want = [as_tuples(ev) for ev in hip_ctc.ctc_spot_keywords(device_log_probs, keywords24)]
    assert sum(len(w) for w in want) > 10
    assert [as_tuples(ev) for ev in hip_ctc.ctc_spot_keywords_samples(utts, keywords24)] == want
    from k2transducerasr_amd import K2HipError, OfflineRecognizer
    from k2transducerasr_amd.synth import write_synthetic_model
    p = str(tmp_path / "ctc.k2w")
    write_synthetic_model(p, "zipformer2-ctc-tiny-test")
    rec = OfflineRecognizer(p)
    try:
        assert [as_tuples(ev) for ev in rec.spot_keywords(utts, keywords24)] == want
    finally:
        rec.model.close()
    with pytest.raises(K2HipError) as e:   # the capacity rule
        hip_ctc.ctc_spot_keywords_samples(utts, keywords24, max_events=1)
    assert e.value.code == -5 and "max_events" in str(e.value)
    assert [as_tuples(ev) for ev in hip_ctc.ctc_spot_keywords_samples(utts, keywords24)] == want


def test_refusals_leave_everything_usable(hip_ctc, hip_tiny, device_log_probs, keywords24, utts, tmp_path):
    from k2transducerasr_amd import CtcKeywordStream, K2HipError, Keywords, KeywordStream, Model
    from k2transducerasr_amd.synth import write_synthetic_model
    lp = device_log_probs
    ref = [as_tuples(ev) for ev in hip_ctc.ctc_spot_keywords(lp, keywords24)]
    # a transducer model is refused by every new entry
    tkw = Keywords([[5]], 0.5, hip_tiny.vocab_size)
    with pytest.raises(K2HipError) as e:
        CtcKeywordStream(hip_tiny, tkw)
    assert e.value.code == -6 and "CTC" in str(e.value)
    with pytest.raises(K2HipError) as e:
        hip_tiny.ctc_spot_keywords_samples(utts[:1], tkw)
    assert e.value.code == -6
    s = CtcKeywordStream(hip_ctc, keywords24)
    CtcKeywordStream.search_chunk([s], lp[:1, :9])
    before = stream_view(s)
    import ctypes as C
    arr = (C.c_void_p * 1)(s._h.value)
    x = np.zeros((1, 4, hip_tiny.vocab_size), np.float32)
    rc = hip_tiny._L.k2hip_ctc_kws_search_chunk(hip_tiny.handle, arr, 1, x.ctypes.data_as(C.POINTER(C.c_float)), 4, None)
    assert rc == -6 and stream_view(s) == before
    # a CTC model is still refused by the old entries
    with pytest.raises(K2HipError) as e:
        KeywordStream(hip_ctc, keywords24)
    assert e.value.code == -6 and "CTC" in str(e.value)
    with pytest.raises(K2HipError) as e:
        hip_ctc.spot_keywords_samples(utts[:1], keywords24)
    assert e.value.code == -6
    # a graph of another vocabulary size
    with pytest.raises(K2HipError) as e:
        CtcKeywordStream(hip_ctc, Keywords([[5]], 0.5, hip_ctc.vocab_size + 1))
    assert e.value.code == -1 and "vocab_size" in str(e.value)
    # a stream of another model
    p = str(tmp_path / "ctc2.k2w")
    write_synthetic_model(p, "zipformer2-ctc-tiny-test")
    m2 = Model(p, 0)
    foreign = CtcKeywordStream(m2, keywords24)
    s2 = CtcKeywordStream(hip_ctc, keywords24)
    before2 = stream_view(s2)
    bad_calls = (lambda: CtcKeywordStream.search_chunk([s, foreign], lp[:2, :4]),        # another model's stream
                 lambda: CtcKeywordStream.search_chunk([s, s2, s], lp[:3, :4]),          # a stream twice
                 lambda: CtcKeywordStream.search_chunk([s, s2], lp[:2, :4], [4, 5]),      # n_frames outside [0, Tc]
                 lambda: CtcKeywordStream.search_chunk([s, s2], lp[:2, :4], [-1, 4]),
                 lambda: CtcKeywordStream.search_chunk([s, s2], lp[:2, :0]))             # Tc = 0
    for fn in bad_calls:
        with pytest.raises(K2HipError) as e:
            fn()
        assert e.value.code == -1
        assert stream_view(s) == before and stream_view(s2) == before2 and foreign.num_frames() == 0
        CtcKeywordStream.search_chunk([s, s2], lp[:2, :4], [0, 0])   # a valid call behind it: it moves nothing
        assert stream_view(s) == before and stream_view(s2) == before2
    CtcKeywordStream.search_chunk([s, s2], np.stack([lp[0, 9:], lp[1, :26]]))
    CtcKeywordStream.search_chunk([s2], lp[1:2, 26:])
    assert stream_view(s)[0] == ref[0] and stream_view(s2)[0] == ref[1]
    for x in (s, s2, foreign):
        x.close()
    m2.close()
    # a graph destroyed after the stream's creation: the stream keeps its own reference and works
    gone = Keywords(KEYWORDS, THRESHOLDS, hip_ctc.vocab_size)
    s = CtcKeywordStream(hip_ctc, gone)
    gone.close()
    CtcKeywordStream.search_chunk([s], lp[2:3])
    assert as_tuples(s.events()) == ref[2]
    s.reset()
    assert s.num_frames() == 0 and s.events() == [] and np.all(s.state()[0][:, 1:] == -np.inf) and s.state()[1][1, 0] == -1
    CtcKeywordStream.search_chunk([s], lp[2:3])
    assert as_tuples(s.events(clear=True)) == ref[2] and s.events() == []
    s.close()
    # zero keywords: legal, never fires
    s = CtcKeywordStream(hip_ctc, Keywords([], 0.5, hip_ctc.vocab_size))
    CtcKeywordStream.search_chunk([s], lp[:1])
    assert s.events() == [] and s.num_frames() == 35
    s.close()
    assert [as_tuples(ev) for ev in hip_ctc.ctc_spot_keywords(lp, keywords24)] == ref


def test_spotting_changes_no_search(hip_ctc, device_log_probs, keywords24):
    """CTC greedy and prefix-beam results of the same model are identical before and after a keyword call on the same handle"""
    lp = device_log_probs
    greedy0 = hip_ctc.ctc_greedy(lp)
    beam0, sc0 = hip_ctc.ctc_prefix_beam_search(lp, 4, want_scores=True)
    assert sum(len(ev) for ev in hip_ctc.ctc_spot_keywords(lp, keywords24)) > 0
    greedy1 = hip_ctc.ctc_greedy(lp)
    beam1, sc1 = hip_ctc.ctc_prefix_beam_search(lp, 4, want_scores=True)
    assert repr(greedy1) == repr(greedy0) and repr(beam1) == repr(beam0) and np.array_equal(sc0, sc1)
