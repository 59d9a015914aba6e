"""Keyword spotting on the GPU (csrc/kws.hip through the k2hip_kws_* entries, k2hip_offline_spot_keywords_from_samples and the two debug
ops), against the float64 twin (tests/kws_twin.py) and the float32 host reference (csrc/kws_ref.h).

Bounds (none of them taken from what the engine gives):
  * a cell (stay / emit, a log-softmax value): CELL_TOL = 2e-4, the bound of tests/test_align_gpu.py;
  * the token passing on planes whose values are multiples of 0.25: sums along a path are exact in float32, so events, sum_logp and the
    carried block equal the host reference bit for bit;
  * end to end: tests/test_kws.py shows from the twin alone that every decision an event depends on clears its error bound at least 10
    times on this input, so every (keyword, start, end) equals the twin's, and sum_logp, a sum of end - start + 1 cells, is within
    (end - start + 1) * CELL_TOL;
  * chunking: bit-identical events and carried blocks, whatever the chunk list;
  * the fused route scores the DEVICE encoder's frames: against spot_keywords on the engine's own encoder_proj output the events are equal
    and sum_logp agrees within the relative bound tests/test_align_gpu.py uses for the fused route."""
import numpy as np
import pytest

from kws_cases import KEYWORDS, THRESHOLD, hand_cases, random_cases, wide_keywords
from kws_twin import build_trie, fresh_state, token_passing, trie_cells
from test_align_gpu import CELL_TOL, debug_op, fused_score_ok
from test_kws import ref_dp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def enc_tiny(oracle_tiny, utts):
    f = [oracle_tiny.fbank(u) for u in utts]
    return oracle_tiny.encoder(oracle_tiny.pad_sequence(f).reshape(len(utts), -1, 80))


@pytest.fixture(scope="module")
def wide_pair(tmp_path_factory):
    """the tiny preset with a vocabulary of 3000 (as tests/test_align_gpu.py)"""
    from k2transducerasr_amd import Model
    from k2transducerasr_amd.synth import write_synthetic_model
    from oracle import Oracle
    p = str(tmp_path_factory.mktemp("kws") / "wide.k2w")
    write_synthetic_model(p, "zipformer2-tiny-test", blank_bias=2.4, meta_overrides={"vocab_size": "3000"})
    return Model(p, 0), Oracle(p)


@pytest.fixture(scope="module")
def keywords18(hip_tiny):
    from k2transducerasr_amd import Keywords
    return Keywords(KEYWORDS, THRESHOLD, hip_tiny.vocab_size)


@pytest.fixture(scope="module")
def twin_events(oracle_tiny, enc_tiny):
    """the twin over the whole fixture, once: per stream (events, cells)"""
    trie = build_trie(KEYWORDS, THRESHOLD)
    out = []
    for b in range(enc_tiny.shape[0]):
        stay, emit = trie_cells(oracle_tiny, enc_tiny[b], trie)
        out.append((token_passing(trie, stay, emit)[0], stay, emit))
    return trie, out


def as_tuples(events):
    return [(e["keyword"], e["start"], e["end"], float(e["sum_logp"])) for e in events]


CELL_FRAMES = ([1, 16, 33], [35, 1, 16])   # three streams per call: strip edges (strips of 32 frames), a streaming chunk, one frame


@pytest.mark.parametrize("which", ["tiny", "conformer", "wide"])
def test_cells_against_the_twin(which, request):
    """"trie_logprobs" into NaN-prefilled planes: every cell of every frame and state is written and within CELL_TOL of the twin's"""
    if which == "tiny":
        hip, ora, words = request.getfixturevalue("hip_tiny"), request.getfixturevalue("oracle_tiny"), KEYWORDS
        assert hip.vocab_size == 37
    elif which == "conformer":
        hip, ora, words = request.getfixturevalue("hip_conformer"), request.getfixturevalue("oracle_conformer"), KEYWORDS
        assert hip.vocab_size == 41
    else:
        hip, ora = request.getfixturevalue("wide_pair")
        words = wide_keywords()
        assert hip.vocab_size == 3000
    trie = build_trie(words, 0.5)
    S, J = len(trie["parent"]), hip.joiner_dim
    assert S == 18 or len(trie["children"][0]) == 70
    ids = np.array([t for w in words for t in w], np.int64)
    lens = np.array([len(w) for w in words], np.int32)
    thr = np.full(len(words), 0.5, np.float32)
    worst = 0.0
    for call, frames in enumerate(CELL_FRAMES):
        B, Tp = len(frames), max(frames)
        nf = np.array(frames, np.int32)
        enc = np.random.default_rng(5 + call).standard_normal((B, Tp, J)).astype(np.float32)
        total = int(nf.sum()) * S
        stay = np.full(total, np.nan, np.float32)
        emit = np.full(total, np.nan, np.float32)
        debug_op(hip, "trie_logprobs", [B, Tp, len(words)], [enc, nf, ids, lens, thr, stay, emit], outs=(5, 6))
        o = 0
        for b, T in enumerate(frames):
            ws, we = trie_cells(ora, enc[b, :T], trie)
            gs, ge = stay[o: o + T * S].reshape(T, S), emit[o: o + T * S].reshape(T, S)
            o += T * S
            assert not np.isnan(gs).any() and not np.isnan(ge).any(), (which, call, b)
            assert np.all(ge[:, 0] == -np.inf)
            ds, de = float(np.abs(gs - ws).max()), float(np.abs(ge[:, 1:] - we[:, 1:]).max())
            worst = max(worst, ds, de)
            assert ds <= CELL_TOL and de <= CELL_TOL, (which, call, b, T, ds, de)
    print(f"trie_logprobs {which}: worst cell difference {worst:.3g} (bound {CELL_TOL:g})")


def run_dp(hip, case, a=None, start=None):
    streams = case["streams"]
    B, S = len(streams), len(case["parent"])
    nf = np.array([s.shape[0] for s, _ in streams], np.int32)
    Tp = int(nf.max())
    stay = np.concatenate([s.reshape(-1) for s, _ in streams]).astype(np.float32)
    emit = np.concatenate([e.reshape(-1) for _, e in streams]).astype(np.float32)
    if a is None:
        a64, s64 = fresh_state(S)
        a, start = np.tile(a64.astype(np.float32), (B, 1)), np.tile(s64.astype(np.int32), (B, 1))
    a, start = np.ascontiguousarray(a.copy()), np.ascontiguousarray(start.copy())
    ek = np.full((B, Tp), -7, np.int64)
    es, ee = np.full((B, Tp), -7, np.int32), np.full((B, Tp), -7, np.int32)
    em = np.full((B, Tp), -7, np.float32)
    n = np.full(B, -7, np.int32)
    debug_op(hip, "trie_dp", [B, Tp, S], [nf, case["parent"], case["depth"], case["kw"], case["bar"], stay, emit, a, start, ek, es, ee, em, n],
             outs=(7, 8, 9, 10, 11, 12, 13))
    events = [[(int(ek[b, i]), int(es[b, i]), int(ee[b, i]), float(em[b, i])) for i in range(n[b])] for b in range(B)]
    return events, a, start


def test_dp_equals_the_host_reference_bit_for_bit(hip_tiny):
    """"trie_dp" on planes of multiples of 0.25 with -inf cells against csrc/kws_ref.h: events, sum_logp and the carried block, for S in
    {1, 2, 65, 257, 1024} x T in {1, 2, 64} and chains deeper than T; the hand-built cases (an exact ve == vs tie, a == bar, two and three
    terminals in one frame, the reset) also against their written-down answers; and a second call that resumes from the first one's
    carried block"""
    fired = 0
    for case in hand_cases() + random_cases():
        events, a, start = run_dp(hip_tiny, case)
        want = [ref_dp(case["parent"], case["depth"], case["kw"], case["bar"], s, e) for s, e in case["streams"]]
        for b, (wev, wa, ws) in enumerate(want):
            assert events[b] == wev, (case["name"], b, events[b][:3], wev[:3])
            assert a[b].tobytes() == wa.tobytes() and start[b].tobytes() == ws.tobytes(), (case["name"], b)
            fired += len(wev)
            if "expect" in case:
                assert events[b] == case["expect"][b], (b, events[b])
                for c, (va, vs) in case["states"][b].items():
                    assert a[b, c] == va and start[b, c] == vs, (b, c)
        if case["name"].startswith("chain"):   # resumed: the same planes again behind the carried block
            events2, a2, start2 = run_dp(hip_tiny, case, a, start)
            for b, (s, e) in enumerate(case["streams"]):
                wev, wa, ws = ref_dp(case["parent"], case["depth"], case["kw"], case["bar"], s, e, want[b][1], want[b][2])
                assert events2[b] == wev and a2[b].tobytes() == wa.tobytes() and start2[b].tobytes() == ws.tobytes(), (case["name"], b)
    assert fired > 100


def test_end_to_end_against_the_twin(hip_tiny, enc_tiny, keywords18, twin_events):
    """Model.spot_keywords on the oracle's encoder_out of the `utts` fixture (5 streams x 35 frames), the 18-state set, threshold
    exp(-2.45): every (keyword, start, end) equals the twin's and sum_logp is within (end - start + 1) * CELL_TOL.  Nothing is excused.
    On this random model no winning path contains a stay arc (end - start + 1 is the keyword's length for every event); stays are
    covered by test_dp_equals_the_host_reference_bit_for_bit."""
    _, twin = twin_events
    got = hip_tiny.spot_keywords(enc_tiny, keywords18)
    assert sum(len(ev) for ev, _, _ in twin) == 17
    worst = 0.0
    for b, (wev, _, _) in enumerate(twin):
        g = as_tuples(got[b])
        assert [e[:3] for e in g] == [e[:3] for e in wev], (b, g, wev)
        for (k, s, e, v), (_, _, _, wv), full in zip(g, wev, got[b]):
            worst = max(worst, abs(v - wv) / (e - s + 1))
            assert abs(v - wv) <= (e - s + 1) * CELL_TOL, (b, k, s, e, v, wv)
            assert full["score"] == np.float32(full["sum_logp"]) / np.float32(len(KEYWORDS[k]))
    print(f"spot_keywords against the twin: 17 events, worst sum_logp difference per arc {worst:.3g} (bound {CELL_TOL:g})")


CHUNKINGS = ([1] * 35, [3] * 11 + [2], [16, 16, 3], [35])


def test_chunking_is_bit_identical(hip_tiny, enc_tiny, keywords18):
    """the same input as chunk lists [1]*35, [3]*11 + [2], [16,16,3] and [35]: events and the carried block are bit-identical; then one
    call that mixes two graphs and n_frames [35, 0, 20, 35, 7]: the stream with 0 is unchanged, the others equal a run of their own"""
    from k2transducerasr_amd import Keywords, KeywordStream
    B, Tp, _ = enc_tiny.shape
    assert Tp == 35 and B == 5
    results = []
    for chunks in CHUNKINGS:
        assert sum(chunks) == Tp
        streams = [KeywordStream(hip_tiny, keywords18) for _ in range(B)]
        t = 0
        for n in chunks:
            KeywordStream.search_chunk(streams, enc_tiny[:, t: t + n])
            t += n
        assert all(s.num_frames() == Tp for s in streams)
        results.append([(as_tuples(s.events()), s.state()[0].tobytes(), s.state()[1].tobytes()) for s in streams])
        for s in streams:
            s.close()
    assert sum(len(r[0]) for r in results[0]) == 17
    for r in results[1:]:
        assert r == results[0]
    # two graphs in one call, per-stream frame counts, a stream that sits the call out
    other = Keywords([[35], [23, 7], [33]], 0.2, hip_tiny.vocab_size)
    graphs = [keywords18, other, other, keywords18, other]
    nf = [35, 0, 20, 35, 7]
    streams = [KeywordStream(hip_tiny, g) for g in graphs]
    KeywordStream.search_chunk(streams[1:2], enc_tiny[1:2, :5])     # some history for the stream that will sit out
    before = (as_tuples(streams[1].events()), streams[1].state()[0].tobytes(), streams[1].state()[1].tobytes(), streams[1].num_frames())
    KeywordStream.search_chunk(streams, enc_tiny, nf)
    assert (as_tuples(streams[1].events()), streams[1].state()[0].tobytes(), streams[1].state()[1].tobytes(), streams[1].num_frames()) == before
    for b in (0, 2, 3, 4):
        alone = KeywordStream(hip_tiny, graphs[b])
        KeywordStream.search_chunk([alone], enc_tiny[b: b + 1, : nf[b]])
        assert streams[b].num_frames() == nf[b]
        assert as_tuples(streams[b].events()) == as_tuples(alone.events()), b
        assert streams[b].state()[0].tobytes() == alone.state()[0].tobytes() and streams[b].state()[1].tobytes() == alone.state()[1].tobytes(), b
        alone.close()
    assert as_tuples(streams[0].events()) == results[0][0][0] and as_tuples(streams[3].events()) == results[0][3][0]
    # reset: frame count 0, no tokens, no events -- and the same events again
    streams[0].reset()
    assert streams[0].num_frames() == 0 and streams[0].events() == [] and np.all(streams[0].state()[0][1:] == -np.inf)
    KeywordStream.search_chunk(streams[:1], enc_tiny[:1])
    assert as_tuples(streams[0].events()) == results[0][0][0]
    for s in streams:
        s.close()


def test_fused_route_equals_spot_keywords_on_the_engines_frames(hip_tiny, utts, keywords18):
    feats = [hip_tiny.fbank(u) for u in utts]
    enc = hip_tiny.encoder_proj(hip_tiny.pad_sequence(feats).reshape(len(utts), -1, 80))
    want = hip_tiny.spot_keywords(enc, keywords18)
    got = hip_tiny.spot_keywords_samples(utts, keywords18)
    assert sum(len(w) for w in want) > 0
    for b, (g, w) in enumerate(zip(got, want)):
        assert [(e["keyword"], e["start"], e["end"]) for e in g] == [(e["keyword"], e["start"], e["end"]) for e in w], b
        assert all(fused_score_ok(float(x["sum_logp"]), float(y["sum_logp"])) for x, y in zip(g, w)), (b, g, w)
    from k2transducerasr_amd import OfflineRecognizer   # the recognizer's method is the same call
    assert OfflineRecognizer.spot_keywords is not None


def test_errors_leave_everything_usable(hip_tiny, enc_tiny, utts, keywords18, tmp_path):
    from k2transducerasr_amd import K2HipError, Keywords, KeywordStream, Model
    from k2transducerasr_amd.synth import write_synthetic_model
    ref = [as_tuples(ev) for ev in hip_tiny.spot_keywords(enc_tiny, keywords18)]
    # a CTC model
    p = str(tmp_path / "ctc.k2w")
    write_synthetic_model(p, "zipformer2-ctc-tiny-test")
    ctc = Model(p, 0)
    try:
        ckw = Keywords([[5]], 0.5, ctc.vocab_size)
        with pytest.raises(K2HipError) as e:
            KeywordStream(ctc, ckw)
        assert e.value.code == -6 and "CTC" in str(e.value)
        with pytest.raises(K2HipError) as e:
            ctc.spot_keywords_samples(utts[:1], ckw)
        assert e.value.code == -6 and "CTC" in str(e.value)
    finally:
        ctc.close()
    # a vocab mismatch
    with pytest.raises(K2HipError) as e:
        KeywordStream(hip_tiny, Keywords([[5]], 0.5, hip_tiny.vocab_size + 1))
    assert e.value.code == -1 and "vocab_size" in str(e.value)
    # Tc = 0 and a bad n_frames change no stream
    s = KeywordStream(hip_tiny, keywords18)
    KeywordStream.search_chunk([s], enc_tiny[:1, :9])
    before = (as_tuples(s.events()), s.state()[0].tobytes(), s.state()[1].tobytes())
    for fn in (lambda: KeywordStream.search_chunk([s], enc_tiny[:1, :0]), lambda: KeywordStream.search_chunk([s], enc_tiny[:1, :4], [5]),
               lambda: KeywordStream.search_chunk([s, s], enc_tiny[:2, :4])):
        with pytest.raises(K2HipError) as e:
            fn()
        assert e.value.code == -1
        assert (as_tuples(s.events()), s.state()[0].tobytes(), s.state()[1].tobytes()) == before
    KeywordStream.search_chunk([s], enc_tiny[:1, 9:])
    assert as_tuples(s.events()) == ref[0]
    s.close()
    # a graph destroyed after the stream's creation: the stream keeps its own reference and works
    gone = Keywords(KEYWORDS, THRESHOLD, hip_tiny.vocab_size)
    s = KeywordStream(hip_tiny, gone)
    gone.close()
    KeywordStream.search_chunk([s], enc_tiny[2:3])
    assert as_tuples(s.events()) == ref[2]
    s.close()
    # zero keywords: legal, never fires
    s = KeywordStream(hip_tiny, Keywords([], 0.5, hip_tiny.vocab_size))
    KeywordStream.search_chunk([s], enc_tiny[:1])
    assert s.events() == [] and s.num_frames() == 35
    s.close()
    assert [as_tuples(ev) for ev in hip_tiny.spot_keywords(enc_tiny, keywords18)] == ref


def test_spotting_changes_no_search(hip_tiny, enc_tiny, keywords18):
    """a greedy call and a beam-4 call give identical results before and after a keyword call on the same handle"""
    greedy0 = hip_tiny.greedy_batch(enc_tiny)
    beam0, sc0 = hip_tiny.beam_search(enc_tiny, 4, want_scores=True)
    hip_tiny.spot_keywords(enc_tiny, keywords18)
    assert hip_tiny.greedy_batch(enc_tiny) == greedy0
    beam1, sc1 = hip_tiny.beam_search(enc_tiny, 4, want_scores=True)
    assert beam1 == beam0 and np.array_equal(sc0, sc1)
