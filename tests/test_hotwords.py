"""Hotword biasing without a GPU: the host graph of libk2hip.so (k2hip_hotwords_*) against hand-derived walks and against the Python
twin (tests/hotword_twin.py), the hotwords file loader, and the twin's own self-checks on the CPU oracle -- with c = 0 and with an
empty list it must equal oracle.modified_beam_search exactly on every committed case the GPU tests compare the engine with."""
import numpy as np
import pytest

from hotword_twin import (KAT_FLIP, SCORE, TINY_BEAMS, WIDE_BEAMS, WIDE_VOCAB, TwinGraph, draw_phrases, icefall_modified_beam_search,
                          kat_flip_score, tiny_phrases, twin_batch, twin_beam_search, wide_enc, wide_phrases)
from kat_model import frames, write_kat_model, write_wide_model


def _walk(hw, tokens, state=0):
    out = []
    for t in tokens:
        state, b = hw.step(state, t)
        out.append(float(b))
    return out, state


def test_graph_known_answers():
    from k2transducerasr_amd import Hotwords
    hw = Hotwords([[5, 6, 7], [6, 8]], 1.5, 20)
    assert hw.num_states == 6                      # root, 5, 56, 567, 6, 68
    # 5, 6, 8: the failure link from state "5 6" to state "6" is taken, then [6, 8] is committed: +3.0 in all, back at the root
    assert _walk(hw, [5, 6, 8]) == ([1.5, 1.5, 0.0], 0)
    # 5, 6, 9: the partial match breaks and gives its bonus back
    assert _walk(hw, [5, 6, 9]) == ([1.5, 1.5, -3.0], 0)
    assert _walk(hw, [5, 6, 7]) == ([1.5, 1.5, 1.5], 0)
    # blank and unk leave the state alone
    b, s = _walk(hw, [5, 0, 2, 6])
    assert b == [1.5, 0.0, 0.0, 1.5] and s != 0 and float(hw.pending(s)) == 3.0
    assert float(hw.pending(0)) == 0.0
    # an empty list is a graph of the root alone
    e = Hotwords([], 1.5, 20)
    assert e.num_states == 1 and _walk(e, [5, 6, 7]) == ([0.0, 0.0, 0.0], 0)


@pytest.mark.parametrize("phrases, score, vocab, named", [
    ([[5, 6], []], 1.5, 20, "phrase 1 is empty"),
    ([[5, 20]], 1.5, 20, "phrase 0"),
    ([[5, -1]], 1.5, 20, "phrase 0"),
    ([[4], [5, 0]], 1.5, 20, "phrase 1 contains blank"),
    ([[5, 2, 6]], 1.5, 20, "phrase 0 contains unk"),
    ([[5, 6], [7], [5, 6, 7]], 1.5, 20, "phrase 0 is a proper prefix of phrase 2"),
    ([[5, 6, 7], [5, 6]], 1.5, 20, "phrase 1 is a proper prefix of phrase 0"),
    ([[5, 6], [7, 8], [5, 6]], 1.5, 20, "phrase 2 duplicates phrase 0"),
    ([[5, 6]], -1.0, 20, "score_per_token"),
    ([[5, 6]], float("nan"), 20, "score_per_token"),
    ([[5, 6]], float("inf"), 20, "score_per_token"),
])
def test_graph_rejections(phrases, score, vocab, named):
    from k2transducerasr_amd import Hotwords, K2HipError
    with pytest.raises(K2HipError) as e:
        Hotwords(phrases, score, vocab)
    assert e.value.code == -1 and named in str(e.value), str(e.value)


def test_graph_size_cap():
    """the device form is dense: states x vocab_size may not exceed K2HIP_HOTWORDS_MAX_ENTRIES (1 << 23)"""
    from k2transducerasr_amd import Hotwords, K2HipError
    V = 1 << 20
    ok = Hotwords([[10 + i, 3] for i in range(3)], 1.0, V)      # 7 states
    assert ok.num_states == 7
    with pytest.raises(K2HipError) as e:
        Hotwords([[10 + i, 3] for i in range(4)], 1.0, V)       # the 9th state would pass 8 x 2^20
    assert e.value.code == -1 and "phrase 3" in str(e.value) and "entries" in str(e.value)


def test_graph_equals_the_twin_on_random_walks():
    """k2hip_hotwords_step / _pending against the twin's graph, bit for bit (c = 1.5: every sum is a small multiple of it)"""
    from k2transducerasr_amd import Hotwords
    rng = np.random.default_rng(2024)
    pairs = 0
    for trial in range(300):
        V = int(rng.integers(5, 12))
        c = float(rng.choice([0.0, 0.5, 1.5, 2.25]))
        cand = [[int(x) for x in rng.choice([v for v in range(V) if v not in (0, 2)], size=int(rng.integers(1, 5)))] for _ in range(8)]
        phrases = []
        for p in cand:   # a legal set: no duplicates, nobody a prefix of another
            if not any(p[: len(q)] == q or q[: len(p)] == p for q in phrases):
                phrases.append(p)
        hw, tw = Hotwords(phrases, c, V), TwinGraph(phrases, c, V)
        assert hw.num_states == tw.num_states
        for s in range(tw.num_states):
            assert hw.pending(s).tobytes() == tw.pending(s).tobytes()
        for walk in range(10):
            s = 0
            for v in rng.integers(0, V, size=12):
                n, b = hw.step(s, int(v))
                n2, b2, _ = tw.step(s, int(v))
                assert (n, b.tobytes()) == (n2, b2.tobytes()), (phrases, s, v)
                s = n
            pairs += 1
    assert pairs == 3000


def test_hotwords_file(tmp_path):
    from k2transducerasr_amd import Hotwords, K2HipError, TokenTable
    syms = ["<blk>", "<sos/eos>", "<unk>", "▁HE", "LL", "O", "▁WOR", "LD"]
    tok = tmp_path / "tokens.txt"
    tok.write_text("".join(f"{s} {i}\n" for i, s in enumerate(syms)), encoding="utf-8")
    table = TokenTable(str(tok))
    f = tmp_path / "hotwords.txt"
    f.write_text("▁HE LL O\n\n  ▁WOR   LD \n", encoding="utf-8")
    hw = Hotwords.load(table, str(f), 2.0)
    assert hw.num_states == 6
    assert _walk(hw, [3, 4, 5]) == ([2.0, 2.0, 2.0], 0) and _walk(hw, [6, 7]) == ([2.0, 2.0], 0)
    f.write_text("▁HE LL O\n▁WOR LDS\n", encoding="utf-8")
    with pytest.raises(K2HipError) as e:
        Hotwords.load(table, str(f), 2.0)
    assert e.value.code == -1 and "line 2" in str(e.value) and "LDS" in str(e.value)
    f.write_text("▁HE LL\n\n▁HE LL O\n", encoding="utf-8")
    with pytest.raises(K2HipError) as e:
        Hotwords.load(table, str(f), 2.0)
    assert e.value.code == -1 and "line 1 is a proper prefix of line 3" in str(e.value)
    f.write_text("▁HE <unk>\n", encoding="utf-8")
    with pytest.raises(K2HipError) as e:
        Hotwords.load(table, str(f), 2.0)
    assert "line 1 contains unk" in str(e.value)
    with pytest.raises(K2HipError) as e:
        Hotwords.load(table, str(tmp_path / "missing.txt"), 2.0)
    assert e.value.code == -2


def test_null_arguments_are_errors():
    import ctypes as C
    from k2transducerasr_amd import load_library
    L = load_library()
    assert L.k2hip_hotwords_create(None, None, 0, C.c_float(1.0), 20, None) == -1
    assert L.k2hip_hotwords_num_states(None) == -1
    assert L.k2hip_hotwords_destroy(None) == 0
    L.k2hip_set_hotwords.argtypes = [C.c_void_p, C.c_void_p]
    assert L.k2hip_set_hotwords(None, None) == -1


# ---- the twin on the CPU oracle ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def enc_tiny(oracle_tiny, utts):
    f = [oracle_tiny.fbank(u) for u in utts]
    return oracle_tiny.encoder(oracle_tiny.pad_sequence(f).reshape(len(utts), -1, 80))


@pytest.fixture(scope="module")
def wide_oracle(tmp_path_factory):
    from oracle import Oracle
    p = str(tmp_path_factory.mktemp("hw_wide") / "wide.k2w")
    write_wide_model(p, WIDE_VOCAB)
    return Oracle(p)


def _twin_is_the_oracle(ora, enc, beam, phrases):
    want, mg, sc, tr = ora.modified_beam_search(enc, beam, want_margins=True, want_scores=True, want_trace=True)
    V = ora.vocab_size
    for what, graph in (("no graph", None), ("empty list", TwinGraph([], SCORE, V)), ("c = 0", TwinGraph(phrases, 0.0, V))):
        got, gsc, gmg, gtr, ev = twin_batch(ora, enc, beam, graph)
        assert got == want, what                       # exactly: no near-tie excuse on the committed cases
        np.testing.assert_allclose(gsc, sc, atol=1e-4, rtol=0)
        assert (gtr["idx"] == tr["idx"]).all() and (gtr["n"] == tr["n"]).all(), what    # the same selection on every frame
        assert ev["bonus"] == 0 and ev["broken"] == 0      # (c = 0 still walks the graph and commits: it only earns nothing)
    for b in range(enc.shape[0]):                      # and the function it extends
        ys, ts, lp = icefall_modified_beam_search(ora, enc[b], beam)
        assert (ys, ts) == want[b]
    return want


@pytest.mark.parametrize("beam", TINY_BEAMS)
def test_twin_equals_oracle_unbiased_tiny(oracle_tiny, enc_tiny, beam):
    want = oracle_tiny.modified_beam_search(enc_tiny, beam)
    phrases = tiny_phrases(want)
    assert len(phrases) >= 3
    _twin_is_the_oracle(oracle_tiny, enc_tiny, beam, phrases)
    # biased: bonuses, broken matches and committed matches all occur on these cases, and results move
    got, _, _, _, ev = twin_batch(oracle_tiny, enc_tiny, beam, TwinGraph(phrases, SCORE, oracle_tiny.vocab_size))
    assert min(ev.values()) >= 1, ev
    assert got != want


@pytest.mark.parametrize("beam", WIDE_BEAMS)
def test_twin_equals_oracle_unbiased_wide(wide_oracle, beam):
    enc = wide_enc()
    want = wide_oracle.modified_beam_search(enc, beam)
    phrases = wide_phrases(want)
    assert len(phrases) >= 6
    _twin_is_the_oracle(wide_oracle, enc, beam, phrases)
    got, _, _, _, ev = twin_batch(wide_oracle, enc, beam, TwinGraph(phrases, SCORE, WIDE_VOCAB))
    assert min(ev.values()) >= 1, ev
    assert got != want


def test_twin_kat_flip(tmp_path):
    """hotword_twin.KAT_FLIP: token 5 against a slightly better 6, the phrase [5, 7] flips the result (derivation there)"""
    from oracle import Oracle
    p = str(tmp_path / "kat.k2w")
    write_kat_model(p)
    ora = Oracle(p)
    enc = frames(KAT_FLIP["rows"])
    plain = twin_beam_search(ora, enc, KAT_FLIP["beam"])
    assert (plain["ys"], plain["ts"]) == KAT_FLIP["unbiased"] == ora.modified_beam_search(enc[None], KAT_FLIP["beam"])[0]
    r = twin_beam_search(ora, enc, KAT_FLIP["beam"], TwinGraph(KAT_FLIP["phrases"], SCORE, 8))
    assert (r["ys"], r["ts"]) == KAT_FLIP["biased"]
    assert r["events"] == dict(bonus=2, broken=0, committed=1)
    assert abs(r["lp"] - kat_flip_score()) < 1e-5
    # an unfinished match earns nothing: without the frame that offers 7 the bonus of [5] is taken back and 6 wins again
    cut = twin_beam_search(ora, frames([KAT_FLIP["rows"][0], KAT_FLIP["rows"][2]]), KAT_FLIP["beam"], TwinGraph(KAT_FLIP["phrases"], SCORE, 8))
    assert cut["ys"] == [6]
