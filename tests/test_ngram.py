"""N-gram LM shallow fusion without a GPU: the host automaton of libk2hip.so (k2hip_ngram_lm_*) against hand-derived walks and against
the Python twin (tests/ngram_twin.py), the ARPA loader and its rejections, and the twin's own self-checks on the CPU oracle -- with
scale = 0 and without an LM it must equal oracle.modified_beam_search exactly on every committed case the GPU tests compare the
engine with, and on those cases every LM event class must occur and the twin's own decisions must not be near-ties."""
import numpy as np
import pytest

import parity
from kat_model import frames, write_kat_model, write_wide_model
from ngram_twin import (BOS, EOS, EVENTS, KAT_LM_FLIP, LM_UNK, SCALE, TINY_BEAMS, WIDE_BEAMS, WIDE_VOCAB, TwinLm, arpa_text, draw_lm,
                        kat_lm_flip_score, tiny_lm, twin_batch, twin_beam_search, wide_enc, wide_lm)

f32 = np.float32

# a 3-gram of a handful of entries over V = 12 (tokens 0 and 2 are blank / unk; token 9 has no unigram)
SMALL = [((BOS,), -99.0, -0.25), ((LM_UNK,), -7.0, 0.0), ((EOS,), -1.0, 0.0),
         ((1,), -2.0, 0.0), ((3,), -2.5, 0.0), ((4,), -3.0, -0.5), ((5,), -3.5, -0.75), ((6,), -4.0, -1.0), ((7,), -4.5, 0.0),
         ((8,), -5.0, 0.0), ((10,), -5.5, 0.0), ((11,), -6.0, 0.0),
         ((BOS, 4), -1.0, -0.125), ((4, 5), -0.5, -1.5), ((5, 6), -0.75, -2.0), ((5, EOS), -0.3, 0.0),
         ((BOS, 4, 5), -0.25, 0.0), ((4, 5, 6), -0.125, 0.0), ((5, 6, 7), -0.0625, 0.0)]


def _lm(entries=SMALL, V=12):
    from k2transducerasr_amd import NgramLm
    return NgramLm(entries, V)


def _walk(lm, tokens, state=None):
    state = lm.start_state if state is None else state
    out = []
    for t in tokens:
        state, lp = lm.step(state, t)
        out.append(float(lp))
    return out, state


def test_lm_known_answers():
    lm = _lm()
    # states by (length, ids): (), (<s>), (4), (5), (<s> 4), (4 5), (5 6)
    assert (lm.order, lm.num_states, lm.start_state) == (3, 7, 1)
    assert lm.num_arcs == 9 + 3 + 3          # unigrams of real tokens, kept bigrams ((5, </s>) is ignored), trigrams
    # <s> 4 5: a bigram hit from the start state, then a full-order hit
    assert _walk(lm, [4, 5]) == ([-1.0, -0.25], 5)
    # then 6: (4 5 6) directly; then 7: (5 6 7) directly; then 7 again: the state is () -- (6 7) and (7) are no states
    assert _walk(lm, [4, 5, 6, 7]) == ([-1.0, -0.25, -0.125, -0.0625], 0)
    # one back-off: from (<s> 4), token 6 has no arc; bow(<s> 4) = -0.125, then (4) has no 6 either: bow(4) = -0.5, unigram 6 = -4
    assert _walk(lm, [4, 6]) == ([-1.0, float(f32(f32(f32(0) + f32(-0.125)) + f32(-0.5)) + f32(-4.0))], 0)
    # from (4 5), token 6 hits; from (5 6) token 5: bow(5 6) = -2, state (6) does not exist -> (): unigram 5, next state (5)
    assert _walk(lm, [5], state=6) == ([-2.0 + -3.5], 3)
    # a back-off by one that ends above the unigrams: from (<s> 4) ... token 5 hits directly; from (4 5) token 6 -> direct; use
    # state (<s> 4) and token 5's sibling: from (4 5) token 5: bow(4 5) = -1.5 -> state (5): no (5 5) -> bow(5) = -0.75 -> unigram
    assert _walk(lm, [5], state=5) == ([float(f32(f32(-1.5) + f32(-0.75)) + f32(-3.5))], 3)
    # from state (4), token 5: the bigram (4 5) directly, next state (4 5)
    assert _walk(lm, [5], state=2) == ([-0.5], 5)
    # the <unk> fallback: token 9 has no unigram -- from the start state bow(<s>) = -0.25, then <unk> = -7, next state ()
    assert _walk(lm, [9]) == ([-7.25], 0)
    # blank and unk leave the state alone and earn nothing
    assert _walk(lm, [4, 0, 2, 5]) == ([-1.0, 0.0, 0.0, -0.25], 5)
    # no <s> entries: the start state is the empty history
    assert _lm([e for e in SMALL if BOS not in e[0]]).start_state == 0


@pytest.mark.parametrize("entries, V, named", [
    ([((4,), -1.0, 0.0), ((4, 5, 6, 7, 8, 1), -1.0, 0.0)], 12, "entry 1: order 6"),
    ([((4,), -1.0, 0.0), ((12,), -1.0, 0.0)], 12, "entry 1: token id 12"),
    ([((4,), -1.0, 0.0), ((0,), -1.0, 0.0)], 12, "entry 1 contains blank"),
    ([((4,), -1.0, 0.0), ((4, 2), -1.0, 0.0)], 12, "entry 1 contains unk"),
    ([((4,), float("nan"), 0.0)], 12, "entry 0: non-finite"),
    ([((4,), -1.0, float("inf"))], 12, "entry 0: non-finite"),
    (SMALL + [((4, 5), -0.5, 0.0)], 12, "entry 19 duplicates entry 13"),
    (SMALL + [((7, 8, 1), -0.5, 0.0)], 12, "entry 19: its history has no entry of its own"),
    (SMALL + [((4, EOS, 5), -0.5, 0.0)], 12, "entry 19: </s> inside a history"),
    ([e for e in SMALL if e[0] != (LM_UNK,)], 12, "token id 9 has no unigram"),
])
def test_lm_rejections(entries, V, named):
    from k2transducerasr_amd import K2HipError
    with pytest.raises(K2HipError) as e:
        _lm(entries, V)
    assert e.value.code == -1 and named in str(e.value), str(e.value)


def test_lm_equals_the_twin_on_random_walks():
    """k2hip_ngram_lm_step against TwinLm: next state and float32 bits"""
    rng = np.random.default_rng(2025)
    pairs = 0
    for trial in range(120):
        V = int(rng.integers(6, 14))
        order = int(rng.integers(1, 6))
        fake = [([int(x) for x in rng.choice([v for v in range(V) if v not in (0, 2)], size=6)], None) for _ in range(4)]
        entries = draw_lm(fake, V, rng, order=order, n_cut=10, n_random=10, n_no_unigram=2)
        lm, tw = _lm(entries, V), TwinLm(entries, V)
        assert (lm.order, lm.num_states, lm.num_arcs, lm.start_state) == (max(len(e[0]) for e in entries), tw.num_states, tw.num_arcs, tw.start)
        for walk in range(10):
            s = tw.start if walk % 2 else int(rng.integers(tw.num_states))
            for v in rng.integers(0, V, size=14):
                n, lp = lm.step(s, int(v))
                n2, lp2, _ = tw.step(s, int(v))
                assert (n, lp.tobytes()) == (n2, lp2.tobytes()), (entries, s, v)
                s = n
            pairs += 1
    assert pairs == 1200


SYMS = ["<blk>", "<sos/eos>", "<unk>", "▁A", "B", "C", "▁D", "E", "F", "G", "H", "I"]


def _table(tmp_path):
    from k2transducerasr_amd import TokenTable
    tok = tmp_path / "tokens.txt"
    tok.write_text("".join(f"{s} {i}\n" for i, s in enumerate(SYMS)), encoding="utf-8")
    return TokenTable(str(tok))


def test_arpa_round_trip(tmp_path):
    """text -> k2hip_ngram_lm_load equals the array form: same automaton, same float32 bits on every (state, token)"""
    from k2transducerasr_amd import NgramLm
    table = _table(tmp_path)
    p = tmp_path / "lm.arpa"
    p.write_text("a header line\n\n" + arpa_text(SMALL, SYMS), encoding="utf-8")
    a, b = NgramLm.load(table, str(p)), _lm()
    assert (a.order, a.num_states, a.num_arcs, a.start_state) == (b.order, b.num_states, b.num_arcs, b.start_state)
    for s in range(a.num_states):
        for v in range(12):
            (n1, l1), (n2, l2) = a.step(s, v), b.step(s, v)
            assert (n1, l1.tobytes()) == (n2, l2.tobytes()), (s, v)
    # log10 -> natural log: parsed as double, times ln 10 in double, rounded to float32
    p.write_text("\\data\\\nngram 1=2\n\n\\1-grams:\n-1.2345678\t▁A\n-0.1\t<unk>\n\n\\end\\\n", encoding="utf-8")
    lm = NgramLm.load(table, str(p))
    assert lm.step(0, 3)[1].tobytes() == f32(-1.2345678 * np.log(10.0)).tobytes()
    assert lm.step(0, 4)[1].tobytes() == f32(-0.1 * np.log(10.0)).tobytes()


ARPA_OK = ["\\data\\", "ngram 1=4", "ngram 2=2", "", "\\1-grams:", "-1.0\t<unk>", "-99\t<s>\t-0.5", "-1.5\t▁A\t-0.25", "-2.0\tB", "",
           "\\2-grams:", "-0.5\t<s> ▁A", "-0.25\t▁A B", "", "\\end\\"]


def _mut(**at):
    lines = list(ARPA_OK)
    for k, v in at.items():
        lines[int(k[1:])] = v
    return "\n".join(x for x in lines if x is not None) + "\n"


@pytest.mark.parametrize("text, named", [
    ("\n".join(ARPA_OK[1:]) + "\n", "no \\data\\"),
    ("\n".join(ARPA_OK[:-1]) + "\n", "line 14: no \\end\\"),
    (_mut(L1="ngram 1=5"), "line 11"),                                  # counts disagree: the section closes with 4 entries
    (_mut(L2="ngram 2=1"), "line 13"),                                  # one entry too many
    ("\\data\\\nngram 1=1\nngram 2=0\nngram 3=0\nngram 4=0\nngram 5=0\nngram 6=0\n", "line 7: order 6"),
    (_mut(L8="-2.0\tZ"), "line 9: word 'Z'"),
    (_mut(L8="nan\tB"), "line 9: not a finite"),
    (_mut(L8="-1e999\tB"), "line 9: not a finite"),
    (_mut(L8="-2.0x\tB"), "line 9: not a finite"),
    (_mut(L12="-0.25\tB ▁A"), None),                                   # (fine: B has an entry of its own)
    (_mut(L12="-0.25\tZ B"), "line 13: word 'Z'"),
    (_mut(L8="-2.0\tC", L12="-0.25\tB ▁A"), "line 13: its history has no entry"),
    (_mut(L12="-0.5\t<s> ▁A"), "line 13 duplicates line 12"),
    (_mut(L8="-2.0\t<blk>"), "line 9 contains blank"),
    (_mut(L8="-2.0"), "line 9: a 1-gram line has 1 fields"),
    (_mut(L10="\\3-grams:"), "line 11"),
    ("\\data\\\nngram 1=%d\n" % ((1 << 24) + 1), "line 2"),
])
def test_arpa_rejections(tmp_path, text, named):
    from k2transducerasr_amd import K2HipError, NgramLm
    table = _table(tmp_path)
    p = tmp_path / "bad.arpa"
    p.write_text(text, encoding="utf-8")
    if named is None:
        NgramLm.load(table, str(p))
        return
    with pytest.raises(K2HipError) as e:
        NgramLm.load(table, str(p))
    assert e.value.code == -1 and named in str(e.value), str(e.value)


def test_arpa_missing_file_and_null_arguments(tmp_path):
    import ctypes as C
    from k2transducerasr_amd import K2HipError, NgramLm, load_library
    with pytest.raises(K2HipError) as e:
        NgramLm.load(_table(tmp_path), str(tmp_path / "missing.arpa"))
    assert e.value.code == -2
    L = load_library()
    assert L.k2hip_ngram_lm_create(None, None, None, None, 0, 20, None) == -1
    assert L.k2hip_ngram_lm_num_states(None) == -1 and L.k2hip_ngram_lm_order(None) == -1
    assert L.k2hip_ngram_lm_destroy(None) == 0
    L.k2hip_set_ngram_lm.argtypes = [C.c_void_p, C.c_void_p, C.c_float]
    assert L.k2hip_set_ngram_lm(None, None, 0.5) == -1


# ---- the twin on the CPU oracle ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def enc_tiny(oracle_tiny, utts):
    f = [oracle_tiny.fbank(u) for u in utts]
    return oracle_tiny.encoder(oracle_tiny.pad_sequence(f).reshape(len(utts), -1, 80))


@pytest.fixture(scope="module")
def wide_oracle(tmp_path_factory):
    from oracle import Oracle
    p = str(tmp_path_factory.mktemp("lm_wide") / "wide.k2w")
    write_wide_model(p, WIDE_VOCAB)
    return Oracle(p)


def _committed_case(ora, enc, beam, entries):
    """no LM and scale = 0: the twin is the oracle, exactly.  With the LM: every event class occurs, a result moves, and the twin's own
    per-frame selection margins and final-pick margin stay at or above the near-tie threshold for at least 7 of every 8 streams."""
    want, mg, sc, tr = ora.modified_beam_search(enc, beam, want_margins=True, want_scores=True, want_trace=True)
    lm = TwinLm(entries, ora.vocab_size)
    for what, kw in (("no LM", {}), ("scale = 0", dict(lm=lm, scale=0.0))):
        got, gsc, gmg, gtr, ev = twin_batch(ora, enc, beam, **kw)
        assert got == want, what
        np.testing.assert_allclose(gsc, sc, atol=1e-4, rtol=0)
        assert (gtr["idx"] == tr["idx"]).all() and (gtr["n"] == tr["n"]).all(), what
    got, gsc, gmg, gtr, ev = twin_batch(ora, enc, beam, lm=lm, scale=SCALE)
    assert min(ev[k] for k in EVENTS) >= 1, ev
    assert got != want
    clear = int((gmg.min(axis=1) >= parity.LOGIT_TOL).sum())
    print(f"beam {beam}: events {ev}, {sum(g != w for g, w in zip(got, want))}/{len(want)} streams moved, {clear}/{len(want)} streams clear of near-ties")
    assert 8 * (len(want) - clear) <= len(want), f"{len(want) - clear} of {len(want)} streams have a near-tie of their own"


@pytest.mark.parametrize("beam", TINY_BEAMS)
def test_twin_tiny(oracle_tiny, enc_tiny, beam):
    unbiased = oracle_tiny.modified_beam_search(enc_tiny, beam)
    _committed_case(oracle_tiny, enc_tiny, beam, tiny_lm(unbiased, oracle_tiny.vocab_size, beam))


@pytest.mark.parametrize("beam", WIDE_BEAMS)
def test_twin_wide(wide_oracle, beam):
    enc = wide_enc()
    unbiased = wide_oracle.modified_beam_search(enc, beam)
    _committed_case(wide_oracle, enc, beam, wide_lm(unbiased, beam))


def test_twin_kat_lm_flip(tmp_path):
    """ngram_twin.KAT_LM_FLIP: token 5 against a slightly better 6, the bigram (5, 7) flips the result (derivation there)"""
    from oracle import Oracle
    p = str(tmp_path / "kat.k2w")
    write_kat_model(p)
    ora = Oracle(p)
    K = KAT_LM_FLIP
    enc = frames(K["rows"])
    plain = twin_beam_search(ora, enc, K["beam"])
    assert (plain["ys"], plain["ts"]) == K["plain"] == ora.modified_beam_search(enc[None], K["beam"])[0]
    r = twin_beam_search(ora, enc, K["beam"], TwinLm(K["entries"], 8), K["scale"])
    assert (r["ys"], r["ts"]) == K["fused"]
    assert abs(r["lp"] - kat_lm_flip_score()) < 1e-5
    # the C library's automaton gives the same terms
    lm = _lm(K["entries"], 8)
    assert _walk(lm, [5, 7]) == ([-4.0, -1.0], 0) and _walk(lm, [6, 7]) == ([-4.0, -4.0], 0)
