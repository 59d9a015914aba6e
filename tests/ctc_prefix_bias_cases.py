"""The inputs of the biased CTC prefix beam search tests (helper of test_ctc_prefix_bias.py, which checks them on the CPU, and
test_ctc_prefix_bias_gpu.py, which runs them on the device).

The log-prob rows are those of ctc_prefix_cases.py; what is committed here are the phrase lists and LM seeds that go with them.  Phrases
are cut (hotword_twin.draw_phrases) from the alternatives the UNBIASED twin returns at beam 8, so partial, broken and committed matches
occur; the LMs are ngram_twin.draw_lm over the same alternatives (n-grams that really occur, holes in the unigrams), scaled by LM_SCALE.
score_per_token is 1.5, exact in float32 with its small multiples.

The rule of ctc_prefix_cases.py holds unchanged: a case is asserted exactly only where every gap of the float64 twin -- per frame the
last selected against the first rejected KEY, and the consecutive finals -- is at least G = 8 E, E the worst difference between the
float32 and the float64 twin's gaps while their selections agree.  The bonus and the LM terms change the size of the keys, so E is
measured anew, per group of shapes and per table kind (hw: hotwords only, lm: LM only, both), worst over the group's beams:

    group      inputs                                         E hw      E lm      E both    G (one per group, >= 8 x the worst E)
    small      V = 3 exhaustive / re-spelled, the flip        5.1e-7    5.1e-7    5.1e-7    4.1e-6
    ragged     V = 37, T = 1, 2, 7, 70, beam 1 / 4 / 8        3.62e-5   2.65e-5   2.23e-5   2.9e-4
    wide       V = 600, T = 70, beam 4 / 8                    3.94e-5   3.79e-5   3.92e-5   3.2e-4
    long       V = 37, T = 300, beam 4                        1.08e-4   1.15e-4   1.09e-4   9.3e-4

(the unbiased groups of ctc_prefix_cases.py have 1.81e-5 / 2.51e-5 / 7.53e-5: the context score makes the keys larger.)
The seeds were found by a search on the CPU over the twin (ragged: the first common phrase / LM seed; wide and long: the phrase seed with the widest
gaps among the first dozen, then the first LM seed; each clears G for every row, kind and beam of the case);
test_ctc_prefix_bias.py re-measures E on these inputs and asserts both 8 E <= G and every gap >= G."""
import numpy as np

import ctc_prefix_cases as base
from ctc_prefix_twin import prefix_beam_search
from hotword_twin import TwinGraph, draw_phrases
from ngram_twin import TwinLm, draw_lm

SCORE = 1.5            # score_per_token
LM_SCALE = 0.5
KINDS = ("hw", "lm", "both")
G_SMALL, G_RAGGED, G_WIDE, G_LONG = 4.1e-6, 2.9e-4, 3.2e-4, 9.3e-4

# ---- committed seeds -------------------------------------------------------------------------------------------------------------
RAGGED_PHRASES, RAGGED_PHRASE_SEED, RAGGED_LM_SEED = 6, 22, 22
WIDE_PHRASES, WIDE_PHRASE_SEED, WIDE_LM_SEED, WIDE_HUB_ARCS = 12, 0, 1, 100
LONG_PHRASES, LONG_PHRASE_SEED, LONG_LM_SEED = 10, 11, 129

# ---- small: V = 3 (blank, a, unk) -- one biasable token.  [a] commits at once, [a, a] is pending in between --------------------------
SMALL_V = 3
EXHAUSTIVE_PHRASES = [[1]]
RESPELLED_PHRASES = [[1, 1]]
# unigram a, the bigram (a, a) with a back-off weight on [a], the sentence start and <unk>; natural log, before LM_SCALE
SMALL_LM_ENTRIES = [((-1,), -99.0, -0.25), ((-3,), -7.5, 0.0), ((1,), -2.0, -0.5), ((1, 1), -0.75, 0.0), ((-1, 1), -1.25, 0.0)]

# ---- the hand-built flip: V = 4 (blank, a, unk, b), three frames, beam 2, phrase [a, b], score_per_token 1.5 -----------------------
# Every value is a multiple of 0.25 and so is every sum below (there is no logaddexp of two finite values on the way: no two paths
# spell the same prefix inside the beam, see the derivation), so float32 and float64 give the same numbers.
#                  blank    a     unk    b
#   frame 0        -8      -1.5   -16   -1.25
#   frame 1        -8      -16    -16   -0.5
#   frame 2        -0.25   -inf   -inf  -inf
# Frame 0, from the empty prefix (tot 0): candidates [] -8, [a] -1.5, [unk] -16, [b] -1.25.
#   unbiased: {[b] -1.25, [a] -1.5}.   biased: bonus[0][a] = +1.5 (a opens the phrase), key [a] = 0, key [b] = -1.25: {[a], [b]};
#   [a]: hs = 1, ctx = 1.5.  [b]: hs = 0, ctx = 0.
# Frame 1, row (-8, -16, -16, -0.5): b is the only live column.
#   [a] + b: x = -1.5 - 0.5 = -2;  [b] + b: x = pb_[b] + lp = -inf (a repeat needs a blank in between);
#   stays: [a]: spb = -1.5 - 8 = -9.5, spnb = -1.5 - 16 = -17.5 -- a logaddexp of two finite values, but of a candidate that is never
#   selected below; [b]: spb = -1.25 - 8, spnb = pnb + lp(b) = -1.25 - 0.5 = -1.75, st = -1.75 + log1p(e^-7.5) = -1.74945 (again a
#   stay; it IS selected, but only the runner-up of the biased result hangs on it, 2.7 below the winner).
#   unbiased keys: [b] stay -1.74945, [a, b] -2, [a] stay -9.5 -> {[b], [a, b]}.
#   biased keys:   [a, b]: cb = 1.5 + bonus[1][b] = 3.0 (the phrase ends: committed, hs back to 0), key = -2 + 3 = 1;
#                  [b] stay -1.74945; [a] stay -9.5 + 1.5 -> {[a, b], [b]}.
# Frame 2, only blank is finite: no extension is a candidate, every stay has spnb = -inf and st = tot - 0.25 exactly.
#   tot [a, b] = -2.25; tot [b] = -1.99945.
# Final: unbiased [b] (-1.99945) before [a, b] (-2.25); biased final [a, b] = (-2.25 + 3.0) - pending[0] = 0.75 EXACTLY, [b] -1.99945.
# The result flips from [b] @ frame 0 to [a, b] @ frames 0, 1, and the best score is exactly 0.75 in either number format.
FLIP_ROWS = np.array([[-8, -1.5, -16, -1.25], [-8, -16, -16, -0.5], [-0.25, -np.inf, -np.inf, -np.inf]], np.float32)
FLIP_BEAM, FLIP_PHRASES = 2, [[1, 3]]
FLIP_UNBIASED = ([3], [0])
FLIP_BIASED = ([1, 3], [0, 1], 0.75)


def _alternatives(rows, beam=8):
    """(tokens, timestamps) of every alternative the unbiased float64 twin returns on the rows"""
    return [(h["tokens"], h["timestamps"]) for lp in rows for h in prefix_beam_search(np.asarray(lp, np.float64), beam)["hyps"]]


_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def small_graph(phrases):
    return TwinGraph(phrases, SCORE, SMALL_V)


def small_lm():
    return TwinLm(SMALL_LM_ENTRIES, SMALL_V).scaled(LM_SCALE)


def flip_graph():
    return TwinGraph(FLIP_PHRASES, SCORE, FLIP_ROWS.shape[1])


def ragged_tables(phrase_seed=None, lm_seed=None):
    """(TwinGraph, scaled TwinLm) of the ragged batch: one pair for the whole call"""
    phrase_seed = RAGGED_PHRASE_SEED if phrase_seed is None else phrase_seed
    lm_seed = RAGGED_LM_SEED if lm_seed is None else lm_seed
    lp, nf = base.ragged_rows()
    alts = _memo("ragged alts", lambda: _alternatives([lp[r, : nf[r]] for r in range(len(base.RAGGED_SEEDS))]))
    V = lp.shape[2]
    graph = TwinGraph(draw_phrases(alts, RAGGED_PHRASES, np.random.default_rng(phrase_seed)), SCORE, V)
    return graph, TwinLm(draw_lm(alts, V, np.random.default_rng(lm_seed)), V).scaled(LM_SCALE)


def wide_tables(phrase_seed=None, lm_seed=None):
    """V = 600; the LM has a hub state -- the history [first token of the unbiased result] -- with more than 64 arcs, so the walk's
    64-ary narrowing runs on the step behind that token"""
    phrase_seed = WIDE_PHRASE_SEED if phrase_seed is None else phrase_seed
    lm_seed = WIDE_LM_SEED if lm_seed is None else lm_seed
    alts = _memo("wide alts", lambda: _alternatives([base.wide_row()]))
    V = base.WIDE_V
    graph = TwinGraph(draw_phrases(alts, WIDE_PHRASES, np.random.default_rng(phrase_seed)), SCORE, V)
    rng = np.random.default_rng(lm_seed)
    ent = draw_lm(alts, V, rng, n_cut=80, n_random=200, n_no_unigram=6)
    have = {ids for ids, _, _ in ent}
    hub = wide_hub()
    if (hub,) not in have:
        ent.append(((hub,), np.float32(-4.0), np.float32(-0.5)))
    for w in rng.choice([v for v in range(3, V) if (v,) in have], size=WIDE_HUB_ARCS, replace=False):
        if (hub, int(w)) not in have:
            ent.append(((hub, int(w)), np.float32(rng.uniform(-1.5, -0.1)), np.float32(rng.uniform(-1.0, -0.05))))
    return graph, TwinLm(ent, V).scaled(LM_SCALE)


def wide_hub():
    return _memo("wide alts", lambda: _alternatives([base.wide_row()]))[0][0][0]


def long_tables(phrase_seed=None, lm_seed=None):
    phrase_seed = LONG_PHRASE_SEED if phrase_seed is None else phrase_seed
    lm_seed = LONG_LM_SEED if lm_seed is None else lm_seed
    alts = _memo("long alts", lambda: _alternatives([base.long_row()], base.LONG_BEAM))
    V = base.LONG_V
    graph = TwinGraph(draw_phrases(alts, LONG_PHRASES, np.random.default_rng(phrase_seed)), SCORE, V)
    return graph, TwinLm(draw_lm(alts, V, np.random.default_rng(lm_seed), n_cut=80), V).scaled(LM_SCALE)


def pick(kind, graph, lm):
    """the (graph, lm) pair of a table kind"""
    return (graph if kind in ("hw", "both") else None), (lm if kind in ("lm", "both") else None)


def strict_cases():
    """(name, lp [T][V], beams, graph, lm, G) of every case the GPU tests assert exactly; every table kind of every case"""
    ex, _ = base.exhaustive_rows()
    rg, nf = base.ragged_rows()
    out = []
    for kind in KINDS:
        g, lm = pick(kind, small_graph(EXHAUSTIVE_PHRASES), small_lm())
        out += [(f"exhaustive T=1 {kind}", ex[0, :1], (8,), g, lm, G_SMALL), (f"exhaustive T=2 {kind}", ex[1], (8,), g, lm, G_SMALL)]
        g, lm = pick(kind, small_graph(RESPELLED_PHRASES), small_lm())
        out.append((f"re-spelled {kind}", base.respelled_row(), (base.RESPELLED_BEAM,), g, lm, G_SMALL))
        g, lm = pick(kind, *ragged_tables())
        out += [(f"ragged row {r} {kind}", rg[r, : nf[r]], base.RAGGED_BEAMS, g, lm, G_RAGGED) for r in range(len(base.RAGGED_SEEDS))]
        g, lm = pick(kind, *wide_tables())
        out.append((f"wide {kind}", base.wide_row(), base.WIDE_BEAMS, g, lm, G_WIDE))
        g, lm = pick(kind, *long_tables())
        out.append((f"long {kind}", base.long_row(), (base.LONG_BEAM,), g, lm, G_LONG))
    out.append(("flip hw", FLIP_ROWS, (FLIP_BEAM,), flip_graph(), None, G_SMALL))
    return out


# ---- end to end: the tiny CTC model's log-probs of the fixture batch (5 streams, T' = 35, V = 37), beam 4 ---------------------------------
# Phrases and a trigram drawn from the unbiased twin's results over the log-probs at hand (the oracle's on the CPU, the device's own on
# the GPU: equal token sequences wherever the unbiased search is strict).  E over the oracle's log-probs: hw 4.46e-6, lm 5.26e-6, both
# 7.81e-6; G = 8 E = 6.3e-5; the smallest gap of any stream and kind is 1.4e-3.  Every stream clears it (test_ctc_prefix_bias.py); the GPU test asserts the same on the device's log-probs.
FIXTURE_BEAM, FIXTURE_PHRASES, FIXTURE_PHRASE_SEED, FIXTURE_LM_SEED, G_FIXTURE = 4, 6, 1, 0, 6.3e-5


def fixture_entries(lp, phrase_seed=None, lm_seed=None):
    """(phrases, LM entries before scaling) for log-probs lp [B][T'][V]"""
    phrase_seed = FIXTURE_PHRASE_SEED if phrase_seed is None else phrase_seed
    lm_seed = FIXTURE_LM_SEED if lm_seed is None else lm_seed
    best = [_alternatives([lp[b]], FIXTURE_BEAM)[0] for b in range(lp.shape[0])]
    return draw_phrases(best, FIXTURE_PHRASES, np.random.default_rng(phrase_seed)), draw_lm(best, lp.shape[2], np.random.default_rng(lm_seed))


def fixture_tables(lp, phrase_seed=None, lm_seed=None):
    phrases, entries = fixture_entries(lp, phrase_seed, lm_seed)
    return TwinGraph(phrases, SCORE, lp.shape[2]), TwinLm(entries, lp.shape[2]).scaled(LM_SCALE)
