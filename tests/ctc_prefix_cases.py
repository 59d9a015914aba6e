"""The inputs of the CTC prefix beam search tests (helper of test_ctc_prefix.py, which checks them on the CPU, and
test_ctc_prefix_gpu.py, which runs them on the device).

Seeded normal logits, log-softmaxed in float64, rounded to float32 (ctc_prefix_twin.seeded_log_probs).  A case is asserted strictly
(tokens, timestamps, order exact) only if every gap the float64 twin reports on it -- per frame the last selected against the first
rejected candidate, and the consecutive ranks of the last frame -- is at least G.  G is measured, not chosen: E = the worst difference
between the float32 and the float64 twin's gaps on the group's inputs while their selections agree, G = 8 E (two scores each off by E
in opposite directions give 2 E; the factor four covers the device's exp / log1p differing from numpy's by a few ulp more).  E grows
with the size of the scores (one float32 ulp of a score near -1000 is 6e-5), so it is measured per group of like shapes:

    group      inputs                                              E         G = 8 E (rounded up)
    small      V = 3 (exhaustive, re-spelled), hand-built rows     5.1e-7    4.1e-6
    ragged     V = 37, T = 1, 2, 7, 70, beam 1 / 4 / 8             1.81e-5   1.5e-4
    wide       V = 600, T = 70, beam 4 / 8                         2.51e-5   2.1e-4
    long       V = 37, T = 300, beam 4                             7.53e-5   6.1e-4
    fixture    the tiny CTC model's log_probs, T' = 35, beam 4     4.2e-6    3.4e-5

The seeds were found by a search on the CPU over the twin (first ones whose gaps clear G at every beam of the case); test_ctc_prefix.py
re-measures E on these inputs and asserts both 8 E <= G and every gap >= G."""
import numpy as np

from ctc_prefix_twin import seeded_log_probs

G_SMALL, G_RAGGED, G_WIDE, G_LONG, G_FIXTURE = 4.1e-6, 1.5e-4, 2.1e-4, 6.1e-4, 3.4e-5

# ---- hand-built rows (columns: blank, a, b): multiples of 0.25, exact in float32 --------------------------------------------------
TIE_LOWER_ID = (np.array([[-4, -0.5, -0.5]], np.float32), 2)                      # equal tokens: [a] before [b]
TIE_STAY = (np.array([[-0.5, -0.5, -4]], np.float32), 1)                          # stay against extension: the empty prefix survives
# after frame 0: slot 0 = [] and slot 1 = [a], both -0.25 (the stay has the lower flat index); frame 1: [] + b ties with [a] + b
TIE_LOWER_SLOT = (np.array([[-0.25, -0.25, -8], [-8, -8, -1]], np.float32), 2)
PEAKY_A_BLANK_A = np.array([[-20, 0, -20], [0, -20, -20], [-20, 0, -20]], np.float32)
PEAKY_A_A_A = np.array([[-20, 0, -20], [-20, 0, -20], [-20, 0, -20]], np.float32)

# ---- the re-spelled prefix: V = 3, T = 10, beam 4 -- the twin counts a fold into a slot whose history parent is another node ------
RESPELLED_V, RESPELLED_T, RESPELLED_BEAM, RESPELLED_SEED = 3, 10, 4, 2


def respelled_row():
    return seeded_log_probs(RESPELLED_SEED, RESPELLED_T, RESPELLED_V, 2.0)


# ---- exhaustive: V = 3, beam 8, T = 1 (2 prefixes + the empty one) and T = 2 (5 prefixes), nothing pruned -----------------------------
def exhaustive_rows():
    """[2][2][3] and n_frames (1, 2)"""
    lp = np.stack([seeded_log_probs(41, 2, 3), seeded_log_probs(42, 2, 3)])
    return lp, np.array([1, 2], np.int32)


# ---- ragged: V = 37, n_frames = 1, 2, 7, 70, then a T = 70 row with 2 % -inf cells and a row that is -inf everywhere ----------------
RAGGED_FRAMES = [1, 2, 7, 70, 70, 70]
RAGGED_SEEDS = [1004, 1001, 1004, 1000, 2007]
RAGGED_BEAMS = (1, 4, 8)
RAGGED_ALL_INF_ROW = 5


def ragged_rows(V=37):
    Tp = max(RAGGED_FRAMES)
    lp = np.zeros((len(RAGGED_FRAMES), Tp, V), np.float32)
    for r, seed in enumerate(RAGGED_SEEDS):
        T = RAGGED_FRAMES[r]
        lp[r, :T] = seeded_log_probs(seed, T, V)
        lp[r, T:] = seeded_log_probs(seed + 500, Tp, V)[T:]      # frames behind n_frames: ordinary values that must not be read
    lp[4][np.random.default_rng(3007).random((Tp, V)) < 0.02] = -np.inf
    lp[RAGGED_ALL_INF_ROW] = -np.inf
    return lp, np.array(RAGGED_FRAMES, np.int32)


# ---- wide (columns above 256 and above 512) and long (long histories) ----------------------------------------------------------------
WIDE_V, WIDE_T, WIDE_SEED, WIDE_BEAMS = 600, 70, 1009, (4, 8)
LONG_V, LONG_T, LONG_SEED, LONG_BEAM = 37, 300, 1065, 4


def wide_row():
    return seeded_log_probs(WIDE_SEED, WIDE_T, WIDE_V)


def long_row():
    return seeded_log_probs(LONG_SEED, LONG_T, LONG_V)


def strict_cases():
    """(name, lp [T][V], beams, G) of every seeded case that the GPU tests assert exactly"""
    ex, _ = exhaustive_rows()
    rg, nf = ragged_rows()
    out = [("exhaustive T=1", ex[0, :1], (8,), G_SMALL), ("exhaustive T=2", ex[1], (8,), G_SMALL),
           ("re-spelled", respelled_row(), (RESPELLED_BEAM,), G_SMALL)]
    out += [(f"ragged row {r}", rg[r, : nf[r]], RAGGED_BEAMS, G_RAGGED) for r in range(len(RAGGED_SEEDS))]
    out += [("wide", wide_row(), WIDE_BEAMS, G_WIDE), ("long", long_row(), (LONG_BEAM,), G_LONG)]
    return out
