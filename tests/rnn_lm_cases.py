"""The cases of the neural LM rescoring tests (test_rnn_lm.py on the CPU, test_rnn_lm_gpu.py on the device): the LMs, the hypothesis
sets, the measured bound and the recognizer's LM seeds and scales."""
import numpy as np

# name -> (V, E, H, L, seed)
#   A  the baseline
#   B  E != H; H a multiple of 32 that is no power of two; three layers
#   C  V = 165: five full 32-column tiles plus five columns -- every wave of the score kernel gets a tile and the last tile is ragged
LMS = {"A": (37, 64, 64, 1, 11), "B": (37, 32, 96, 3, 12), "C": (165, 32, 32, 2, 13)}

# E32: the largest per-token error of the float32 numpy restatement (rnn_lm_twin.restate32) against the float64 twin over every LM and
# every hypothesis set below, with and without eos, measured on the CPU (test_rnn_lm.py re-measures it and holds it to this constant;
# DESIGN.md "Neural LM rescoring" records the run).  The host reference and the device get 8 E32 + 1e-6 per token log-prob and P times
# that per total of P positions: the margin covers another summation order and a few ulp of expf / tanhf, and a wrong gate, row or
# column is wrong by 1e-1 and more.
E32 = 7.4e-7   # measured 7.372e-07


def token_bound():
    return 8 * E32 + 1e-6


def total_bound(positions):
    return max(int(positions), 1) * token_bound()


def _tokens(rng, V, n):
    return rng.integers(0, V, size=n).tolist()


def hyp_sets(V, seed=5):
    """name -> list of token-id lists.  Lengths come from {0, 1, 2, 31, 32, 33}; Hn from {1, 33, 70} (+ the six strictly decreasing
    lengths).  "fall" (70 hypotheses, shuffled): with eos the active-row count falls 70, 64, 33, 32 (29 steps), 31, 1; without eos
    64, 33, 32 (29 steps), 31, 1 -- every strip count of the step kernel from three strips to one row, and a_t = 33 / 32 / 31 around
    the strip's edge."""
    rng = np.random.default_rng(seed + V)
    fall = [0] * 6 + [1] * 31 + [2] + [31] + [32] * 30 + [33]
    rng.shuffle(fall)
    sets = {
        "one": [_tokens(rng, V, 33)],
        "one_empty": [[]],
        "equal33": [_tokens(rng, V, 2) for _ in range(33)],
        "drawn33": [_tokens(rng, V, n) for n in rng.choice([0, 1, 2, 31, 32, 33], size=33)],
        "decreasing": [_tokens(rng, V, n) for n in (33, 32, 31, 2, 1, 0)],
        "fall": [_tokens(rng, V, n) for n in fall],
    }
    sets["fall"][int(np.argmax([len(h) for h in sets["fall"]]))][-1] = V - 1   # the last column as a target (and as an input)
    sets["one"][0][0] = V - 1
    return sets


# The recognizer tests: LM A's shape (V = 37, the tiny models' vocabulary) with these seeds and scales, chosen on the CPU with the twins
# (test_rnn_lm.py asserts the two conditions on the twin side): beam 4, nbest 4 over the five fixture utterances; no adjacent pair of a
# stream's keys falls inside the bound, and at least two of the five streams change their top entry.
RECOGNIZER = {"transducer": dict(preset="zipformer2-tiny-test", method="modified_beam_search", seed=1, scale=2.0),
              "ctc": dict(preset="zipformer2-ctc-tiny-test", method="ctc_prefix_beam_search", seed=37, scale=2.0)}
# (seeds 0 .. 39 x scales 0.25, 0.5, 1, 2 were searched for the largest smallest gap between a stream's adjacent keys among the choices
# that change at least two tops: 0.149 for the transducer lists, 0.400 for the CTC lists, four tops changed in both.)
# Adjacent keys of the chosen inputs differ by at least this much -- far above the bound, because the device's own search scores differ
# from the twins' by float rounding.
KEY_GAP = 1e-2
