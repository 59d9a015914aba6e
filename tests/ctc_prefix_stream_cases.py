"""The inputs of the streaming CTC prefix beam search tests beyond tests/ctc_prefix_cases.py (helper of test_ctc_prefix_stream.py, which
checks them on the CPU, and test_ctc_prefix_stream_gpu.py, which runs them on the device).

The seeded V = 37 cases of ctc_prefix_cases.py have NO fold relation that crosses a 16-frame boundary (test_ctc_prefix_stream.py
counts them): alone they would pass a carry that forgets every relation at a boundary.  Hence the small-vocabulary rows:

    the re-spelled row     V = 3, T = 10, beam 4 (ctc_prefix_cases.respelled_row): every split and chunking crosses folds
    SMALL4                 V = 4, T = 48, seeded_log_probs(3000, 48, 4, 2.0), beams 4 and 8, chunks of 16 (the streaming chunk length)

SMALL4 figures, measured on the CPU by test_ctc_prefix_stream.py: smallest twin gap 8.6e-3 (beam 4) and 3.5e-3 (beam 8); E (float32
against float64 twin, as ctc_prefix_cases.py defines it) 1.2e-6 and 1.4e-6, so G = 8 E is about 1e-5, far below the gaps; the float32
and float64 selections agree; beam 8 has two re-spelled folds."""
import numpy as np

import ctc_prefix_cases as cases
from ctc_prefix_twin import seeded_log_probs

SMALL4_SEED, SMALL4_T, SMALL4_V, SMALL4_BEAMS, SMALL4_CHUNK = 3000, 48, 4, (4, 8), 16
SMALL4_MIN_GAP = {4: 8.6e-3, 8: 3.5e-3}     # rounded down from 8.61e-3 / 3.54e-3
SMALL4_E = {4: 1.3e-6, 8: 1.5e-6}                # rounded up from 1.23e-6 / 1.4e-6
CHUNK = 16


def small4_row():
    return seeded_log_probs(SMALL4_SEED, SMALL4_T, SMALL4_V, 2.0)


def respelled_chunkings():
    """every two-chunk split of the re-spelled row and its uniform chunkings, as lists of chunk lengths"""
    T = cases.RESPELLED_T
    out = [[s, T - s] for s in range(1, T)]
    for c in (1, 2, 3, 4):
        out.append([min(c, T - t) for t in range(0, T, c)])
    return out


def uniform(T, c):
    return [min(c, T - t) for t in range(0, T, c)]


def embed(lp, V):
    """lp [..., v] inside a vocabulary of V: the columns >= v at -inf.  The search is unchanged by that (-inf candidates are dropped,
    the flat-index order k V + v keeps the order of k v' + v)"""
    lp = np.asarray(lp, np.float32)
    out = np.full(lp.shape[:-1] + (V,), -np.inf, np.float32)
    out[..., : lp.shape[-1]] = lp
    return out
