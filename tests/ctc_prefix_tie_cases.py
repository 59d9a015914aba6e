"""Inputs of the CTC prefix beam search that TIE ON PURPOSE (helper of test_ctc_prefix_tie_cases_ref.py, which checks them on the CPU,
and test_ctc_prefix_ties_gpu.py, which runs them through every form of the kernel).  The seeded cases of ctc_prefix_cases.py are accepted
only when every gap clears G, so ties are filtered out of them by construction; here the ties are planted in log_probs [T'][V] itself
(the debug op "ctc_prefix_beam" takes it directly; rows need not be normalised).  T' = 12, at most 3 rows per V and family.

MIRRORED family (arithmetic inexact, ties exact by symmetry), V in {65, 257, 600}.  Every column sits on a floor, -9 in every frame,
unless driven.  A duplicate GROUP is a set of columns equal in EVERY frame: its prefixes are mirror images ([a] / [b], [a, b] / [b, a]),
so their pb / pnb / tot and their folds are bit-equal in any deterministic arithmetic.  Groups, where V admits them: one thread at three
strides (5, 261, 517); neighbouring lanes (17, 18); the row seams of the wave reduction 15|16, 31|32, 47|48; the wave seam 63|64;
255|256 (the columns requested a frame ahead against the looped ones); 511|512; the later twin at V - 1 (3, V - 1; at V = 65 / 257 column
V - 1 already is the right half of a seam pair); two far-apart columns (100, 300).  Frames 0 and 1 are equal: blank and three random
groups at random float32 levels in [-5, -0.3], each of a few single columns driven with probability 0.4.  Frames 2 .. 11 drive blank,
a DESIGNATED group in [-0.8, -0.3] and two random other groups and the singles (probability 0.4) in [-5, -2]: the designated group's
extensions of the best slot beat its stay candidate (at most -2 + log 3 with a fold), so every group is the top of a frame and its seam
is decided at the beam cut even at beam 1.  The designated groups go round (row r starts at group r); in the LAST frame the single
column 40 is the designated one: one thread then holds the best candidate of EVERY slot, and what it hands on is the N-best itself.
Rows: "main" as above; "floor0": frames 0 and 1 entirely on the floor, blank included -- the beam fills by flat index alone, the stay,
then v = 1, 2, ..., and frame 1 folds every one of them; "level": in frames 0 and 1 the group (17, 18) sits at blank's level, so
the stay candidate ties with extensions and the two terms of frame 1's folds are equal.

DYADIC family (arithmetic exact, ties exact whatever their formation), V in {2, 9, 65, 256, 257, 600}.  Every finite value is a multiple
of 1/8 in [-3, 0].  Even frames: blank at -inf, tokens drawn from few levels (many equal); odd frames: only blank finite.  Every
logaddexp then has a -inf operand, which the kernel returns exactly, and every sum is exact in float32: -1.5 + -2.5 ties with -2 + -2
across slots and across the beam cut, and the device's scores must be BIT-EQUAL to the twin's.  V = 2 has one finite candidate per slot;
at V = 9 three tokens of frame 0 are at -inf, so five candidates are finite: fewer than `beam`.  THIS FAMILY HAS NO FOLDS: all live
prefixes have one length (every even frame appends exactly one token), and a fold's logaddexp would have two finite operands as soon
as the stay survives.  Folds on ties come from the mirrored family.

THE ACCEPTANCE RULE.  The float64 twin (ctc_prefix_twin.prefix_beam_search with a Forms table) carries with every score how it was
formed.  check_case accepts (lp, beam) only if, in every frame, for every selected candidate i and EVERY candidate j ranked after it
with tot_i - tot_j < G (or equal), the two are equally formed, or both exact and equal; the same for adjacent final scores.  A
rejected case is not excused anywhere: it is not in the suite (find_seed takes the first seed accepted at every beam 1 .. 8).

G is measured by the rule of ctc_prefix_cases.py: E = the worst difference between the float32 and the float64 twin's gaps on these
inputs while their selections agree, G = 8 E, per family and V, over beams 1 .. 8 and all rows (test_ctc_prefix_tie_cases_ref.py
re-measures it):

    family     V      E          G = 8 E (rounded up)     smallest gap that is no tie
    mirrored   65     1.11e-6    8.9e-6                   0.118
    mirrored   257    4.58e-7    3.7e-6                   0.031
    mirrored   600    8.05e-7    6.5e-6                   0.037
    dyadic     all    0          0 (exact ties are always examined)    0.125
"""
import functools

import numpy as np

from ctc_prefix_twin import THREADS, Forms, prefix_beam_search

T = 12
BEAMS = tuple(range(1, 9))
FLOOR = np.float32(-9)
MIRRORED_VS, DYADIC_VS = (65, 257, 600), (2, 9, 65, 256, 257, 600)
G_MIRRORED = {65: 8.9e-6, 257: 3.7e-6, 600: 6.5e-6}
G_DYADIC = 0.0
SEAMS = ((15, 16), (31, 32), (47, 48), (63, 64), (255, 256), (511, 512))
SINGLES = (9, 11, 23, 40, 57, 150, 400)      # (none of 1 .. 7, the tokens of floor0's slots)
LEVEL_GROUP = (17, 18)


def groups_of(V):
    g = [(5, 261, 517), (17, 18)] + list(SEAMS) + [(3, V - 1), (100, 300)]
    g = [tuple(c for c in cols if c < V) for cols in g]
    taken = set()
    out = []
    for cols in g:
        if len(cols) >= 2 and not taken & set(cols):
            out.append(cols)
            taken |= set(cols)
    return out


def mirrored_rows(V, seed):
    """[3][T][V] float32: main, floor0, level"""
    groups = groups_of(V)
    singles = [c for c in SINGLES if c < V and not any(c in g for g in groups)]
    rows = np.full((3, T, V), FLOOR, np.float32)
    for r in range(3):
        rng = np.random.default_rng([seed, V, r])
        lv = lambda lo, hi: np.float32(rng.uniform(lo, hi))
        for t in [0] + list(range(2, T)):
            row = rows[r, t]
            if t == 0:
                if r == 1:
                    continue                                        # floor0: nothing driven, blank included
                row[0] = lv(-5, -0.3)
                for g in rng.choice(len(groups), 3, replace=False):
                    row[list(groups[g])] = lv(-5, -0.3)
                for c in singles:
                    if rng.random() < 0.4:
                        row[c] = lv(-5, -0.3)
                if r == 2:
                    row[list(LEVEL_GROUP)] = row[0]
            else:
                des = (40,) if t == T - 1 else groups[(t - 2 + r) % len(groups)]
                row[0] = lv(-5, -2)
                others = [g for g in groups if g != des]
                for g in rng.choice(len(others), 2, replace=False):
                    row[list(others[g])] = lv(-5, -2)
                for c in singles:
                    if c not in des and rng.random() < 0.4:
                        row[c] = lv(-5, -2)
                row[list(des)] = lv(-0.8, -0.3)
        rows[r, 1] = rows[r, 0]
    return rows


DYADIC_LEVELS = np.array([-0.5, -1.0, -1.5, -2.0, -2.5], np.float32)


def dyadic_rows(V, seed):
    """[2][T][V] float32"""
    rows = np.full((2, T, V), -np.inf, np.float32)
    for r in range(2):
        rng = np.random.default_rng([seed, V, r, 77])
        for t in range(T):
            if t % 2:
                rows[r, t, 0] = np.float32(-0.125 * rng.integers(0, 25))
            else:
                n = 3 if r == 0 else 5
                rows[r, t, 1:] = DYADIC_LEVELS[rng.integers(0, n, V - 1)]
                few = rng.choice(np.arange(1, V), min(V - 1, 6), replace=False)        # a handful on top, in pairs
                rows[r, t, few] = np.float32(-0.125) * rng.integers(0, 3, len(few)).astype(np.float32)
        if V == 9:
            rows[r, 0, [2, 5, 7]] = -np.inf
    return rows + np.float32(0)         # (one zero: -0.125 x 0 is -0.0)


# ---- the committed seeds: the first per family and V that check_case accepts at every beam and coverage() counts in full ---------------
MIRRORED_SEEDS = {65: 0, 257: 0, 600: 0}
DYADIC_SEEDS = {2: 0, 9: 0, 65: 0, 256: 0, 257: 0, 600: 0}
ROW_NAMES = {"mirrored": ("main", "floor0", "level"), "dyadic": ("three levels", "five levels")}


@functools.lru_cache(maxsize=None)
def rows_of(family, V):
    return mirrored_rows(V, MIRRORED_SEEDS[V]) if family == "mirrored" else dyadic_rows(V, DYADIC_SEEDS[V])


def g_of(family, V):
    return G_MIRRORED[V] if family == "mirrored" else G_DYADIC


def all_cases():
    """(family, V, row index, lp [T][V]) of every committed row"""
    return [(f, V, r, rows_of(f, V)[r]) for f, Vs in (("mirrored", MIRRORED_VS), ("dyadic", DYADIC_VS)) for V in Vs for r in range(rows_of(f, V).shape[0])]


_runs = {}


def reference(family, V, r, beam):
    """the float64 twin with formation tracking on a committed row, computed once and shared: (run, Forms)"""
    key = (family, V, r, beam)
    if key not in _runs:
        F = Forms()
        _runs[key] = (prefix_beam_search(rows_of(family, V)[r].astype(np.float64), beam, np.float64, forms=F), F)
    return _runs[key]


def tracked(lp, beam):
    F = Forms()
    return prefix_beam_search(np.asarray(lp, np.float64), beam, np.float64, forms=F), F


def check_run(run, F, G):
    """the acceptance rule on a tracked float64 run: None if accepted, else a description of the first offending pair"""
    exact = np.array(F.exact)
    for t, fr in enumerate(run["frames"]):
        tot, form = fr["tot"], fr["form"]
        for i in range(fr["n_sel"]):
            d = tot[i] - tot[i + 1:]
            near = (d < G) | (d == 0)
            ok = (form[i + 1:] == form[i]) | (exact[form[i + 1:]] & exact[form[i]] & (d == 0))
            bad = np.flatnonzero(near & ~ok)
            if len(bad):
                j = i + 1 + int(bad[0])
                return f"frame {t}: candidates {int(fr['idx'][i])} and {int(fr['idx'][j])} are {tot[i] - tot[j]:.3g} apart and not equally formed"
    hy = run["hyps"]
    for a, b in zip(hy, hy[1:]):
        d = a["score"] - b["score"]
        if (d < G or d == 0) and not (a["form"] == b["form"] or (F.exact[a["form"]] and F.exact[b["form"]] and d == 0)):
            return f"final scores {a['score']} and {b['score']} are not equally formed"
    return None


def check_case(lp, beam, G):
    """(accepted, the tracked float64 run, its Forms, the reason of a rejection)"""
    run, F = tracked(lp, beam)
    why = check_run(run, F, G)
    return why is None, run, F, why


def smallest_non_tie_gap(run):
    """the smallest positive difference between a selected candidate and any candidate behind it, and between final scores"""
    g = np.inf
    for fr in run["frames"]:
        tot = fr["tot"]
        for i in range(fr["n_sel"]):
            d = tot[i] - tot[i + 1:]
            d = d[d > 0]
            if len(d):
                g = min(g, float(d.min()))
    return g


def measured_e(lp, beam):
    """E of one (row, beam): the worst difference between the float32 and the float64 twin's gaps while their selections agree; whether
    the two agree in picks, tokens, timestamps and order; the worst difference of their final scores"""
    a, b = prefix_beam_search(np.asarray(lp, np.float64), beam, np.float64), prefix_beam_search(np.asarray(lp, np.float32), beam, np.float32)
    e = 0.0
    for t, (pa, pb) in enumerate(zip(a["picks"], b["picks"])):
        if pa != pb:
            return e, False, np.inf
        if np.isfinite(a["cut_gaps"][t]) and np.isfinite(b["cut_gaps"][t]):
            e = max(e, abs(a["cut_gaps"][t] - b["cut_gaps"][t]))
    for ga, gb in zip(a["rank_gaps"], b["rank_gaps"]):
        e = max(e, abs(ga - gb))
    same = [(h["tokens"], h["timestamps"]) for h in a["hyps"]] == [(h["tokens"], h["timestamps"]) for h in b["hyps"]]
    return e, same, max(abs(x["score"] - y["score"]) for x, y in zip(a["hyps"], b["hyps"]))


# ---- coverage ------------------------------------------------------------------------------------------------------------------------------
BEHIND = 8      # pairs are counted between a selected candidate and the ranked ones behind it plus the first BEHIND rejected ones
KINDS = ("ranked", "cut", "slots", "lower_slot_higher_column", "stay_ext", "thread", "thread_stride") + tuple(f"seam {a}|{b}" for a, b in SEAMS) + (
    "fold_tied_slot", "final", "floor_selected", "few_candidates")


def thread_of(k, v):
    return k if v == 0 else v % THREADS


def count_run(run, lp, beam, c):
    V = lp.shape[1]
    for t, fr in enumerate(run["frames"]):
        tot, idx, n_sel = fr["tot"], fr["idx"], fr["n_sel"]
        c["few_candidates"] += len(tot) < beam
        c["floor_selected"] += any(int(i) % V and lp[t, int(i) % V] == FLOOR for i in idx[:n_sel])
        c["cut"] += len(tot) > n_sel and tot[n_sel - 1] == tot[n_sel]
        st = fr["slot_tot"]
        for j, k in fr["folds"]:
            c["fold_tied_slot"] += any(st[q] == st[j] for q in range(len(st)) if q != j) or any(st[q] == st[k] for q in range(len(st)) if q != k)
        for i in range(n_sel):
            for j in range(i + 1, min(len(tot), n_sel + BEHIND)):
                if tot[j] != tot[i]:
                    break
                (ki, vi), (kj, vj) = divmod(int(idx[i]), V), divmod(int(idx[j]), V)
                c["ranked"] += j < n_sel
                c["slots"] += ki != kj
                c["lower_slot_higher_column"] += ki < kj and vi > vj >= 1
                c["stay_ext"] += (vi == 0) != (vj == 0)
                same_thread = thread_of(ki, vi) == thread_of(kj, vj)
                c["thread"] += same_thread
                c["thread_stride"] += same_thread and vi != vj and vi >= 1 and vj >= 1
                for a, b in SEAMS:
                    c[f"seam {a}|{b}"] += {vi, vj} == {a, b}
    hy = run["hyps"]
    c["final"] += sum(a["score"] == b["score"] for a, b in zip(hy, hy[1:]))


def admitted(family, V, beam):
    """the kinds that this family, V and beam can show at all"""
    mirrored = family == "mirrored"
    adm = {"cut"}
    if family == "dyadic" and V == 2:
        adm = set()                                 # one candidate per frame: nothing to tie with
    if beam >= 2 and V > 2:
        adm |= {"ranked", "final"}
    if beam >= 2 and V >= 9:
        adm |= {"slots", "lower_slot_higher_column", "thread"}
    if mirrored:
        adm |= {"stay_ext"} | ({"floor_selected"} if beam >= 2 else set())      # (at beam 1 the stay takes floor0's only slot)
        adm |= {f"seam {a}|{b}" for a, b in SEAMS if b < V}
        if beam >= 2:
            adm |= {"fold_tied_slot"}
        if V > 517:
            adm |= {"thread", "thread_stride"}
    if family == "dyadic" and ((V == 2 and beam >= 2) or (V == 9 and beam >= 6)):
        adm |= {"few_candidates"}
    return adm


def coverage(family, V, beam):
    """the counts of KINDS over the committed rows of (family, V) at one beam; raises on a zero wherever V and the beam admit the kind"""
    c = {k: 0 for k in KINDS}
    rows = rows_of(family, V)
    for r in range(rows.shape[0]):
        count_run(reference(family, V, r, beam)[0], rows[r], beam, c)
    c = {k: int(v) for k, v in c.items()}
    missing = [k for k in sorted(admitted(family, V, beam)) if c[k] == 0]
    if missing:
        raise AssertionError(f"{family} V={V} beam={beam}: no {missing} (counts {c})")
    return c


def find_seed(family, V, seeds=range(50)):
    """the first seed whose rows check_case accepts at every beam, with the G of the table"""
    gen = mirrored_rows if family == "mirrored" else dyadic_rows
    for seed in seeds:
        rows = gen(V, seed)
        if all(check_case(rows[r], beam, g_of(family, V))[0] for r in range(rows.shape[0]) for beam in BEAMS):
            return seed
    return None


# ---- the biased key tie: a dyadic row, a dyadic hotword bonus -------------------------------------------------------------------------------
# V = 9, two frames, blank at -inf, every column not named at -3.  The phrase [3, 6] earns 0.25 per matched token (TwinGraph: pending =
# 0.25 x depth; a partial match that breaks gives its 0.25 back).
#   frame 0: column 3 at -1.25, column 4 at -1.0.  Keys: [3] = -1.25 + 0.25 = -1.0 (biased), [4] = -1.0 (unbiased): a key tie of two
#            different acoustic totals; the lower flat index goes first: slot 0 = [3] (tot -1.25, ctx 0.25), slot 1 = [4] (tot -1.0).
#   frame 1: column 6 at -1.0, column 7 at -0.75.  [3] + 6 (flat 6): (-1.25 - 1.0) + (0.25 + 0.25) = -1.75, acoustic -2.25; [4] + 7 (flat
#            16): -1.75, acoustic -1.75: again a biased key against an unbiased one of another slot, flat 6 first.  Behind them [3] + 7
#            (flat 7: -2.0 + 0.25 - 0.25) and [4] + 6 (flat 15: -2.0) tie for rank 3.
#   final = (tot + ctx) - pending: [3, 6] (committed, nothing pending) -1.75 and [4, 7] -1.75: a final tie, the lower slot first.
BIAS_V, BIAS_BEAMS, BIAS_SCORE, BIAS_PHRASES = 9, (2, 3), 0.25, [[3, 6]]
BIAS_WANT = {2: [([3, 6], -1.75), ([4, 7], -1.75)], 3: [([3, 6], -1.75), ([4, 7], -1.75), ([3, 7], -2.0)]}


def bias_row():
    lp = np.full((2, BIAS_V), -np.inf, np.float32)
    lp[:, 1:] = -3.0
    lp[0, 3], lp[0, 4] = -1.25, -1.0
    lp[1, 6], lp[1, 7] = -1.0, -0.75
    return lp
