"""Keyword spotting on the CTC trellis restated in float64 (helper of test_ctc_kws.py / test_ctc_kws_gpu.py).

The definition is the text in include/k2hip.h ("Keyword spotting for CTC models").  The trie is kws_twin.build_trie's; rc(s) is the
root's child whose token equals tok(s), or -1.  A stream's carried block is v [2][S] / st [2][S]: plane 0 = n (the path's last frame
carried tok(c)), plane 1 = b (blanks after tok(c)); the root's n entry is (0, frame count), the root's b entry is (-inf, hold).
`token_passing` runs the recursion, the hold rule, the detection and the reset, and can record every comparison's gap.
`brute_force_frame` enumerates frame labellings explicitly."""
import itertools

import numpy as np

from kws_twin import build_trie  # noqa: F401  (re-exported)

BLANK = 0


def root_children(trie):
    S = len(trie["parent"])
    rc = np.full(S, -1, np.int64)
    for s in range(1, S):
        rc[s] = trie["children"][0].get(int(trie["tok"][s]), -1) if "children" in trie else next(
            (r for r in range(1, S) if trie["parent"][r] == 0 and trie["tok"][r] == trie["tok"][s]), -1)
    return rc


def fresh_state(S):
    v = np.full((2, S), -np.inf)
    st = np.full((2, S), -1, np.int64)
    v[0, 0], st[0, 0] = 0.0, 0
    return v, st


def token_passing(trie, lp, v=None, st=None, hold_rule=True, gaps=None, trace=None):
    """lp [T][V] -> (events [(keyword, start, end, sum_logp)], v, st).  gaps (a list): the absolute difference of the two sides of every
    comparison between finite values -- predecessor choices, the b choice, threshold tests of entered terminals, choices among
    candidates, hold tests.  trace (a list): per frame the root child closed by the hold, or -1.  hold_rule=False: the hold never closes
    an arc (what the fixture test compares against)."""
    parent, tok, depth, kw, bar = (trie[k] for k in ("parent", "tok", "depth", "kw", "bar"))
    rc = root_children(trie)
    S = len(parent)
    if v is None:
        v, st = fresh_state(S)
    v, st = v.copy(), st.copy()
    events = []

    def better(a, b):   # a strictly better than b, the gap recorded
        if gaps is not None and np.isfinite(a) and np.isfinite(b):
            gaps.append(abs(a - b))
        return a > b

    for row in np.asarray(lp, np.float64):
        n, b, sn, sb = v[0], v[1], st[0], st[1]
        ta, hold = int(sn[0]), int(sb[0])
        closed = False
        if hold >= 0:
            if gaps is not None and np.isfinite(row[tok[hold]]) and np.isfinite(row[0]):
                gaps.append(abs(row[tok[hold]] - row[0]))
            if row[tok[hold]] >= row[0]:
                closed = hold_rule
            else:
                hold = -1
        if trace is not None:
            trace.append(hold if closed else -1)
        nn, nb = np.full(S, -np.inf), np.full(S, -np.inf)
        nsn, nsb = np.full(S, -1, np.int64), np.full(S, -1, np.int64)
        entered = np.zeros(S, bool)
        for c in range(1, S):
            p = parent[c]
            best, bs = -np.inf, -1
            if p == 0:
                if not (closed and c == hold):
                    best, bs = 0.0, ta
            else:
                if tok[p] != tok[c]:
                    best, bs = n[p], sn[p]
                if better(b[p], best):
                    best, bs = b[p], sb[p]
            self_loop = False
            if better(n[c], best):
                best, bs, self_loop = n[c], sn[c], True
            nn[c] = best + row[tok[c]]
            nsn[c] = bs if nn[c] > -np.inf else -1
            entered[c] = (not self_loop) and nn[c] > -np.inf
            from_n = not better(b[c], n[c])
            nb[c] = (n[c] if from_n else b[c]) + row[0]
            nsb[c] = (sn[c] if from_n else sb[c]) if nb[c] > -np.inf else -1
        cand = []
        for c in range(1, S):
            if kw[c] >= 0 and entered[c]:
                if gaps is not None:
                    gaps.append(abs(nn[c] - bar[c]))
                if nn[c] >= bar[c]:
                    cand.append(c)
        if cand:
            win = min(cand, key=lambda c: (-depth[c], -nn[c], kw[c]))
            if gaps is not None:
                gaps += [abs(nn[c] - nn[win]) for c in cand if c != win and depth[c] == depth[win]]
            events.append((int(kw[win]), int(nsn[win]), ta, float(nn[win])))
            hold = int(rc[win])
            nn[:], nb[:], nsn[:], nsb[:] = -np.inf, -np.inf, -1, -1
        nn[0], nsn[0], nb[0], nsb[0] = 0.0, ta + 1, -np.inf, hold
        v, st = np.stack([nn, nb]), np.stack([nsn, nsb])
    return events, v, st


def path_of(trie, c):
    out = []
    while c > 0:
        out.append(int(trie["tok"][c]))
        c = int(trie["parent"][c])
    return out[::-1]


def collapse(labels):
    out, prev = [], BLANK
    for x in labels:
        if x != BLANK and x != prev:
            out.append(x)
        prev = x
    return out


def brute_force_frame(trie, lp, t, R, closed):
    """After frame t with the last event at frame R (-1: none): for every non-root state c the best labelling of frames s..t, R < s <= t,
    over the symbols {path(c)'s tokens, blank} whose first label is a token (the keyword begins at s), that collapses to path(c), and that
    does not begin through a closed root arc (closed[s] = the root child the hold closes at frame s, or -1).
    -> {c: (n, entered, starts_n, b, starts_b)}: n over the labellings ending on tok(c), entered = a best one is no self loop (the last two
    labels are not both tok(c)), b over those ending on a blank; starts_*: the start frames of the best ones."""
    out = {}
    for c in range(1, len(trie["parent"])):
        path = path_of(trie, c)
        symbols = sorted(set(path)) + [BLANK]
        first = int(trie["children"][0][path[0]])   # the root child the labellings enter through
        best = {"n": (-np.inf, set()), "b": (-np.inf, set())}
        best_entry = -np.inf   # the best labelling ending on tok(c) that is no self loop
        for s in range(R + 1, t + 1):
            if closed[s] == first:
                continue
            for labels in itertools.product(symbols, repeat=t - s + 1):
                if labels[0] == BLANK or collapse(labels) != path:
                    continue
                val = sum(lp[s + i, x] for i, x in enumerate(labels))
                if val == -np.inf:
                    continue
                key = "b" if labels[-1] == BLANK else "n"
                if val > best[key][0]:
                    best[key] = (val, {s})
                elif val == best[key][0]:
                    best[key][1].add(s)
                if key == "n" and not (len(labels) >= 2 and labels[-2] == labels[-1]):
                    best_entry = max(best_entry, val)
        n, b = best["n"], best["b"]
        out[c] = (n[0], n[0] > -np.inf and best_entry == n[0], n[1], b[0], b[1])
    return out
