"""CTC prefix beam search with N-best restated in numpy (helper of test_ctc_prefix.py / test_ctc_prefix_gpu.py).

The definition is the text in include/k2hip.h ("CTC prefix beam search with N-best") and DESIGN.md; csrc/ctc_prefix_ref.h is the same in
C++.  lp [T][V] are log-softmaxed rows.  A live hypothesis is a prefix y with pb (paths ending in blank), pnb (paths ending in y's last
token), tot = logaddexp(pb, pnb); the start is the empty prefix with pb = 0, pnb = -inf.  Per frame: the stay candidate of slot k (flat
index k V) has spb = tot_k + lp(t, 0), spnb = pnb_k + lp(t, e_k); the extension of slot k by v has x = (v == e_k ? pb_k : tot_k) +
lp(t, v) and -- if a live slot j spells y_k + [v] AS A TOKEN SEQUENCE -- joins j's stay candidate (spnb_j = logaddexp(spnb_j, x)),
otherwise it is the candidate k V + v.  Candidates at -inf are dropped, the rest ordered by (total desc, flat index asc), the first
`beam` are the new slots in that order; with none left slot 0's stay candidate survives.  The dtype is the caller's: float64 is the
yardstick, float32 shows how far the device's number format can move a score."""
import itertools

import numpy as np

BLANK = 0


def collapse(labels):
    out, prev = [], -1
    for v in labels:
        if v != BLANK and v != prev:
            out.append(int(v))
        prev = v
    return out


def _lae(a, b, dt):
    m, n = (a, b) if a > b else (b, a)
    if n == -np.inf:
        return dt(m)
    return dt(m + np.log1p(np.exp(dt(n - m))))


class _Hyp:
    __slots__ = ("tokens", "timestamps", "token_log_probs", "pb", "pnb", "tot", "node", "parent_node")


def prefix_beam_search(lp, beam, dtype=np.float64):
    """lp [T][V] (the frames that count) -> dict(hyps: the live slots after the last frame in rank order, each dict(tokens, timestamps,
    token_log_probs, score, pb, pnb); cut_gaps [T]: per frame, total of the last selected minus total of the first rejected candidate
    (inf where nothing was rejected); rank_gaps: the gaps between consecutive selected ranks of the last frame; respelled_folds: folds
    into a slot whose history parent is not the folded slot's node; picks [T]: the selected flat indexes per frame)"""
    dt = np.dtype(dtype).type
    lp = np.asarray(lp, dtype)
    T, V = lp.shape
    ninf = dt(-np.inf)
    h0 = _Hyp()
    h0.tokens, h0.timestamps, h0.token_log_probs = [], [], []
    h0.pb, h0.pnb, h0.tot, h0.node, h0.parent_node = dt(0), ninf, dt(0), -1, -1
    cur, next_node, respelled = [h0], 0, 0
    cut_gaps, picks, rank_gaps = [], [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            row = lp[t]
            n = len(cur)
            fold_par = [-1] * n
            for j in range(n):
                for k in range(n):
                    if j != k and cur[j].tokens[:-1] == cur[k].tokens and len(cur[j].tokens) == len(cur[k].tokens) + 1:
                        fold_par[j] = k
                        respelled += cur[j].parent_node != cur[k].node
            cands = []   # (total, flat index, pb, pnb)
            for k, h in enumerate(cur):
                e = h.tokens[-1] if h.tokens else -1
                spb = dt(h.tot + row[0])
                spnb = dt(h.pnb + row[e]) if e >= 0 else ninf
                if fold_par[k] >= 0:
                    p = cur[fold_par[k]]
                    ep = p.tokens[-1] if p.tokens else -1
                    spnb = _lae(spnb, dt((p.pb if e == ep else p.tot) + row[e]), dt)
                cands.append((_lae(spb, spnb, dt), k * V, spb, spnb))
                folded = {cur[j].tokens[-1] for j in range(n) if fold_par[j] == k}
                for v in range(1, V):
                    if v in folded:
                        continue
                    x = dt((h.pb if v == e else h.tot) + row[v])
                    cands.append((x, k * V + v, ninf, x))
            stay0 = cands[0]
            cands = [c for c in cands if c[0] > ninf]
            cands.sort(key=lambda c: (-c[0], c[1]))
            if not cands:
                cands = [stay0]
            sel = cands[:beam]
            cut_gaps.append(float(sel[-1][0] - cands[beam][0]) if len(cands) > beam else np.inf)
            rank_gaps = [float(a[0] - b[0]) for a, b in zip(sel, sel[1:])]
            picks.append([c[1] for c in sel])
            nxt = []
            for tot, idx, pb, pnb in sel:
                k, v = divmod(idx, V)
                src = cur[k]
                h = _Hyp()
                h.tokens, h.timestamps, h.token_log_probs = list(src.tokens), list(src.timestamps), list(src.token_log_probs)
                h.pb, h.pnb, h.tot, h.node, h.parent_node = pb, pnb, tot, src.node, src.parent_node
                if v:
                    h.tokens.append(v)
                    h.timestamps.append(t)
                    h.token_log_probs.append(row[v])
                    h.parent_node, h.node = src.node, next_node
                    next_node += 1
                nxt.append(h)
            cur = nxt
    hyps = [dict(tokens=h.tokens, timestamps=h.timestamps, token_log_probs=np.array(h.token_log_probs, dtype), score=float(h.tot),
                 pb=float(h.pb), pnb=float(h.pnb)) for h in cur]
    return dict(hyps=hyps, cut_gaps=cut_gaps, rank_gaps=rank_gaps, respelled_folds=int(respelled), picks=picks)


def min_gap(res):
    """the smallest reported gap of a run: every frame's cut gap and the last frame's rank gaps"""
    return min([g for g in res["cut_gaps"]] + list(res["rank_gaps"]) + [np.inf])


def brute_force(lp):
    """{collapsed prefix (tuple): (full sum, sum over paths ending in blank, sum over paths ending in the last token)} over every
    labelling of the T frames, float64"""
    lp = np.asarray(lp, np.float64)
    T, V = lp.shape
    acc = {}
    for lab in itertools.product(range(V), repeat=T):
        s = float(lp[np.arange(T), list(lab)].sum())
        key = tuple(collapse(lab))
        a = acc.setdefault(key, [-np.inf, -np.inf, -np.inf])
        a[0] = np.logaddexp(a[0], s)
        i = 1 if lab[-1] == BLANK else 2
        a[i] = np.logaddexp(a[i], s)
    return {k: tuple(v) for k, v in acc.items()}


def seeded_log_probs(seed, T, V, scale=1.0):
    """seeded normal logits, log-softmaxed in float64, rounded to float32 (the inputs of the GPU tests)"""
    z = np.random.default_rng(seed).standard_normal((T, V)) * scale
    z = z - z.max(axis=1, keepdims=True)
    return (z - np.log(np.exp(z).sum(axis=1, keepdims=True))).astype(np.float32)


def find_respelled(seeds, V, T, beam):
    """the first seed of `seeds` on which the float64 twin counts a re-spelled fold, or None"""
    for seed in seeds:
        if prefix_beam_search(seeded_log_probs(seed, T, V, 2.0), beam)["respelled_folds"] > 0:
            return seed
    return None
