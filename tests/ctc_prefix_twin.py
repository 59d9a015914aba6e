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
    __slots__ = ("tokens", "timestamps", "token_log_probs", "pb", "pnb", "tot", "node", "parent_node", "fpb", "fpnb", "ftot")


class Forms:
    """How a score was formed: hash-consed expressions over the float32 INPUT VALUES (a leaf is a value's bits, not its place: two
    columns at one level are one leaf).  `add` and `logaddexp` are unordered binary nodes (both are commutative bit for bit: IEEE
    addition, and m + log1p(exp(n - m)) with m the larger); x + 0 is x; anything with -inf short-circuits as the kernel does (a sum is
    -inf, a logaddexp returns its other operand untouched).  Id 0 is -inf.  Equal ids mean bit-equal scores on ANY implementation that
    follows the definition's operations, whatever its exp / log1p.  exact[id]: no logaddexp with two finite operands anywhere in the
    history and every sum's value (as the run computed it) a float32 -- such a score is the same number in float32 and float64."""

    def __init__(self):
        self.ids, self.exact = {}, [True]
        self.zero = self.leaf(np.float32(0))

    def _get(self, key, exact):
        i = self.ids.get(key)
        if i is None:
            i = self.ids[key] = len(self.exact)
            self.exact.append(bool(exact))
        return i

    def leaf(self, x):
        x = np.float32(x)
        if x == -np.inf:
            return 0
        return self._get(("in", int((x + np.float32(0)).view(np.int32))), True)      # (-0.0 + 0.0 = +0.0: one zero)

    def add(self, a, b, value):
        if a == 0 or b == 0:
            return 0
        if a == self.zero:
            return b
        if b == self.zero:
            return a
        return self._get(("add", min(a, b), max(a, b)), self.exact[a] and self.exact[b] and float(np.float32(value)) == float(value))

    def lae(self, a, b):
        if a == 0:
            return b
        if b == 0:
            return a
        return self._get(("lae", min(a, b), max(a, b)), False)


THREADS = 256      # the kernel's workgroup: thread v mod 256 holds column v of every slot, thread k slot k's stay candidate
# deliberately WRONG searches (tests/test_ctc_prefix_tie_cases_ref.py shows that the tie cases tell each from the definition)
RULES = ("higher_index", "column_before_slot", "thread_keeps_later", "thread_list_short", "extension_beats_stay", "fold_later_timestamps",
         "fold_skipped_on_tie", "final_last_first")
SELECTION_RULES = RULES[:5]      # the ones that break a frame's selection; the others break a fold or the final order


def _wrong_selection(cands, beam, V, rule):
    """the first `beam` of `cands` (sorted by the definition) under a broken selection rule"""
    if rule == "higher_index":
        return sorted(cands, key=lambda c: (-c[0], -c[1]))[:beam]
    if rule == "column_before_slot":
        return sorted(cands, key=lambda c: (-c[0], c[1] % V, c[1] // V))[:beam]
    if rule == "extension_beats_stay":
        return sorted(cands, key=lambda c: (-c[0], c[1] % V == 0, c[1]))[:beam]
    # the per-thread lists, then `beam` rounds over the lists' heads in the definition's order
    lists = {}
    for c in cands:
        k, v = divmod(c[1], V)
        lists.setdefault(k if v == 0 else v % THREADS, []).append(((0, 0, k) if v == 0 else (1, v, k), c))
    for th, lst in lists.items():
        lst.sort(key=lambda e: e[0])                 # a thread's insertion order: its stay candidate, then columns up, slots up
        if rule == "thread_keeps_later":             # `>=` in the insertion: an equal entry goes in FRONT of the earlier ones
            seq = sorted(range(len(lst)), key=lambda i: (-lst[i][1][0], -i))[:beam]
        else:                                        # "thread_list_short": a list of beam - 1 entries
            seq = sorted(range(len(lst)), key=lambda i: (-lst[i][1][0], lst[i][1][1]))[: max(beam - 1, 1)]
        lists[th] = [lst[i][1] for i in seq]
    out = []
    for _ in range(beam):
        best = None
        for th, lst in lists.items():
            if lst and (best is None or (-lst[0][0], lst[0][1]) < (-lists[best][0][0], lists[best][0][1])):
                best = th
        if best is None:
            break
        out.append(lists[best].pop(0))
    return out


def prefix_beam_search(lp, beam, dtype=np.float64, forms=None, rule=None):
    """lp [T][V] (the frames that count) -> dict(hyps: the live slots after the last frame in rank order, each dict(tokens, timestamps,
    token_log_probs, score, pb, pnb); cut_gaps [T]: per frame, total of the last selected minus total of the first rejected candidate
    (inf where nothing was rejected); rank_gaps: the gaps between consecutive selected ranks of the last frame; respelled_folds: folds
    into a slot whose history parent is not the folded slot's node; picks [T]: the selected flat indexes per frame).
    forms: a Forms table -- every score then also carries how it was formed (hyps get "form"; "frames" [T] holds per frame dict(tot, idx,
    form: arrays over ALL finite candidates in the definition's order, n_sel, folds [(j, k)], slot_tot: the live slots' totals before
    the frame)).  rule: one of RULES, a deliberately wrong search; None is the definition."""
    assert rule is None or rule in RULES, rule
    dt = np.dtype(dtype).type
    lp = np.asarray(lp, dtype)
    T, V = lp.shape
    ninf = dt(-np.inf)
    F = forms
    h0 = _Hyp()
    h0.tokens, h0.timestamps, h0.token_log_probs = [], [], []
    h0.pb, h0.pnb, h0.tot, h0.node, h0.parent_node = dt(0), ninf, dt(0), -1, -1
    h0.fpb, h0.fpnb, h0.ftot = (F.zero, 0, F.zero) if F else (None, None, None)
    cur, next_node, respelled = [h0], 0, 0
    cut_gaps, picks, rank_gaps, frames = [], [], [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            row = lp[t]
            rf = [F.leaf(x) for x in row] if F else None
            n = len(cur)
            fold_par = [-1] * n
            for j in range(n):
                for k in range(n):
                    if j != k and cur[j].tokens[:-1] == cur[k].tokens and len(cur[j].tokens) == len(cur[k].tokens) + 1:
                        fold_par[j] = k
                        respelled += cur[j].parent_node != cur[k].node
            cands = []   # (total, flat index, pb, pnb, form of the total, of pb, of pnb)
            for k, h in enumerate(cur):
                e = h.tokens[-1] if h.tokens else -1
                spb = dt(h.tot + row[0])
                spnb = dt(h.pnb + row[e]) if e >= 0 else ninf
                fspb = F.add(h.ftot, rf[0], spb) if F else None
                fspnb = (F.add(h.fpnb, rf[e], spnb) if e >= 0 else 0) if F else None
                if fold_par[k] >= 0 and not (rule == "fold_skipped_on_tie" and cur[fold_par[k]].tot == h.tot):
                    p = cur[fold_par[k]]
                    ep = p.tokens[-1] if p.tokens else -1
                    x = dt((p.pb if e == ep else p.tot) + row[e])
                    if F:
                        fspnb = F.lae(fspnb, F.add(p.fpb if e == ep else p.ftot, rf[e], x))
                    spnb = _lae(spnb, x, dt)
                cands.append((_lae(spb, spnb, dt), k * V, spb, spnb, F.lae(fspb, fspnb) if F else None, fspb, fspnb))
                folded = {cur[j].tokens[-1] for j in range(n) if fold_par[j] == k}
                for v in range(1, V):
                    if v in folded:
                        continue
                    x = dt((h.pb if v == e else h.tot) + row[v])
                    fx = F.add(h.fpb if v == e else h.ftot, rf[v], x) if F else None
                    cands.append((x, k * V + v, ninf, x, fx, 0, fx))
            stay0 = cands[0]
            cands = [c for c in cands if c[0] > ninf]
            cands.sort(key=lambda c: (-c[0], c[1]))
            if not cands:
                cands = [stay0]
            sel = _wrong_selection(cands, beam, V, rule) if rule in SELECTION_RULES else cands[:beam]
            cut_gaps.append(float(sel[-1][0] - cands[beam][0]) if len(cands) > beam else np.inf)
            rank_gaps = [float(a[0] - b[0]) for a, b in zip(sel, sel[1:])]
            picks.append([c[1] for c in sel])
            if F:
                frames.append(dict(tot=np.array([c[0] for c in cands], np.float64), idx=np.array([c[1] for c in cands], np.int64),
                                   form=np.array([c[4] for c in cands], np.int64), n_sel=len(sel),
                                   folds=[(j, fold_par[j]) for j in range(n) if fold_par[j] >= 0], slot_tot=[float(h.tot) for h in cur]))
            nxt = []
            for tot, idx, pb, pnb, ftot, fpb, fpnb in sel:
                k, v = divmod(idx, V)
                src = cur[k]
                h = _Hyp()
                h.tokens, h.timestamps, h.token_log_probs = list(src.tokens), list(src.timestamps), list(src.token_log_probs)
                h.pb, h.pnb, h.tot, h.node, h.parent_node = pb, pnb, tot, src.node, src.parent_node
                h.fpb, h.fpnb, h.ftot = fpb, fpnb, ftot
                if v:
                    h.tokens.append(v)
                    h.timestamps.append(t)
                    h.token_log_probs.append(row[v])
                    h.parent_node, h.node = src.node, next_node
                    next_node += 1
                elif rule == "fold_later_timestamps" and fold_par[k] >= 0:      # the folded path's frames in place of the slot's own
                    h.timestamps = list(cur[fold_par[k]].timestamps) + [t]
                nxt.append(h)
            cur = nxt
    if rule == "final_last_first":
        cur = sorted(cur, key=lambda h: -h.tot)[::-1]
        cur.sort(key=lambda h: -h.tot)               # (stable: equal totals stay reversed)
    hyps = [dict(tokens=h.tokens, timestamps=h.timestamps, token_log_probs=np.array(h.token_log_probs, dtype), score=float(h.tot),
                 pb=float(h.pb), pnb=float(h.pnb)) for h in cur]
    res = dict(hyps=hyps, cut_gaps=cut_gaps, rank_gaps=rank_gaps, respelled_folds=int(respelled), picks=picks)
    if F:
        for d, h in zip(hyps, cur):
            d["form"] = h.ftot
        res["frames"] = frames
    return res


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
