"""Keyword spotting on the transducer lattice restated in float64 (helper of test_kws.py / test_kws_gpu.py).

The definition is the text in include/k2hip.h ("Keyword spotting ...") and DESIGN.md.  The trie numbers its states in insertion order,
root = 0; state s has parent, tok, depth, kw (the keyword ending there or -1) and bar = depth * log(threshold).  Cells come from the
oracle's decoder / joiner operators (as tests/align_twin.py takes them) followed by a float64 log-softmax:
    stay(t,s) = logaddexp(lp(t,s,blank), lp(t,s,unk))
    emit(t,c) = lp(t, parent(c), tok(c))          c != root
with ctx(s) the last context_size ids of [blank] * context_size + path(s).  `token_passing` runs the recursion, the detection and the
reset, and can record every decision's margin over its error bound."""
import itertools

import numpy as np

BLANK, UNK = 0, 2


def build_trie(keywords, thresholds):
    """-> dict(parent, tok, depth, kw int arrays [S], bar float64 [S], children: per state {token: child})"""
    thr = np.broadcast_to(np.asarray(thresholds, np.float64), (len(keywords),))
    parent, tok, depth, kw, kids = [-1], [-1], [0], [-1], [{}]
    for p, word in enumerate(keywords):
        s = 0
        for v in word:
            v = int(v)
            if v not in kids[s]:
                kids[s][v] = len(parent)
                parent.append(s); tok.append(v); depth.append(depth[s] + 1); kw.append(-1); kids.append({})
            s = kids[s][v]
        assert kw[s] < 0, "duplicate keyword"
        kw[s] = p
    bar = np.array([depth[s] * np.log(thr[kw[s]]) if kw[s] >= 0 else 0.0 for s in range(len(parent))])
    return dict(parent=np.array(parent), tok=np.array(tok), depth=np.array(depth), kw=np.array(kw), bar=bar, children=kids)


def contexts(trie, cs):
    S = len(trie["parent"])
    ctx = np.full((S, cs), BLANK, np.int64)
    for s in range(1, S):
        ctx[s, :-1] = ctx[trie["parent"][s], 1:]
        ctx[s, -1] = trie["tok"][s]
    return ctx


def trie_cells(oracle, enc, trie):
    """enc [T, J] -> (stay, emit) float64 [T][S]; emit[:, 0] = -inf"""
    S, T = len(trie["parent"]), enc.shape[0]
    dec = oracle.decoder(contexts(trie, oracle.context_size))                  # [S, J]
    stay = np.empty((T, S))
    emit = np.full((T, S), -np.inf)
    for t in range(T):
        logits = np.asarray(oracle.joiner(np.repeat(enc[t: t + 1], S, 0), dec), np.float64)   # [S, V]
        m = logits.max(axis=1, keepdims=True)
        lp = logits - (m + np.log(np.exp(logits - m).sum(axis=1, keepdims=True)))
        stay[t] = np.logaddexp(lp[:, BLANK], lp[:, UNK])
        if S > 1:
            emit[t, 1:] = lp[trie["parent"][1:], trie["tok"][1:]]
    return stay, emit


def fresh_state(S):
    a = np.full(S, -np.inf)
    a[0] = 0.0
    start = np.full(S, -1, np.int64)
    start[0] = 0
    return a, start


def token_passing(trie, stay, emit, a=None, start=None, ratios=None, tol=None):
    """frames stay / emit [T][S] from the carried block (a, start) (fresh when None) -> (events, a, start); an event is
    (keyword, start, end, sum_logp).  start[0] is the stream's frame count.  With `ratios` (a list) and `tol` (the bound of one
    cell), every decision that an event depends on appends margin / bound: the threshold test of every terminal's emit-entered value
    (bound: its arcs x tol), the predecessor choice at a terminal whose emit value reaches its bar and along every winning path (bound:
    the arcs of both sides x tol), and the choice among candidates of one depth (bound: the arcs of both x tol)."""
    parent, depth, kw, bar = trie["parent"], trie["depth"], trie["kw"], trie["bar"]
    S, T = len(parent), stay.shape[0]
    if a is None:
        a, start = fresh_state(S)
    a, start = a.copy(), start.copy()
    events = []
    hist = []      # since the last event: per frame (ve, vs, by_emit, starts before the frame)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            ta = int(start[0])
            na, ns = np.full(S, -np.inf), np.full(S, -1, np.int64)
            ve_, vs_, by = np.full(S, -np.inf), np.full(S, -np.inf), np.zeros(S, bool)
            sp_ = np.full(S, -1, np.int64)
            for c in range(1, S):
                p = parent[c]
                ap, sp = (0.0, ta) if p == 0 else (a[p], start[p])
                ve, vs = ap + emit[t, c], a[c] + stay[t, c]
                e = bool(ve >= vs)
                na[c], ns[c] = (ve, sp) if e else (vs, start[c])
                if not na[c] > -np.inf:
                    ns[c] = -1
                ve_[c], vs_[c], by[c], sp_[c] = ve, vs, e, sp
            hist.append((ve_, vs_, by, sp_, start.copy(), ta))
            cand = [c for c in range(1, S) if kw[c] >= 0 and by[c] and na[c] >= bar[c]]
            if ratios is not None:
                for c in range(1, S):
                    if kw[c] < 0 or not ve_[c] > -np.inf:
                        continue
                    n_e = ta - sp_[c] + 1
                    ratios.append(abs(ve_[c] - bar[c]) / (n_e * tol))
                    if ve_[c] >= bar[c] and vs_[c] > -np.inf:
                        ratios.append(abs(ve_[c] - vs_[c]) / ((n_e + ta - start[c] + 1) * tol))
                for c1, c2 in itertools.combinations(cand, 2):
                    if depth[c1] == depth[c2]:
                        ratios.append(abs(na[c1] - na[c2]) / ((2 * ta - ns[c1] - ns[c2] + 2) * tol))
            if cand:
                win = min(cand, key=lambda c: (-depth[c], -na[c], kw[c]))
                events.append((int(kw[win]), int(ns[win]), ta, float(na[win])))
                if ratios is not None:   # the predecessor choices along the winning path, backwards
                    c = win
                    for ve_h, vs_h, by_h, _, st_h, ta_h in reversed(hist):
                        if c == 0:
                            break
                        if ve_h[c] > -np.inf and vs_h[c] > -np.inf:
                            p = parent[c]
                            n_e = ta_h - (ta_h if p == 0 else st_h[p]) + 1
                            ratios.append(abs(ve_h[c] - vs_h[c]) / ((n_e + ta_h - st_h[c] + 1) * tol))
                        if by_h[c]:
                            c = parent[c]
                na[1:], ns[1:] = -np.inf, -1
                hist = []
            na[0], ns[0] = 0.0, ta + 1
            a, start = na, ns
    return events, a, start


def brute_force_frame(trie, stay, emit, t, R):
    """the values after frame t by enumerating every path whose emits all lie after frame R (the last event): per non-root state
    (best value, entered by its emit arc at t under the emit-wins tie rule, the set of start frames of the best paths)"""
    parent = trie["parent"]
    S = len(parent)
    out = {}
    for c in range(1, S):
        chain = [c]
        while parent[chain[-1]] != 0:
            chain.append(parent[chain[-1]])
        chain.reverse()                                   # root's child .. c
        d = len(chain)
        best, by_emit, starts = -np.inf, True, set()
        paths = [(es, _path(stay, emit, chain, es, t)) for es in itertools.combinations(range(R + 1, t + 1), d)]   # emit frames e_1 < .. < e_d
        for es, v in paths:
            if v > best:
                best, starts = v, {es[0]}
            elif v == best:
                starts.add(es[0])
        if best > -np.inf:
            by_emit = any(es[-1] == t and v == best for es, v in paths)
        out[c] = (best, by_emit, starts)
    return out


def _path(stay, emit, chain, es, t):
    v = 0.0
    for i, e in enumerate(es):
        v += emit[e, chain[i]]
        nxt = es[i + 1] if i + 1 < len(es) else t + 1
        v += sum(stay[f, chain[i]] for f in range(e + 1, nxt))
    return v
