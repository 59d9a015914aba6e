"""Hotword and n-gram LM biasing of the CTC prefix beam search restated in numpy (helper of test_ctc_prefix_bias.py /
test_ctc_prefix_bias_gpu.py).

The definition is the text in include/k2hip.h ("Hotword and n-gram LM biasing of the CTC prefix beam search") and DESIGN.md;
csrc/ctc_prefix_bias_ref.h is the same in C++.  It is ctc_prefix_twin.prefix_beam_search with three more values per live slot: hs (state
of hotword_twin.TwinGraph, start 0), ls (state of an already SCALED ngram_twin.TwinLm, start lm.start) and ctx (the accumulated context
score, start 0), all functions of the slot's token sequence alone.  pb / pnb / tot stay purely acoustic.  Per frame:
    stay candidate of slot k        key = st_k + ctx_k
    extension k V + v, not folded   cb = ctx_k + bonus[hs_k][v], key = x + cb        (the hotword bonus takes part in the selection)
a candidate is dropped when its ACOUSTIC total is -inf; the rest are ordered by (key desc, flat index asc); the first `beam` are the new
slots in that order.  A selected extension takes hs' = next[hs_k][v], then (term, ls') = Step(ls_k, v) and ctx' = cb + term -- the LM
term is in no key of that frame, in every later one.  Unk (2) leaves both states alone and earns nothing; a slot that receives a fold
keeps its own hs / ls / ctx.  After the last frame final_q = (tot_q + ctx_q) - pending[hs_q]; the entries are ordered by (final desc,
slot asc).  The dtype is the caller's, as in ctc_prefix_twin.

`bonus_after_selection=True` is the deliberately WEAKER stand-in: the bonus of an extension joins ctx only once it is selected (key =
x + ctx_k), as the transducer search does it.  test_ctc_prefix_bias.py shows that the committed cases tell the two apart."""
import numpy as np

from ctc_prefix_twin import _lae

BLANK, UNK = 0, 2
HW_EVENTS = ("bonus", "broken", "committed")
LM_EVENTS = ("full", "back1", "uni", "unk")


def dense_graph(graph):
    """next [S][V] int32, bonus [S][V] float32, pending [S] float32 of a hotword_twin.TwinGraph (what the model uploads)"""
    S, V = graph.num_states, graph.V
    nxt, bonus = np.zeros((S, V), np.int32), np.zeros((S, V), np.float32)
    for s in range(S):
        for v in range(V):
            n, b, _ = graph.step(s, v)
            nxt[s, v], bonus[s, v] = n, b
    return nxt, bonus, np.array([graph.pending(s) for s in range(S)], np.float32)


def lm_tables(lm):
    """the sparse device form of an already scaled ngram_twin.TwinLm: dict(states [S][4] int32 = (arc begin, arc end, back-off state,
    back-off weight bits), arc_tok / arc_lp / arc_next [A], uni_lp / uni_next [V], start)"""
    states, tok, alp, anx = [], [], [], []
    for h in lm.hist:
        arcs = sorted(k[-1] for k in lm.lp if k[:-1] == h and len(k) == len(h) + 1) if h else []
        lo = len(tok)
        for w in arcs:
            tok.append(w)
            alp.append(lm.lp[h + (w,)])
            anx.append(lm.state_of[lm._longest_state(h + (w,), lm.N - 1)])
        bo = lm.state_of[lm._longest_state(h, len(h) - 1)] if h else 0
        bow = np.float32(lm.bo[h]) if h else np.float32(0)
        states.append([lo, len(tok), bo, int(np.array([bow], np.float32).view(np.int32)[0])])
    uni_lp, uni_next = np.zeros(lm.V, np.float32), np.zeros(lm.V, np.int32)
    for v in range(lm.V):
        if v in (BLANK, UNK):
            continue
        if (v,) in lm.lp:
            uni_lp[v], uni_next[v] = lm.lp[(v,)], lm.state_of[lm._longest_state((v,), lm.N - 1)]
        else:
            uni_lp[v] = lm.unk
    return dict(states=np.array(states, np.int32).reshape(-1, 4), arc_tok=np.array(tok, np.int32), arc_lp=np.array(alp, np.float32),
                arc_next=np.array(anx, np.int32), uni_lp=uni_lp, uni_next=uni_next, start=int(lm.start))


def walk(tokens, graph=None, lm=None, dtype=np.float64):
    """(ctx, hs, ls) of a token sequence: the same additions in the same order as the search makes them"""
    dt = np.dtype(dtype).type
    ctx, hs, ls = dt(0), 0, (lm.start if lm is not None else 0)
    for v in tokens:
        if graph is not None:
            hs, b, _ = graph.step(hs, v)
            ctx = dt(ctx + dt(b))
        if lm is not None and v not in (BLANK, UNK):
            ls, term, _ = lm.step(ls, v)
            ctx = dt(ctx + dt(term))
    return ctx, hs, ls


class _Hyp:
    __slots__ = ("tokens", "timestamps", "token_log_probs", "pb", "pnb", "tot", "node", "parent_node", "hs", "ls", "ctx")


def biased_prefix_beam_search(lp, beam, graph=None, lm=None, dtype=np.float64, bonus_after_selection=False, lae=_lae):
    """lp [T][V] (the frames that count); graph: a TwinGraph or None; lm: a SCALED TwinLm or None; lae(a, b, dt): the logaddexp (numpy's by
    default; test_ctc_prefix_bias.py passes the C library's expf / log1pf to meet the host reference bit for bit).  Returns dict(hyps: the final
    entries in (final desc, slot asc) order, each dict(tokens, timestamps, token_log_probs, score (= final), tot, ctx, hs, ls, slot);
    cut_gaps [T]: per frame, key of the last selected minus key of the first rejected candidate (inf where nothing was rejected);
    final_gaps: the gaps between consecutive finals; events: counts over the selected extensions; respelled_folds; picks [T])"""
    dt = np.dtype(dtype).type
    lp = np.asarray(lp, dtype)
    T, V = lp.shape
    ninf = dt(-np.inf)
    if graph is not None:
        g_next, g_bonus, g_pending = dense_graph(graph)
        g_end = {(s, v): graph.step(s, v)[2] for s in range(graph.num_states) for v in range(V)}
    h0 = _Hyp()
    h0.tokens, h0.timestamps, h0.token_log_probs = [], [], []
    h0.pb, h0.pnb, h0.tot, h0.node, h0.parent_node = dt(0), ninf, dt(0), -1, -1
    h0.hs, h0.ls, h0.ctx = 0, (lm.start if lm is not None else 0), dt(0)
    cur, next_node, respelled = [h0], 0, 0
    cut_gaps, picks = [], []
    events = {k: 0 for k in HW_EVENTS + LM_EVENTS}
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
            cands = []   # (key, flat index, pb, pnb, acoustic total, cb)
            for k, h in enumerate(cur):
                e = h.tokens[-1] if h.tokens else -1
                spb = dt(h.tot + row[0])
                spnb = dt(h.pnb + row[e]) if e >= 0 else ninf
                if fold_par[k] >= 0:
                    p = cur[fold_par[k]]
                    ep = p.tokens[-1] if p.tokens else -1
                    spnb = lae(spnb, dt((p.pb if e == ep else p.tot) + row[e]), dt)
                st = lae(spb, spnb, dt)
                cands.append((dt(st + h.ctx), k * V, spb, spnb, st, h.ctx))
                folded = {cur[j].tokens[-1] for j in range(n) if fold_par[j] == k}
                for v in range(1, V):
                    if v in folded:
                        continue
                    x = dt((h.pb if v == e else h.tot) + row[v])
                    cb = dt(h.ctx + dt(g_bonus[h.hs, v])) if graph is not None else h.ctx
                    cands.append((dt(x + (h.ctx if bonus_after_selection else cb)), k * V + v, ninf, x, x, cb))
            stay0 = cands[0]
            cands = [c for c in cands if c[4] > ninf]
            cands.sort(key=lambda c: (-c[0], c[1]))
            if not cands:
                cands = [stay0]
            sel = cands[:beam]
            cut_gaps.append(float(sel[-1][0] - cands[beam][0]) if len(cands) > beam else np.inf)
            picks.append([c[1] for c in sel])
            nxt = []
            for _, idx, pb, pnb, tot, cb in sel:
                k, v = divmod(idx, V)
                src = cur[k]
                h = _Hyp()
                h.tokens, h.timestamps, h.token_log_probs = list(src.tokens), list(src.timestamps), list(src.token_log_probs)
                h.pb, h.pnb, h.tot, h.node, h.parent_node = pb, pnb, tot, src.node, src.parent_node
                h.hs, h.ls, h.ctx = src.hs, src.ls, src.ctx
                if v:
                    h.tokens.append(v)
                    h.timestamps.append(t)
                    h.token_log_probs.append(row[v])
                    h.parent_node, h.node = src.node, next_node
                    next_node += 1
                    h.ctx = cb
                    if graph is not None:
                        b = g_bonus[src.hs, v]
                        events["bonus"] += int(b > 0)
                        events["broken"] += int(b < 0)
                        events["committed"] += int(g_end[(src.hs, v)])
                        h.hs = int(g_next[src.hs, v])
                    if lm is not None and v != UNK:
                        h.ls, term, ev = lm.step(src.ls, v)
                        h.ctx = dt(cb + dt(term))
                        if ev in events:
                            events[ev] += 1
                nxt.append(h)
            cur = nxt
        final = [dt(dt(h.tot + h.ctx) - dt(g_pending[h.hs] if graph is not None else 0)) for h in cur]
    order = sorted(range(len(cur)), key=lambda q: (-final[q], q))
    hyps = [dict(tokens=cur[q].tokens, timestamps=cur[q].timestamps, token_log_probs=np.array(cur[q].token_log_probs, dtype),
                 score=float(final[q]), tot=float(cur[q].tot), ctx=cur[q].ctx, hs=cur[q].hs, ls=cur[q].ls, slot=q) for q in order]
    final_gaps = [float(final[a] - final[b]) if final[b] > ninf else np.inf for a, b in zip(order, order[1:])]
    return dict(hyps=hyps, cut_gaps=cut_gaps, final_gaps=final_gaps, events=events, respelled_folds=int(respelled), picks=picks)


def min_gap(res):
    """the smallest reported gap of a run: every frame's cut gap on the keys and the consecutive gaps of final"""
    return min(list(res["cut_gaps"]) + list(res["final_gaps"]) + [np.inf])


def measured_e(lp, beam, graph=None, lm=None):
    """the worst difference between the float32 and the float64 twin's gaps while their selections agree; the float64 run; agreement"""
    a = biased_prefix_beam_search(lp, beam, graph, lm, np.float64)
    b = biased_prefix_beam_search(lp, beam, graph, lm, np.float32)
    e = 0.0
    for t, (pa, pb) in enumerate(zip(a["picks"], b["picks"])):
        if pa != pb:
            return e, a, False
        if np.isfinite(a["cut_gaps"][t]) and np.isfinite(b["cut_gaps"][t]):
            e = max(e, abs(a["cut_gaps"][t] - b["cut_gaps"][t]))
    if [h["slot"] for h in a["hyps"]] != [h["slot"] for h in b["hyps"]]:
        return e, a, False
    for ga, gb in zip(a["final_gaps"], b["final_gaps"]):
        if np.isfinite(ga) and np.isfinite(gb):
            e = max(e, abs(ga - gb))
    return e, a, True
