"""The carry of the BIASED streaming CTC prefix beam search restated in numpy (helper of test_ctc_prefix_stream_bias.py /
test_ctc_prefix_stream_bias_gpu.py).  ctc_prefix_bias_twin.biased_prefix_beam_search stays the definition of the search over a whole row and
ctc_prefix_stream_twin.StreamTwin that of the unbiased carry; this one restates what crosses a chunk boundary once a slot also has
(ctx, hs, ls):

  * between chunks a stream is its live slots in SELECTION-RANK order, each (tokens, timestamps, token log-probs, pb, pnb, ctx, hs, ls).
    ctx keeps the pending bonus of a match under way (it may complete in the next chunk); the tie rule "lower flat index" of the next
    frame depends on the slot order, so the slots are not carried in final order;
  * a chunk sees (pb, pnb, last token, length, ctx, hs, ls) and the relation tables of StreamTwin; the frame step is the biased one;
  * after a chunk final_q = (tot_q + ctx_q) - pending[hs_q] and the order (final desc, slot asc) are formed for REPORTING: entry 0 is the
    result, its score is final.

`carry` selects the rule, so that tests can show that the inputs tell the correct carry from weaker ones:
  "full"          the rule of the project;
  "reset_states"  hs / ls go back to the start state at a boundary (ctx is kept);
  "ctx_final"     ctx is carried with the pending bonus already subtracted;
  "final_order"   the slots are carried in final order."""
import numpy as np

from ctc_prefix_bias_twin import UNK, dense_graph
from ctc_prefix_stream_twin import HostCarry, _bits, _lae, relation_tables, same_sequence


class _H:
    __slots__ = ("org", "suf", "ts", "yp", "pb", "pnb", "tot", "last", "length", "hs", "ls", "ctx")


class BiasStreamTwin:
    def __init__(self, beam, graph=None, lm=None, dtype=np.float64, carry="full"):
        self.beam, self.dt, self.carry, self.graph, self.lm = beam, np.dtype(dtype).type, carry, graph, lm
        dt = self.dt
        if graph is not None:
            self.g_next, self.g_bonus, self.g_pending = dense_graph(graph)
        self.frames = 0
        self.slots = [dict(tokens=(), timestamps=(), token_log_probs=(), pb=dt(0), pnb=dt(-np.inf), tot=dt(0), ctx=dt(0), hs=0,
                           ls=(lm.start if lm is not None else 0))]
        self.fin, self.ord = [dt(0)], [0]
        self.picks, self.cut_gaps = [], []

    def _spells(self, rel, relx, hj, hk, Tc):
        if hj.length != hk.length + 1:
            return False
        if hj.suf:
            return same_sequence(rel, relx, hj.org, hj.suf[:-1], hk.org, hk.suf)
        w = tuple(hk.suf) + (hj.last,)
        return len(w) <= Tc and same_sequence(rel, relx, hj.org, (), hk.org, w)

    def chunk(self, lp, Tc=None):
        dt, graph, lm = self.dt, self.graph, self.lm
        lp = np.asarray(lp, dt)
        n_frames, V = lp.shape
        Tc = n_frames if Tc is None else Tc
        assert 1 <= n_frames <= Tc
        ninf = dt(-np.inf)
        rel, relx = relation_tables([s["tokens"] for s in self.slots], Tc)
        cur = []
        for a, s in enumerate(self.slots):
            h = _H()
            h.org, h.suf, h.ts, h.yp = a, [], [], []
            h.pb, h.pnb = s["pb"], s["pnb"]
            h.tot = _lae(h.pb, h.pnb, dt)
            h.last = s["tokens"][-1] if s["tokens"] else -1
            h.length = len(s["tokens"])
            h.hs, h.ls, h.ctx = s["hs"], s["ls"], s["ctx"]
            if self.carry == "reset_states":
                h.hs, h.ls = 0, (lm.start if lm is not None else 0)
            cur.append(h)
        with np.errstate(invalid="ignore", over="ignore"):
            for t in range(n_frames):
                row = lp[t]
                n = len(cur)
                fold_par = [-1] * n
                for j in range(n):
                    for k in range(n):
                        if j != k and self._spells(rel, relx, cur[j], cur[k], Tc):
                            fold_par[j] = k
                cands = []   # (key, flat index, pb, pnb, acoustic total, cb)
                for k, h in enumerate(cur):
                    e = h.last
                    spb = dt(h.tot + row[0])
                    spnb = dt(h.pnb + row[e]) if e >= 0 else ninf
                    if fold_par[k] >= 0:
                        p = cur[fold_par[k]]
                        spnb = _lae(spnb, dt((p.pb if e == p.last else p.tot) + row[e]), dt)
                    st = _lae(spb, spnb, dt)
                    cands.append((dt(st + h.ctx), k * V, spb, spnb, st, h.ctx))
                    folded = {cur[j].last for j in range(n) if fold_par[j] == k}
                    for v in range(1, V):
                        if v in folded:
                            continue
                        x = dt((h.pb if v == e else h.tot) + row[v])
                        cb = dt(h.ctx + dt(self.g_bonus[h.hs, v])) if graph is not None else h.ctx
                        cands.append((dt(x + cb), k * V + v, ninf, x, x, cb))
                stay0 = cands[0]
                cands = [c for c in cands if c[4] > ninf]
                cands.sort(key=lambda c: (-c[0], c[1]))
                if not cands:
                    cands = [stay0]
                sel = cands[: self.beam]
                self.cut_gaps.append(float(sel[-1][0] - cands[self.beam][0]) if len(cands) > self.beam else np.inf)
                self.picks.append([c[1] for c in sel])
                nxt = []
                for _, idx, pb, pnb, tot, cb in sel:
                    k, v = divmod(idx, V)
                    src = cur[k]
                    h = _H()
                    h.org, h.suf, h.ts, h.yp = src.org, list(src.suf), list(src.ts), list(src.yp)
                    h.pb, h.pnb, h.tot, h.last, h.length = pb, pnb, tot, src.last, src.length
                    h.hs, h.ls, h.ctx = src.hs, src.ls, src.ctx
                    if v:
                        h.suf.append(v)
                        h.ts.append(t)
                        h.yp.append(row[v])
                        h.last, h.length = v, src.length + 1
                        h.ctx = cb
                        if graph is not None:
                            h.hs = int(self.g_next[src.hs, v])
                        if lm is not None and v != UNK:
                            h.ls, term, _ = lm.step(src.ls, v)
                            h.ctx = dt(cb + dt(term))
                    nxt.append(h)
                cur = nxt
            fin = [dt(dt(h.tot + h.ctx) - dt(self.g_pending[h.hs] if graph is not None else 0)) for h in cur]
        order = sorted(range(len(cur)), key=lambda q: (-fin[q], q))
        new = []
        for h in cur:
            s = self.slots[h.org]
            new.append(dict(tokens=s["tokens"] + tuple(h.suf), timestamps=s["timestamps"] + tuple(self.frames + t for t in h.ts),
                            token_log_probs=s["token_log_probs"] + tuple(h.yp), pb=h.pb, pnb=h.pnb, tot=h.tot, ctx=h.ctx, hs=h.hs, ls=h.ls))
        if self.carry == "ctx_final" and graph is not None:
            for s in new:
                s["ctx"] = dt(s["ctx"] - dt(self.g_pending[s["hs"]]))
        if self.carry == "final_order":
            new, fin, order = [new[q] for q in order], [fin[q] for q in order], list(range(len(order)))
        self.slots, self.fin, self.ord = new, fin, order
        self.frames += n_frames
        return self

    def entries(self):
        """what the stream reports: the live prefixes in (final desc, slot asc) order, as biased_prefix_beam_search returns its hyps"""
        return [dict(tokens=list(self.slots[q]["tokens"]), timestamps=list(self.slots[q]["timestamps"]),
                     token_log_probs=np.array(self.slots[q]["token_log_probs"], self.dt), score=float(self.fin[q]), tot=float(self.slots[q]["tot"]),
                     ctx=self.slots[q]["ctx"], hs=self.slots[q]["hs"], ls=self.slots[q]["ls"], slot=q) for q in self.ord]

    def result(self):
        """(tokens, score) of entry 0"""
        e = self.entries()[0]
        return e["tokens"], e["score"]

    def pending_slots(self):
        """live slots whose match is under way (pending bonus not zero)"""
        return 0 if self.graph is None else sum(float(self.g_pending[s["hs"]]) != 0.0 for s in self.slots)

    def reordered(self):
        return self.ord != list(range(len(self.ord)))

    def final_gaps(self):
        f = [self.fin[q] for q in self.ord]
        return [float(a - b) if b > -np.inf else np.inf for a, b in zip(f, f[1:])]


def chunked_biased_search(lp, beam, chunks, graph=None, lm=None, dtype=np.float64, carry="full", after=None):
    """lp [T][V] through a BiasStreamTwin in chunks of the given lengths (an int: uniform, the last one shorter); after(twin) runs behind
    every chunk"""
    lp = np.asarray(lp)
    T = lp.shape[0]
    if isinstance(chunks, int):
        chunks = [min(chunks, T - t) for t in range(0, T, chunks)]
    assert sum(chunks) == T
    tw = BiasStreamTwin(beam, graph, lm, dtype, carry)
    t = 0
    for n in chunks:
        tw.chunk(lp[t: t + n], max(chunks))
        t += n
        if after:
            after(tw)
    return tw


def same_entries(got, want):
    """two entry lists equal in everything: lists, order, slot, hs, ls, and (final, tot, ctx) in the dtype's own bits"""
    if len(got) != len(want):
        return False
    for x, y in zip(got, want):
        if list(x["tokens"]) != list(y["tokens"]) or list(x["timestamps"]) != list(y["timestamps"]):
            return False
        if not np.array_equal(x["token_log_probs"], y["token_log_probs"]):
            return False
        if (x["slot"], x["hs"], x["ls"]) != (y["slot"], y["hs"], y["ls"]):
            return False
        if not (x["score"] == y["score"] and x["tot"] == y["tot"] and x["ctx"] == y["ctx"]):
            return False
    return True


# ---- the device blocks, built the way the host class builds them ------------------------------------------------------------------------
class SideLayout:
    """CtcPrefixResumeBiasLayout{K} of csrc/ctc_prefix_layout.h (offsets in int32 words)"""

    def __init__(self, K):
        self.K = K
        self.in_ints, self.in_ctx, self.in_hs, self.in_ls = 1 + 3 * K, 1, 1 + K, 1 + 2 * K
        self.out_ints, self.out_ctx, self.out_hs, self.out_ls, self.out_fin, self.out_ord = 5 * K, 0, K, 2 * K, 3 * K, 4 * K


class BiasHostCarry(HostCarry):
    """CtcPrefixHistory with its side blocks in Python: HostCarry's slots plus (ctx bits, hs, ls) per slot and the last step's fin / ord.
    S / S_lm: the sizes of the stream's graph and of the LM (0: none); lm_on: the row runs the LM (flag bit 0)."""

    def __init__(self, beam, S=0, S_lm=0, start=0, lm_on=False):
        super().__init__(beam)
        self.S, self.S_lm, self.lm_on = S, S_lm, bool(lm_on)
        self.slots[0].update(ctx=_bits(0.0), hs=0, ls=start if lm_on else 0)
        self.fin, self.ord = [_bits(0.0)], [0]

    def fill_side_in(self):
        L, K = SideLayout(self.beam), self.beam
        blk = np.zeros(L.in_ints, np.int32)
        blk[0] = int(self.lm_on)
        for k, s in enumerate(self.slots):
            assert 0 <= s["hs"] < max(self.S, 1) and (not self.lm_on or 0 <= s["ls"] < self.S_lm), (k, s["hs"], s["ls"])
            blk[L.in_ctx + k], blk[L.in_hs + k], blk[L.in_ls + k] = s["ctx"], s["hs"], s["ls"]
        return blk

    def apply(self, out, side_out, Tc, n_frames):
        L = SideLayout(self.beam)
        side_out = np.asarray(side_out, np.int32)
        n = int(out[0])
        assert 1 <= n <= self.beam, n
        hs, ls = side_out[L.out_hs: L.out_hs + n], side_out[L.out_ls: L.out_ls + n]
        assert sorted(int(q) for q in side_out[L.out_ord: L.out_ord + n]) == list(range(n)), side_out[L.out_ord: L.out_ord + n]
        assert all(0 <= int(h) < max(self.S, 1) for h in hs) and (not self.lm_on or all(0 <= int(x) < self.S_lm for x in ls)), (hs, ls)
        self.apply_out(out, Tc, n_frames)
        for k, s in enumerate(self.slots):
            s.update(ctx=int(side_out[L.out_ctx + k]), hs=int(hs[k]), ls=int(ls[k]))
        self.fin = [int(v) for v in side_out[L.out_fin: L.out_fin + n]]
        self.ord = [int(q) for q in side_out[L.out_ord: L.out_ord + n]]

    def entries(self):
        """the slots in final order, each with its final score (float32 bits)"""
        return [dict(self.slots[q], final=self.fin[q], slot=q) for q in self.ord]
