"""The carry of the streaming CTC prefix beam search restated in numpy (helper of test_ctc_prefix_stream.py /
test_ctc_prefix_stream_gpu.py).  It does not replace tests/ctc_prefix_twin.py, which stays the definition of the search over a whole row;
this one restates what crosses a chunk boundary, the way csrc/ctc_prefix_hist.h and the resumed kernel split it:

  * between chunks a stream is its live slots in rank order, each (tokens, timestamps, token log-probs, pb, pnb) -- the host's side;
  * a chunk sees of them only (pb, pnb, last token, length) and the relation tables rel[a][b] = |x| if seq(a) = seq(b) + x with
    0 < |x| <= Tc (relx[a][b] = x), else -1 -- built here from the carried tokens as CtcPrefixHistory.fill_in builds them from its tree;
  * inside the chunk a hypothesis is (carried origin, tokens appended in the chunk), and "slot j spells slot k + [e_j]" is decided as
    SEQUENCE identity through the tables (same_sequence below);
  * the chunk's result is per survivor (origin, appended tokens / chunk-relative frames / log-probs, pb, pnb): StreamTwin.chunk applies
    it to the carried slots, frames made absolute.

`carry` selects the rule, so that tests can show that the inputs tell a correct carry from a weaker one:
  "sequence"   the rule of the project;
  "in_chunk"   a fold relation is only seen inside the chunk: same carried origin and a non-empty suffix appended in this chunk;
  "node"       node identity: j folds into k only if j was made by extending k's own history node (a re-spelled prefix is missed)."""
import numpy as np


def _lae(a, b, dt):
    m, n = (a, b) if a > b else (b, a)
    if n == -np.inf:
        return dt(m)
    return dt(m + np.log1p(np.exp(dt(n - m))))


def relation_tables(seqs, Tc):
    """rel [n][n], relx {(a, b): x} of the carried token tuples, cap Tc (0 on the diagonal, as BeamHistory / CtcPrefixHistory)"""
    n = len(seqs)
    rel = -np.ones((n, n), np.int64)
    relx = {}
    for a in range(n):
        for b in range(n):
            d = len(seqs[a]) - len(seqs[b])
            if a == b:
                rel[a, b] = 0
            elif 0 < d <= Tc and seqs[a][: len(seqs[b])] == seqs[b]:
                rel[a, b] = d
                relx[a, b] = seqs[a][len(seqs[b]):]
    return rel, relx


def same_sequence(rel, relx, a, u, b, w):
    """seq(a) + u == seq(b) + w, the carried sequences known only through the tables"""
    if len(u) > len(w):
        return same_sequence(rel, relx, b, w, a, u)
    d = len(w) - len(u)
    if tuple(u) != tuple(w[d:]):
        return False
    if d == 0:
        return a == b
    return rel[a, b] == d and tuple(relx[a, b]) == tuple(w[:d])


class _H:
    __slots__ = ("org", "suf", "ts", "yp", "pb", "pnb", "tot", "last", "length", "node", "parent_node")


class StreamTwin:
    def __init__(self, beam, dtype=np.float64, carry="sequence"):
        self.beam, self.dt, self.carry = beam, np.dtype(dtype).type, carry
        self.frames = 0
        self.slots = [dict(tokens=(), timestamps=(), token_log_probs=(), pb=self.dt(0), pnb=self.dt(-np.inf))]
        self.cut_gaps, self.picks, self.rank_gaps = [], [], []
        self.boundary_folds = 0      # folds of the run decided through the tables (not inside one chunk's own suffixes)
        self._next_node = 0
        self._nodes = [(-1, -2)]     # carried (node, parent_node) per slot, for the "node" rule and the re-spelled count
        self.respelled_folds = 0

    def hyps(self):
        return [dict(tokens=list(s["tokens"]), timestamps=list(s["timestamps"]), token_log_probs=np.array(s["token_log_probs"], self.dt),
                     score=float(_lae(s["pb"], s["pnb"], self.dt)), pb=float(s["pb"]), pnb=float(s["pnb"])) for s in self.slots]

    def _spells(self, rel, relx, hj, hk):
        """does hj spell hk + [hj.last]?"""
        if hj.length != hk.length + 1:
            return False
        if self.carry == "node":
            return hj.parent_node == hk.node
        if self.carry == "in_chunk":
            return hj.org == hk.org and len(hj.suf) > 0 and tuple(hj.suf[:-1]) == tuple(hk.suf)
        if hj.suf:
            return same_sequence(rel, relx, hj.org, hj.suf[:-1], hk.org, hk.suf)
        w = tuple(hk.suf) + (hj.last,)     # a carried slot with nothing appended: seq(a) = seq(b) + s_k + [e_a]
        return len(w) <= self._Tc and same_sequence(rel, relx, hj.org, (), hk.org, w)

    def chunk(self, lp, Tc=None):
        """continue over the rows of lp [n][V] (a chunk of capacity Tc >= n: the cap of the relation tables)"""
        dt = self.dt
        lp = np.asarray(lp, dt)
        n_frames, V = lp.shape
        self._Tc = Tc = n_frames if Tc is None else Tc
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
            h.node, h.parent_node = self._nodes[a]
            cur.append(h)
        with np.errstate(invalid="ignore", over="ignore"):
            for t in range(n_frames):
                row = lp[t]
                n = len(cur)
                fold_par = [-1] * n
                for j in range(n):
                    for k in range(n):
                        if j != k and self._spells(rel, relx, cur[j], cur[k]):
                            fold_par[j] = k
                            self.respelled_folds += cur[j].parent_node != cur[k].node
                            self.boundary_folds += not (cur[j].org == cur[k].org and len(cur[j].suf) > 0)
                cands = []
                for k, h in enumerate(cur):
                    e = h.last
                    spb = dt(h.tot + row[0])
                    spnb = dt(h.pnb + row[e]) if e >= 0 else ninf
                    if fold_par[k] >= 0:
                        p = cur[fold_par[k]]
                        spnb = _lae(spnb, dt((p.pb if e == p.last else p.tot) + row[e]), dt)
                    cands.append((_lae(spb, spnb, dt), k * V, spb, spnb))
                    folded = {cur[j].last for j in range(n) if fold_par[j] == k}
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
                sel = cands[: self.beam]
                self.cut_gaps.append(float(sel[-1][0] - cands[self.beam][0]) if len(cands) > self.beam else np.inf)
                self.rank_gaps = [float(a[0] - b[0]) for a, b in zip(sel, sel[1:])]
                self.picks.append([c[1] for c in sel])
                nxt = []
                for tot, idx, pb, pnb in sel:
                    k, v = divmod(idx, V)
                    src = cur[k]
                    h = _H()
                    h.org, h.suf, h.ts, h.yp = src.org, list(src.suf), list(src.ts), list(src.yp)
                    h.pb, h.pnb, h.tot, h.last, h.length, h.node, h.parent_node = pb, pnb, tot, src.last, src.length, src.node, src.parent_node
                    if v:
                        h.suf.append(v)
                        h.ts.append(t)
                        h.yp.append(row[v])
                        h.last, h.length = v, src.length + 1
                        h.parent_node, h.node = src.node, self._next_node
                        self._next_node += 1
                    nxt.append(h)
                cur = nxt
        # the out block applied to the carried slots: (origin, appended, pb, pnb), frames made absolute
        new, nodes = [], []
        for h in cur:
            s = self.slots[h.org]
            new.append(dict(tokens=s["tokens"] + tuple(h.suf), timestamps=s["timestamps"] + tuple(self.frames + t for t in h.ts),
                            token_log_probs=s["token_log_probs"] + tuple(h.yp), pb=h.pb, pnb=h.pnb))
            nodes.append((h.node, h.parent_node))
        self.slots, self._nodes = new, nodes
        self.frames += n_frames
        return self


def chunked_search(lp, beam, chunks, dtype=np.float64, carry="sequence", Tc=None):
    """lp [T][V] through a StreamTwin in chunks of the given lengths (an int: uniform, the last one shorter) -> the twin"""
    lp = np.asarray(lp)
    T = lp.shape[0]
    if isinstance(chunks, int):
        chunks = [min(chunks, T - t) for t in range(0, T, chunks)]
    assert sum(chunks) == T
    tw = StreamTwin(beam, dtype, carry)
    t = 0
    for n in chunks:
        tw.chunk(lp[t: t + n], max(chunks) if Tc is None else Tc)
        t += n
    return tw


def same_hyps(a, b):
    """two hypothesis lists equal in everything, scores bit for bit (the dtype's own bits)"""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x["tokens"] != y["tokens"] or x["timestamps"] != y["timestamps"] or not np.array_equal(x["token_log_probs"], y["token_log_probs"]):
            return False
        for k in ("score", "pb", "pnb"):
            if not (x[k] == y[k]):
                return False
    return True


# ---- the device blocks, built the way the host class builds them ------------------------------------------------------------------------
HASH_SEED, HASH_MUL, M64 = 0x243F6A8885A308D3, 0x9E3779B97F4A7C15, (1 << 64) - 1


class Layout:
    """CtcPrefixResumeLayout{K, Tc} of csrc/ctc_prefix_layout.h (offsets in int32 words)"""

    def __init__(self, K, Tc):
        self.K, self.Tc = K, Tc
        self.in_ints = 1 + 8 * K + K * K + K * K * Tc
        self.in_pb, self.in_pnb, self.in_e, self.in_len, self.in_hash, self.in_phash = 1, 1 + K, 1 + 2 * K, 1 + 3 * K, 1 + 4 * K, 1 + 6 * K
        self.in_rel, self.in_relx = 1 + 8 * K, 1 + 8 * K + K * K
        self.out_ints = 1 + 9 * K + 3 * K * Tc
        self.out_org, self.out_napp, self.out_pb, self.out_pnb, self.out_hash, self.out_phash, self.out_tot = (
            1, 1 + K, 1 + 2 * K, 1 + 3 * K, 1 + 4 * K, 1 + 6 * K, 1 + 8 * K)
        self.out_ys, self.out_ts, self.out_yp = 1 + 9 * K, 1 + 9 * K + K * Tc, 1 + 9 * K + 2 * K * Tc


def _bits(x):
    return int(np.float32(x).view(np.int32))


def _i32(u):
    u &= 0xFFFFFFFF
    return u - (1 << 32) if u >= (1 << 31) else u


class HostCarry:
    """CtcPrefixHistory of csrc/ctc_prefix_hist.h in Python: the slots a stream carries between chunk calls of the resumed kernel, the in
    block it builds for the next chunk and the out block it applies (tests drive the debug op "ctc_prefix_resume" with it)"""

    def __init__(self, beam):
        self.beam, self.frames = beam, 0
        self.slots = [dict(tokens=(), timestamps=(), token_log_probs=(), pb=_bits(0.0), pnb=_bits(-np.inf), tot=_bits(0.0), hash=HASH_SEED, phash=0)]

    def fill_in(self, Tc):
        L, K = Layout(self.beam, Tc), self.beam
        blk = np.zeros(L.in_ints, np.int32)
        blk[0] = len(self.slots)
        blk[L.in_pb: L.in_pb + K] = blk[L.in_pnb: L.in_pnb + K] = _bits(-np.inf)
        blk[L.in_e: L.in_e + K] = -1
        rel, relx = relation_tables([s["tokens"] for s in self.slots], Tc)
        blk[L.in_rel: L.in_rel + K * K] = -1
        for k in range(K):
            blk[L.in_rel + k * K + k] = 0
        for k, s in enumerate(self.slots):
            blk[L.in_pb + k], blk[L.in_pnb + k] = s["pb"], s["pnb"]
            blk[L.in_e + k] = s["tokens"][-1] if s["tokens"] else -1
            blk[L.in_len + k] = len(s["tokens"])
            blk[L.in_hash + 2 * k], blk[L.in_hash + 2 * k + 1] = _i32(s["hash"]), _i32(s["hash"] >> 32)
            blk[L.in_phash + 2 * k], blk[L.in_phash + 2 * k + 1] = _i32(s["phash"]), _i32(s["phash"] >> 32)
            for j in range(len(self.slots)):
                if j != k:
                    blk[L.in_rel + k * K + j] = rel[k, j]
                    if rel[k, j] > 0:
                        o = L.in_relx + (k * K + j) * Tc
                        blk[o: o + rel[k, j]] = relx[k, j]
        return blk

    def apply_out(self, out, Tc, n_frames):
        L, K = Layout(self.beam, Tc), self.beam
        out = np.asarray(out, np.int32)
        n = int(out[0])
        assert 1 <= n <= K, n
        new = []
        for k in range(n):
            org, na = int(out[L.out_org + k]), int(out[L.out_napp + k])
            assert 0 <= org < len(self.slots) and 0 <= na <= n_frames, (k, org, na)
            s = self.slots[org]
            ys = tuple(int(v) for v in out[L.out_ys + k * Tc: L.out_ys + k * Tc + na])
            ts = tuple(int(v) for v in out[L.out_ts + k * Tc: L.out_ts + k * Tc + na])
            yp = tuple(int(v) for v in out[L.out_yp + k * Tc: L.out_yp + k * Tc + na])       # float32 bits
            assert all(v >= 1 for v in ys) and all(0 <= t < n_frames for t in ts), (k, ys, ts)
            h = lambda o: (int(out[o]) & 0xFFFFFFFF) | ((int(out[o + 1]) & 0xFFFFFFFF) << 32)
            new.append(dict(tokens=s["tokens"] + ys, timestamps=s["timestamps"] + tuple(self.frames + t for t in ts),
                            token_log_probs=s["token_log_probs"] + yp, pb=int(out[L.out_pb + k]), pnb=int(out[L.out_pnb + k]),
                            tot=int(out[L.out_tot + k]), hash=h(L.out_hash + 2 * k), phash=h(L.out_phash + 2 * k)))
            # the hashes are the kernel's rolling hashes of the sequence: opaque to the carry, but a cheap check of the block
            hh, ph = HASH_SEED, 0
            for v in new[-1]["tokens"]:
                ph, hh = hh, (hh * HASH_MUL + v + 1) & M64
            assert (hh, ph) == (new[-1]["hash"], new[-1]["phash"]), k
        self.slots = new
        self.frames += n_frames
