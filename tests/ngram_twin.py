"""N-gram LM shallow fusion of the modified beam search restated in Python (helper of test_ngram.py / test_ngram_gpu.py).

The definition is the text in include/k2hip.h ("n-gram LM shallow fusion") and DESIGN.md; this file says it again with dicts of
tuples and numpy float32: `TwinLm` is the back-off automaton written from that definition (histories are tuples, nothing is
precomputed per arc), `twin_beam_search` is hotword_twin.twin_beam_search extended by copy -- the same oracle decoder / joiner
operators, the term of a selected candidate added AFTER the frame's top-k and after the hotword bonus, BEFORE HypothesisList.add,
nothing taken back for the LM at the end.  It returns the margins and a per-frame trace in the oracle's tap format, and counts the
LM events that occurred."""
import numpy as np
import torch

from hotword_twin import TwinGraph  # noqa: F401  (the hotword graph the search can carry beside the LM)

BLANK, UNK = 0, 2
BOS, EOS, LM_UNK = -1, -2, -3
f32 = np.float32


class TwinLm:
    """entries: [(ids, log_prob, backoff)], natural log; ids may hold BOS / EOS / LM_UNK."""

    def __init__(self, entries, vocab_size):
        self.V = vocab_size
        self.N = max([len(e[0]) for e in entries] + [1])
        self.lp, self.bo, self.unk = {}, {}, None
        for ids, lp, bo in entries:
            ids = tuple(int(x) for x in ids)
            if LM_UNK in ids:
                if len(ids) == 1:
                    self.unk = f32(lp)
                continue
            self.bo[ids] = f32(bo)                       # the back-off weight of the history `ids`, should it be a state
            if ids[-1] in (BOS, EOS):
                continue                                 # ignored as predicted words
            self.lp[ids] = f32(lp)
        hist = {k[:-1] for k in self.lp if len(k) >= 2}
        self.hist = [()] + sorted(hist, key=lambda h: (len(h), h))
        self.state_of = {h: i for i, h in enumerate(self.hist)}
        self.start = self.state_of.get((BOS,), 0)

    @property
    def num_states(self):
        return len(self.hist)

    @property
    def num_arcs(self):
        return len(self.lp)

    def scaled(self, scale):
        """the tables multiplied by scale once, entry by entry in float32 (what the model uploads)"""
        t = TwinLm.__new__(TwinLm)
        t.__dict__.update(self.__dict__)
        s = f32(scale)
        t.lp = {k: f32(v * s) for k, v in self.lp.items()}
        t.bo = {k: f32(v * s) for k, v in self.bo.items()}
        t.unk = None if self.unk is None else f32(self.unk * s)
        return t

    def _longest_state(self, seq, max_len):
        for n in range(min(len(seq), max_len), 0, -1):
            if seq[len(seq) - n:] in self.state_of:
                return seq[len(seq) - n:]
        return ()

    def step(self, s, w):
        """(next state, log-prob, event) for a hypothesis in state s that appends token w; event: 'full' (a hit at order N), 'hit'
        (a direct hit below it), 'back1' (after one back-off, above the unigrams), 'uni' (backed off to a unigram), 'unk'"""
        if w in (BLANK, UNK):
            return s, f32(0), None
        h = self.hist[s]
        g, acc, nback = h, f32(0), 0
        while g + (w,) not in self.lp and g != ():
            acc = f32(acc + self.bo[g])
            g = self._longest_state(g, len(g) - 1)
            nback += 1
        if g + (w,) not in self.lp:
            return 0, f32(acc + self.unk), "unk"
        nxt = self.state_of[self._longest_state(h + (w,), self.N - 1)]
        ev = ("full" if len(g) == self.N - 1 else "hit") if nback == 0 else "uni" if g == () else "back1" if nback == 1 else "back"
        return nxt, f32(acc + self.lp[g + (w,)]), ev


EVENTS = ("full", "back1", "uni", "unk")


def twin_beam_search(oracle, enc_out, beam=4, lm=None, scale=0.0, graph=None):
    """One stream, enc_out [T', J].  lm: a TwinLm (scaled here), graph: a hotword TwinGraph.  Returns dict(ys, ts, lp (log-prob of
    the pick, LM terms included), margins [T'+1], idx / val [T', 2 beam], n [T'], events)."""
    cs = oracle.context_size
    lms = lm.scaled(scale) if lm is not None else None
    ys0 = [BLANK] * cs
    B = {tuple(ys0): dict(ys=ys0, log_prob=torch.zeros(1, dtype=torch.float32), timestamp=[], state=0, lst=lms.start if lms else 0)}
    T = enc_out.shape[0]
    idx = np.full((T, 2 * beam), -1, np.int32)
    val = np.full((T, 2 * beam), -np.inf, np.float32)
    nsurv = np.zeros(T, np.int32)
    margins = np.full(T + 1, np.inf, np.float32)
    events = {k: 0 for k in EVENTS}
    for t in range(T):
        A = list(B.values())
        B = {}
        ys_log_probs = torch.cat([h["log_prob"].reshape(1, 1) for h in A])
        decoder_out = oracle.decoder(np.array([h["ys"][-cs:] for h in A], np.int64))
        logits = torch.from_numpy(oracle.joiner(np.repeat(enc_out[t: t + 1], len(A), 0), decoder_out))
        log_probs = logits.log_softmax(dim=-1)
        log_probs.add_(ys_log_probs)
        V = log_probs.size(-1)
        log_probs = log_probs.reshape(-1)
        # the 2 * beam best in (score desc, flat index asc) order.  (A full sort, not torch.topk: of a block of exactly tied scores that
        # reaches past the 2 * beam-th place topk returns whichever members it likes, not the lowest flat indexes.)
        ti = torch.from_numpy(np.lexsort((np.arange(log_probs.numel()), -log_probs.numpy()))[: 2 * beam].copy())
        tv = log_probs[ti]
        idx[t, : len(ti)] = ti.numpy()
        val[t, : len(ti)] = tv.numpy()
        want = min(beam, log_probs.numel())
        if len(ti) > want:
            margins[t] = tv[want - 1] - tv[want]
        for k in range(want):
            hyp = A[int(ti[k]) // V]
            tok = int(ti[k]) % V
            new_ys, new_ts, state, lst = hyp["ys"][:], hyp["timestamp"][:], hyp["state"], hyp["lst"]
            new_log_prob = tv[k].reshape(1)
            if tok not in (BLANK, UNK):
                new_ys.append(tok)
                new_ts.append(t)
                if graph is not None:
                    state, bonus, _ = graph.step(state, tok)
                    new_log_prob = new_log_prob + torch.tensor([bonus], dtype=torch.float32)
                if lms is not None:
                    lst, term, ev = lms.step(lst, tok)
                    new_log_prob = new_log_prob + torch.tensor([term], dtype=torch.float32)
                    if ev in events:
                        events[ev] += 1
            key = tuple(new_ys)
            if key in B:
                B[key]["log_prob"] = torch.logaddexp(B[key]["log_prob"], new_log_prob)
            else:
                B[key] = dict(ys=new_ys, log_prob=new_log_prob, timestamp=new_ts, state=state, lst=lst)
        nsurv[t] = len(B)
    final = []
    for h in B.values():
        lp = h["log_prob"]
        if graph is not None:
            lp = lp - torch.tensor([graph.pending(h["state"])], dtype=torch.float32)
        final.append((h, lp))
    norm = [float(lp / len(h["ys"])) for h, lp in final]
    best = int(np.argmax(norm))   # (first maximum)
    if len(norm) > 1:
        margins[T] = norm[best] - max(x for i, x in enumerate(norm) if i != best)
    h, lp = final[best]
    return dict(ys=h["ys"][cs:], ts=h["timestamp"], lp=float(lp), margins=margins, idx=idx, val=val, n=nsurv, events=events)


def twin_batch(oracle, enc, beam, lm=None, scale=0.0, graph=None):
    """every stream of enc [B, T', J]: (results [(tokens, timestamps)], scores [B], margins [B, T'+1], trace dict, events)"""
    runs = [twin_beam_search(oracle, enc[b], beam, lm, scale, graph) for b in range(enc.shape[0])]
    trace = dict(idx=np.stack([r["idx"] for r in runs]), val=np.stack([r["val"] for r in runs]), n=np.stack([r["n"] for r in runs]), beam=beam)
    events = {k: int(sum(r["events"][k] for r in runs)) for k in EVENTS}
    return ([(r["ys"], r["ts"]) for r in runs], np.array([r["lp"] for r in runs], np.float32), np.stack([r["margins"] for r in runs]), trace,
            events)


def draw_lm(results, vocab_size, rng, order=3, n_cut=40, n_random=40, n_no_unigram=3):
    """A seeded LM: n-grams cut from the token sequences an unbiased run emitted (so high-order hits occur) with high
    probabilities, random ones besides, unigrams for every real token except a few EMITTED ones (so the <unk> fallback occurs), the
    <s> and <unk> unigrams.  Every history has its own entry.  Returns [(ids, log_prob, backoff)] with float32 values."""
    real = [v for v in range(vocab_size) if v not in (BLANK, UNK)]
    emitted = sorted({int(t) for toks, _ in results for t in toks})
    holes = set(int(x) for x in rng.choice(emitted, size=min(n_no_unigram, max(len(emitted) // 4, 1)), replace=False)) if emitted else set()
    ent = {}

    def put(ids, lo, hi):
        if ids not in ent:
            ent[ids] = (f32(rng.uniform(lo, hi)), f32(rng.uniform(-1.0, -0.05)))

    put((BOS,), -99.0, -99.0)
    ent[(LM_UNK,)] = (f32(-7.5), f32(0))
    for v in real:
        if v not in holes:
            put((v,), -6.0, -3.0)

    def put_chain(seq):
        if any(x in holes or x in (BLANK, UNK) for x in seq):
            return
        for n in range(2, len(seq) + 1):
            put(tuple(seq[:n]), -1.5, -0.1)

    seqs = [[BOS] + [int(t) for t in toks] for toks, _ in results if len(toks) >= 2]
    for _ in range(n_cut if order >= 2 else 0):
        if not seqs:
            break
        s = seqs[rng.integers(len(seqs))]
        n = int(rng.integers(2, order + 1))
        o = int(rng.integers(0, max(len(s) - n, 0) + 1))
        put_chain(s[o: o + n])
    for _ in range(n_random if order >= 2 else 0):
        put_chain([int(x) for x in rng.choice(real, size=int(rng.integers(2, order + 1)))])
    out = []
    for ids, (lp, bo) in sorted(ent.items(), key=lambda kv: (len(kv[0]), kv[0])):
        out.append((ids, lp, bo if len(ids) < order else f32(0)))
    return out


def arpa_text(entries, symbols):
    """the entries as a text ARPA file over `symbols` (token strings by id); natural log -> log10 with 9 digits"""
    name = {BOS: "<s>", EOS: "</s>", LM_UNK: "<unk>"}
    N = max(len(e[0]) for e in entries)
    by = [[e for e in entries if len(e[0]) == n] for n in range(1, N + 1)]
    out = ["\\data\\"] + [f"ngram {n + 1}={len(b)}" for n, b in enumerate(by)] + [""]
    for n, b in enumerate(by):
        out.append(f"\\{n + 1}-grams:")
        for ids, lp, bo in b:
            words = " ".join(name.get(i) or symbols[i] for i in ids)
            out.append(f"{float(lp) / np.log(10.0):.9g}\t{words}" + (f"\t{float(bo) / np.log(10.0):.9g}" if n + 1 < N else ""))
        out.append("")
    return "\n".join(out + ["\\end\\", ""])


# ---- the cases test_ngram_gpu.py runs the engine on, and test_ngram.py checks the twin on without a GPU ---------------------------
SCALE = 0.5
TINY_BEAMS = (2, 4, 8)      # the tiny model over the `utts` fixture's encoder output
TINY_LM_SEED = {2: 109, 4: 1, 8: 9}      # per beam (test_ngram.py checks the conditions these seeds were picked for)
WIDE_VOCAB, WIDE_SEED, WIDE_B, WIDE_T, WIDE_J = 400, 11, 8, 40, 64     # kat_model.write_wide_model + a seeded random encoder output
WIDE_BEAMS = (4, 8)
WIDE_LM_SEED = {4: 1, 8: 5}


def wide_enc():
    return np.random.default_rng(WIDE_SEED).standard_normal((WIDE_B, WIDE_T, WIDE_J)).astype(np.float32)


def tiny_lm(unbiased, vocab_size, beam=4):
    return draw_lm(unbiased, vocab_size, np.random.default_rng(TINY_LM_SEED[beam]))


def wide_lm(unbiased, beam=4):
    return draw_lm(unbiased, WIDE_VOCAB, np.random.default_rng(WIDE_LM_SEED[beam]), n_cut=80, n_random=200, n_no_unigram=6)


# ---- the KAT-model flip case (tests/kat_model.py: logits = tanh(enc + dec), only token 3's logit depends on the context) ----------
# The frames of hotword_twin.KAT_FLIP: t0 offers 5 (1.0) against a slightly better 6 (1.1), t1 offers 7 (3.0), t2 blank (3.0); beam 2.
# LM: unigrams of 1, 3, 4, 5, 6, 7 at u = -4 each, the bigram (5, 7) at b = -1 with bow(5) = -0.5; scale 0.5, so the scaled terms
# are u' = -2, b' = -0.5 (exact in float32).
#   t0, ctx [0, 0]: p(6) = 0.338, p(5) = 0.325 -> the selection is {6, 5} (unbiased sums); both earn u'.  [5] is a state, [6] is not.
#   t1: both carry the same u', so the selection is the unbiased one: {[6]+7 = 0.173, [5]+7 = 0.166} (anything else <= 0.024).
#       [6, 7] earns the unigram u' = -2 (state 0), [5, 7] the bigram b' = -0.5: [5, 7] is now ahead by e^1.5 x 0.166 / 0.173 = 4.3.
#   t2: both take blank: [5, 7]+other = 0.166 x 4.48 x 0.070 = 0.052 (in [6, 7]'s units) < [6, 7]+blank = 0.173 x 0.511 = 0.088.
#   Final pick, both of length 2 + 2: without the LM [6, 7] (0.338 > 0.325), with it [5, 7].  No two candidates spell the same
#   sequence on the way, so the score is the plain sum along the path:
#   score = log p(5 | t0, ctx [0, 0]) + log p(7 | t1, ctx [0, 5]) + log p(0 | t2, ctx [5, 7]) + u' + b'
KAT_LM_FLIP = dict(rows=[{5: 1.0, 6: 1.1}, {7: 3.0}, {0: 3.0}], beam=2, scale=0.5, plain=([6, 7], [0, 1]), fused=([5, 7], [0, 1]),
                   entries=[((v,), -4.0, -0.5 if v == 5 else 0.0) for v in (1, 3, 4, 5, 6, 7)] + [((5, 7), -1.0, 0.0)])


def kat_lm_flip_score():
    """the hand value above, in float64 from the closed form of the KAT model"""
    def logp(row, tok, boost):
        x = np.full(8, -3.0)
        for k, v in row.items():
            x[k] = v
        x[3] += boost
        z = np.tanh(x)
        return z[tok] - np.log(np.exp(z).sum())
    r = KAT_LM_FLIP["rows"]
    return logp(r[0], 5, 0.1 * (0.5 + 0.5)) + logp(r[1], 7, 0.1 * (0.5 + 5)) + logp(r[2], 0, 0.1 * (5 + 7)) + (-2.0) + (-0.5)
