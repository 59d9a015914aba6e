"""The hotword-biased modified beam search restated in Python (helper of test_hotwords.py / test_hotwords_gpu.py).

The definition is the text in include/k2hip.h ("hotword biasing") and DESIGN.md; this file says it again with dicts and torch ops:
`TwinGraph` is the trie with Aho-Corasick failure links (step / pending), `twin_beam_search` is `icefall_modified_beam_search` of
tests/test_oracle_beam.py extended by it -- the same oracle decoder / joiner operators, torch log_softmax / topk / logaddexp, the
bonus of a selected candidate added AFTER the frame's top-k and BEFORE HypothesisList.add, pending bonuses taken back before the final
length-normalised pick.  It also returns the margins and a per-frame trace in the oracle's tap format (idx, val, n, beam), so that
parity.assert_beam_match / localise_beam work on it, and counts the bonus events that occurred."""
import numpy as np
import torch

from test_oracle_beam import icefall_modified_beam_search  # noqa: F401  (the search this one extends; compared in test_hotwords.py)

BLANK, UNK = 0, 2


class TwinGraph:
    def __init__(self, phrases, c, vocab_size):
        self.c, self.V = np.float32(c), vocab_size
        self.goto, self.depth, self.end, self.fail = [{}], [0], [False], [0]
        for p in phrases:
            s = 0
            for v in p:
                if v not in self.goto[s]:
                    self.goto[s][v] = len(self.goto)
                    self.goto.append({})
                    self.depth.append(self.depth[s] + 1)
                    self.end.append(False)
                    self.fail.append(0)
                s = self.goto[s][v]
            self.end[s] = True
        queue = list(self.goto[0].values())
        while queue:
            s = queue.pop(0)
            for v, n in self.goto[s].items():
                f = self.fail[s]
                while f and v not in self.goto[f]:
                    f = self.fail[f]
                self.fail[n] = self.goto[f].get(v, 0)
                queue.append(n)

    @property
    def num_states(self):
        return len(self.goto)

    def pending(self, s):
        return np.float32(self.c * np.float32(self.depth[s]))

    def delta(self, s, v):
        while s and v not in self.goto[s]:
            s = self.fail[s]
        return self.goto[s].get(v, 0)

    def step(self, s, v):
        """(next state, bonus, committed) for a hypothesis in state s that appends token v"""
        if v in (BLANK, UNK):
            return s, np.float32(0), False
        n = self.delta(s, v)
        bonus = np.float32(self.pending(n) - self.pending(s))
        return (0 if self.end[n] else n), bonus, self.end[n]


def twin_beam_search(oracle, enc_out, beam=4, graph=None):
    """One stream, enc_out [T', J].  Returns dict(ys, ts, lp (finalized log-prob of the pick), margins [T'+1], idx / val [T', 2 beam],
    n [T'], events = counts of 'bonus' (a selected candidate earned > 0), 'broken' (< 0: a partial match broke), 'committed')."""
    cs = oracle.context_size
    ys0 = [BLANK] * cs
    B = {tuple(ys0): dict(ys=ys0, log_prob=torch.zeros(1, dtype=torch.float32), timestamp=[], state=0)}
    T = enc_out.shape[0]
    idx = np.full((T, 2 * beam), -1, np.int32)
    val = np.full((T, 2 * beam), -np.inf, np.float32)
    nsurv = np.zeros(T, np.int32)
    margins = np.full(T + 1, np.inf, np.float32)
    events = dict(bonus=0, broken=0, committed=0)
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
            new_ys, new_ts, state = hyp["ys"][:], hyp["timestamp"][:], hyp["state"]
            new_log_prob = tv[k].reshape(1)
            if tok not in (BLANK, UNK):
                new_ys.append(tok)
                new_ts.append(t)
                if graph is not None:
                    state, bonus, committed = graph.step(state, tok)
                    new_log_prob = new_log_prob + torch.tensor([bonus], dtype=torch.float32)
                    events["bonus"] += bonus > 0
                    events["broken"] += bonus < 0
                    events["committed"] += bool(committed)
            key = tuple(new_ys)
            if key in B:
                B[key]["log_prob"] = torch.logaddexp(B[key]["log_prob"], new_log_prob)
            else:
                B[key] = dict(ys=new_ys, log_prob=new_log_prob, timestamp=new_ts, state=state)
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


def twin_batch(oracle, enc, beam, graph=None):
    """every stream of enc [B, T', J]: (results [(tokens, timestamps)], scores [B], margins [B, T'+1], trace dict, events)"""
    runs = [twin_beam_search(oracle, enc[b], beam, graph) for b in range(enc.shape[0])]
    trace = dict(idx=np.stack([r["idx"] for r in runs]), val=np.stack([r["val"] for r in runs]), n=np.stack([r["n"] for r in runs]), beam=beam)
    events = {k: int(sum(r["events"][k] for r in runs)) for k in ("bonus", "broken", "committed")}
    return ([(r["ys"], r["ts"]) for r in runs], np.array([r["lp"] for r in runs], np.float32), np.stack([r["margins"] for r in runs]), trace,
            events)


def draw_phrases(results, n_phrases, rng, min_len=2, max_len=3):
    """Phrases cut from the token sequences an unbiased run emitted (so matches really occur), made a legal phrase set: no
    blank / unk, no duplicates, no phrase a proper prefix of another."""
    seqs = [t for t, _ in results if len(t) >= min_len]
    out = []
    for _ in range(2000 * n_phrases):
        if len(out) >= n_phrases or not seqs:
            break
        s = seqs[rng.integers(len(seqs))]
        L = int(rng.integers(min_len, min(max_len, len(s)) + 1))
        o = int(rng.integers(0, len(s) - L + 1))
        p = [int(x) for x in s[o: o + L]]
        if BLANK in p or UNK in p:
            continue
        if any(p[: len(q)] == q or q[: len(p)] == p for q in out):
            continue
        out.append(p)
    return out


# ---- the cases test_hotwords_gpu.py runs the engine on, and test_hotwords.py checks the twin on without a GPU ---------------------
# (committed seeds: for every one of them the twin with c = 0 and with an empty list equals the CPU oracle exactly)
SCORE = 1.5                 # exactly representable, as are its small multiples
TINY_BEAMS = (2, 4, 8)      # the tiny model over the `utts` fixture's encoder output
TINY_PHRASES, TINY_PHRASE_SEED = 6, 7
WIDE_VOCAB, WIDE_SEED, WIDE_B, WIDE_T, WIDE_J = 400, 11, 8, 40, 64     # kat_model.write_wide_model + a seeded random encoder output
WIDE_BEAMS = (4, 8)
WIDE_PHRASES = 12


def wide_enc():
    return np.random.default_rng(WIDE_SEED).standard_normal((WIDE_B, WIDE_T, WIDE_J)).astype(np.float32)


def tiny_phrases(unbiased):
    return draw_phrases(unbiased, TINY_PHRASES, np.random.default_rng(TINY_PHRASE_SEED))


def wide_phrases(unbiased):
    return draw_phrases(unbiased, WIDE_PHRASES, np.random.default_rng(WIDE_SEED))


# ---- the KAT-model flip case (tests/kat_model.py: logits = tanh(enc + dec), only token 3's logit depends on the context) ----------
# Frames: t0 offers 5 (1.0) against a slightly better 6 (1.1), t1 offers 7 (3.0), t2 blank (3.0); beam 2; phrase [5, 7], c = 1.5.
# Every other pre-tanh input is -3 (token 3: -3 + boost, boost = 0.1 (e_prev + e_cur) with e_blank = 0.5, e_v = v).
#   t0, ctx [0, 0] (boost 0.1): p(6) = 0.338, p(5) = 0.325, the others 0.056 each -> the selection is {6, 5} (unbiased scores);
#       [5] enters the graph: +1.5.
#   t1: unbiased  [6]+7 = 0.338 x 0.511 = 0.173, [5]+7 = 0.166, anything else <= 0.338 x 0.070 -> {[6, 7], [5, 7]}
#       biased    [5] carries e^1.5: [5]+7 = 0.744 (equivalent probability), [6]+7 = 0.173, [5]+other = 0.102 -> {[5, 7], [6, 7]};
#       [5, 7] ends the phrase: +1.5 more, committed, state = root.
#   t2: both hypotheses take blank (x 0.511; [5, 7]+other = 0.744 x 0.070 = 0.052 < [6, 7]+blank = 0.088).
#   Final pick, both of length 2 + 2: unbiased [6, 7] (0.338 > 0.325), biased [5, 7]; nothing pending.  No two candidates spell
#   the same sequence on the way, so the score is the plain sum along the path:
#   score = log p(5 | t0, ctx [0, 0]) + log p(7 | t1, ctx [0, 5]) + log p(0 | t2, ctx [5, 7]) + 3.0
KAT_FLIP = dict(rows=[{5: 1.0, 6: 1.1}, {7: 3.0}, {0: 3.0}], beam=2, phrases=[[5, 7]], unbiased=([6, 7], [0, 1]), biased=([5, 7], [0, 1]))


def kat_flip_score():
    """the hand value above, in float64 from the closed form of the KAT model"""
    def logp(row, tok, boost):
        x = np.full(8, -3.0)
        for k, v in row.items():
            x[k] = v
        x[3] += boost
        z = np.tanh(x)
        return z[tok] - np.log(np.exp(z).sum())
    r = KAT_FLIP["rows"]
    return logp(r[0], 5, 0.1 * (0.5 + 0.5)) + logp(r[1], 7, 0.1 * (0.5 + 5)) + logp(r[2], 0, 0.1 * (5 + 7)) + 3.0
