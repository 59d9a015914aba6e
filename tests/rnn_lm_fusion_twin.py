"""Neural LM shallow fusion of the modified beam search restated in Python (helper of test_rnn_lm_fusion.py /
test_rnn_lm_fusion_gpu.py).

The definition is the text in include/k2hip.h ("Neural LM shallow fusion").  `FusionLm` steps rnn_lm_twin.Twin -- torch's own
Embedding + LSTM + Linear + log_softmax in float64 -- one token at a time; `twin_beam_search` is ngram_twin.twin_beam_search extended
by copy: the same oracle decoder / joiner operators in the same precision, the same trace and margins, the neural term
fl32(scale * q_parent[token]) added after the hotword bonus and the n-gram term and before HypothesisList.add, nothing at the end."""
import numpy as np
import torch

from ngram_twin import BLANK, EVENTS, UNK

f32 = np.float32


class FusionLm:
    """the LM of a rnn_lm_twin.Twin as the search carries it: a state is (h, c) [L, 1, H] float64, its row q [V] float64"""

    def __init__(self, twin):
        self.tw = twin

    def _advance(self, state, token):
        tw = self.tw
        with torch.no_grad():
            x = tw.emb(torch.tensor([[int(token)]], dtype=torch.long))
            y, (h, c) = tw.rnn(x, state)
            q = torch.log_softmax(tw.out(y[0, -1]), dim=-1).numpy().copy()
        return (h, c), q

    def start(self):
        z = torch.zeros(self.tw.L, 1, self.tw.H, dtype=torch.float64)
        return self._advance((z, z.clone()), self.tw.sos)

    def step(self, state, token):
        return self._advance(state, token)


class Oracle64:
    """the decoder and joiner operators of a model file restated in float64 numpy from its tensors (decoder: embedding, grouped Conv1d of
    kernel 2 without bias, ReLU, joiner.decoder_proj; joiner: tanh(enc + dec) through joiner.output_linear): the yardstick the float32
    twin's own score error is measured against (rnn_lm_fusion_cases.SCORE_E32)"""

    def __init__(self, path, oracle):
        from k2transducerasr_amd.k2w import read_k2w
        t = read_k2w(path)
        t = dict(t[1]) if isinstance(t, tuple) else dict(t)
        g = lambda k: np.asarray(t[k], np.float64)   # noqa: E731
        self.emb, self.conv = g("decoder.embedding.weight"), g("decoder.conv.weight")
        self.dw, self.db = g("joiner.decoder_proj.weight"), g("joiner.decoder_proj.bias")
        self.ow, self.ob = g("joiner.output_linear.weight"), g("joiner.output_linear.bias")
        self.context_size, self.vocab_size = oracle.context_size, oracle.vocab_size

    def decoder(self, ctx):
        ctx = np.asarray(ctx, np.int64).reshape(-1, 2)
        DD, cpg = self.conv.shape[0], self.conv.shape[1]
        e = self.emb[ctx]                                    # [n, 2, DD]
        h = np.zeros((ctx.shape[0], DD))
        for co in range(DD):
            g0 = (co // cpg) * cpg
            h[:, co] = np.einsum("nkc,ck->n", e[:, :, g0: g0 + cpg], self.conv[co])
        return np.maximum(h, 0) @ self.dw.T + self.db

    def joiner(self, enc, dec):
        return np.tanh(np.asarray(enc, np.float64) + dec) @ self.ow.T + self.ob


def twin_beam_search(oracle, enc_out, beam=4, lm=None, scale=0.0, graph=None, nlm=None, nscale=0.0, nbest=0, dtype=torch.float32):
    """One stream, enc_out [T', J].  lm: an ngram_twin.TwinLm (scaled here), graph: a hotword TwinGraph, nlm: a FusionLm with weight
    nscale (None or nscale == 0: the search of ngram_twin, to the bit).  Returns dict(ys, ts, lp, margins [T'+1], idx / val
    [T', 2 beam], n [T'], events, gaps [T'] (the smallest consecutive gap among the top beam + 1 candidates of each frame), nl (the float64
    sum of the pick's neural terms), alts (with nbest: the final hypotheses in pick order, dicts of tokens / timestamps / score / nl /
    norm / token_log_probs -- the acoustic log-softmax term of each token at the frame it was appended)).  dtype = torch.float64 with
    an Oracle64: the same search with nothing rounded to float32 (the trace arrays stay float32)."""
    cs = oracle.context_size
    lms = lm.scaled(scale) if lm is not None else None
    fuse = nlm is not None and nscale > 0
    st0, q0 = nlm.start() if fuse else (None, None)
    ys0 = [BLANK] * cs
    B = {tuple(ys0): dict(ys=ys0, log_prob=torch.zeros(1, dtype=dtype), timestamp=[], state=0, lst=lms.start if lms else 0,
                          nst=st0, nq=q0, nl=0.0, yp=[])}
    T = enc_out.shape[0]
    idx = np.full((T, 2 * beam), -1, np.int32)
    val = np.full((T, 2 * beam), -np.inf, np.float32)
    nsurv = np.zeros(T, np.int32)
    margins = np.full(T + 1, np.inf, np.float32)
    gaps = np.full(T, np.inf, np.float64)
    events = {k: 0 for k in EVENTS}
    for t in range(T):
        A = list(B.values())
        B = {}
        ys_log_probs = torch.cat([h["log_prob"].reshape(1, 1) for h in A])
        decoder_out = oracle.decoder(np.array([h["ys"][-cs:] for h in A], np.int64))
        logits = torch.from_numpy(oracle.joiner(np.repeat(enc_out[t: t + 1], len(A), 0), decoder_out))
        log_probs = logits.log_softmax(dim=-1)
        acoustic = log_probs.clone()
        log_probs.add_(ys_log_probs)
        V = log_probs.size(-1)
        log_probs = log_probs.reshape(-1)
        ti = torch.from_numpy(np.lexsort((np.arange(log_probs.numel()), -log_probs.numpy()))[: 2 * beam].copy())
        tv = log_probs[ti]
        idx[t, : len(ti)] = ti.numpy()
        val[t, : len(ti)] = tv.numpy()
        want = min(beam, log_probs.numel())
        if len(ti) > want:
            margins[t] = tv[want - 1] - tv[want]
        top = tv.numpy()[: beam + 1].astype(np.float64)
        if len(top) > 1:
            gaps[t] = float(np.min(top[:-1] - top[1:]))
        for k in range(want):
            hyp = A[int(ti[k]) // V]
            tok = int(ti[k]) % V
            new_ys, new_ts, state, lst = hyp["ys"][:], hyp["timestamp"][:], hyp["state"], hyp["lst"]
            nst, nq, nl, yp = hyp["nst"], hyp["nq"], hyp["nl"], hyp["yp"]
            new_log_prob = tv[k].reshape(1)
            if tok not in (BLANK, UNK):
                new_ys.append(tok)
                new_ts.append(t)
                yp = yp + [float(acoustic[int(ti[k]) // V, tok])]
                if graph is not None:
                    state, bonus, _ = graph.step(state, tok)
                    new_log_prob = new_log_prob + torch.tensor([bonus], dtype=dtype)
                if lms is not None:
                    lst, term, ev = lms.step(lst, tok)
                    new_log_prob = new_log_prob + torch.tensor([term], dtype=dtype)
                    if ev in events:
                        events[ev] += 1
                if fuse:
                    term = float(nscale) * float(nq[tok])
                    if dtype == torch.float32:
                        term = f32(term)                           # the float64 product rounded to float32, then the float32 sum
                    new_log_prob = new_log_prob + torch.tensor([term], dtype=dtype)
                    nl = nl + float(term)
            key = tuple(new_ys)
            if key in B:
                B[key]["log_prob"] = torch.logaddexp(B[key]["log_prob"], new_log_prob)
            else:
                if fuse and tok not in (BLANK, UNK):
                    nst, nq = nlm.step(nst, tok)
                B[key] = dict(ys=new_ys, log_prob=new_log_prob, timestamp=new_ts, state=state, lst=lst, nst=nst, nq=nq, nl=nl, yp=yp)
        nsurv[t] = len(B)
    final = []
    for h in B.values():
        lp = h["log_prob"]
        if graph is not None:
            lp = lp - torch.tensor([graph.pending(h["state"])], dtype=dtype)
        final.append((h, lp))
    norm = [float(lp / len(h["ys"])) for h, lp in final]
    best = int(np.argmax(norm))   # (first maximum)
    if len(norm) > 1:
        margins[T] = norm[best] - max(x for i, x in enumerate(norm) if i != best)
    h, lp = final[best]
    out = dict(ys=h["ys"][cs:], ts=h["timestamp"], lp=float(lp), margins=margins, idx=idx, val=val, n=nsurv, events=events, gaps=gaps,
               nl=h["nl"])
    if nbest:
        order = sorted(range(len(norm)), key=lambda i: (-norm[i], i))[:nbest]
        out["alts"] = [dict(tokens=final[i][0]["ys"][cs:], timestamps=final[i][0]["timestamp"], score=float(final[i][1]), nl=final[i][0]["nl"],
                            norm=norm[i], token_log_probs=np.array(final[i][0]["yp"], np.float64)) for i in order]
        sn = sorted(norm, reverse=True)
        out["norm_gap"] = min([np.inf] + [a - b for a, b in zip(sn, sn[1:])])
    return out


def twin_batch(oracle, enc, beam, nlm=None, nscale=0.0, lm=None, scale=0.0, graph=None, nbest=0, dtype=torch.float32):
    """every stream of enc [B, T', J]: (results [(tokens, timestamps)], scores [B], margins [B, T'+1], trace dict, runs)"""
    runs = [twin_beam_search(oracle, enc[b], beam, lm, scale, graph, nlm, nscale, nbest, dtype) for b in range(enc.shape[0])]
    trace = dict(idx=np.stack([r["idx"] for r in runs]), val=np.stack([r["val"] for r in runs]), n=np.stack([r["n"] for r in runs]), beam=beam)
    return ([(r["ys"], r["ts"]) for r in runs], np.array([r["lp"] for r in runs], np.float32), np.stack([r["margins"] for r in runs]), trace, runs)


def case_gap(run):
    """the smallest gap the acceptance rule looks at: consecutive gaps among the top beam + 1 candidates of every frame, and adjacent
    final normalised scores"""
    return float(min(float(np.min(run["gaps"])), run.get("norm_gap", np.inf)))
