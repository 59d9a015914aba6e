"""LODR (low-order density ratio) beside the neural LM shallow fusion, restated in Python (helper of test_lodr.py / test_lodr_gpu.py).

The definition is the text in include/k2hip.h ("LODR").  `twin_beam_search` is rnn_lm_fusion_twin.twin_beam_search extended by copy:
the same oracle decoder / joiner operators in the same precision, the same trace, margins and gaps, and behind the neural term
fl32(nscale * q_parent[token]) the LODR term Step(state, token) of `lodr` (an ngram_twin.TwinLm) over its tables scaled ONCE by
lscale <= 0, added last and before HypothesisList.add; nothing at the end.  The LODR term exists only where the neural term does: with
nlm None or nscale == 0 it is off whatever lodr says, and with lodr None or lscale == 0 the search is rnn_lm_fusion_twin's to the bit.
`lodr_total` is the rescoring definition's lodr_i: the float32 sum of the scaled steps of a token list from the start state."""
import numpy as np
import torch

from ngram_twin import BLANK, EVENTS, UNK

f32 = np.float32


def lodr_terms(lodr, lscale, tokens):
    """the scaled step of every token of `tokens` from the start state, in order: [float32]"""
    ls = lodr.scaled(lscale)
    s, out = ls.start, []
    for w in tokens:
        s, term, _ = ls.step(s, int(w))
        out.append(f32(term))
    return out


def lodr_total(lodr, lscale, tokens):
    """lodr_i of the rescoring: the float32 sum, in token order from the start state, of the scaled steps (no eos term)"""
    acc = f32(0)
    for term in lodr_terms(lodr, lscale, tokens):
        acc = f32(acc + term)
    return acc


def rescored_order(scores, lengths, lm_totals, scale, lodr_totals, ctc):
    """rnn_lm_twin.rescored_order extended by the LODR totals: the stable order by (score_i + scale lm_i) + lodr_i, divided by
    (length + 2) under the transducer search; (order, keys in float64)"""
    keys = [((s + scale * l) + d) if ctc else ((s + scale * l) + d) / (n + 2) for s, n, l, d in zip(scores, lengths, lm_totals, lodr_totals)]
    return sorted(range(len(keys)), key=lambda i: (-keys[i], i)), keys


def twin_beam_search(oracle, enc_out, beam=4, lm=None, scale=0.0, graph=None, nlm=None, nscale=0.0, nbest=0, dtype=torch.float32,
                     lodr=None, lscale=0.0):
    """One stream, enc_out [T', J].  The arguments and the result of rnn_lm_fusion_twin.twin_beam_search, and lodr: an ngram_twin.TwinLm
    (scaled here by lscale <= 0).  The result also holds dl (the float32 terms of the pick's tokens, in order), smax (the largest
    absolute partial score the search saw) and, per alternative, dl / dst (its LODR terms and final LODR state)."""
    assert lscale <= 0
    cs = oracle.context_size
    lms = lm.scaled(scale) if lm is not None else None
    fuse = nlm is not None and nscale > 0
    lds = lodr.scaled(lscale) if (fuse and lodr is not None and lscale != 0) else None
    st0, q0 = nlm.start() if fuse else (None, None)
    ys0 = [BLANK] * cs
    B = {tuple(ys0): dict(ys=ys0, log_prob=torch.zeros(1, dtype=dtype), timestamp=[], state=0, lst=lms.start if lms else 0,
                          nst=st0, nq=q0, nl=0.0, yp=[], dst=lds.start if lds else 0, dl=[])}
    T = enc_out.shape[0]
    idx = np.full((T, 2 * beam), -1, np.int32)
    val = np.full((T, 2 * beam), -np.inf, np.float32)
    nsurv = np.zeros(T, np.int32)
    margins = np.full(T + 1, np.inf, np.float32)
    gaps = np.full(T, np.inf, np.float64)
    events = {k: 0 for k in EVENTS}
    smax = 0.0
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
            nst, nq, nl, yp, dst, dl = hyp["nst"], hyp["nq"], hyp["nl"], hyp["yp"], hyp["dst"], hyp["dl"]
            new_log_prob = tv[k].reshape(1)
            smax = max(smax, abs(float(new_log_prob)))
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
                    smax = max(smax, abs(float(new_log_prob)))
                if lds is not None:                                # the LODR term last: ((.. + n-gram) + neural) + Step_lodr
                    dst, term, _ = lds.step(dst, tok)
                    new_log_prob = new_log_prob + torch.tensor([term], dtype=dtype)
                    dl = dl + [f32(term)]
                    smax = max(smax, abs(float(new_log_prob)))
            key = tuple(new_ys)
            if key in B:
                B[key]["log_prob"] = torch.logaddexp(B[key]["log_prob"], new_log_prob)
                smax = max(smax, abs(float(B[key]["log_prob"])))
            else:
                if fuse and tok not in (BLANK, UNK):
                    nst, nq = nlm.step(nst, tok)
                B[key] = dict(ys=new_ys, log_prob=new_log_prob, timestamp=new_ts, state=state, lst=lst, nst=nst, nq=nq, nl=nl, yp=yp,
                              dst=dst, dl=dl)
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
               nl=h["nl"], dl=h["dl"], smax=smax)
    if nbest:
        order = sorted(range(len(norm)), key=lambda i: (-norm[i], i))[:nbest]
        out["alts"] = [dict(tokens=final[i][0]["ys"][cs:], timestamps=final[i][0]["timestamp"], score=float(final[i][1]), nl=final[i][0]["nl"],
                            norm=norm[i], token_log_probs=np.array(final[i][0]["yp"], np.float64), dl=final[i][0]["dl"],
                            dst=final[i][0]["dst"]) for i in order]
        sn = sorted(norm, reverse=True)
        out["norm_gap"] = min([np.inf] + [a - b for a, b in zip(sn, sn[1:])])
    return out


def twin_batch(oracle, enc, beam, nlm=None, nscale=0.0, lm=None, scale=0.0, graph=None, nbest=0, dtype=torch.float32, lodr=None, lscale=0.0):
    """every stream of enc [B, T', J]: (results [(tokens, timestamps)], scores [B], margins [B, T'+1], trace dict, runs)"""
    runs = [twin_beam_search(oracle, enc[b], beam, lm, scale, graph, nlm, nscale, nbest, dtype, lodr, lscale) for b in range(enc.shape[0])]
    trace = dict(idx=np.stack([r["idx"] for r in runs]), val=np.stack([r["val"] for r in runs]), n=np.stack([r["n"] for r in runs]), beam=beam)
    return ([(r["ys"], r["ts"]) for r in runs], np.array([r["lp"] for r in runs], np.float32), np.stack([r["margins"] for r in runs]), trace, runs)
