"""The modified beam search with N-best output and token log-probs restated in Python (helper of test_nbest.py / test_nbest_gpu.py).

The definition is the text in include/k2hip.h ("N-best hypotheses and token log-probs") and DESIGN.md.  This is `twin_beam_search` of
tests/hotword_twin.py -- the same oracle decoder / joiner operators, torch log_softmax / topk / logaddexp, the hotword bonus added after
the frame's top-k and before HypothesisList.add -- with two things more: every hypothesis carries, parallel to its timestamps, the
UNBIASED log-softmax value of each emitted token at the frame it was emitted (the first-inserted hypothesis keeps its own at a merge),
and instead of the best survivor all of them come back, ordered by the final pick's quantity (finalized log-prob) / len(ys),
descending, ties in insertion order."""
import numpy as np
import torch

from hotword_twin import BLANK, UNK, TwinGraph  # noqa: F401  (TwinGraph: re-exported for the tests)


def nbest_twin_search(oracle, enc_out, beam=4, graph=None):
    """One stream, enc_out [T', J].  Returns dict(alts = [dict(tokens, timestamps, token_log_probs (float32 array), score (finalized
    log-prob), norm (score / (length + 2)))] in final order, order = the survivors' insertion indexes in that order, min_gap = the
    smallest difference between adjacent normalised scores in the final order (inf with fewer than two survivors))."""
    cs = oracle.context_size
    ys0 = [BLANK] * cs
    B = {tuple(ys0): dict(ys=ys0, log_prob=torch.zeros(1, dtype=torch.float32), timestamp=[], yp=[], state=0)}
    for t in range(enc_out.shape[0]):
        A = list(B.values())
        B = {}
        ys_log_probs = torch.cat([h["log_prob"].reshape(1, 1) for h in A])
        decoder_out = oracle.decoder(np.array([h["ys"][-cs:] for h in A], np.int64))
        logits = torch.from_numpy(oracle.joiner(np.repeat(enc_out[t: t + 1], len(A), 0), decoder_out))
        unbiased = logits.log_softmax(dim=-1)              # the token log-prob term, before the hypothesis' log-prob is added
        log_probs = unbiased + ys_log_probs
        V = log_probs.size(-1)
        log_probs = log_probs.reshape(-1)
        want = min(beam, log_probs.numel())
        flat = log_probs.numpy()
        ti = torch.from_numpy(np.lexsort((np.arange(flat.size), -flat))[:want].copy())   # (score desc, flat index asc) over ALL candidates
        tv = log_probs[ti]
        for k in range(want):
            a = int(ti[k]) // V
            hyp, tok = A[a], int(ti[k]) % V
            new_ys, new_ts, new_yp, state = hyp["ys"][:], hyp["timestamp"][:], hyp["yp"][:], hyp["state"]
            new_log_prob = tv[k].reshape(1)
            if tok not in (BLANK, UNK):
                new_ys.append(tok)
                new_ts.append(t)
                new_yp.append(float(unbiased[a, tok]))
                if graph is not None:
                    state, bonus, _ = graph.step(state, tok)
                    new_log_prob = new_log_prob + torch.tensor([bonus], dtype=torch.float32)
            key = tuple(new_ys)
            if key in B:   # the first-inserted hypothesis keeps its timestamps, token log-probs and state
                B[key]["log_prob"] = torch.logaddexp(B[key]["log_prob"], new_log_prob)
            else:
                B[key] = dict(ys=new_ys, log_prob=new_log_prob, timestamp=new_ts, yp=new_yp, state=state)
    surv = list(B.values())
    fin = []
    for h in surv:
        lp = h["log_prob"]
        if graph is not None:
            lp = lp - torch.tensor([graph.pending(h["state"])], dtype=torch.float32)
        fin.append(lp)
    norm = [float(lp / len(h["ys"])) for h, lp in zip(surv, fin)]      # (float32 division; len counts the ctx blanks)
    order = sorted(range(len(surv)), key=lambda i: (-norm[i], i))
    alts = [dict(tokens=surv[i]["ys"][cs:], timestamps=surv[i]["timestamp"], token_log_probs=np.array(surv[i]["yp"], np.float32),
                 score=float(fin[i]), norm=norm[i]) for i in order]
    gaps = [alts[i]["norm"] - alts[i + 1]["norm"] for i in range(len(alts) - 1)]
    return dict(alts=alts, order=order, min_gap=min(gaps) if gaps else float("inf"))


def nbest_twin_batch(oracle, enc, beam, graph=None):
    """every stream of enc [B, T', J]: [nbest_twin_search result]"""
    return [nbest_twin_search(oracle, enc[b], beam, graph) for b in range(enc.shape[0])]


# ---- the merge case on the KAT model (tests/kat_model.py: logits = tanh(enc + dec), only token 3's logit depends on the context) -----
# Frames: t0 offers blank and 5 alike (1.0 each), t1 offers blank (1.5) over 5 (1.0); every other pre-tanh input is -3 (token 3:
# -3 + boost, boost = 0.1 (e_prev + e_cur), e_blank = 0.5, e_v = v); beam 4.
#   t0, ctx [0, 0]: p(0) = p(5) = 0.329, the others 0.057 -> the hypotheses are [] (from blank, the lower index on the tie), [5]
#       (timestamp 0, token log-prob log p_t0(5)), [3], [1].
#   t1: p(0) = 0.362, p(5) = 0.314 under ctx [0, 0], a hair less under ctx [0, 5] (boost 0.55 instead of 0.1).  The selection in rank
#       order: [] + blank, [5] + blank, [] + 5, [5] + 5 (anything from [3] / [1] is < 0.057 x 0.37).  [5] + blank is inserted FIRST and
#       spells [5] with timestamp 0; [] + 5 spells [5] too (timestamp 1, token log-prob log p_t1(5)) and is merged into it: the survivor
#       keeps timestamp 0 and log p_t0(5), not log p_t1(5) -- the two differ by 0.05.
#   With the phrase [5] (c = 1.5, committed at once, nothing pending): t0's selection is unbiased and the same; at t1 [5] carries +1.5, so
#       the rank order becomes [5] + blank, [5] + 5, [] + blank, [] + 5 -- the same four, [5] + blank still before [] + 5; [] + 5 earns
#       its own +1.5 before the merge.  Both parts of the merged [5] carry +1.5: its score is the unbiased one + 1.5, its token
#       log-probs are the unbiased ones.
KAT_MERGE = dict(rows=[{0: 1.0, 5: 1.0}, {0: 1.5, 5: 1.0}], beam=4, phrases=[[5]])


def kat_merge_logp(frame, tok, boost):
    """log p(tok | frame, context boost) in float64 from the closed form of the KAT model"""
    x = np.full(8, -3.0)
    for k, v in KAT_MERGE["rows"][frame].items():
        x[k] = v
    x[3] += boost
    z = np.tanh(x)
    return z[tok] - np.log(np.exp(z).sum())
