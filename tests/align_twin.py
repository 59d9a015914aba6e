"""Forced alignment and full-sum scoring on the RNN-T lattice restated in float64 (helper of test_align.py / test_align_gpu.py).

The definition is the text in include/k2hip.h ("Forced alignment and full-sum scoring ...") and DESIGN.md.  Cells come from the oracle's
decoder / joiner operators (as tests/nbest_twin.py takes its logits) followed by a float64 log-softmax:
    stay(t,u) = logaddexp(lp(t,u,blank), lp(t,u,unk))     (t,u) -> (t+1,u)
    emit(t,u) = lp(t,u,y_{u+1})                            (t,u) -> (t+1,u+1), u < U
with the context of position u the last context_size ids of [blank, blank, y_1 .. y_u].  `lattice_dp` runs the forward (logaddexp) and
the Viterbi (max, the emit predecessor wins exact ties) recursions over two planes [T][U+1] and backtraces."""
import itertools

import numpy as np

BLANK, UNK = 0, 2


def lattice_cells(oracle, enc, target):
    """enc [T, J] (the frames that count), target: U ids -> (stay, emit) float64 [T][U+1]; emit[:, U] = -inf"""
    cs = oracle.context_size
    T, U = enc.shape[0], len(target)
    ys = [BLANK] * cs + [int(y) for y in target]
    ctx = np.array([ys[u: u + cs] for u in range(U + 1)], np.int64)
    dec = oracle.decoder(ctx)                                   # [U+1, J]
    stay = np.empty((T, U + 1))
    emit = np.full((T, U + 1), -np.inf)
    for t in range(T):
        logits = np.asarray(oracle.joiner(np.repeat(enc[t: t + 1], U + 1, 0), dec), np.float64)   # [U+1, V]
        m = logits.max(axis=1, keepdims=True)
        lp = logits - (m + np.log(np.exp(logits - m).sum(axis=1, keepdims=True)))
        stay[t] = np.logaddexp(lp[:, BLANK], lp[:, UNK])
        if U:
            emit[t, :U] = lp[np.arange(U), np.asarray(target, np.int64)]
    return stay, emit


def in_band(t, u, T, U):
    return u <= t and U - u <= T - t


def lattice_dp(stay, emit):
    """-> dict(total, best, timestamps [U], token_log_probs [U]); cells outside the reachable band are never read"""
    T, U1 = stay.shape
    U = U1 - 1
    assert 0 <= U <= T
    f = np.full(U1, -np.inf)
    v = np.full(U1, -np.inf)
    f[0] = v[0] = 0.0
    bp = np.zeros((T, U1), bool)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            nf = np.full(U1, -np.inf)
            nv = np.full(U1, -np.inf)
            for u in range(U1):
                fs = vs = fe = ve = -np.inf
                if in_band(t, u, T, U):
                    fs, vs = f[u] + stay[t, u], v[u] + stay[t, u]
                if u > 0 and in_band(t, u - 1, T, U):
                    fe, ve = f[u - 1] + emit[t, u - 1], v[u - 1] + emit[t, u - 1]
                nf[u] = np.logaddexp(fs, fe) if max(fs, fe) > -np.inf else -np.inf
                by_emit = u > 0 and ve >= vs
                nv[u] = ve if by_emit else vs
                bp[t, u] = by_emit
            f, v = nf, nv
    ts, yp = [0] * U, [0.0] * U
    u = U
    for t in range(T, 0, -1):
        if u > 0 and bp[t - 1, u]:
            ts[u - 1] = t - 1
            yp[u - 1] = float(emit[t - 1, u - 1])
            u -= 1
    assert u == 0
    return dict(total=float(f[U]), best=float(v[U]), timestamps=ts, token_log_probs=np.array(yp))


def path_score(stay, emit, timestamps):
    """the log-prob of the path that emits y_{u+1} at frame timestamps[u] and stays everywhere else"""
    T, U1 = stay.shape
    assert len(timestamps) == U1 - 1
    u, lp = 0, 0.0
    for t in range(T):
        if u < U1 - 1 and timestamps[u] == t:
            lp += emit[t, u]
            u += 1
        else:
            lp += stay[t, u]
    assert u == U1 - 1, "the timestamps do not describe a path"
    return lp


def brute_force(stay, emit):
    """(total, best) by enumerating all C(T, U) paths"""
    T, U1 = stay.shape
    lps = [path_score(stay, emit, list(c)) for c in itertools.combinations(range(T), U1 - 1)]
    lps = np.array(lps)
    m = lps.max()
    if m == -np.inf:
        return -np.inf, -np.inf
    return float(m + np.log(np.exp(lps - m).sum())), float(m)


def align_twin(oracle, enc_out, targets, n_frames=None):
    """every stream of enc_out [B, T', J]: dict(stay, emit) + lattice_dp's result"""
    out = []
    for b in range(enc_out.shape[0]):
        T = enc_out.shape[1] if n_frames is None else int(n_frames[b])
        stay, emit = lattice_cells(oracle, enc_out[b, :T], targets[b])
        out.append(dict(stay=stay, emit=emit, **lattice_dp(stay, emit)))
    return out
