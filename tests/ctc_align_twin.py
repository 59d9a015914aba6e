"""CTC forced alignment and full-sum scoring restated in float64 (helper of test_ctc_align.py / test_ctc_align_gpu.py).

The definition is the text in include/k2hip.h ("CTC forced alignment and full-sum scoring ...") and DESIGN.md.  lp [T][V] are
log-softmaxed rows; the target y_1 .. y_U has the extended sequence z = [blank, y_1, blank, .., y_U, blank], S = 2U + 1 states; state s
at frame t is reached from s, s-1 and -- when z_s is a token and differs from z_{s-2} -- s-2, every arrival pays lp(t, z_s); frame 0
starts in state 0 or 1; the path ends in state S-1 or S-2.  The tie rule is the one of csrc/ctc_lattice_ref.h: the lowest state index
wins (s-2 over s-1 over s), at the end S-2 over S-1; a cell outside the reachable band counts as -inf and its back-pointer is 1."""
import itertools

import numpy as np

BLANK = 0


def in_band(t, s, T, S):
    return s <= 2 * t + 1 and S - 1 - s <= 2 * (T - 1 - t) + 1


def min_frames(target):
    y = [int(v) for v in target]
    return len(y) + sum(a == b for a, b in zip(y, y[1:]))


def collapse(labels):
    out, prev = [], -1
    for v in labels:
        if v != BLANK and v != prev:
            out.append(int(v))
        prev = v
    return out


def ctc_lattice(lp, target):
    """lp [T][V] (the frames that count), target: U ids in [1, V) -> dict(total, best, timestamps [U], end_frames [U],
    token_log_probs [U], states [T] (the best path))"""
    lp = np.asarray(lp, np.float64)
    y = [int(v) for v in target]
    T, U = lp.shape[0], len(y)
    S = 2 * U + 1
    assert T >= 1 and min_frames(y) <= T
    z = [y[(s - 1) // 2] if s & 1 else BLANK for s in range(S)]
    skip = [bool(s & 1) and s >= 3 and z[s] != z[s - 2] for s in range(S)]
    f = np.full((T, S), -np.inf)
    v = np.full((T, S), -np.inf)
    bp = np.ones((T, S), np.int64)
    for s in range(min(S, 2)):
        if in_band(0, s, T, S):
            f[0, s] = v[0, s] = lp[0, z[s]]
    for t in range(1, T):
        for s in range(S):
            if not in_band(t, s, T, S):
                continue
            x = lp[t, z[s]]
            acc, m, p = f[t - 1, s], v[t - 1, s], 0
            if s > 0:
                acc = np.logaddexp(acc, f[t - 1, s - 1])
                if v[t - 1, s - 1] >= m:
                    m, p = v[t - 1, s - 1], 1
            if skip[s]:
                acc = np.logaddexp(acc, f[t - 1, s - 2])
                if v[t - 1, s - 2] >= m:
                    m, p = v[t - 1, s - 2], 2
            f[t, s] = acc + x
            v[t, s] = m + x
            bp[t, s] = p
    s = S - 1
    if U == 0:
        total = f[T - 1, 0]
    else:
        total = np.logaddexp(f[T - 1, S - 2], f[T - 1, S - 1])
        if v[T - 1, S - 2] >= v[T - 1, S - 1]:
            s = S - 2
    best = v[T - 1, s]
    states = [0] * T
    for t in range(T - 1, -1, -1):
        states[t] = s
        if t > 0:
            s = max(0, s - (int(bp[t, s]) if in_band(t, s, T, S) else 1))
    ts, en = [0] * U, [0] * U
    for t in range(T - 1, -1, -1):
        if states[t] & 1:
            ts[(states[t] - 1) // 2] = t
    for t in range(T):
        if states[t] & 1:
            en[(states[t] - 1) // 2] = t
    return dict(total=float(total), best=float(best), timestamps=ts, end_frames=en,
                token_log_probs=np.array([lp[ts[u], y[u]] for u in range(U)], np.float64), states=states)


def path_score(lp, target, timestamps, end_frames):
    """the score of the frame labelling that (timestamps, end_frames) describe: y_{u+1} on its frames, blank elsewhere"""
    lp = np.asarray(lp, np.float64)
    lab = np.zeros(lp.shape[0], np.int64)
    for u, y in enumerate(target):
        lab[timestamps[u]: end_frames[u] + 1] = int(y)
    assert collapse(lab) == [int(v) for v in target]
    return float(lp[np.arange(lp.shape[0]), lab].sum())


def brute_force(lp, target):
    """(total, best) over every labelling of the T frames that collapses to the target"""
    lp = np.asarray(lp, np.float64)
    T, V = lp.shape
    y = [int(v) for v in target]
    scores = [sum(lp[t, lab[t]] for t in range(T)) for lab in itertools.product(range(V), repeat=T) if collapse(lab) == y]
    scores = [s for s in scores if s != -np.inf]
    if not scores:
        return -np.inf, -np.inf
    m = max(scores)
    return float(m + np.log(sum(np.exp(s - m) for s in scores))), float(m)


def all_targets(V, max_len):
    for n in range(max_len + 1):
        yield from (list(t) for t in itertools.product(range(1, V), repeat=n))
