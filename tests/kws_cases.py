"""Shared inputs of the keyword-spotting tests (test_kws.py on the CPU, test_kws_gpu.py on the GPU): the keyword sets of the issue and
the token-passing cases on planes whose values are multiples of 0.25 (sums along a path are exact in float32 and float64 alike), with
-inf cells.  A DP case is one trie walked by several streams: dict(name, parent, depth, kw, bar, streams=[(stay, emit)], and, for the
hand-built ones, expect=[events per stream] with an event = (keyword, start, end, sum_logp))."""
import numpy as np

KEYWORDS = [[23, 7, 35], [34, 33, 4], [33, 4], [35, 34], [29, 29, 35], [5, 6, 7], [23, 35], [35], [34, 33]]   # 9 keywords, 18 states
THRESHOLD = float(np.exp(-2.45))
NINF = -np.inf


def wide_keywords():
    """70 keywords with distinct first tokens on a vocabulary of 3000: the root has 70 children (more than one tile's 64 lanes), and
    their tokens are spread over many column tiles; lengths 1 .. 3, some sharing later tokens"""
    out = []
    for i in range(70):
        first = 3 + 41 * i
        out.append([first, 1, 2999][: 1 + i % 3] if i % 5 == 0 else [first, 3 + (977 * i) % 2990, 3 + (13 * i) % 50][: 1 + i % 3])
    return out


def _planes(rng, T, S, inf_share):
    stay = (-0.25 * rng.integers(0, 9, size=(T, S))).astype(np.float32)
    emit = (-0.25 * rng.integers(0, 9, size=(T, S))).astype(np.float32)
    if inf_share:
        stay[rng.random(stay.shape) < inf_share] = NINF
        emit[rng.random(emit.shape) < inf_share] = NINF
    emit[:, 0] = NINF
    return stay, emit


def _random_trie(rng, S, chain=False, max_depth=6):
    parent, depth = np.full(S, -1, np.int32), np.zeros(S, np.int32)
    for c in range(1, S):
        p = c - 1 if chain else int(rng.integers(0, c))
        while not chain and depth[p] >= max_depth:
            p = int(parent[p])
        parent[c], depth[c] = p, depth[p] + 1
    kw = np.full(S, -1, np.int32)
    term = [c for c in range(1, S) if rng.random() < 0.4 or (chain and c == S - 1)]
    for i, c in enumerate(rng.permutation(term)):       # keyword indices in no particular order of the states
        kw[c] = i
    # bars that values reach exactly now and then: a multiple of 0.25 near the typical path sum (-1 per arc)
    bar = np.where(kw >= 0, -0.25 * rng.integers(2, 7, size=S) * np.maximum(depth, 1), 0).astype(np.float32)
    return parent, depth, kw, bar


def random_cases():
    """S in {1, 2, 65, 257, 1024} x T in {1, 2, 64}, three streams each (one with -inf cells), and chains deeper than T"""
    rng = np.random.default_rng(20)
    cases = []
    for S in (1, 2, 65, 257, 1024):
        for T in (1, 2, 64):
            parent, depth, kw, bar = _random_trie(rng, S)
            cases.append(dict(name=f"random S={S} T={T}", parent=parent, depth=depth, kw=kw, bar=bar,
                              streams=[_planes(rng, T, S, share) for share in (0.0, 0.0, 0.15)]))
    for S, T in ((65, 2), (65, 64), (257, 64)):
        parent, depth, kw, bar = _random_trie(rng, S, chain=True)
        cases.append(dict(name=f"chain S={S} T={T}", parent=parent, depth=depth, kw=kw, bar=bar, streams=[_planes(rng, T, S, 0.0), _planes(rng, T, S, 0.05)]))
    return cases


def _stream(T, S, stay=(), emit=()):
    """planes of -inf emits and 0 stays, then the listed cells (t, s, value)"""
    st, em = np.zeros((T, S), np.float32), np.full((T, S), NINF, np.float32)
    for t, s, v in stay:
        st[t, s] = v
    for t, s, v in emit:
        em[t, s] = v
    return st, em


def hand_cases():
    """the rules one by one.  Trie: 1 = keyword 1 (depth 1), 2 = keyword 0 (depth 1), 3 -> 4 = keyword 2 (depth 2), 5 -> 6 no keyword"""
    parent = np.array([-1, 0, 0, 0, 3, 0, 5], np.int32)
    depth = np.array([0, 1, 1, 1, 2, 1, 2], np.int32)
    kw = np.array([-1, 1, 0, -1, 2, -1, -1], np.int32)
    bar = np.array([0, -0.5, -0.5, 0, -1.0, 0, 0], np.float32)
    S = 7
    streams, expect, states = [], [], []
    # 0: an exact ve == vs tie at state 5 in frame 1 (ve = -0.75 from the root, vs = -0.5 - 0.25): emit wins, so start moves 0 -> 1
    streams.append(_stream(2, S, stay=[(1, 5, -0.25)], emit=[(0, 5, -0.5), (1, 5, -0.75)]))
    expect.append([])
    states.append({5: (-0.75, 1)})
    # 1: a == bar exactly fires (keyword 1 at -0.5); 2: one step below does not
    streams.append(_stream(1, S, emit=[(0, 1, -0.5)]))
    expect.append([(1, 0, 0, -0.5)])
    states.append({1: (NINF, -1)})
    streams.append(_stream(1, S, emit=[(0, 1, -0.75)]))
    expect.append([])
    states.append({1: (-0.75, 0)})
    # 3: two terminals of one depth qualify in one frame: the larger a wins (keyword 0 at -0.25 over keyword 1 at -0.5)
    streams.append(_stream(1, S, emit=[(0, 1, -0.5), (0, 2, -0.25)]))
    expect.append([(0, 0, 0, -0.25)])
    states.append({1: (NINF, -1), 2: (NINF, -1)})
    # 4: equal a: the smaller keyword index wins (keyword 0 sits in state 2, keyword 1 in state 1)
    streams.append(_stream(1, S, emit=[(0, 1, -0.25), (0, 2, -0.25)]))
    expect.append([(0, 0, 0, -0.25)])
    states.append({})
    # 5: three terminals qualify in frame 1: the deepest wins although its a is the lowest (keyword 2 at -0.75, start 0)
    streams.append(_stream(2, S, emit=[(0, 3, -0.25), (1, 1, -0.25), (1, 2, -0.25), (1, 4, -0.5)]))
    expect.append([(2, 0, 1, -0.75)])
    states.append({1: (NINF, -1), 3: (NINF, -1)})
    # 6: the reset: keyword 1 fires in frame 1 and kills the token in state 3, so keyword 2 does not complete in frame 2 ...
    streams.append(_stream(3, S, emit=[(0, 3, -0.25), (1, 1, -0.25), (2, 4, -0.25)]))
    expect.append([(1, 1, 1, -0.25)])
    states.append({3: (NINF, -1), 4: (NINF, -1)})
    # 7: ... as it does when keyword 1 stays below its bar
    streams.append(_stream(3, S, emit=[(0, 3, -0.25), (1, 1, -0.75), (2, 4, -0.25)]))
    expect.append([(2, 0, 2, -0.5)])
    states.append({})
    # 8: the root restarts at t + 1: an event in every frame, each starting where it ends
    streams.append(_stream(3, S, emit=[(0, 1, -0.25), (1, 1, -0.5), (2, 2, -0.25)]))
    expect.append([(1, 0, 0, -0.25), (1, 1, 1, -0.5), (0, 2, 2, -0.25)])
    states.append({})
    return [dict(name="hand", parent=parent, depth=depth, kw=kw, bar=bar, streams=streams, expect=expect, states=states)]

