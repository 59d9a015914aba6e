"""Case lists of the CTC keyword spotter's tests (test_ctc_kws.py on the CPU, test_ctc_kws_gpu.py on the GPU).

A case is dict(name, parent, tok, depth, kw int32 [S], bar float32 [S], rc int32 [S], V, streams = [lp float32 [T][V]], and optionally
blocks = [(v float32 [2][S], st int32 [2][S]) or None per stream] (the carried block a stream resumes from), expect = [events per stream]
with an event (keyword, start, end, sum_logp), states = [{(plane, c): (value, start)} per stream] (cells after the last frame; plane 0 = n,
plane 1 = b).  All log-probs and bars are multiples of 0.25 (or -inf), so every sum is exact in float32 and in float64 alike.

The fixture set of the end-to-end tests: KEYWORDS with one threshold per keyword length, on the `utts` fixture's log-probs of
zipformer2-ctc-tiny-test (5 x 35 x 37)."""
import numpy as np

from ctc_kws_twin import build_trie, fresh_state, root_children

INF = np.inf

KEYWORDS = [[13], [34], [12], [13, 14], [34, 30], [13, 14, 34], [34, 30, 12], [30], [13, 34], [30, 9], [12, 13], [13, 34, 30], [30, 9, 12], [31],
            [34, 13], [30, 12], [31, 13], [34, 13, 30], [30, 12, 31], [13, 30], [13, 34, 13], [13, 30, 31], [13, 13], [12, 12, 13]]
THRESHOLD_BY_LENGTH = {1: np.exp(-1.0), 2: np.exp(-1.5), 3: np.exp(-1.8)}
THRESHOLDS = [float(THRESHOLD_BY_LENGTH[len(k)]) for k in KEYWORDS]


def tables(trie):
    """the int32 / float32 arrays the native entries take"""
    return dict(parent=np.asarray(trie["parent"], np.int32), tok=np.asarray(trie["tok"], np.int32), depth=np.asarray(trie["depth"], np.int32),
                kw=np.asarray(trie["kw"], np.int32), bar=np.asarray(trie["bar"], np.float32), rc=root_children(trie).astype(np.int32))


def rows(V, *frames, rest=-8.0):
    """one [T][V] plane: every frame a {column: value} dict, the other columns `rest`"""
    lp = np.full((len(frames), V), rest, np.float32)
    for t, f in enumerate(frames):
        for k, x in f.items():
            lp[t, k] = x
    return lp


def block(S, frames, hold, cells):
    """a carried block: cells = {(plane, c): (value, start)}, the others (-inf, -1)"""
    v, st = fresh_state(S)
    st[0, 0], st[1, 0] = frames, hold
    for (pl, c), (x, s) in cells.items():
        v[pl, c], st[pl, c] = x, s
    return v.astype(np.float32), st.astype(np.int32)


def case(name, words, bars, V, streams, expect, blocks=None, states=None):
    """bars: bar of keyword p (taken as given: a multiple of 0.25)"""
    trie = build_trie(words, 0.5)
    for s in range(len(trie["parent"])):
        trie["bar"][s] = bars[trie["kw"][s]] if trie["kw"][s] >= 0 else 0.0
    c = dict(name=name, V=V, streams=streams, expect=expect, **tables(trie))
    if blocks is not None:
        c["blocks"] = blocks
    if states is not None:
        c["states"] = states
    return c


def hand_cases():
    A, B, C = 1, 3, 4   # tokens (V = 5)
    out = []
    # Keyword A B: state 1 = A, state 2 = A B.  One frame (absolute frame 7) with lp(B) = -0.5, lp(A) = -4, lp(blank) = -0.25 behind carried cells.
    fr = rows(5, {0: -0.25, A: -4, B: -0.5})
    out.append(case(
        "ties", [[A, B]], [-1.5], 5, [fr, fr, fr],
        # stream 0: n[1] = b[1] = n[2] = -1, the three-way tie for n[2]: n[parent] wins, start 5, the state is entered; n == bar exactly
        # stream 1: b[1] = n[2] = -1 above n[1]: b[parent] wins the tie with the self loop, start 3
        # stream 2: the self loop alone is best: no event; n[1] = b[1] and n[2] = b[2] tie for b: n wins (starts 5 and 1)
        expect=[[(0, 5, 7, -1.5)], [(0, 3, 7, -1.5)], []],
        blocks=[block(3, 7, -1, {(0, 1): (-1, 5), (1, 1): (-1, 3), (0, 2): (-1, 1)}),
                block(3, 7, -1, {(0, 1): (-1.25, 5), (1, 1): (-1, 3), (0, 2): (-1, 1)}),
                block(3, 7, -1, {(0, 1): (-1.25, 5), (1, 1): (-1.25, 3), (0, 2): (-1, 1), (1, 2): (-1, 0)})],
        states=[{(0, 0): (0, 8), (1, 0): (-INF, -1), (0, 2): (-INF, -1)}, {(0, 2): (-INF, -1)},
                {(0, 0): (0, 8), (0, 1): (-4, 7), (0, 2): (-1.5, 1), (1, 1): (-1.5, 5), (1, 2): (-1.25, 1)}]))
    # the same frame under a bar a quarter higher: n[2] = -1.5 < bar, no event, the cell lives on with the parent's start
    out.append(case("below_bar", [[A, B]], [-1.25], 5, [fr], expect=[[]], blocks=[block(3, 7, -1, {(0, 1): (-1, 5), (1, 1): (-1, 3), (0, 2): (-1, 1)})],
                    states=[{(0, 2): (-1.5, 5), (1, 2): (-1.25, 1), (1, 1): (-1.25, 5)}]))
    # keyword A A behind a block: n[parent] is not allowed (the same token), b[parent] ties with the self loop and wins
    out.append(case("repeat_tie", [[A, A]], [-2.0], 5, [rows(5, {0: -0.25, A: -0.5})], expect=[[(0, 3, 7, -1.5)]],
                    blocks=[block(3, 7, -1, {(0, 1): (-0.5, 5), (1, 1): (-1, 3), (0, 2): (-1, 1)})]))
    # several terminals in one frame.  Keywords 0 = A, 1 = B, 2 = C A, 3 = C B, every bar -2.
    words, bars = [[A], [B], [C, A], [C, B]], [-2.0] * 4
    out.append(case(
        "terminals", words, bars, 5,
        [rows(5, {C: -0.25}, {A: -0.5, B: -0.5}),                  # four candidates: depth 2 first, then equal values: the smaller keyword
         rows(5, {C: -0.25}, {A: -0.5, B: -0.25}),                 # three and more: depth 2, then the larger value: keyword 3
         rows(5, {A: -0.5, B: -0.25}, {B: -0.25}),                 # two of one depth: the larger value, keyword 1; then B is held
         rows(5, {A: -0.25, B: -0.25})],                           # two of one depth and one value: the smaller keyword
        expect=[[(2, 0, 1, -0.75)], [(3, 0, 1, -0.5)], [(1, 0, 0, -0.25)], [(0, 0, 0, -0.25)]]))
    # the reset: keyword 0 = A fires at frame 0 and takes B's cell with it, so B C cannot complete at frame 1
    out.append(case("reset", [[A], [B, C]], [-1.0, -1.0], 5, [rows(5, {A: -0.25, B: -0.25}, {C: -0.25}), rows(5, {A: -3, B: -0.25}, {C: -0.25})],
                    expect=[[(0, 0, 0, -0.25)], [(1, 0, 1, -0.5)]]))
    # the hold: a one-token keyword over a three-frame run of its token fires once; a blank frame releases it; a frame with both log-probs
    # -inf does not (-inf >= -inf closes the arc)
    a, bl = {0: -2, A: -0.25}, {0: -0.25, A: -2}
    out.append(case("hold", [[A]], [-1.0], 5,
                    [rows(5, a, a, a), rows(5, a, a, bl, a), rows(5, a, {0: -INF, A: -INF}, a), rows(5, a, {0: -INF, A: -2}, a)],
                    expect=[[(0, 0, 0, -0.25)], [(0, 0, 0, -0.25), (0, 3, 3, -0.25)], [(0, 0, 0, -0.25)], [(0, 0, 0, -0.25)]],
                    states=[{(1, 0): (-INF, 1), (0, 0): (0, 3)}, {(1, 0): (-INF, 1)}, {(1, 0): (-INF, 1)}, {(1, 0): (-INF, 1)}]))
    # a longer keyword's event holds the root arc of its last token: B A fires at frame 1, A goes on through frame 2 and keyword 0 = A is silent
    out.append(case("hold_after_longer", [[A], [B, A]], [-1.0, -2.0], 5, [rows(5, {B: -0.25}, {A: -0.25, 0: -2}, {A: -0.25, 0: -2})],
                    expect=[[(1, 0, 1, -0.5)]], states=[{(1, 0): (-INF, 1)}]))
    # rc = -1: the last token of B A is no root child, nothing is held, and the keyword fires again at once
    ba = ({B: -0.25}, {A: -0.25, 0: -2})
    out.append(case("rc_minus", [[B, A]], [-2.0], 5, [rows(5, *ba, *ba)], expect=[[(0, 0, 1, -0.5), (0, 2, 3, -0.5)]], states=[{(1, 0): (-INF, -1)}]))
    # a repeated token must pass through b: A A over the frames A A - A.  Frame 1 cannot complete it (n[parent] is not allowed); the best
    # labelling starts at frame 1 (A - A, -0.75), not at frame 0 (A A - A, -1.0)
    out.append(case("repeat_through_b", [[A, A]], [-2.0], 5, [rows(5, {A: -0.25}, {A: -0.25}, {0: -0.25}, {A: -0.25})], expect=[[(0, 1, 3, -0.75)]]))
    return out


def random_trie(rng, S, V, max_depth=6):
    """a random trie of S states over the tokens 1 .. V - 1: distinct tokens under one parent, every leaf and about half of the inner
    states terminal, bar = -depth (a multiple of 0.25: n == bar happens)"""
    parent, tok, depth, used = [-1], [-1], [0], [set()]
    open_states = [0]
    while len(parent) < S:
        p = open_states[int(rng.integers(0, len(open_states)))] if rng.random() < 0.7 else open_states[-1]
        free = [t for t in (rng.permutation(V - 1)[:8] + 1) if int(t) not in used[p]]
        if not free or depth[p] >= max_depth:
            open_states.remove(p)
            if not open_states:
                raise ValueError("the trie is full")
            continue
        used[p].add(int(free[0]))
        parent.append(p); tok.append(int(free[0])); depth.append(depth[p] + 1); used.append(set())
        open_states.append(len(parent) - 1)
    parent, tok, depth = np.array(parent), np.array(tok), np.array(depth)
    inner = np.zeros(S, bool)
    inner[parent[1:]] = True
    kw = np.full(S, -1)
    term = [s for s in range(1, S) if not inner[s] or rng.random() < 0.5]
    kw[term] = np.arange(len(term))
    bar = np.where(kw >= 0, -1.0 * depth, 0.0)
    return dict(parent=parent, tok=tok, depth=depth, kw=kw, bar=bar)


def random_plane(rng, T, V, tok):
    """multiples of 0.25 in (-2, 0] with -inf cells; the columns the trie reads are what matters"""
    lp = (-0.25 * rng.integers(0, 8, size=(T, V))).astype(np.float32)
    lp[rng.random((T, V)) < 0.15] = -INF
    return lp


def random_case(seed, S, T, V):
    rng = np.random.default_rng(seed)
    trie = random_trie(rng, S, V)
    return dict(name=f"random S={S} T={T} V={V}", V=V, streams=[random_plane(rng, T, V, trie["tok"])], **tables(trie))


HOST_S, HOST_T = (1, 2, 65, 257, 1024), (1, 2, 17, 64)
GPU_S, GPU_T, GPU_V = (1, 2, 65, 257, 1024), (1, 2, 15, 16, 17, 33, 64), (5, 37, 3000)


def host_cases():
    return [random_case(1000 + 10 * i + j, S, T, (5, 37, 3000)[(i + j) % 3]) for i, S in enumerate(HOST_S) for j, T in enumerate(HOST_T)]
