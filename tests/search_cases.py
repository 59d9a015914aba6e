"""Adversarial inputs for the transducer greedy search (csrc/greedy.hip) and their float64 reference.  Importable without a GPU:
tests/test_search_ties_gpu.py runs the cases on the device, tests/test_search_screen_ref.py runs the self-checks below on the host.

THE MODEL (write_case_model, in the style of kat_model.write_wide_model): joiner.decoder_proj weight and bias are exactly zero, so
the decoder's contribution to the joiner input is +0 whatever the context, the batch's t0 quirk or the emissions so far, and frame
t's logits are  l[t] = tanh(enc[t]) W^T + b.  The expected result is therefore per frame: [(argmax_t, t) for t if argmax_t not in
{blank 0, unk 2}], argmax with the reference's later-index-wins rule.  reference() is numpy float64 on the same arrays.

NOISE BOUND per column v (noise_bound), for the f32 value any search form computes against the float64 one, c_v = sum_k |w_vk|:
  * the sum: exact f32 products of |a_k| <= 1 accumulated in f32 in some order, the k slices' sums added in a tree -- (J + 8) 2^-24 c_v
    (J - 1 + 7 additions, each within 2^-24 of a partial sum that c_v bounds, first order; the count rounded up);
  * tanhf: the libm figure tests/family_kernels.py uses (LIBM_TANH = 10 * 2^-24 relative, |tanh| <= 1) on every a_k -- 10 * 2^-24 c_v;
  * the bias add: one ulp of the result, 2^-23 (c_v + |b_v|).
A decision between two columns is safe when their float64 values are further apart than the SUM of their bounds; every frame that is
held to float64 keeps 10 x that sum (or is an exact tie between columns with identical data).

FRAME KINDS, fixed by the generator (Case.kind[b, t]), no frame left out:
  F64   the token must be the float64 one in EVERY form of the search;
  FORMS a sub-noise twin frame (true margin about one f32 ulp): float64 cannot say which twin wins, so the forms that share k_greedy's
        column arithmetic must agree with each other token for token, and every form must name one of the two twins.

PLANTED COLUMNS.  Every planted group has a weight row of magnitude ~0.25 per element and "its" frames: activations whose signs are
the row's signs, so that the group's logit is ~ +c_v (16 at J = 64, 130 at J = 512) while every other group sees a random-sign sum.
Background columns have small random weights.  check_case() asserts from the float64 logits that everything outside the frame's
group stays at least 0.5 AND the pair's screen bounds + 0.1 below it.
  * exact duplicates (equal weights and bias): DUP_PAIRS -- inside one 16-column screen tile, at columns 15 | 16, in tiles t and t + 8
    (the same wave of the screen), in tiles of different waves, on either side of every slab boundary of 2 and 4 parts
    (slab_boundaries: greedy_parts' cper formula), with the later twin at V - 1 (V = 1101: the padded tail follows), and with blank or
    unk as a twin: (0, k) emits k, (1, 2) emits nothing (V = 1200), (2, k) emits k (V = 1101).
  * candidate-list limits: groups of 8, 9 and 100 duplicates on 8 frames of one stream (screen_round's kScreenCand = 64 pairs).
  * f16-adversarial twins (a, b): w_a = h + 0.49 ulp16(h) s, w_b = h - 0.49 ulp16(h) s for an f16 row h (both round to h), the
    activation a_k = s_k (1 - 0.45 * 2^-11) rounds to s_k in f16.  The screen computes the same sum for both; in truth a is ahead by
    D = sum |a_k| 0.98 ulp16(h_k).  The biases take D - m back: a truly wins by m = 10 x the pair's noise bound, the screen sees b
    ahead by D - m -- 0.42 (J = 64), 0.38, 0.30 and 0.14 (J = 512) of eps_a + eps_b (REVERSAL_FLOOR).  Dropping a is what a too small eps does.
  * bias-decided twins (a, b), a < b: equal rows, a ahead by m through its bias alone -- a search that left the bias out of a
    comparison would see a tie and take b.
  * sub-noise twins: equal rows with the bias, the first or the last weight one f32 ulp apart, and a row against its own reversal in k
    under activations of one magnitude (equal exact sums, different rounding paths)."""
import dataclasses

import numpy as np

from k2transducerasr_amd.config import make_zipformer2_meta
from k2transducerasr_amd.k2w import write_k2w

U = 2.0 ** -24
LIBM_TANH = 10.0 * U          # == family_kernels.LIBM_TANH (test_search_screen_ref.py holds the two together)
F64, FORMS = 0, 1
JS = (64, 128, 256, 512)      # the four screen_round<NS> instantiations
VS = (1200, 1101)
GF = 8                        # frames per round (csrc/sweep.h)
K_SCREEN_CAND = 64            # csrc/greedy.hip kScreenCand
BLANK, UNK = 0, 2
# what the adversarial twins reach, (screen's lead of the wrong twin) / (eps_a + eps_b), per J: just under the achieved figures, so that
# the construction cannot weaken unnoticed (m grows with J (J + 18), the lead D - m shrinks)
REVERSAL_FLOOR = {64: 0.41, 128: 0.37, 256: 0.29, 512: 0.14}


def f16(x):
    return np.asarray(x, np.float32).astype(np.float16)


def ulp16(h):
    """the f16 spacing at the (normal) f16 value h"""
    h = np.abs(np.asarray(h, np.float64))
    return 2.0 ** (np.floor(np.log2(h)) - 10)


def slab_boundaries(V, parts):
    """first column of parts 1 .. parts - 1 (k_greedy: cper = ((ncg + G - 1) / G + 7) & ~7 column groups of 4)"""
    ncg = ((V + 3) // 4 * 4) >> 2
    cper = ((ncg + parts - 1) // parts + 7) & ~7
    return [4 * cper * p for p in range(1, parts) if 4 * cper * p < V]


def eps_emulated(W, b):
    """csrc/model.cpp's per-column screen bound (joiner.output_linear.weight#eps) from its formula; test_search_screen_ref.py holds
    it to the loader's own output"""
    W = np.asarray(W, np.float32)
    J = W.shape[1]
    cs = np.abs(W.astype(np.float64)).sum(1)
    bound = cs * (2.0 ** -10 + 2.0 ** -20 + 2.2 * (J + 8) * 2.0 ** -24) + (np.abs(np.asarray(b, np.float64)) + 1.0) * 2.0 ** -20 + J * 2.0 ** -24
    e = np.nextafter((bound * 1.01).astype(np.float32), np.float32(np.inf))
    bad = ~np.isfinite(W).all(1) | (np.abs(W) >= 65504.0).any(1) | ~np.isfinite(bound)
    e[bad] = np.inf
    return e


def noise_bound(W, b):
    c = np.abs(np.asarray(W, np.float64)).sum(1)
    J = W.shape[1]
    return c * (J + 8) * U + c * LIBM_TANH + 2.0 * U * (c + np.abs(np.asarray(b, np.float64)))


def logits64(W, b, enc):
    return np.tanh(np.asarray(enc, np.float64)) @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)


def reference(W, b, enc):
    """enc [B, T, J] -> (argmax [B, T] with later-index-wins, top-2 margin [B, T]) in float64"""
    l = logits64(W, b, enc)
    V = l.shape[-1]
    arg = V - 1 - np.argmax(l[..., ::-1], axis=-1)
    top2 = np.partition(l, V - 2, axis=-1)[..., V - 2:]
    return arg, top2[..., 1] - top2[..., 0]


def expected(arg):
    """per stream ([tokens], [timestamps]) as the search entries return them"""
    return [([int(y) for y in row if y not in (BLANK, UNK)], [t for t, y in enumerate(row) if y not in (BLANK, UNK)]) for row in arg]


def per_frame(result, T):
    """([tokens], [timestamps]) -> the frame's token, -1 where nothing was emitted"""
    out = np.full(T, -1, np.int64)
    toks, ts = result
    assert len(toks) == len(ts) and len(set(ts)) == len(ts), result
    for y, t in zip(toks, ts):
        out[t] = y
    return out


@dataclasses.dataclass
class Case:
    name: str
    enc: np.ndarray        # [B, T, J] f32
    kind: np.ndarray       # [B, T] F64 / FORMS
    group: list            # [B][T] the planted columns that may win the frame
    counts: tuple = None   # (decided, fallen back) rounds of the screen under one part per stream, where the case pins them


@dataclasses.dataclass
class Model:
    J: int
    V: int
    W: np.ndarray
    b: np.ndarray
    dup_pairs: list
    dup8: list
    dup9: list
    dup100: list
    adv: list              # (a, b): a wins in truth, the screen's sums say b
    biased: list           # (a, b), a < b: equal weights, a ahead by its bias alone
    sub: list              # (a, b) sub-noise twins
    rows: dict             # column -> (signs s [J], magnitudes [J]) of the activation that makes it win
    cases: list

    def write(self, path):
        write_case_model(path, self.W, self.b)


def write_case_model(path, W, b, decoder_dim=8, seed=5):
    rng = np.random.default_rng(seed)
    V, J = W.shape
    meta = make_zipformer2_meta(encoder_dims=[16], num_encoder_layers=[1], feedforward_dims=[16], num_heads=[1], cnn_module_kernels=[3],
                                downsampling_factors=[1], joiner_dim=J, decoder_dim=decoder_dim, vocab_size=V, comment="search-cases")
    tensors = [
        ("decoder.embedding.weight", rng.standard_normal((V, decoder_dim)).astype(np.float32)),
        ("decoder.conv.weight", (rng.standard_normal((decoder_dim, 4, 2)) * 0.5).astype(np.float32)),
        ("joiner.decoder_proj.weight", np.zeros((J, decoder_dim), np.float32)),
        ("joiner.decoder_proj.bias", np.zeros(J, np.float32)),
        ("joiner.output_linear.weight", np.ascontiguousarray(W, np.float32)),
        ("joiner.output_linear.bias", np.ascontiguousarray(b, np.float32)),
    ]
    write_k2w(path, meta, tensors)
    return meta


def dup_pairs(V):
    # unk is column 2 and can be one twin only: the later one at V = 1200 (first-wins would emit 1), the earlier one at V = 1101
    pairs = [(35, 41), (15, 16), (16 * 5 + 3, 16 * 13 + 3), (16 * 6 + 7, 16 * 9 + 2), (V - 40, V - 1), (0, 500),
             (1, 2) if V == 1200 else (2, 700)]
    for parts in (2, 4):
        for c in slab_boundaries(V, parts):
            if (c - 1, c) not in pairs:
                pairs.append((c - 1, c))
    return pairs


A_HI = np.float32(1.0 - 0.45 * 2.0 ** -11)    # rounds to 1.0 in f16 (0.05 f16 ulp inside the midpoint 1 - 2^-12: tanhf's error is 1e-3 of that)


def f16_row(rng, J):
    """an f16-representable row near the bottom of the binade [0.25, 0.5): ulp16 / |h| is close to its largest, 2^-10"""
    return ((0.25 + rng.integers(1, 48, J) * 2.0 ** -12) * rng.choice([-1.0, 1.0], J)).astype(np.float32)


def build(J, V, seed=None):
    rng = np.random.default_rng(1000 * J + V if seed is None else seed)
    W = (rng.standard_normal((V, J)) * 0.02).astype(np.float32)
    b = np.full(V, -1.0, np.float32)
    used, rows = set(), {}

    def take(cols):
        assert not (set(cols) & used), cols
        used.update(cols)

    def free(n, lo=40):
        out = []
        c = lo
        while len(out) < n:
            if c not in used and c not in (BLANK, 1, UNK):
                out.append(c)
            c += 1
        take(out)
        return out

    def plant(cols, h, mag=None):
        mag = np.full(J, 0.9, np.float32) if mag is None else mag
        for c in cols:
            W[c] = h
            b[c] = 0.0
            rows[c] = (np.sign(h).astype(np.float32), mag)

    pairs = dup_pairs(V)
    take({c for p in pairs for c in p})
    for p in pairs:
        plant(p, (rng.uniform(0.2, 0.3, J) * rng.choice([-1.0, 1.0], J)).astype(np.float32),
              rng.uniform(0.5, 0.99, J).astype(np.float32))
    dup8 = [50, 51, 300, 301, 650, 651, 900, 1000]      # several tiles, waves and slabs
    take(dup8)
    dup9 = free(4, 120) + free(5, 800)
    dup100 = free(100, 700)
    for g in (dup8, dup9):
        plant(g, (rng.uniform(0.2, 0.3, J) * rng.choice([-1.0, 1.0], J)).astype(np.float32))
    # (the 100: a row twice as heavy, and below -- once every group's frame is known -- a bias that keeps them under the background
    # on every frame but their own, where they still win by far: idle, they would tie 100-fold on top of any slab that holds none of
    # the frame's group and overflow its candidate list)
    plant(dup100, (rng.uniform(0.45, 0.55, J) * rng.choice([-1.0, 1.0], J)).astype(np.float32))
    # f16-adversarial twins: (a before b in one tile), (a behind b, other tile and slab)
    adv = [tuple(free(2, 420)), tuple(reversed(free(1, 260) + free(1, 930)))]
    for a_, b_ in adv:
        h = f16_row(rng, J)
        s = np.sign(h)
        d = (0.49 * ulp16(h) * s).astype(np.float64)
        W[a_] = (h + d).astype(np.float32)
        W[b_] = (h - d).astype(np.float32)
        assert (f16(W[a_]) == f16(h)).all() and (f16(W[b_]) == f16(h)).all()
        mag = np.full(J, A_HI, np.float32)
        rows[a_] = rows[b_] = (s.astype(np.float32), mag)
        enc = np.arctanh((s * mag).astype(np.float64)).astype(np.float32)
        act = np.tanh(enc.astype(np.float64))
        D = float(act @ (W[a_].astype(np.float64) - W[b_].astype(np.float64)))
        b[a_] = b[b_] = 0.0
        m = 10.0 * float(noise_bound(W[[a_, b_]], np.ones(2)).sum())     # (|b| <= 1 stands in for the bias that m itself decides)
        b[b_] = np.nextafter(np.nextafter(np.float32(D - m), np.float32(-1)), np.float32(-1))   # rounded DOWN: the margin is >= m
        assert D - m > 0 and D - float(b[b_]) >= m, (J, D, m)
    # bias-decided twins: equal rows, the EARLIER column ahead by m through its bias alone (without the bias add: a tie, the later index)
    biased = [tuple(free(2, 480))]
    for a_, b_ in biased:
        h = (rng.uniform(0.2, 0.3, J) * rng.choice([-1.0, 1.0], J)).astype(np.float32)
        plant((a_, b_), h)
        m = 10.0 * float(noise_bound(W[[a_, b_]], np.ones(2)).sum())
        b[a_] = np.nextafter(np.nextafter(np.float32(m), np.float32(1)), np.float32(1))          # rounded UP
        assert float(b[a_]) >= m
    # sub-noise twins
    sub = []
    for kind in ("bias", "w_first", "w_last", "reversed"):
        a_, b_ = free(2, 540 if kind != "reversed" else 200)
        if kind == "reversed":
            b_ = free(1, 1040)[0]
        h = (rng.uniform(0.2, 0.3, J) * rng.choice([-1.0, 1.0], J)).astype(np.float32)
        mag = rng.uniform(0.5, 0.99, J).astype(np.float32)
        W[a_] = W[b_] = h
        b[a_] = b[b_] = 0.1
        if kind == "bias":
            b[b_] = np.nextafter(np.float32(0.1), np.float32(1))
        elif kind == "w_first":
            W[a_, 0] = np.nextafter(h[0], np.float32(np.sign(h[0])))
        elif kind == "w_last":
            W[b_, J - 1] = np.nextafter(h[J - 1], np.float32(np.sign(h[J - 1])))
        else:
            h = np.abs(h)
            W[a_], W[b_] = h, h[::-1].copy()
            mag = np.full(J, 0.8125, np.float32)
        rows[a_] = rows[b_] = (np.sign(W[a_]).astype(np.float32), mag)
        sub.append((a_, b_))

    def frame(col):
        s, mag = rows[col]
        return np.arctanh((s * mag).astype(np.float64)).astype(np.float32)

    idle = max(float(np.tanh(frame(c).astype(np.float64)) @ W[dup100[0]].astype(np.float64)) for c in rows if c not in dup100)
    b[dup100] = np.float32(-np.ceil(idle + 3.0))

    def case(name, plan, counts=None):
        """plan [B][T] of (kind, group)"""
        B, T = len(plan), len(plan[0])
        enc = np.zeros((B, T, J), np.float32)
        kind = np.zeros((B, T), np.int64)
        for bi, row in enumerate(plan):
            assert len(row) == T
            for t, (k, g) in enumerate(row):
                enc[bi, t] = frame(g[0])
                kind[bi, t] = k
        return Case(name, enc, kind, [[tuple(g) for _, g in row] for row in plan], counts)

    # T' = 19: two full rounds of GF = 8 frames and a partial one (every emission restarts the round one frame on)
    T = 19
    seq = [(F64, p) for p in pairs]
    dup_plan = [[seq[(bi * 5 + t) % len(seq)] for t in range(T)] for bi in range(3)]
    advsub = [(F64, p) for p in adv + biased] + [(FORMS, p) for p in sub]
    mixed = [(F64, p) for p in pairs[:4] + adv + biased] + [(FORMS, p) for p in sub]
    cases = [
        case("duplicate_pairs", dup_plan),
        case("adversarial_and_sub_noise", [[advsub[(bi * 3 + t) % len(advsub)] for t in range(T)] for bi in range(4)]),
        case("mixed", [[mixed[(7 * bi + 3 * t) % len(mixed)] for t in range(T)] for bi in range(2)]),
        # one stream, 8 frames, every frame emits: the rounds cover 8, 7, .. 1 frames.  8 duplicates: 64 pairs in the first round, the
        # list exactly full, every round decided; 9: 72 in the first round (falls back), 63 and fewer afterwards; 100: every round
        case("dup8", [[(F64, dup8)] * GF], counts=(GF, 0)),
        case("dup9", [[(F64, dup9)] * GF], counts=(GF - 1, 1)),
        case("dup100", [[(F64, dup100)] * GF], counts=(0, GF)),
    ]
    return Model(J, V, W, b, pairs, dup8, dup9, dup100, adv, biased, sub, rows, cases)


def screen_emulated(W, b, enc_row):
    """what the f16 screen's sum is for one frame: exact products of the f16-rounded activations (tanh in f32) and weights + bias"""
    a = np.tanh(np.asarray(enc_row, np.float64)).astype(np.float32)
    return f16(a).astype(np.float64) @ f16(W).astype(np.float64).T + np.asarray(b, np.float64)


def check_case(m, c):
    """the generator's promises, from float64: raises AssertionError.  Returns (argmax, margin)."""
    arg, margin = reference(m.W, m.b, c.enc)
    l = logits64(m.W, m.b, c.enc)
    nb = noise_bound(m.W, m.b)
    eps = eps_emulated(m.W, m.b).astype(np.float64)
    B, T, _ = c.enc.shape
    assert B <= 4 and T <= 19
    for bi in range(B):
        for t in range(T):
            g = list(c.group[bi][t])
            row = l[bi, t]
            rest = np.delete(row, g)
            top = row[g].max()
            # nothing outside the group comes near: 0.5, and further than the screen's bounds could bridge
            assert top - rest.max() >= 0.5, (c.name, bi, t, top - rest.max())
            assert top - rest.max() >= eps[g].max() + np.delete(eps, g).max() + 0.1, (c.name, bi, t)
            assert arg[bi, t] in g
            if c.kind[bi, t] == FORMS:
                assert len(g) == 2 and abs(row[g[0]] - row[g[1]]) < nb[g].sum(), (c.name, bi, t)
            elif (m.W[g] == m.W[g[0]]).all() and (m.b[g] == m.b[g[0]]).all():
                assert arg[bi, t] == max(g) and (row[g] == row[g[0]]).all(), (c.name, bi, t)      # exact duplicates: the last index
            elif tuple(g) in m.biased:
                a_, b_ = g
                assert arg[bi, t] == a_ < b_ and (m.W[a_] == m.W[b_]).all()
                assert margin[bi, t] >= 10.0 * (nb[a_] + nb[b_]) and row[a_] - row[b_] <= 0.5 * (eps[a_] + eps[b_])
            else:
                a_, b_ = g
                assert (a_, b_) in m.adv and arg[bi, t] == a_
                assert row[a_] - row[b_] >= 10.0 * (nb[a_] + nb[b_]), (c.name, bi, t, row[a_] - row[b_], nb[a_] + nb[b_])
                assert margin[bi, t] >= 10.0 * (nb[a_] + nb[b_])
                s = screen_emulated(m.W[[a_, b_]], m.b[[a_, b_]], c.enc[bi, t])
                assert s[1] > s[0], (c.name, bi, t, s)                                          # the screen's order is reversed
                assert s[1] - s[0] <= eps[a_] + eps[b_]                                         # ... within the bounds: a stays a candidate
            # however the vocabulary is split (1, 2, 4 parts by switch, 5 by default at these sizes): no slab's candidate list can
            # overflow on this frame -- at most 8 columns within twice the bounds of the slab's top, so 64 over a round's 8 frames
            if len(g) <= 8:
                for parts in (1, 2, 4, 5):
                    edges = [0] + slab_boundaries(m.V, parts) + [m.V]
                    for lo, hi in zip(edges[:-1], edges[1:]):
                        n = int((row[lo:hi] + 2 * eps[lo:hi] >= (row[lo:hi] - 2 * eps[lo:hi]).max()).sum())
                        assert n <= 8, (c.name, bi, t, parts, lo, hi, n)
    return arg, margin


def screen_reversal_ratio(m):
    """(b ahead of a in the emulated screen) / (eps_a + eps_b) for the model's adversarial twins"""
    eps = eps_emulated(m.W, m.b).astype(np.float64)
    out = []
    for a_, b_ in m.adv:
        s_, mag = m.rows[a_]
        s = screen_emulated(m.W[[a_, b_]], m.b[[a_, b_]], np.arctanh((s_ * mag).astype(np.float64)).astype(np.float32))
        out.append(float((s[1] - s[0]) / (eps[a_] + eps[b_])))
    return out
