"""Inputs built to tie for the modified beam search (csrc/beam.hip), their float64 reference and the promises that make the comparison
exact.  Importable without a GPU: tests/test_beam_ties_gpu.py runs the cases on the device, tests/test_beam_cases_ref.py runs the
self-checks, the C oracle and the sensitivity variants on the host.

THE MODEL (search_cases.write_case_model): joiner.decoder_proj weight and bias are exactly zero, so frame t's logits are the same row
for every hypothesis, whatever its context.  The joiner is SPARSE: a planted column has ONE non-zero weight, W_LEVER, on "its" lever (a
joiner dimension); a lever drives one column or a group of 2 or 3 duplicate columns.  Every column -- planted or not -- has the bias
FLOOR = -W_LEVER; every other column has no weight at all.  A column's logit is  w * tanh(enc[d]) + b  in any summation order (the
other J - 1 products are exact zeros), so the MFMA sweep, the slab exchange and the GEMM each give a column and its duplicates the same
bits.  A lever left at enc = 0 has tanh = 0 and its columns sit at exactly FLOOR: the floor -- unplanted columns and idle levers alike --
is a several-hundred-fold exact tie that only the flat index orders.  A driven lever lifts its columns to a level in [-6.5, -0.5]:
5.5 and more above the floor, and below zero, so a padded column (logit 0) would win every frame if the search counted it.
What the cases probe is selection, ranking, merging and the final pick; column arithmetic belongs to test_search_ties_gpu.py and the
GEMM tests.

PLANTED GROUPS (groups(V), each on a lever of its own): (0, 70), blank with a token -- two sequences; unk on its own lever, driven to
blank's level in half of blank's frames (equal weight, bias and input: equal bits) -- blank with unk, two candidates of ONE hypothesis
that spell the same sequence, an exact logaddexp(x, x); the triple (5, 133, 197), one lane at three 64-strides;
neighbouring lanes (20, 21); 63 | 64; 255 | 256 (chunk and slab boundary) and 511 | 512 where V has them; the later twin at V - 1; one
lane at a low and the highest stride of the NE = 16 / excl paths (V >= 600); and single columns.

FRAMES.  Case "repeat": frames 0 and 1 of every stream are the SAME row.  Their two orders of the same two terms tie by commutativity
(0 + a + b == 0 + b + a in any float format), which no later pair of equal frames would (lp + a + b is not lp + b + a): exactly tied
hypotheses in different slots, merges of two exactly tied paths (the first-inserted one keeps its timestamp), at beam 8 the three-way
merge [k] + blank, [k] + unk, [] + k, and -- carried to the end -- exactly tied normalised scores in the final order.  Case "floor":
frame 0 drives no lever, one lever or one triple, so the floor's lowest flat indexes fill the beam.  Case "distinct": frames 0 and 1
drive eight single columns to eight levels.  Every later frame drives 1 to 8
levers at random levels (one designated group on top, so that every group decides a frame at beam 1 too), sometimes two groups at
ONE level.  Ties that straddle the beam cut, and beams only partly filled by strong candidates, follow from these and are COUNTED,
not assumed (coverage()).

REFERENCE.  twin() restates the search (per hypothesis the top candidates, then the rank over their union by score descending and flat
index ascending, expansion, merges by logaddexp in insertion order, the final order by log-prob / (length + 2) with ties in insertion
order) in numpy at a chosen dtype; float64 is the reference.  One logit per distinct (weight row, bias) is computed and shared, the
association is the kernel's ((l - mx) - lse) + lp, logaddexp is mx + log1p(exp(-|a - b|)).

NOISE BOUND (noise_terms / score_bound), for the float32 score and token log-prob of any form against float64, U = 2^-24:
  * a logit: tanhf within LIBM_TANH = 10 U (search_cases) of a value <= 1, times |w|; the product's rounding U |w|; the bias add's,
    U (|w| + |b|):                                      E_l = (LIBM_TANH + U) |w| + U (|w| + |b|)        (0 for a column without weight)
  * the token log-prob u = (l - mx) - lse.  mx is one of the computed logits, exactly, and cancels between the two terms, so the
    logits' errors enter as l_v's own and -- through lse, a weighted mean -- at most the largest one: 2 E_l.  Roundings: fl(l - mx),
    U R with R >= |l - mx| the model's logit range; in lse the same U R on every exponent, expf within LIBM_EXP = 4 U relative
    (2 ulp; OCML and glibc document 1), the sum of V positive terms -- a chain of ceil(V / 64) per lane and a 6-level tree on the
    device, (ceil(V / 64) + 6) U relative; ONE chain of V in the C oracle, V U -- and logf within LIBM_LOG = 4 U of |lse| <= log V;
    the last subtraction U (R + log V):
        E_u = 2 E_l + 2 U R + LIBM_EXP + E_sum + LIBM_LOG log V + U (R + log V)
  * the score after T' frames: every path adds one u per frame, each addition rounded at the score's magnitude, at most S =
    the largest |score| among the candidates the run ever ranked (taken from the float64 run): T' (E_u + U S);
  * a merge passes its inputs' errors on with weights that sum to 1 and adds fl(a - b) (U S), expf (LIBM_EXP; e^-x <= 1 and
    |d log1p(e^-x) / dx| <= 1), log1pf (LIBM_LOG log 2) and its final addition (U S): E_m = 2 U S + LIBM_EXP + LIBM_LOG log 2, times
    M = the number of merges the run made (no path can have been through more).
        score_bound = T' (E_u + U S) + M E_m          token log-prob bound = E_u

PROMISES (check_case raises otherwise), per case, stream and beam: every consecutive pair among the top beam + 1 candidates of every
frame, and every adjacent pair of normalised scores in the final order, is EXACTLY tied in the float64 run and in the float32 run of
the same twin -- and in three more runs whose tanh values are moved by a few U, as another tanhf would: a tie that rests on equal data
survives all five, two different sums that merely rounded alike do not; and the twin carries with every score HOW it was formed
(_sym_add: 0 + a, the commutative a + b, every longer sum and every merge in its order), and a tie counts only between equal
formations -- or is 10 x the bound apart in float64 (the normalised scores: 10 x the two entries' own bound / (length + 2) + U
|score|); all runs select the same candidates in the same order, make the same merges and return identical tokens, timestamps
and order.  No third kind, no excuse list.  SEEDS are the first draws per V that keep the promises AND cover every kind and every
duplicate position at every beam that admits it (required())."""
import dataclasses
import math

import numpy as np

from search_cases import LIBM_TANH, U, write_case_model

BLANK, UNK = 0, 2
J = 64
VS = (200, 400, 600, 1021, 1029)
BEAMS = (1, 2, 4, 5, 8)
W_LEVER, FLOOR = 12.0, -12.0
LEVELS = (-6.5, -0.5)
T_FRAMES = 12
LIBM_EXP = LIBM_LOG = 4.0 * U
MARGIN = 10.0
RULES = ("high_index_first", "lane_last_max", "merge_keeps_later", "merge_into_dead", "pad_in_lse", "final_last", "cut_keeps_high")
# the first seed per V whose cases keep every promise and cover every kind (find_seed; test_beam_cases_ref.py re-checks them)
SEEDS = {200: 0, 400: 7, 600: 0, 1021: 0, 1029: 0}


def groups(V):
    """name -> columns of every planted group, in lever order"""
    g = {"blank|tok": (BLANK, 70), "unk": (UNK,), "lane-strides": (5, 5 + 64 * 2, 5 + 64 * 3), "neighbours": (20, 21), "63|64": (63, 64)}
    if V > 257:
        g["255|256"] = (255, 256)
    if V > 513:
        g["511|512"] = (511, 512)
    g["last"] = (V - 50, V - 1)
    if V >= 600:
        hi = 40 + 64 * ((V - 2 - 40) // 64)
        g["high-stride"] = (40 + 64 * (2 if V == 600 else 7), hi)
    for c in (9, 30, 44, 100, 120, 140, 160, 180) + ((300, 390) if V >= 400 else ()):
        g[f"single{c}"] = (c,)
    cols = [c for v in g.values() for c in v]
    assert len(set(cols)) == len(cols) and max(cols) < V and len(g) <= J, (V, g)
    return g


DUP_POSITIONS = ("blank|unk", "blank|tok", "lane-strides", "neighbours", "63|64", "255|256", "511|512", "last", "high-stride")


@dataclasses.dataclass
class Case:
    name: str
    enc: np.ndarray        # [B, T', J] f32


@dataclasses.dataclass
class Model:
    V: int
    W: np.ndarray          # [V, J] f32
    b: np.ndarray          # [V] f32
    groups: dict
    cases: list

    def write(self, path):
        write_case_model(path, self.W, self.b)


def enc_of(level):
    """the lever input that lifts a column to `level`"""
    return np.float32(np.arctanh((level - FLOOR) / W_LEVER))


def build(V, seed=None):
    rng = np.random.default_rng(7919 * V + (SEEDS[V] if seed is None else seed))
    g = groups(V)
    names = list(g)
    W = np.zeros((V, J), np.float32)
    b = np.full(V, FLOOR, np.float32)
    for d, n in enumerate(names):
        for c in g[n]:
            W[c, d] = W_LEVER
    dups = [n for n in names if len(g[n]) > 1]
    singles = [n for n in names if len(g[n]) == 1]     # (singles[0] is unk)

    def row(levels):
        e = np.zeros(J, np.float32)
        for n, lv in levels.items():
            e[names.index(n)] = enc_of(lv)
        return e

    def spaced(k, lo=LEVELS[0], hi=LEVELS[1], gap=0.12):
        while True:
            x = np.sort(rng.uniform(lo, hi, k))[::-1]
            if k < 2 or np.diff(x).max() <= -gap:
                return [float(v) for v in x]

    turn = [0]

    def random_frame(last=False):
        """1 .. 8 driven levers; the group whose turn it is on top (in a stream's last frame a pair of real tokens: its two
        extensions of the best hypothesis tie in score and length, the final order's tie); one frame in four puts two groups at ONE
        level"""
        top = dups[turn[0] % len(dups)]
        turn[0] += 1
        if last and top == "blank|tok":
            top = dups[turn[0] % len(dups)]
            turn[0] += 1
        k = int(rng.choice([1, 2, 3, 6, 7, 8], p=[0.1, 0.1, 0.1, 0.3, 0.2, 0.2]))
        others = [n for n in names if n != top]
        chosen = [top] + [others[i] for i in rng.permutation(len(others))[: k - 1]]
        lv = dict(zip(chosen, spaced(k)))
        if k >= 3 and rng.random() < 0.25:
            lv[chosen[2]] = lv[chosen[1]]            # two groups, one level: the tie crosses groups
        if "blank|tok" in lv and rng.random() < 0.5:
            lv["unk"] = lv["blank|tok"]              # blank with unk: one hypothesis, one sequence, twice
        return row(lv)

    def stream(prologue):
        return np.stack(prologue + [random_frame(i == T_FRAMES - 1) for i in range(len(prologue), T_FRAMES)])

    x = spaced(5, -4.5, -0.5, 0.4)
    rep = [
        # blank and 70 at one level, unk below it, over two singles: [] (blank and unk), [70], [s]; the second copy of the frame merges
        # [] + 70, [70] + blank and [70] + unk -- three ways at beam 8 -- and ties [70, s] with [s, 70].  (unk AT blank's level would
        # make [] and [70] equal in exact arithmetic, 2 x + 2 log 2 both, through different sums: a tie no format guarantees)
        row({"blank|tok": x[0], "unk": x[1], singles[1]: x[2], singles[2]: x[3]}),
        # two singles and a pair, blank on the floor: [a, b] and [b, a] tie in score AND length -- the final order's tie
        row({singles[3]: x[0], singles[4]: x[1], "neighbours": x[2]}),
        # blank and 70 WITHOUT unk over a pair: [] and [70] tie; the second copy ties [] + blank, [] + 70, [70] + blank, [70] + 70 and
        # merges the exactly tied [] + 70 (first: timestamp 1) and [70] + blank (timestamp 0) from beam 4 on.  Ten driven columns: at
        # beam 8 no floor column -- unk among them, which would add e^-11 to [] and undo the tie -- enters the first frame's beam
        row({"blank|tok": x[0], "63|64": x[1], singles[5]: x[2], "last": x[3], "lane-strides": x[4]}),
    ]
    flo = [row({}), row({singles[6]: x[1]}), row({"lane-strides": x[0]})]
    # eight singles at eight levels, twice over: at least `beam` strong candidates, no two alike, before any tie exists
    tokens = [n for n in singles if n != "unk"][:8]
    dis = [row(dict(zip(tokens, spaced(8, gap=0.3)))), row(dict(zip(tokens[::-1], spaced(8, gap=0.3))))]
    cases = [Case("repeat", np.stack([stream([r, r]) for r in rep])), Case("floor", np.stack([stream([r]) for r in flo])),
             Case("distinct", np.stack([stream(dis)]))]
    return Model(V, W, b, g, cases)


# ---- the search, restated ----------------------------------------------------------------------------------------------------------
def unique_logits(W, b, enc, dtype, jitter=0):
    """[T', V] logits at `dtype`: ONE value per distinct (weight row, bias), shared by the columns that have it.  A row has at most one
    non-zero weight, so the value is that product plus the bias -- no sum, no BLAS."""
    key = np.concatenate([np.asarray(W, np.float64), np.asarray(b, np.float64)[:, None]], 1)
    uq, inv = np.unique(key, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    assert ((uq[:, :-1] != 0).sum(1) <= 1).all(), "a planted column has ONE non-zero weight"
    d = np.abs(uq[:, :-1]).argmax(1)
    a = (np.tanh(np.asarray(enc, np.float64)) * (1.0 + jitter * 3.0 * U)).astype(dtype)    # jitter: another tanhf, within LIBM_TANH
    w = uq[np.arange(len(uq)), d].astype(dtype)
    l = a[:, d] * w[None, :] + uq[:, -1].astype(dtype)[None, :]
    return l[:, inv]


def _lane_last(ids, need):
    """the order a wave takes tied tokens in when every lane (token % 64) reports its LAST maximum: per round the lowest of the lanes'
    highest remaining tokens"""
    left, out = sorted(int(i) for i in ids), []
    while left and len(out) < need:
        last = {}
        for v in left:
            last[v % 64] = v
        pick = min(last.values())
        out.append(pick)
        left.remove(pick)
    return out + left


def tie_sorted(score, ids, need, rule, V=None):
    """ids ordered by (score descending, id ascending); under a wrong `rule` the tied blocks that reach into the first `need` places
    are re-ordered the wrong way"""
    order = np.lexsort((ids, -score))
    ids, score = ids[order], score[order]
    if rule not in ("high_index_first", "lane_last_max"):
        return ids, score
    ids = ids.copy()
    i = 0
    while i < min(need, len(ids)):
        j = i + 1
        while j < len(ids) and score[j] == score[i]:
            j += 1
        if j - i > 1:
            blk = ids[i:j]
            ids[i:j] = blk[::-1] if rule == "high_index_first" else _lane_last(blk, need - i)
        i = j
    return ids, score


def _sym_add(sym, term):
    """how a score was formed, as far as float arithmetic lets two formations agree for certain: 0 + a is a, a + b is b + a, every
    longer sum keeps its order"""
    if sym == ():
        return ("u", term)
    if sym[0] == "u":
        return ("sum2",) + tuple(sorted([sym[1], term]))
    return ("add", sym, term)


def logaddexp(a, b, dtype):
    a, b = dtype(a), dtype(b)
    return dtype(max(a, b) + np.log1p(np.exp(-abs(a - b))))


def twin(W, b, enc, beam, dtype=np.float64, rule=None, jitter=0):
    """One stream, enc [T', J].  Returns dict(alts = every survivor in final order as dict(tokens, timestamps, token_log_probs, score,
    norm), frames = per frame dict(idx, val: the top beam + 1 candidates (flat index = slot * V + token) in rank order, merges:
    [(rank, rank of the latest equal entry before it)], n: survivors, onfloor: which of idx sit on the floor), selected = every token ever selected,
    smax = the largest |score| ranked or produced by a merge, merges = how many merges were made).  rule: None, or one of RULES -- a
    deliberately WRONG search, for the sensitivity test.  jitter: every tanh value moved by jitter * 3 U relative, the same for equal
    inputs -- what another tanhf within LIBM_TANH would do; ties that rest on equal data survive it, ties that rest on how two
    different sums happened to round do not."""
    assert rule is None or rule in RULES, rule
    dtype = np.dtype(dtype).type
    W, b = np.asarray(W), np.asarray(b)
    V = W.shape[0]
    logits = unique_logits(W, b, enc, dtype, jitter)
    idle = ~(W != 0).any(1)
    hyps = [dict(ys=[], ts=[], yp=[], lp=dtype(0), sym=())]
    rows = {}
    frames, selected, smax, nmerge = [], set(), 0.0, 0
    tie_rule = rule if rule in ("high_index_first", "lane_last_max") else None
    for t in range(enc.shape[0]):
        l = logits[t]
        rowid = rows.setdefault(np.asarray(enc[t], np.float32).tobytes(), len(rows))
        on_floor = idle | (l == dtype(FLOOR))
        # (pad_in_lse: the columns from V to the lanes' next multiple of 64 -- the padded ones among them -- as the zeros they hold)
        pool = np.concatenate([l, np.zeros(-V % 64, dtype)]) if rule == "pad_in_lse" else l
        mx = pool.max()
        lse = np.log(np.exp(pool - mx).sum(dtype=dtype))
        u = (l - mx) - lse
        nA = len(hyps)
        want = min(beam, nA * V)
        # per hypothesis its own top candidates (one more than the beam needs: the runner-up behind the cut), then the rank over the union
        flat, val = [], []
        tok_ids = np.arange(V)
        for k, h in enumerate(hyps):
            sc = u + h["lp"]
            ids, s = tie_sorted(sc, tok_ids, want + 1, tie_rule)
            flat.append(k * V + ids[: want + 1])
            val.append(s[: want + 1])
        flat, val = np.concatenate(flat), np.concatenate(val)
        flat, val = tie_sorted(val, flat, want + 1, "high_index_first" if rule == "high_index_first" else None)
        flat, val = flat[: want + 1].copy(), val[: want + 1].copy()
        if rule == "cut_keeps_high" and len(val) > want and val[want - 1] == val[want]:
            i0 = want - 1
            while i0 > 0 and val[i0 - 1] == val[want]:
                i0 -= 1
            # the whole tied block, the floor's tail included: its HIGHEST flat indexes take the places inside the beam
            blk = np.concatenate([(k * V + np.flatnonzero(u + h["lp"] == val[want])) for k, h in enumerate(hyps)])
            flat[i0:want] = np.sort(blk)[-(want - i0):]
        smax = max(smax, float(np.abs(val).max()))
        new, where, merges, dead = [], {}, [], set()
        syms = [_sym_add(hyps[int(i) // V]["sym"], (rowid, float(l[int(i) % V]))) for i in flat]
        for r in range(want):
            k, tok = int(flat[r]) // V, int(flat[r]) % V
            selected.add(tok)
            h = hyps[k]
            real = tok not in (BLANK, UNK)
            ys = h["ys"] + [tok] if real else h["ys"]
            key = tuple(ys)
            if key in where:
                q, last = where[key]
                merges.append((r, last))
                nmerge += 1
                if rule == "merge_into_dead" and last in dead:
                    pass                             # added to an entry that was merged away itself: the mass goes nowhere
                else:
                    new[q]["lp"] = logaddexp(new[q]["lp"], val[r], dtype)
                    new[q]["sym"] = ("lae", new[q]["sym"], syms[r]) if new[q]["sym"][0] == "lae" else ("lae",) + tuple(sorted([new[q]["sym"], syms[r]], key=repr))
                    smax = max(smax, abs(float(new[q]["lp"])))
                if rule == "merge_keeps_later":
                    new[q]["ts"] = h["ts"] + [t] if real else h["ts"]
                    new[q]["yp"] = h["yp"] + [u[tok]] if real else h["yp"]
                dead.add(r)
                where[key] = (q, r)
            else:
                where[key] = (len(new), r)
                new.append(dict(ys=ys, ts=h["ts"] + [t] if real else h["ts"], yp=h["yp"] + [u[tok]] if real else h["yp"], lp=val[r], sym=syms[r]))
        frames.append(dict(idx=flat, val=val, merges=merges, n=len(new), want=want, onfloor=on_floor[flat % V], nA=nA, sym=syms))
        hyps = new
    norm = [h["lp"] / dtype(len(h["ys"]) + 2) for h in hyps]
    order = sorted(range(len(hyps)), key=lambda i: (-norm[i], -i if rule == "final_last" else i))
    alts = [dict(tokens=hyps[i]["ys"], timestamps=hyps[i]["ts"], token_log_probs=np.array(hyps[i]["yp"], np.float64), score=float(hyps[i]["lp"]),
                 norm=norm[i], sym=(hyps[i]["sym"], len(hyps[i]["ys"]))) for i in order]
    return dict(alts=alts, order=order, frames=frames, selected=selected, smax=smax, merges=nmerge)


# ---- the bound -----------------------------------------------------------------------------------------------------------------------
def noise_terms(W, b, chain=None):
    """(E_u, R): the bound of one token log-prob and the logit range it was derived with; chain = the longest run of sequential
    additions in the form's sum of exponentials (default: the device's lanes and tree; V for the C oracle's single loop)"""
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
    V = W.shape[0]
    w = np.abs(W).max(1)
    e_l = float(np.where(w > 0, (LIBM_TANH + U) * w + U * (w + np.abs(b)), 0.0).max())
    R = float((b + w).max() - (b - w).min())
    e_sum = (math.ceil(V / 64) + 6 if chain is None else chain) * U
    logv = math.log(V)
    return 2 * e_l + 2 * U * R + LIBM_EXP + e_sum + LIBM_LOG * logv + U * (R + logv), R


def score_bound(W, b, ref, T, chain=None):
    """ref: the float64 twin's result for the stream and beam in question"""
    e_u, _ = noise_terms(W, b, chain)
    S = ref["smax"]
    return T * (e_u + U * S) + ref["merges"] * (2 * U * S + LIBM_EXP + LIBM_LOG * math.log(2.0))


# ---- the promises --------------------------------------------------------------------------------------------------------------------
def _position(m, a, b_):
    """the duplicate position two tied tokens of one hypothesis belong to, or None (two groups at one level, or the floor)"""
    for name, cols in m.groups.items():
        if a in cols and b_ in cols:
            return name
    return "blank|unk" if {a, b_} == {BLANK, UNK} else None


def check_stream(m, enc, beam):
    """the promises for one stream and beam.  Returns (float64 result, score bound, counts of every kind and duplicate position)"""
    V, T = m.V, enc.shape[0]
    r64 = twin(m.W, m.b, enc, beam, np.float64)
    others = [twin(m.W, m.b, enc, beam, dt, jitter=j) for dt, j in ((np.float32, 0), (np.float32, 1), (np.float32, -2), (np.float64, 1))]
    bound = score_bound(m.W, m.b, r64, T)
    cnt = dict.fromkeys(("a", "b", "c", "d", "e_tie", "e_merge", "f", "g", "h", "ties") + DUP_POSITIONS, 0)
    for t, f in enumerate(r64["frames"]):
        gap = -np.diff(f["val"])
        tied = gap == 0
        # a tie is a tie of two scores formed the same way from the same data; two different formations that agree are luck
        same = np.array([a == b_ for a, b_ in zip(f["sym"], f["sym"][1:])], bool)
        assert np.array_equal(tied, same), (beam, t, "a tie between two differently formed scores, or equal formations apart", gap, same)
        for o in others:
            g = o["frames"][t]
            assert np.array_equal(f["idx"], g["idx"]) and f["merges"] == g["merges"] and f["n"] == g["n"], (beam, t, "float32 selects otherwise")
            assert np.array_equal(tied, np.diff(g["val"]) == 0), (beam, t, "a tie in one format only", gap, -np.diff(g["val"]))
        assert (tied | (gap >= MARGIN * bound)).all(), (beam, t, "a gap that is neither a tie nor safe", gap[~tied].min(), bound)
        want = f["want"]
        cnt["ties"] += int(tied.sum())
        cnt["g"] += 1                                  # every logit is below zero, by construction (checked in check_case)
        tok, slot = f["idx"] % V, f["idx"] // V
        fl = f["onfloor"]
        if not tied[: want].any() and not fl[:want].any():
            cnt["a"] += 1
        cnt["c"] += int(fl[:want].any())
        if len(tied) >= want and tied[want - 1]:
            cnt["d"] += 1
        for i in np.flatnonzero(tied):
            if slot[i] == slot[i + 1]:
                pos = _position(m, int(tok[i]), int(tok[i + 1]))
                if pos:
                    cnt[pos] += 1
                elif not fl[i] and not fl[i + 1]:
                    cnt["b"] += 1
            else:
                cnt["e_tie"] += 1                      # exactly tied candidates of two hypotheses (with exactly tied log-probs)
        into = {}
        for r, q in f["merges"]:
            if f["val"][r] == f["val"][q] and slot[r] != slot[q]:
                cnt["e_merge"] += 1                    # two exactly tied paths from different hypotheses
            if q in into:
                cnt["f"] += 1                          # merged into an entry that was merged away itself
            into[r] = q
    a64 = r64["alts"]
    key = lambda a: (a["tokens"], a["timestamps"])     # noqa: E731
    for o in others:
        assert [key(a) for a in a64] == [key(a) for a in o["alts"]] and r64["order"] == o["order"], (beam, "float32 ends otherwise")
    for i, (x, y) in enumerate(zip(a64, a64[1:])):
        gap = x["norm"] - y["norm"]
        assert (gap == 0) == (x["sym"] == y["sym"]), (beam, "a final tie between two differently formed scores")
        for o in others:
            assert (gap == 0) == (o["alts"][i]["norm"] == o["alts"][i + 1]["norm"]), (beam, "a final tie in one format only")
        if gap == 0:
            cnt["h"] += 1
        else:
            need = sum(bound / (len(a["tokens"]) + 2) + 2 * U * abs(a["norm"]) for a in (x, y))
            assert gap >= MARGIN * need, (beam, "final order", gap, need)
    return r64, bound, cnt


def check_case(m, c):
    """every stream of the case at every beam -> {beam: (results [B], bounds [B], counts summed over the streams)}"""
    B, T, _ = c.enc.shape
    assert B <= 3 and T <= 16
    l = unique_logits(m.W, m.b, c.enc.reshape(B * T, J), np.float64)
    assert l.max() < 0 and (l >= FLOOR).all()          # every logit below a padded column's 0; nothing below the floor
    on = l > FLOOR
    assert (l[on] >= LEVELS[0] - 1e-3).all(), "a driven lever stays 5.5 above the floor"
    out = {}
    for beam in BEAMS:
        res, bounds, total = [], [], None
        for s in range(B):
            r, bd, cnt = check_stream(m, c.enc[s], beam)
            res.append(r)
            bounds.append(bd)
            total = cnt if total is None else {k: total[k] + cnt[k] for k in cnt}
        out[beam] = (res, bounds, total)
    return out


def required(V, beam):
    """the kinds and duplicate positions that must occur at least once at this V and beam.  What a beam cannot show: beam 1 keeps one
    hypothesis (no slots to tie, nothing to merge, one survivor); a tie across two groups needs both inside beam + 1 places beside the
    designated top group; two exactly tied paths that merge are [] + k and [k] + blank, which rank behind the equally tied [] + blank
    and so need three places (beam 4); the three-way merge is asked for at beam 8."""
    g = groups(V)
    need = ["a", "c", "d", "g", "ties"]
    need += [p for p in DUP_POSITIONS if p in g or p == "blank|unk"]
    if beam >= 2:
        need += ["e_tie", "h"]
    if beam >= 4:
        need += ["b", "e_merge"]
    if beam >= 8:
        need += ["f"]
    return need


def coverage(m):
    """{beam: counts over all of the model's cases}; raises where a required count is zero"""
    per_case = [check_case(m, c) for c in m.cases]
    out = {}
    for beam in BEAMS:
        tot = {}
        for pc in per_case:
            for k, v in pc[beam][2].items():
                tot[k] = tot.get(k, 0) + int(v)
        missing = [k for k in required(m.V, beam) if tot[k] == 0]
        assert not missing, (m.V, beam, "never exercised", missing)
        out[beam] = tot
    return out


def find_seed(V, tries=200):
    """the first seed whose model keeps the promises and the coverage (how SEEDS was drawn)"""
    why = []
    for seed in range(tries):
        try:
            coverage(build(V, seed))
            return seed, why
        except AssertionError as e:
            why.append((seed, str(e)[:160]))
    raise AssertionError((V, why[-5:]))


def different(a, ref, tol):
    """does result `a` differ from `ref`: tokens, timestamps, number or order of the alternatives, or a score / token log-prob by more
    than tol"""
    x, y = a["alts"], ref["alts"]
    if [(h["tokens"], h["timestamps"]) for h in x] != [(h["tokens"], h["timestamps"]) for h in y]:
        return True
    return any(abs(h["score"] - k["score"]) > tol or (len(h["tokens"]) and np.abs(h["token_log_probs"] - k["token_log_probs"]).max() > tol)
               for h, k in zip(x, y))
