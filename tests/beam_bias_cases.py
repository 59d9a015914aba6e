"""Inputs built to tie for the BIASED modified beam search -- the HW = true instantiations of csrc/beam.hip: hotword bonuses, the n-gram LM
walk of lm_walk.h, the final pick on lp - pending(state) -- with their float64 reference and the promises that make the comparison
exact.  Importable without a GPU: tests/test_beam_bias_ties_gpu.py runs the cases on the device, tests/test_beam_bias_cases_ref.py runs
the self-checks, the older restatements and the sensitivity variants on the host.  Everything rests on tests/beam_cases.py: the same
sparse-joiner model (beam_cases.build(V): zero decoder_proj, levers, floor, duplicate groups), V, beams and T' = 12, its logits, its
tie order, its logaddexp and its way of carrying with every score HOW it was formed.

BIASES, per V.  Two hotword lists over planted tokens, A and B (phrases(V, which)), c = hotword_twin.SCORE = 1.5, exactly representable
as are its multiples: one-token phrases on the HIGHER column of a duplicate pair (63 | 64: "64", the later twin V - 1, blank's twin
70, the highest stride of the NE = 16 / excl paths where V has it) and on a single; two phrases that start on the two columns of ONE
pair (A: "20 9 30" and "21 44") -- both columns earn, so no unbiased duplicate is left behind; a three-token phrase whose inner state
has a failure link into another phrase (A: "100 120 140" with "120 160"); in B a phrase that ends on a column of the triple.  An n-gram LM of order 3
(draw_lm: seeded): log-probs and back-offs are multiples of 1 / 8 and the scale is 0.5, so every scaled table entry, every back-off sum
and every term is a multiple of 1 / 16 of modest size: exact in float32.  Unigrams for every real token but two planted levers' (the
<unk> rule), bigrams and trigrams over the planted tokens, <s> with bigrams of its own (the start state is not state 0); a column and
its duplicates are ONE word to the LM (draw_lm says why).
CONFIGURATIONS: "hw" (list A), "lm", "both" (A and the LM), "bothB" (B and the LM: what stream 2 of the resumed test walks).

FRAMES are drawn by this file (cases(V), seeds in SEEDS): case "match" scripts the first frames so that the phrases are entered,
continued, committed, broken and left through a failure link, and repeats a frame with blank and 70 on top -- [70] earns, and the
second copy merges [] + 70, with this frame's bonus, INTO the first-inserted [70] + blank; case "repeat" opens three streams with a
frame repeated (beam_cases' commutative ties, over columns that earn nothing from the root in either list).  Later frames are
beam_cases' random ones, a designated duplicate group on top in turn; a stream's last frame puts a token that starts a phrase 0.3 ..
0.6 above one that commits at once -- the take-back changes the winner -- in case "match" "20 | 21" over "63 | 64": two tied hypotheses
of equal length with equal non-zero pending.

THE HAZARD the lists and scripts are built around: a broken match hands back what it earned, and (s + c) - c equals s in exact
arithmetic and usually, not always, in float32.  A hypothesis that went through one must never be COMPARED with its unbiased duplicate.
Nothing is excused: the formation check below rejects every draw in which it happens.

REFERENCE.  twin() is beam_cases.twin with a graph (hotword_twin.TwinGraph) and an LM (ngram_twin.TwinLm, already scaled) passed in.
It keeps the kernel's association: the selection value untouched (the rank, the cut and the tap's val are unbiased), then
(val + bonus) + term for a selected candidate that appends a real token, merges by logaddexp of the BIASED values in insertion
order, the first-inserted entry's timestamps, graph state and LM state kept, the final order on (lp - pending(state)) / (length + 2)
with ties in insertion order and the reported score lp - pending(state).  A bonus, a term and a take-back that are exactly zero
leave the bits alone (x + 0 = x) and are no part of a formation; every other one is: ("b", ., bonus), ("t", ., term), ("k", ., pending).

BOUND (score_bound).  Bonus, term and take-back are exact values, so each adds one rounding at the score's magnitude: two more per
frame, one at the end.  With E_u, E_m, S and M as in beam_cases -- S now taken over the biased values too --
        score_bound = T' (E_u + 3 U S) + M E_m + U S          token log-prob bound = E_u  (unchanged: taken before the bias)

PROMISES (check_stream raises otherwise), unchanged in kind: every consecutive pair among the top beam + 1 candidates of every frame
and every adjacent pair of final normalised scores is an exact tie between EQUALLY FORMED scores -- in float64, in float32 and in three
jittered runs -- or 10 x the bound apart; all five runs select, merge and end alike.  No third kind, no excuse list.  SEEDS are
draws per V (find_seed: about one in a hundred passes) that keep the promises in all four configurations, cover every kind of COUNTS
at every beam that admits it (required()), keep the final-order promise on the prefixes of ENDS for at least three quarters of the
(stream, beam, end) triples of the resumed test (prefix_share) and tell every wrong variant from the reference (caught())."""
import dataclasses
import functools
import math

import numpy as np

import beam_cases as bc
from beam_cases import BEAMS, BLANK, J, LIBM_EXP, LIBM_LOG, MARGIN, T_FRAMES, U, UNK, VS  # noqa: F401
from hotword_twin import SCORE, TwinGraph
from ngram_twin import BOS, LM_UNK, TwinLm

SCALE = 0.5
CONFIGS = ("hw", "lm", "both", "bothB")
ENDS = (3, 4, 9)              # the inner chunk ends of the resumed test's uneven split 3 / 1 / 5 / 3
BIAS_RULES = ("bonus_before_selection", "no_take_back", "take_back_after_norm", "merge_drops_bonus", "miss_to_root", "no_reset_on_commit",
              "backoff_dropped", "lm_state_stuck")
COUNTS = ("bonus", "giveback", "inside", "fail_link", "commit", "dup_bonus_in", "dup_bonus_cut", "tied_states", "merge_bonus", "final_takeback",
          "final_tie_pending", "full", "back1", "uni", "unk", "lm_from_merged", "ties", "e_merge", "h")
# a seed per V that keeps every promise and covers every kind (find_seed; test_beam_bias_cases_ref.py re-checks them)
SEEDS = {200: 1501, 400: 65, 600: 163, 1021: 288, 1029: 1724}


def phrases(V, which):
    g = bc.groups(V)
    if which == "A":
        p = [[64], [V - 1], [70], [20, 9, 30], [21, 44], [100, 120, 140], [120, 160], [180]]
        if "high-stride" in g:
            p.append([g["high-stride"][1]])
    else:
        p = [[21], [63, 100, 160], [64, 30], [44, 140, 180], [140, 100], [120, 133], [9]]
        if "high-stride" in g:
            p.append([g["high-stride"][0]])
    return p


def classes(V):
    """the planted real tokens by lever: the columns of one duplicate group are ONE word to the LM"""
    out = [tuple(c for c in cols if c not in (BLANK, UNK)) for cols in bc.groups(V).values()]
    return [c for c in out if c]


def draw_lm(V, seed):
    """[(ids, log_prob, backoff)]: every weight a multiple of 1 / 8.  Drawn over classes(V) and written out for every member: the LM
    cannot tell a column from its duplicate, so two tied hypotheses that differ in a duplicate earn the same terms in the same order and
    stay EQUALLY FORMED -- were the terms different, the two sums of multiples of 1 / 16 would soon agree again through different
    additions, the tie no format guarantees."""
    rng = np.random.default_rng(104729 * V + seed)
    C = classes(V)

    def eighths(lo, hi):
        return float(-int(rng.integers(lo, hi + 1)) / 8.0)

    holes = {C[int(rng.integers(len(C)))], (9,) if seed % 2 else (160,)}
    ent = {(BOS,): (-99.0, eighths(1, 8)), (LM_UNK,): (-3.0, 0.0)}

    def put(cls, lp, bo):
        def expand(i):
            if i == len(cls):
                return [()]
            return [(v,) + rest for v in cls[i] for rest in expand(i + 1)]
        for ids in expand(0):
            ent[ids] = (lp, bo)

    ok = [c for c in C if c not in holes]
    floor = sorted(set(range(V)) - {BLANK, UNK} - {v for c in C for v in c})
    for c in ok + [(v,) for v in floor]:
        put((c,), eighths(4, 24), eighths(1, 8))
    for a in [(BOS,)] + ok:
        for b_ in ok:
            if rng.random() < 0.5:
                put((a, b_), eighths(1, 12), eighths(1, 8))
                for c in ok:
                    if rng.random() < 0.3:
                        put((a, b_, c), eighths(1, 8), 0.0)
    return [(ids, lp, bo) for ids, (lp, bo) in sorted(ent.items(), key=lambda kv: (len(kv[0]), kv[0]))]


@dataclasses.dataclass
class Bias:
    graph: object = None      # TwinGraph
    lm: object = None         # TwinLm, scaled
    phrases: object = None
    entries: object = None


@functools.lru_cache(maxsize=None)
def biases(V, seed=None):
    """{configuration: Bias}"""
    seed = SEEDS[V] if seed is None else seed
    entries = draw_lm(V, seed)
    lm = TwinLm(entries, V).scaled(SCALE)
    for k, v in list(lm.lp.items()) + list(lm.bo.items()):
        assert float(v) * 16 == int(float(v) * 16), (k, v)
    pa, pb = phrases(V, "A"), phrases(V, "B")
    ga, gb = TwinGraph(pa, SCORE, V), TwinGraph(pb, SCORE, V)
    return {"hw": Bias(ga, None, pa, None), "lm": Bias(None, lm, None, entries), "both": Bias(ga, lm, pa, entries), "bothB": Bias(gb, lm, pb, entries)}


# ---- the frames ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases(V, seed=None):
    """(beam_cases.Model whose cases are this file's, drawn with SEEDS[V])"""
    seed = SEEDS[V] if seed is None else seed
    base = bc.build(V)
    rng = np.random.default_rng(15485863 * V + seed)
    g = base.groups
    names = list(g)
    dups = [n for n in names if len(g[n]) > 1]

    def row(levels):
        e = np.zeros(J, np.float32)
        for n, lv in levels.items():
            e[names.index(n)] = bc.enc_of(lv)
        return e

    def spaced(k, lo=bc.LEVELS[0], hi=bc.LEVELS[1], gap=0.12):
        while True:
            x = np.sort(rng.uniform(lo, hi, k))[::-1]
            if k < 2 or np.diff(x).max() <= -gap:
                return [float(v) for v in x]

    def scripted(tops, extra=2, close=False):
        """the named levers on top in this order, `extra` random ones below them; close: the second within 0.3 .. 0.6 of the first, so
        that a bonus of 1.5 decides between them"""
        others = [n for n in names if n not in tops and n != "unk"]
        chosen = list(tops) + [others[i] for i in rng.permutation(len(others))[:extra]]
        lv = spaced(len(chosen))
        while close and not 0.3 <= lv[0] - lv[1] <= 0.6:
            lv = spaced(len(chosen))
        return row(dict(zip(chosen, lv)))

    turn = [int(rng.integers(len(dups)))]

    def random_frame():
        top = dups[turn[0] % len(dups)]
        turn[0] += 1
        k = int(rng.choice([1, 2, 3, 6, 7, 8], p=[0.1, 0.1, 0.1, 0.3, 0.2, 0.2]))
        others = [n for n in names if n != top]
        chosen = [top] + [others[i] for i in rng.permutation(len(others))[: k - 1]]
        lv = dict(zip(chosen, spaced(k)))
        if k >= 3 and rng.random() < 0.25:
            lv[chosen[2]] = lv[chosen[1]]
        if "blank|tok" in lv and rng.random() < 0.5:
            lv["unk"] = lv["blank|tok"]
        return row(lv)

    def stream(prologue, last):
        """last: the levers on top of the last frame -- a hypothesis that ends inside a phrase beside one that has just committed"""
        n = T_FRAMES - len(prologue) - 1
        return np.stack(prologue + [random_frame() for i in range(n)] + [scripted(last, 1, close=True)])

    s = lambda c: f"single{c}"     # noqa: E731
    x = spaced(5, -4.5, -0.5, 0.4)
    # (everything else 2 and more below blank | 70: the second copy ranks [70] + blank, [70] + 70, [] + blank, [] + 70 -- [70]'s lead
    # of 1.5 lifts nothing else past [] + 70, so the merge happens from beam 4 on)
    z = spaced(3, bc.LEVELS[0], x[0] - 2.0, 0.4)
    bt = row({"blank|tok": x[0], "unk": z[0], s(30): z[1], s(160): z[2]})
    match = [
        # list A: [20] and [21] enter two phrases (tied, different states), "20 9" goes on and "21 44" commits while [20] + 44 and
        # [21] + 9 break; "20 9 30" commits; "100 120" + 160 leaves through the failure link into "120 160"; + 100 falls back into "100";
        # a single over two pairs whose HIGHER column is a phrase: the cut of an even beam falls inside a pair
        stream([scripted(["neighbours", s(9)]), scripted([s(9), s(44), s(100)]), scripted([s(30), s(100), "63|64"]), scripted([s(100), s(120)]),
                scripted([s(120), s(100), s(140)]), scripted([s(160), s(100), s(140)]), scripted([s(44), "63|64", "last"], 1)], ["neighbours", "63|64"]),
        # list B: the same with "63 100 9" / "64 30", "44 140 160" / "140 180"
        stream([scripted(["63|64", s(100)]), scripted([s(100), s(30), s(44)]), scripted([s(9), s(44), "neighbours"]), scripted([s(44), s(140)]),
                scripted([s(140), s(44), s(160)]), scripted([s(100), s(44), s(160)]), scripted([s(30), "last", "63|64"], 1)], ["63|64", "neighbours"]),
        # blank and 70 at one level, twice: [70] earns (A), and the second copy merges [] + 70 into [70] + blank
        stream([bt, bt, scripted([s(180), "lane-strides"]), scripted([s(120), "lane-strides", s(100)])], [s(100), s(180)]),
    ]
    y = spaced(5, -4.5, -0.5, 0.4)
    # (only columns that earn nothing from the root in either list: [a, b] and [b, a] must stay the commutative 0 + a + b -- with a
    # bonus on a, (a + c) + b and (b + a) + c are equal in exact arithmetic alone)
    free = ["255|256"] if "255|256" in g else []
    free += [s(300), s(390)] if s(300) in g else []
    rep = [row(dict(zip([s(30), s(160), "lane-strides"] + free[:1], y))),
           row(dict(zip(["lane-strides", s(30)] + free[1:] + [s(160)], y))),
           row(dict(zip([s(160), "lane-strides", s(30)] + free[:2], y)))]
    repeat = [stream([r, r], l) for r, l in zip(rep, ([s(44), s(9)], [s(100), s(180)], [s(120), "63|64"]))]
    return bc.Model(V, base.W, base.b, g, [bc.Case("match", np.stack(match)), bc.Case("repeat", np.stack(repeat))])


# ---- the search, restated ------------------------------------------------------------------------------------------------------------
def step_hw(graph, s, tok, rule=None):
    """(next state, bonus, committed, the miss landed inside a phrase, it got there through a failure link) -- TwinGraph's step,
    taken apart so that a miss can be seen and the wrong variants can be told"""
    if graph is None or tok in (BLANK, UNK):
        return s, 0.0, False, False, False
    miss = s != 0 and tok not in graph.goto[s]
    at_root = graph.goto[0].get(tok, 0)
    n = at_root if (rule == "miss_to_root" and miss) else graph.delta(s, tok)
    bonus = float(graph.pending(n)) - float(graph.pending(s))
    end = graph.end[n]
    nxt = n if (rule == "no_reset_on_commit" or not end) else 0
    if rule is None:
        want = graph.step(s, tok)
        assert (nxt, bonus, end) == (want[0], float(want[1]), want[2])
    return nxt, bonus, end, miss and n != 0, miss and n != at_root


def step_lm(lm, s, tok, rule=None):
    """(next state, term, event) -- TwinLm.step, with the two wrong variants"""
    if lm is None:
        return s, 0.0, None
    nxt, term, ev = lm.step(s, tok)
    if ev is None:
        return s, 0.0, None
    term = float(term)
    if ev not in ("full", "hit"):
        if rule == "backoff_dropped":
            g = lm.hist[s]
            while g + (tok,) not in lm.lp and g != ():
                term -= float(lm.bo[g])
                g = lm._longest_state(g, len(g) - 1)
        if rule == "lm_state_stuck" and ev != "unk":
            nxt = s
    return nxt, term, ev


def twin(W, b, enc, beam, dtype=np.float64, graph=None, lm=None, rule=None, jitter=0):
    """beam_cases.twin with a hotword graph and a (scaled) LM.  One stream, enc [T', J].  Returns what beam_cases.twin returns --
    alts' `score` is the finalized lp - pending(state), `carried` the log-prob a stream would keep -- plus events = counts of COUNTS'
    bias kinds.  rule: None or one of BIAS_RULES, a deliberately WRONG biased search."""
    assert rule is None or rule in BIAS_RULES, rule
    dtype = np.dtype(dtype).type
    W, b = np.asarray(W), np.asarray(b)
    V = W.shape[0]
    logits = bc.unique_logits(W, b, enc, dtype, jitter)
    idle = ~(W != 0).any(1)
    hyps = [dict(ys=[], ts=[], yp=[], lp=dtype(0), sym=(), st=0, lst=lm.start if lm is not None else 0, merged=False)]
    rows = {}
    frames, selected, smax, nmerge = [], set(), 0.0, 0
    ev = dict.fromkeys(COUNTS, 0)
    bvec = {}
    tok_ids = np.arange(V)
    for t in range(enc.shape[0]):
        l = logits[t]
        rowid = rows.setdefault(np.asarray(enc[t], np.float32).tobytes(), len(rows))
        on_floor = idle | (l == dtype(bc.FLOOR))
        mx = l.max()
        lse = np.log(np.exp(l - mx).sum(dtype=dtype))
        u = (l - mx) - lse
        nA = len(hyps)
        want = min(beam, nA * V)
        flat, val = [], []
        for k, h in enumerate(hyps):
            sc = u + h["lp"]
            if rule == "bonus_before_selection" and graph is not None:
                if h["st"] not in bvec:
                    v = np.zeros(V)
                    for tok in {x for gt in graph.goto for x in gt}:
                        v[tok] = step_hw(graph, h["st"], tok)[1]
                    bvec[h["st"]] = v.astype(dtype)
                sc = sc + bvec[h["st"]]
            ids, s = bc.tie_sorted(sc, tok_ids, want + 1, None)
            flat.append(k * V + ids[: want + 1])
            val.append(s[: want + 1])
        flat, val = np.concatenate(flat), np.concatenate(val)
        flat, val = bc.tie_sorted(val, flat, want + 1, None)
        flat, val = flat[: want + 1].copy(), val[: want + 1].copy()
        smax = max(smax, float(np.abs(val).max()))
        # what every ranked candidate -- the runner-up behind the cut too -- earns: (val + bonus) + term
        cand = []
        for r in range(len(flat)):
            k, tok = int(flat[r]) // V, int(flat[r]) % V
            h = hyps[k]
            st, bonus, end, inside, via = step_hw(graph, h["st"], tok, rule)
            real = tok not in (BLANK, UNK)
            lst, term, lev = step_lm(lm, h["lst"], tok, rule) if real else (h["lst"], 0.0, None)
            sym = sel = bc._sym_add(h["sym"], (rowid, float(l[tok])))
            v = val[r]
            if rule == "bonus_before_selection":
                bonus_add = 0.0
            else:
                bonus_add = bonus
            nob = v
            if bonus_add != 0.0:
                v = dtype(v + dtype(bonus_add))
                sym = ("b", sym, bonus_add)
            if term != 0.0:
                v = dtype(v + dtype(term))
                nob = dtype(nob + dtype(term))
                sym = ("t", sym, term)
            cand.append(dict(k=k, tok=tok, real=real, st=st, lst=lst, bonus=bonus, end=end, inside=inside, via=via, lev=lev, v=v, nob=nob, sym=sym, sel=sel))
        for i in range(len(val) - 1):
            if val[i] == val[i + 1]:
                a, c = cand[i], cand[i + 1]
                if a["k"] == c["k"]:
                    if a["bonus"] != c["bonus"] and max(a["bonus"], c["bonus"]) > 0:
                        if i + 1 < want:
                            ev["dup_bonus_in"] += 1
                        elif i == want - 1 and c["bonus"] > a["bonus"]:
                            ev["dup_bonus_cut"] += 1
                elif i + 1 < want and graph is not None:
                    sa, sc_ = hyps[a["k"]]["st"], hyps[c["k"]]["st"]
                    if sa and sc_ and sa != sc_ and graph.pending(sa) == graph.pending(sc_):
                        ev["tied_states"] += 1
        new, where, merges, dead = [], {}, [], set()
        for r in range(want):
            c = cand[r]
            h = hyps[c["k"]]
            selected.add(c["tok"])
            smax = max(smax, abs(float(c["v"])))
            ev["bonus"] += c["bonus"] > 0
            ev["giveback"] += c["bonus"] < 0
            ev["inside"] += c["inside"]
            ev["fail_link"] += c["via"]
            ev["commit"] += bool(c["end"])
            if c["lev"] in ev:
                ev[c["lev"]] += 1
            ev["lm_from_merged"] += c["lev"] is not None and h["merged"]
            ys = h["ys"] + [c["tok"]] if c["real"] else h["ys"]
            key = tuple(ys)
            if key in where:
                q, last = where[key]
                merges.append((r, last))
                nmerge += 1
                ev["merge_bonus"] += c["bonus"] > 0 and not cand[last]["real"]
                ev["e_merge"] += val[r] == val[last] and c["k"] != cand[last]["k"]
                add = c["nob"] if rule == "merge_drops_bonus" else c["v"]
                new[q]["lp"] = bc.logaddexp(new[q]["lp"], add, dtype)
                new[q]["sym"] = ("lae", new[q]["sym"], c["sym"]) if new[q]["sym"][0] == "lae" else ("lae",) + tuple(sorted([new[q]["sym"], c["sym"]], key=repr))
                new[q]["merged"] = True
                smax = max(smax, abs(float(new[q]["lp"])))
                dead.add(r)
                where[key] = (q, r)
            else:
                where[key] = (len(new), r)
                new.append(dict(ys=ys, ts=h["ts"] + [t] if c["real"] else h["ts"], yp=h["yp"] + [u[c["tok"]]] if c["real"] else h["yp"], lp=c["v"],
                                sym=c["sym"], st=c["st"], lst=c["lst"], merged=False))
        ev["ties"] += int((np.diff(val) == 0).sum())
        frames.append(dict(idx=flat, val=val, merges=merges, n=len(new), want=want, onfloor=on_floor[flat % V], nA=nA, sym=[c["sel"] for c in cand],
                           biased=[c["v"] for c in cand]))
        hyps = new
    fin = []
    for h in hyps:
        pend = float(graph.pending(h["st"])) if graph is not None else 0.0
        n2 = dtype(len(h["ys"]) + 2)
        take = pend != 0.0 and rule != "no_take_back"
        fl = dtype(h["lp"] - dtype(pend)) if take else h["lp"]
        norm = dtype(h["lp"] / n2 - dtype(pend)) if (rule == "take_back_after_norm" and take) else fl / n2
        fin.append(dict(fl=fl, norm=norm, pend=pend, sym=(("k", h["sym"], pend) if take else h["sym"], len(h["ys"])), raw=h["lp"] / n2))
        smax = max(smax, abs(float(fl)))
    order = sorted(range(len(hyps)), key=lambda i: (-fin[i]["norm"], i))
    ev["final_takeback"] += order[0] != min(range(len(hyps)), key=lambda i: (-fin[i]["raw"], i))
    alts = [dict(tokens=hyps[i]["ys"], timestamps=hyps[i]["ts"], token_log_probs=np.array(hyps[i]["yp"], np.float64), score=float(fin[i]["fl"]),
                 carried=float(hyps[i]["lp"]), norm=fin[i]["norm"], sym=fin[i]["sym"], pend=fin[i]["pend"], st=hyps[i]["st"], lst=hyps[i]["lst"]) for i in order]
    for x, y in zip(alts, alts[1:]):
        if x["norm"] == y["norm"]:
            ev["h"] += 1
            ev["final_tie_pending"] += x["pend"] != 0 and x["pend"] == y["pend"]
    return dict(alts=alts, order=order, frames=frames, selected=selected, smax=smax, merges=nmerge, events=ev)


# ---- the bound -----------------------------------------------------------------------------------------------------------------------
def score_bound(W, b, ref, T, chain=None):
    """ref: the float64 twin's result for the stream, beam and bias in question"""
    e_u, _ = bc.noise_terms(W, b, chain)
    S = ref["smax"]
    return T * (e_u + 3 * U * S) + ref["merges"] * (2 * U * S + LIBM_EXP + LIBM_LOG * math.log(2.0)) + U * S


# ---- the promises --------------------------------------------------------------------------------------------------------------------
RUNS = ((np.float32, 0), (np.float32, 1), (np.float32, -2), (np.float64, 1))


def _final_promise(r64, others, bound, beam):
    a64 = r64["alts"]
    key = lambda a: (a["tokens"], a["timestamps"])     # noqa: E731
    for o in others:
        assert [key(a) for a in a64] == [key(a) for a in o["alts"]] and r64["order"] == o["order"], (beam, "float32 ends otherwise")
    for i, (x, y) in enumerate(zip(a64, a64[1:])):
        gap = x["norm"] - y["norm"]
        assert (gap == 0) == (x["sym"] == y["sym"]), (beam, "a final tie between two differently formed scores")
        for o in others:
            assert (gap == 0) == (o["alts"][i]["norm"] == o["alts"][i + 1]["norm"]), (beam, "a final tie in one format only")
        if gap != 0:
            need = sum(bound / (len(a["tokens"]) + 2) + 2 * U * abs(a["norm"]) for a in (x, y))
            assert gap >= MARGIN * need, (beam, "final order", gap, need)


def check_stream(m, enc, beam, bias):
    """the promises for one stream, beam and bias.  Returns (float64 result, score bound)"""
    T = enc.shape[0]
    r64 = twin(m.W, m.b, enc, beam, np.float64, bias.graph, bias.lm)
    others = [twin(m.W, m.b, enc, beam, dt, bias.graph, bias.lm, jitter=j) for dt, j in RUNS]
    bound = score_bound(m.W, m.b, r64, T)
    for t, f in enumerate(r64["frames"]):
        gap = -np.diff(f["val"])
        tied = gap == 0
        # the RANK is made on the selection values (the parent's biased log-prob + u): a tie is a tie of two equally formed ones
        same = np.array([a == b_ for a, b_ in zip(f["sym"], f["sym"][1:])], bool)
        assert np.array_equal(tied, same), (beam, t, "a tie between two differently formed scores, or equal formations apart", gap, same)
        for o in others:
            g = o["frames"][t]
            assert np.array_equal(f["idx"], g["idx"]) and f["merges"] == g["merges"] and f["n"] == g["n"], (beam, t, "float32 selects otherwise")
            assert np.array_equal(tied, np.diff(g["val"]) == 0), (beam, t, "a tie in one format only", gap, -np.diff(g["val"]))
        assert (tied | (gap >= MARGIN * bound)).all(), (beam, t, "a gap that is neither a tie nor safe", gap[~tied].min(), bound)
    _final_promise(r64, others, bound, beam)
    return r64, bound


def prefix_ok(m, enc, beam, bias, n):
    """does the twin's own final-order promise hold after the first n frames?  Decided from the twin alone."""
    e = enc[:n]
    r64 = twin(m.W, m.b, e, beam, np.float64, bias.graph, bias.lm)
    others = [twin(m.W, m.b, e, beam, dt, bias.graph, bias.lm, jitter=j) for dt, j in RUNS]
    try:
        _final_promise(r64, others, score_bound(m.W, m.b, r64, n), beam)
    except AssertionError:
        return False
    return True


def resumed_bias(V, stream, seed=None):
    """the bias stream `stream` of a resumed call walks: graph A, none, graph B -- the LM sits on the model"""
    return biases(V, seed)[("both", "lm", "bothB")[stream]]


def prefix_share(V, seed=None):
    """(triples whose prefix keeps the final-order promise, all triples) over the resumed test's (case, stream, beam, end)"""
    m = cases(V, seed)
    ok = [prefix_ok(m, c.enc[s], beam, resumed_bias(V, s, seed), n) for c in m.cases for s in range(c.enc.shape[0]) for beam in BEAMS for n in ENDS]
    return sum(ok), len(ok)


def required(V, beam, config):
    """the kinds that must occur at least once at this V, beam and configuration.  What a beam cannot show: beam 1 keeps one hypothesis
    -- no two candidates inside the beam, no slots to tie, nothing to merge, one survivor and so no final order; a phrase left through a
    failure link needs the three-token match alive beside stronger paths (asked from beam 2); a take-back changes the winner where a
    hypothesis that has just committed survives beside the leader that ends inside a phrase AND that leader's tied duplicate, three
    places (asked from beam 4); [] + k into [k] + blank ranks behind
    [k] + k's equals and needs four places, as beam_cases' tied merges do; an LM walk from a merged hypothesis follows such a merge."""
    need = ["ties"]
    hw, lm = config != "lm", config != "hw"
    if hw:
        need += ["bonus", "giveback", "commit", "dup_bonus_cut"]
    if lm:
        need += ["full", "back1", "uni", "unk"]
    if beam >= 2:
        need += ["h"]
        if hw:
            need += ["dup_bonus_in", "tied_states", "inside", "fail_link", "final_tie_pending"]
    if beam >= 4:
        if hw:
            need += ["merge_bonus", "final_takeback"]
        if lm:
            need += ["lm_from_merged"]
    return need


def coverage(V, seed=None):
    """{(configuration, beam): counts over all cases and streams}; raises where a promise breaks or a required count is zero.  The
    hotword kinds are required of "hw" and "both" (list A); "bothB" must keep the promises and show the events of a list at work."""
    m = cases(V, seed)
    out = {}
    for config, bias in biases(V, seed).items():
        for beam in BEAMS:
            tot = dict.fromkeys(COUNTS, 0)
            for c in m.cases:
                assert c.enc.shape[0] <= 3 and c.enc.shape[1] == T_FRAMES
                for s in range(c.enc.shape[0]):
                    try:
                        r, _ = check_stream(m, c.enc[s], beam, bias)
                    except AssertionError as e:
                        raise AssertionError((V, config, c.name, s) + e.args) from None
                    for k, v in r["events"].items():
                        tot[k] += int(v)
            need = required(V, beam, config) if config != "bothB" else ["ties", "bonus", "giveback", "commit", "full", "uni"]
            missing = [k for k in need if tot[k] == 0]
            assert not missing, (V, config, beam, "never exercised", missing)
            out[config, beam] = tot
    ok, n = prefix_share(V, seed)
    assert 4 * ok >= 3 * n, (V, "prefix ends that keep the final-order promise", ok, n)
    return out


HW_RULES = BIAS_RULES[:6]


def caught(V, rule, seed=None):
    """(the (configuration, case, stream, beam) runs on which the twin with `rule` broken differs from the reference -- tokens,
    timestamps, order, or a score by more than the bound --, all runs tried)"""
    m = cases(V, seed)
    out, n = [], 0
    for config in (("hw", "both") if rule in HW_RULES else ("lm", "both")):
        bias = biases(V, seed)[config]
        for c in m.cases:
            for s in range(c.enc.shape[0]):
                for beam in BEAMS:
                    ref = twin(m.W, m.b, c.enc[s], beam, np.float64, bias.graph, bias.lm)
                    n += 1
                    if bc.different(twin(m.W, m.b, c.enc[s], beam, np.float64, bias.graph, bias.lm, rule=rule), ref, score_bound(m.W, m.b, ref, c.enc.shape[1])):
                        out.append((config, c.name, s, beam))
    return out, n


def find_seed(V, tries=200, start=0):
    """the first seed from `start` on whose frames and LM keep the promises and the coverage and tell every wrong variant from the
    reference (how SEEDS was drawn)"""
    why = []
    for seed in range(start, tries):
        try:
            coverage(V, seed)
            blind = [r for r in BIAS_RULES if not caught(V, r, seed)[0]]
            assert not blind, (V, "wrong variants that pass", blind)
            return seed, why
        except AssertionError as e:
            why.append((seed, str(e)[:200]))
    raise AssertionError((V, why[-5:]))
