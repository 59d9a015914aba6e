"""The cases of the LODR tests (test_lodr.py on the CPU, test_lodr_gpu.py on the device).

OPERATOR CASES.  The tiny model and the three short utterances of rnn_lm_fusion_cases (T' about 20) at neural weight SCALE = 0.5,
neural LMs A (V = 37) and C (V = 165), beams 1, 2, 4, 8, N-best 4.  The LODR LM of a case is a bi-gram drawn by
ngram_twin.draw_lm(..., order=2) with LODR_LM_SEED from the plain beam-4 search's output over the case's utterances; its weight is a
member of LSCALES.  A draw is (utterance base, neural LM seed, LODR weight) in the order of draws(): rnn_lm_fusion_cases.draws() with the
weights -0.25, -0.5, -1.0 under each pair.  A draw is ACCEPTED by rnn_lm_fusion_cases' rule, on lodr_twin.twin_beam_search with N-best 4:
every consecutive gap among the top beam + 1 candidates of every frame of every stream, and every adjacent pair of final normalised
scores, is at least parity.LOGIT_TOL.  SEEDS records per (LM name, beam) the FIRST accepted draw with its smallest gap and `moved`: the
number of its streams whose tokens or order of alternatives differ from the same fused search WITHOUT LODR (`python tests/lodr_cases.py`
prints the tables; test_lodr.py re-checks acceptance, the gap, the count, and that none of the FIRST_CHECKED draws in front of a
recorded one is accepted).  On an accepted case the device must equal the twin in tokens, timestamps and the number and order of
alternatives, with nothing excused.

TOGETHER CASES.  LM A at beam 4 with LODR and (a) the hotword graph, (b) the positive-weight tri-gram LM of
rnn_lm_fusion_cases.together_extras.  In (b) two automata are walked at once: the tri-gram (order 3, about a hundred states) and the
LODR bi-gram (order 2, states = its unigram histories) differ in size, so a state of one is no state of the other.

THE SCORE BOUND.  The LODR term of a token is the SAME float32 number on the device and in the twin (the step over the scaled tables is
exact integer look-ups and float32 additions in a fixed order), so LODR adds no error of its own to a score but one more float32
rounding per appended token, each at most 2^-24 of the partial sum relative, bounded here by 2^-23 S with S the largest absolute partial
score the twin saw in the case:
    score_bound(frames, n, S) = rnn_lm_fusion_cases.score_bound(frames, n) + n 2^-23 S
and the acceptance rule needs LOGIT_TOL >= 2 score_bound for every case, which test_lodr.py asserts."""
import numpy as np

import rnn_lm_fusion_cases as fc

STREAMS = fc.STREAMS
BEAMS = fc.BEAMS
NBEST = fc.NBEST
SCALE = fc.SCALE
YP_TOL = fc.YP_TOL
LMS = ("A", "C")
OPERATOR = {"A": "tiny", "C": "tiny165"}
LSCALES = (-0.25, -0.5, -1.0)
LODR_LM_SEED = 7
FIRST_CHECKED = 6     # draws in front of a recorded one that test_lodr.py re-checks as not accepted


def draws(limit=4000):
    """the order in which (utterance base, neural LM seed, LODR weight) triples are tried"""
    return [(base, seed, ls) for base, seed in fc.draws(limit) for ls in LSCALES]


def score_bound(frames, n_tokens, S, scale=SCALE):
    """a reported score of a hypothesis of n_tokens tokens after `frames` frames, device against twin; S: the largest absolute partial
    score of the case"""
    return fc.score_bound(frames, n_tokens, scale) + max(int(n_tokens), 1) * 2.0 ** -23 * float(S)


# (LM name, beam) -> (utterance base, neural LM seed, LODR weight, smallest gap on the twin, moved streams of 3) of the first accepted draw
SEEDS = {
    ("A", 1): (50, 0, -0.25, 0.007618, 0),     # (beam 1 keeps one hypothesis: a term common to all candidates of a parent moves nothing)
    ("A", 2): (50, 0, -0.25, 0.002754, 3),
    ("A", 4): (50, 0, -0.25, 0.001411, 3),
    ("A", 8): (89, 1, -0.25, 0.001022, 3),
    ("C", 1): (50, 0, -0.25, 0.001553, 0),
    ("C", 2): (50, 0, -0.25, 0.003979, 3),
    ("C", 4): (53, 1, -1.0, 0.001069, 3),
    ("C", 8): (713, 0, -1.0, 0.00127, 3),
}
MOVED = sum(v[4] for v in SEEDS.values())      # 18 of the 24 streams of the operator cases differ from the fused search without LODR

# what -> (utterance base, neural LM seed, LODR weight, smallest gap, moved streams of 3): LM A, beam 4
TOGETHER = {
    "hotwords": (50, 0, -0.5, 0.0012, 3),
    "ngram": (50, 0, -0.25, 0.001411, 2),
}


def lodr_lm(ora, enc):
    """(TwinLm, entries) of the case's LODR bi-gram, drawn from the plain search's output"""
    from ngram_twin import TwinLm, draw_lm
    plain = ora.modified_beam_search(enc, 4)
    entries = draw_lm(plain, ora.vocab_size, np.random.default_rng(LODR_LM_SEED), order=2)
    return TwinLm(entries, ora.vocab_size), entries


def moved_streams(with_lodr, without):
    """streams whose tokens or order of alternatives differ between two lists of twin runs (N-best on)"""
    return sum([a["tokens"] for a in x["alts"]] != [a["tokens"] for a in y["alts"]] for x, y in zip(with_lodr, without))


def run_case(ora, enc, beam, nlm, lodr, lscale, extras=None):
    """the twin runs of a case: (with LODR, the same fused search without)"""
    from lodr_twin import twin_batch
    ex = extras or {}
    kw = dict(nlm=nlm, nscale=SCALE, lm=ex.get("lm"), scale=ex.get("scale", 0.0), graph=ex.get("graph"), nbest=NBEST)
    return twin_batch(ora, enc, beam, lodr=lodr, lscale=lscale, **kw)[4], twin_batch(ora, enc, beam, **kw)[4]


def case_smax(runs):
    return max(r["smax"] for r in runs)


if __name__ == "__main__":   # the search that filled the tables above: [seeds|together] [LM name] [beam]
    import sys
    import tempfile
    from lodr_twin import twin_batch
    what = sys.argv[1] if len(sys.argv) > 1 else "seeds"
    with tempfile.TemporaryDirectory() as d:
        oras = {w: fc.make_oracle(d, w)[1] for w in ("tiny", "tiny165")}
        encs, lodrs = {}, {}

        def enc_of(which, base):
            if (which, base) not in encs:
                encs[(which, base)] = fc.encode(oras[which], fc.utterances(base))
                lodrs[(which, base)] = lodr_lm(oras[which], encs[(which, base)])[0]
            return encs[(which, base)], lodrs[(which, base)]

        def search(name, beam, extra_of, label):
            which = OPERATOR[name]
            for base, seed, ls in draws():
                enc, lodr = enc_of(which, base)
                ex = extra_of(oras[which], enc)
                _, nlm, _ = fc.make_lm(d, name, seed)
                kw = dict(nlm=nlm, nscale=SCALE, lm=ex.get("lm"), scale=ex.get("scale", 0.0), graph=ex.get("graph"), nbest=NBEST)
                runs = twin_batch(oras[which], enc, beam, lodr=lodr, lscale=ls, **kw)[4]
                ok, g = fc.accepted(runs)
                if ok:
                    moved = moved_streams(runs, twin_batch(oras[which], enc, beam, **kw)[4])
                    print(f"    {label}: ({base}, {seed}, {ls}, {g:.4g}, {moved}),", flush=True)
                    return
            print(f"# no draw for {label}", flush=True)

        if what == "seeds":
            for name in ([sys.argv[2]] if len(sys.argv) > 2 else LMS):
                for beam in ([int(sys.argv[3])] if len(sys.argv) > 3 else BEAMS):
                    search(name, beam, lambda o, e: {}, f'("{name}", {beam})')
        else:
            for w in ([sys.argv[2]] if len(sys.argv) > 2 else ("hotwords", "ngram")):
                search("A", 4, lambda o, e, w=w: fc.together_extras(o, e, w), f'"{w}"')
