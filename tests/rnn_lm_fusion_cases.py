"""The cases of the neural LM shallow fusion tests (test_rnn_lm_fusion.py on the CPU, test_rnn_lm_fusion_gpu.py on the device).

OPERATOR CASES.  Three short synthetic utterances (seeds base, base + 1, base + 2) through the tiny model's oracle encoder (V = 37
with LMs A and B of rnn_lm_cases.LMS, the V = 165 variant with LM C), beams 1, 2, 4, 8, with an N-best list of 4 and without, LM weight
SCALE.  A case is (LM name, beam, utterance base, LM seed); it is ACCEPTED when, on the twin (rnn_lm_fusion_twin.twin_beam_search,
N-best 4), every consecutive gap among the top beam + 1 candidates of every frame of every stream and every adjacent pair of final
normalised scores is at least parity.LOGIT_TOL.  The smallest gap of a case usually sits on a frame whose candidates all continue ONE
hypothesis, where the LM's term cancels -- so the draw has to vary the audio, not only the LM: SEEDS holds, per (LM name, beam), the FIRST
accepted pair in the order of draws() (utterance base 50, 53, 56 .., LM seeds 0 .. 3 under each), with the smallest gap found
(`python tests/rnn_lm_fusion_cases.py` prints the tables; test_rnn_lm_fusion.py re-checks acceptance, the recorded gap and that no
earlier draw is accepted -- of the FIRST_CHECKED draws in front of it, to keep that test quick -- on the CPU).  On an accepted case the device must equal the twin in tokens, timestamps and the number and
order of alternatives, with nothing excused.

THE SCORE BOUND.  A fused score is the search's own score plus the LM terms of its tokens.  The search's part: the tiny model's
joiner is dense, so the exact-tie construction's bound (beam_cases.score_bound, derived for a sparse planted joiner) does not carry
over, and a worst-case bound of a dense float32 joiner exceeds LOGIT_TOL over an utterance.  The bound is therefore taken from the
REFERENCE'S OWN ERROR, as rnn_lm_cases.E32 is: SCORE_E32 is the largest difference per frame, over every alternative of every operator,
together and wide case, between the float32 twin's score and the same search run in float64 (rnn_lm_fusion_twin.Oracle64: the decoder
and joiner restated in float64 numpy from the model's tensors; dtype = torch.float64), measured on the CPU; test_rnn_lm_fusion.py
re-measures it on the operator and together cases and holds it to this constant.  A score after T' frames gets 8 SCORE_E32 T': the device's own
error is of the twin's kind (another summation order, another libm), and the factor leaves room for both sides' errors adding up.  The LM part of
a hypothesis of n tokens gets scale n rnn_lm_cases.token_bound().  The acceptance rule then needs
    LOGIT_TOL >= 2 (8 SCORE_E32 T' + scale n_max token_bound())
for every operator and together case (T' = 20: 2 (1.76e-4 + 0.5 n_max 6.92e-6), about 4e-4), which test_rnn_lm_fusion.py asserts, and the
GPU tests hold every reported score to score_bound().  The wide case is gated by localised near-ties, not by this inequality; its
scores are held to the same formula at its own T'."""
import numpy as np

import parity
import rnn_lm_cases as lmc

STREAMS = 3
BEAMS = (1, 2, 4, 8)
NBEST = 4
SCALE = 0.5
SCORE_E32 = 1.1e-6        # per frame; measured 1.064e-06 (operator and together cases; the wide case 9.82e-07)
YP_TOL = 2e-5             # token log-probs (test_nbest_gpu.py's figure)
OPERATOR = {"A": "tiny", "B": "tiny", "C": "tiny165"}    # LM name -> model
UTT_SECONDS = (0.55, 0.7, 0.6)


REC_SECONDS = (0.7, 0.6, 0.8, 0.65, 0.75)


def utterances(base, seconds=UTT_SECONDS):
    from k2transducerasr_amd.synth import synth_utterance
    return [synth_utterance(base + u, s) for u, s in enumerate(seconds)]


FIRST_CHECKED = 24    # draws in front of a recorded one that test_rnn_lm_fusion.py re-checks as not accepted (all of them would take minutes)


def draws(limit=4000):
    """the order in which (utterance base, LM seed) pairs are tried"""
    return [(base, seed) for base in range(50, 50 + 3 * (limit // 4), 3) for seed in range(4)]


def score_bound(frames, n_tokens, scale=SCALE):
    """a reported score of a hypothesis of n_tokens tokens after `frames` frames, device against twin"""
    return 8 * SCORE_E32 * int(frames) + scale * max(int(n_tokens), 1) * lmc.token_bound()


# (LM name, beam) -> (utterance base, LM seed, smallest gap found on the twin) of the first accepted draw
SEEDS = {
    ("A", 1): (50, 0, 0.007618),
    ("A", 2): (50, 0, 0.002769),
    ("A", 4): (50, 0, 0.001705),
    ("A", 8): (176, 0, 0.00107),
    ("B", 1): (50, 0, 0.007618),
    ("B", 2): (50, 0, 0.002769),
    ("B", 4): (50, 0, 0.001705),
    ("B", 8): (77, 2, 0.001574),
    ("C", 1): (50, 0, 0.001553),
    ("C", 2): (50, 0, 0.003417),
    ("C", 4): (86, 1, 0.00293),
    ("C", 8): (1367, 3, 0.001125),     # (V = 165 at beam 8: nine candidates of one row rarely keep apart)
}

# hotwords / n-gram LM together with the neural LM: LM A at beam 4, one case each, accepted by the same rule
# what -> (utterance base, LM seed, smallest gap) of the first accepted draw
TOGETHER = {
    "hotwords": (50, 0, 0.001705),
    "ngram": (50, 0, 0.001266),
}

# The recognizer case: five utterances of REC_SECONDS (seeds base ..), the tiny model, LM A, beam 4, N-best 4.  The first draw (in the
# order of draws(), scales 0.5, 1, 2 under each) that is accepted AND whose fused result differs from both the plain search's and the
# rescored N-best list's top entry in at least half of the streams (3 of 5); recorded with that count and the smallest gap.
RECOGNIZER = dict(lm="A", beam=4, nbest=4, base=56, seed=0, scale=0.5, moved=5, gap=0.00148)

# The wide case: B = 32 streams of a 4 s utterance each through the tiny model, beam 4, LM A with seed 0.  With about a hundred frames
# per stream, more than half of all streams have SOME frame whose selection margin (rank beam against rank beam + 1) is below LOGIT_TOL
# whatever the LM's seed (18 to 20 of 32 for seeds 0 .. 17), because those margins sit between candidates of one hypothesis.  So the
# utterances are chosen instead: utt_seeds are the first 32 utterance seeds from 200 upwards whose stream has NO such frame on the twin
# (streams do not see each other), which leaves tight_streams = 0 of 32, inside the issue's "at most 2".
WIDE = dict(lm="A", beam=4, B=32, seconds=4.0, seed=0, utt_seeds=[206, 207, 210, 211, 217, 220, 221, 223, 225, 227, 230, 231, 232, 233, 239, 241, 242, 243, 245, 247, 249, 251, 253, 254,
                       255, 256, 260, 261, 262, 264, 269, 272], tight_streams=0)


def accepted(runs):
    """(ok, smallest gap) of a case's twin runs"""
    from rnn_lm_fusion_twin import case_gap
    g = min(case_gap(r) for r in runs)
    return g >= parity.LOGIT_TOL, g


# ---- what the CPU test and the search below share ------------------------------------------------------------------------------------
def make_lm(tmpdir, name, seed):
    """(path of the .k2w, FusionLm, Twin) of LM `name` drawn with `seed`"""
    import os
    from k2transducerasr_amd.synth import write_synthetic_rnn_lm
    from rnn_lm_fusion_twin import FusionLm
    from rnn_lm_twin import Twin
    V, E, H, L, _ = lmc.LMS[name]
    p = os.path.join(str(tmpdir), f"lm_{name}_{seed}.k2w")
    tw = Twin(write_synthetic_rnn_lm(p, V, E, H, L, seed), L)
    return p, FusionLm(tw), tw


def make_oracle(tmpdir, which):
    import os
    from k2transducerasr_amd.synth import write_synthetic_model
    from oracle import Oracle
    p = os.path.join(str(tmpdir), which + ".k2w")
    write_synthetic_model(p, "zipformer2-tiny-test", meta_overrides={"vocab_size": str(lmc.LMS["C"][0])} if which == "tiny165" else None)
    return p, Oracle(p)


def encode(ora, utts):
    f = [ora.fbank(u) for u in utts]
    return ora.encoder(ora.pad_sequence(f).reshape(len(utts), -1, 80))


def together_extras(ora, enc, what):
    """the hotword graph / n-gram LM of the TOGETHER cases, drawn from the plain search's output: dict(graph=, lm=, scale=, phrases=, entries=)"""
    from hotword_twin import SCORE, TwinGraph, draw_phrases
    from ngram_twin import SCALE as NG_SCALE, TwinLm, draw_lm
    plain = ora.modified_beam_search(enc, 4)
    if what == "hotwords":
        phrases = draw_phrases(plain, 6, np.random.default_rng(5))
        return dict(graph=TwinGraph(phrases, SCORE, ora.vocab_size), phrases=phrases, score=SCORE)
    entries = draw_lm(plain, ora.vocab_size, np.random.default_rng(1))
    return dict(lm=TwinLm(entries, ora.vocab_size), scale=NG_SCALE, entries=entries)


def wide_utterances():
    from k2transducerasr_amd.synth import synth_utterance
    return [synth_utterance(u, WIDE["seconds"]) for u in WIDE["utt_seeds"]]


def recognizer_views(ora, enc, nlm, tw, scale, beam=4, nbest=4):
    """per stream: (plain top, rescored top, fused top) token lists, and the fused twin runs"""
    from rnn_lm_fusion_twin import twin_batch
    from rnn_lm_twin import rescored_order
    _, _, _, _, plain = twin_batch(ora, enc, beam, nbest=nbest)
    _, _, _, _, fused = twin_batch(ora, enc, beam, nlm=nlm, nscale=scale, nbest=nbest)
    views = []
    for p, f in zip(plain, fused):
        al = p["alts"]
        order, _ = rescored_order([a["score"] for a in al], [len(a["tokens"]) for a in al], [tw.score(a["tokens"])[0] for a in al], scale, False)
        views.append((al[0]["tokens"], al[order[0]]["tokens"], f["alts"][0]["tokens"]))
    return views, fused


if __name__ == "__main__":   # the search that filled the tables above
    import sys
    import tempfile
    from k2transducerasr_amd.synth import synth_utterance
    from rnn_lm_fusion_twin import twin_batch, twin_beam_search
    only = sys.argv[1:] or ["seeds", "together", "recognizer", "wide"]
    with tempfile.TemporaryDirectory() as d:
        oras = {w: make_oracle(d, w)[1] for w in ("tiny", "tiny165")}
        encs = {}

        def enc_of(which, base, seconds=UTT_SECONDS):
            if (which, base, seconds) not in encs:
                encs[(which, base, seconds)] = encode(oras[which], utterances(base, seconds))
            return encs[(which, base, seconds)]

        if "seeds" in only:
            for name, which in OPERATOR.items():
                for beam in BEAMS:
                    for base, seed in draws():
                        _, nlm, _ = make_lm(d, name, seed)
                        ok, g = accepted(twin_batch(oras[which], enc_of(which, base), beam, nlm=nlm, nscale=SCALE, nbest=NBEST)[4])
                        if ok:
                            print(f'    ("{name}", {beam}): ({base}, {seed}, {g:.4g}),', flush=True)
                            break
                    else:
                        print(f"# no draw for {name} beam {beam}", flush=True)
        if "together" in only:
            for what in ("hotwords", "ngram"):
                for base, seed in draws():
                    ex = together_extras(oras["tiny"], enc_of("tiny", base), what)
                    _, nlm, _ = make_lm(d, "A", seed)
                    ok, g = accepted(twin_batch(oras["tiny"], enc_of("tiny", base), 4, nlm=nlm, nscale=SCALE, lm=ex.get("lm"), scale=ex.get("scale", 0.0),
                                                graph=ex.get("graph"), nbest=NBEST)[4])
                    if ok:
                        print(f'    "{what}": ({base}, {seed}, {g:.4g}),', flush=True)
                        break
        if "recognizer" in only:
            done = False
            for base, seed in draws():
                for scale in (0.5, 1.0, 2.0):
                    _, nlm, tw = make_lm(d, "A", seed)
                    views, fused = recognizer_views(oras["tiny"], enc_of("tiny", base, REC_SECONDS), nlm, tw, scale)
                    moved = sum(f != p and f != r for p, r, f in views)
                    ok, g = accepted(fused)
                    if ok and 2 * moved >= len(views):
                        print(f"RECOGNIZER base={base}, seed={seed}, scale={scale}, moved={moved}, gap={g:.4g}", flush=True)
                        done = True
                        break
                if done:
                    break
        if "wide" in only:
            _, nlm, _ = make_lm(d, "A", WIDE["seed"])
            found, u = [], 200
            while len(found) < WIDE["B"]:
                e = encode(oras["tiny"], [synth_utterance(u, WIDE["seconds"])])
                mg = twin_beam_search(oras["tiny"], e[0], 4, nlm=nlm, nscale=SCALE)["margins"]
                if float(mg[:-1].min()) >= parity.LOGIT_TOL:
                    found.append(u)
                u += 1
            print(f"WIDE utt_seeds={found}", flush=True)
