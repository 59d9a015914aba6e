"""Time of the CTC prefix beam search of one offline batch at beam 4 and 8, next to the CTC greedy call of the same batch.

    python tools/ctc_prefix_bench.py [preset] [batch] [seconds] [repeats] [--hotwords N] [--ngram-lm]
                                                                            (defaults: zipformer2-ctc-tiny-test 32 10 8)

Three calls from host samples, `repeats` times each, interleaved: offline_greedy_from_samples under greedy_search (the CTC first-argmax
and collapse) and under ctc_prefix_beam_search with beam 4 and beam 8.  Prints the median wall ms per call and, from the engine's own
events of the last call of each kind, the encoder leg and the search leg (k2hip_get_timing: greedy_ms is the leg behind the encoder,
whatever ran there; under the prefix search it holds the search and the collapse that keeps NumTrailingBlank).  One JSON line on
stdout.  There is no time gate.

--hotwords N sets a graph of N phrases (cut from the unbiased beam-4 results; N = 0: an empty graph) with score_per_token 1.5,
--ngram-lm a seeded trigram over the same results at scale 0.5; with either, the beam-4 / beam-8 call is timed once more with
k2hip_set_ctc_prefix_biasing on (beam4_biased / beam8_biased) beside today's figures, which run with the switch off over the same
tables."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from k2transducerasr_amd import Model  # noqa: E402
from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model  # noqa: E402

argv = sys.argv[1:]
n_hotwords, with_lm = None, False
if "--hotwords" in argv:
    i = argv.index("--hotwords")
    n_hotwords = int(argv[i + 1])
    del argv[i: i + 2]
if "--ngram-lm" in argv:
    argv.remove("--ngram-lm")
    with_lm = True
preset = argv[0] if len(argv) > 0 else "zipformer2-ctc-tiny-test"
B = int(argv[1]) if len(argv) > 1 else 32
secs = float(argv[2]) if len(argv) > 2 else 10.0
repeats = int(argv[3]) if len(argv) > 3 else 8

METHODS = {"greedy": ("greedy_search", 0), "beam4": ("ctc_prefix_beam_search", 4), "beam8": ("ctc_prefix_beam_search", 8)}


def draw_tables(results, V, n_phrases):
    """(phrases, LM entries) cut from the token sequences of `results`, seeded: phrases of 2 or 3 real tokens, none a prefix of
    another; unigrams for every real token, bigrams and trigrams that occur"""
    rng = np.random.default_rng(17)
    seqs = [[int(t) for t in tok] for tok, _ in results if len(tok) >= 3]
    phrases = []
    for _ in range(200 * max(n_phrases or 0, 1)):
        if len(phrases) >= (n_phrases or 0) or not seqs:
            break
        s = seqs[rng.integers(len(seqs))]
        n = int(rng.integers(2, 4))
        o = int(rng.integers(0, len(s) - n + 1))
        p = s[o: o + n]
        if 0 in p or 2 in p or any(p[: len(q)] == q or q[: len(p)] == p for q in phrases):
            continue
        phrases.append(p)
    ent = {(-1,): (-99.0, -0.5), (-3,): (-7.5, 0.0)}
    for v in range(V):
        if v not in (0, 2):
            ent[(v,)] = (float(rng.uniform(-6, -3)), float(rng.uniform(-1, -0.05)))
    for s in seqs:
        s = [v for v in s if v not in (0, 2)]
        for o in range(len(s) - 2):
            ent.setdefault(tuple(s[o: o + 2]), (float(rng.uniform(-1.5, -0.1)), float(rng.uniform(-1, -0.05))))
            ent.setdefault(tuple(s[o: o + 3]), (float(rng.uniform(-1.5, -0.1)), 0.0))
    return phrases, [(k, lp, bo) for k, (lp, bo) in sorted(ent.items(), key=lambda kv: (len(kv[0]), kv[0]))]


def main():
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"{preset}.k2w")
        write_synthetic_model(path, preset)
        model = Model(path, 0)
        if model.meta("model_type") != "zipformer2ctc":
            raise SystemExit(f"{preset} is not a CTC model")
        utts = [synth_utterance(500 + u % 8, secs) for u in range(B)]

        def run(kind):
            method, beam = METHODS[kind]
            model.set_decoding_method(method, beam)
            model.set_ctc_prefix_biasing(kind.endswith("_biased"))
            t0 = time.perf_counter()
            out = model.offline_greedy_from_samples(utts)
            return (time.perf_counter() - t0) * 1e3, out

        res = {k: run(k)[1] for k in METHODS}   # (warm: arenas sized)
        tables = {}
        if n_hotwords is not None or with_lm:
            from k2transducerasr_amd import Hotwords, NgramLm
            phrases, entries = draw_tables(res["beam4"], model.vocab_size, n_hotwords)
            if n_hotwords is not None:
                tables["hotwords"] = Hotwords(phrases, 1.5, model.vocab_size)
                model.set_hotwords(tables["hotwords"])
            if with_lm:
                tables["ngram_lm"] = NgramLm(entries, model.vocab_size)
                model.set_ngram_lm(tables["ngram_lm"], 0.5)
            METHODS.update(beam4_biased=("ctc_prefix_beam_search", 4), beam8_biased=("ctc_prefix_beam_search", 8))
            res.update({k: run(k)[1] for k in ("beam4_biased", "beam8_biased")})
        wall = {k: [] for k in METHODS}
        legs, scores = {}, {}
        for _ in range(repeats):
            for k in METHODS:
                ms, out = run(k)
                wall[k].append(ms)
                legs[k] = model.timing()
                if k != "greedy":
                    scores[k] = model.last_scores(B)
                if out != res[k]:
                    raise SystemExit(f"{k}: two calls on the same batch disagree")
        model.set_decoding_method("greedy_search")
        model.set_ctc_prefix_biasing(False)
        for k in [k for k in METHODS if k != "greedy"]:
            if not np.all(np.isfinite(scores[k])) or any(any(a >= b for a, b in zip(ts, ts[1:])) for _, ts in res[k]):
                raise SystemExit(f"{k}: malformed result")
        out = {"preset": preset, "batch": B, "seconds": secs, "repeats": repeats,
               "mean_tokens": {k: round(float(np.mean([len(tok) for tok, _ in res[k]])), 1) for k in METHODS},
               "streams_equal_to_greedy": {k: int(sum(a == b for a, b in zip(res[k], res["greedy"]))) for k in METHODS if k != "greedy"}}
        if tables:
            out["hotword_phrases"], out["ngram_lm"] = (len(phrases) if n_hotwords is not None else None), with_lm
            out["streams_moved_by_biasing"] = {k: int(sum(a != b for a, b in zip(res[k + "_biased"], res[k]))) for k in ("beam4", "beam8")}
        for k in METHODS:
            out[f"{k}_wall_ms"] = round(float(np.median(wall[k])), 3)
            out[f"{k}_encoder_ms"] = round(float(legs[k]["encoder_ms"]), 3)
            out[f"{k}_search_ms"] = round(float(legs[k]["greedy_ms"]), 3)
        print(json.dumps(out))
        model.close()


if __name__ == "__main__":
    main()
