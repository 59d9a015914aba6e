"""Time of the streaming tick of a CTC model with the carried prefix beam search at beam 4 and 8, next to its greedy tick.

    python tools/stream_ctc_prefix_bench.py [--hotwords N] [--ngram-lm] [preset] [streams] [seconds] [warmup]
                                                                                    (defaults: zipformer2-ctc-streaming-tiny-test 32 12 3)

Three groups of `streams` streams in ONE recognizer, fed the same features: greedy (the per-chunk collapse), ctc_prefix_beam = 4 and = 8
(nbest = beam).  Every round ticks each group once (k2hip_online_step over the whole group), so the three are interleaved and see the
same clocks; the first `warmup` rounds size the arenas and are dropped.  Prints the median wall ms per tick and, from the engine's own
events of the ticks, the median encoder leg and search leg (k2hip_get_timing: greedy_ms is the leg behind the encoder, whatever ran
there).  The search is latency-bound -- one workgroup per stream, three barriers per frame, T' frames -- so the figure to read is the
search leg against the whole tick.  --hotwords N (every biased stream gets its own graph of N seeded phrases of 2 - 3 tokens, score 1.5)
and / or --ngram-lm (the model gets a seeded bigram LM over the whole vocabulary, scale 0.5) add two more groups, beam 4 and 8 with the
streams' biasing switch on (OnlineStream.set_ctc_prefix_biasing), interleaved with the unbiased groups: the same tick once more
through the biased kernel.  One JSON line on stdout.  There is no time gate."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from k2transducerasr_amd import Hotwords, NgramLm, OnlineRecognizer  # noqa: E402
from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model  # noqa: E402

argv = sys.argv[1:]
n_hotwords, with_lm = 0, False
if "--hotwords" in argv:
    i = argv.index("--hotwords")
    n_hotwords = int(argv[i + 1])
    del argv[i: i + 2]
if "--ngram-lm" in argv:
    argv.remove("--ngram-lm")
    with_lm = True
preset = argv[0] if len(argv) > 0 else "zipformer2-ctc-streaming-tiny-test"
B = int(argv[1]) if len(argv) > 1 else 32
secs = float(argv[2]) if len(argv) > 2 else 12.0
warmup = int(argv[3]) if len(argv) > 3 else 3

GROUPS = {"greedy": 0, "beam4": 4, "beam8": 8}
BIASED = {"beam4_biased": 4, "beam8_biased": 8} if n_hotwords or with_lm else {}
GROUPS.update(BIASED)


def seeded_phrases(n, V, seed):
    rng = np.random.default_rng(seed)
    out, heads = [], set()
    while len(out) < n:          # (no phrase a prefix of another: distinct first two tokens)
        ph = [int(v) for v in rng.integers(3, V, size=int(rng.integers(2, 4)))]
        if tuple(ph[:2]) not in heads:
            heads.add(tuple(ph[:2]))
            out.append(ph)
    return out


def seeded_lm(V, seed=5):
    rng = np.random.default_rng(seed)
    ent = [((-1,), -99.0, -0.5), ((-3,), -7.5, 0.0)] + [((v,), float(-2.0 - 3.0 * rng.random()), -0.25) for v in range(3, V)]
    pairs = {(int(a), int(b)) for a, b in rng.integers(3, V, size=(8 * V, 2))}
    return NgramLm(ent + [(p, float(-0.25 - 1.5 * rng.random()), 0.0) for p in sorted(pairs)], V)


def main():
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"{preset}.k2w")
        write_synthetic_model(path, preset)
        rec = OnlineRecognizer(path)
        if rec.model.meta("model_type") != "zipformer2ctc":
            raise SystemExit(f"{preset} is not a CTC model")
        feats = [np.ascontiguousarray(rec.model.fbank(synth_utterance(700 + u % 8, secs)), np.float32) for u in range(min(B, 8))]
        V = rec.model.vocab_size
        if with_lm:
            rec.model.set_ngram_lm(seeded_lm(V), 0.5)     # (before any tick: the biased streams start with it; the others never look)
        groups = {k: [rec.create_online_stream(ctc_prefix_beam=beam, nbest=max(beam, 1), ctc_prefix_biasing=k in BIASED,
                                               hotwords=seeded_phrases(n_hotwords, V, 100 + u) if k in BIASED and n_hotwords else None)
                      for u in range(B)] for k, beam in GROUPS.items()}
        try:
            for g in groups.values():
                for u, s in enumerate(g):
                    s.add_features(feats[u % len(feats)])
            batches = {k: rec.batch(g) for k, g in groups.items()}
            wall = {k: [] for k in GROUPS}
            enc = {k: [] for k in GROUPS}
            search = {k: [] for k in GROUPS}
            rounds = 0
            while True:
                decoded = 0
                for k in GROUPS:
                    t0 = time.perf_counter()
                    dec, _ = rec.get_results(batches[k])
                    ms = (time.perf_counter() - t0) * 1e3
                    decoded += sum(dec)
                    if sum(dec) == B and rounds >= warmup:
                        t = rec.model.timing()
                        wall[k].append(ms)
                        enc[k].append(t["encoder_ms"])
                        search[k].append(t["greedy_ms"])
                if decoded == 0:
                    break
                rounds += 1
            if min(len(v) for v in wall.values()) < 5:
                raise SystemExit(f"only {rounds} rounds: feed more seconds")
            out = {"preset": preset, "streams": B, "seconds": secs, "frames_per_chunk": rec.frames_per_chunk, "ticks_timed": len(wall["greedy"]), "hotwords": n_hotwords, "ngram_lm": with_lm,
                   "mean_tokens": {k: round(float(np.mean([len(s.tokens) - 2 for s in g])), 1) for k, g in groups.items()}}
            for k in GROUPS:
                out[f"{k}_tick_wall_ms"] = round(float(np.median(wall[k])), 3)
                out[f"{k}_encoder_ms"] = round(float(np.median(enc[k])), 3)
                out[f"{k}_search_ms"] = round(float(np.median(search[k])), 3)
            for k in [g for g in GROUPS if g != "greedy"]:
                if not all(np.isfinite(s.score) for s in groups[k]) or any(any(a >= b for a, b in zip(s.timestamps, s.timestamps[1:])) for s in groups[k]):
                    raise SystemExit(f"{k}: malformed result")
            print(json.dumps(out))
        finally:
            for g in groups.values():
                for s in g:
                    s.close()
            rec.model.close()


if __name__ == "__main__":
    main()
