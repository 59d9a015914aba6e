"""Time of the CTC prefix beam search of one offline batch at beam 4 and 8, next to the CTC greedy call of the same batch.

    python tools/ctc_prefix_bench.py [preset] [batch] [seconds] [repeats]   (defaults: zipformer2-ctc-tiny-test 32 10 8)

Three calls from host samples, `repeats` times each, interleaved: offline_greedy_from_samples under greedy_search (the CTC first-argmax
and collapse) and under ctc_prefix_beam_search with beam 4 and beam 8.  Prints the median wall ms per call and, from the engine's own
events of the last call of each kind, the encoder leg and the search leg (k2hip_get_timing: greedy_ms is the leg behind the encoder,
whatever ran there; under the prefix search it holds the search and the collapse that keeps NumTrailingBlank).  One JSON line on
stdout.  There is no time gate."""
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
preset = argv[0] if len(argv) > 0 else "zipformer2-ctc-tiny-test"
B = int(argv[1]) if len(argv) > 1 else 32
secs = float(argv[2]) if len(argv) > 2 else 10.0
repeats = int(argv[3]) if len(argv) > 3 else 8

METHODS = {"greedy": ("greedy_search", 0), "beam4": ("ctc_prefix_beam_search", 4), "beam8": ("ctc_prefix_beam_search", 8)}


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
            t0 = time.perf_counter()
            out = model.offline_greedy_from_samples(utts)
            return (time.perf_counter() - t0) * 1e3, out

        res = {k: run(k)[1] for k in METHODS}   # (warm: arenas sized)
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
        for k in ("beam4", "beam8"):
            if not np.all(np.isfinite(scores[k])) or any(any(a >= b for a, b in zip(ts, ts[1:])) for _, ts in res[k]):
                raise SystemExit(f"{k}: malformed result")
        out = {"preset": preset, "batch": B, "seconds": secs, "repeats": repeats,
               "mean_tokens": {k: round(float(np.mean([len(tok) for tok, _ in res[k]])), 1) for k in METHODS},
               "streams_equal_to_greedy": {k: int(sum(a == b for a, b in zip(res[k], res["greedy"]))) for k in ("beam4", "beam8")}}
        for k in METHODS:
            out[f"{k}_wall_ms"] = round(float(np.median(wall[k])), 3)
            out[f"{k}_encoder_ms"] = round(float(legs[k]["encoder_ms"]), 3)
            out[f"{k}_search_ms"] = round(float(legs[k]["greedy_ms"]), 3)
        print(json.dumps(out))
        model.close()


if __name__ == "__main__":
    main()
