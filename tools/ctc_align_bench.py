"""Time of the CTC forced alignment / full-sum scoring of one offline batch, next to the CTC greedy call of the same batch.

    python tools/ctc_align_bench.py [preset] [batch] [seconds] [repeats]   (defaults: zipformer2-ctc-tiny-test 32 10 8)

The targets are the greedy result of the same batch (so every target has an alignment and a realistic length).  Two calls from host
samples, `repeats` times each, interleaved: offline_greedy_from_samples (the CTC first-argmax and collapse) and ctc_align_samples.
Prints the median wall ms per call and, from the engine's own events of the last call of each kind, the encoder leg and the search /
align leg (k2hip_get_timing: greedy_ms is the leg behind the encoder, whatever ran there).  One JSON line on stdout.  There is no time
gate."""
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


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"{preset}.k2w")
        write_synthetic_model(path, preset)
        model = Model(path, 0)
        if model.meta("model_type") != "zipformer2ctc":
            raise SystemExit(f"{preset} is not a CTC model")
        utts = [synth_utterance(500 + u % 8, secs) for u in range(B)]
        greedy = model.offline_greedy_from_samples(utts)
        targets = [np.array(tok, np.int64) for tok, _ in greedy]
        model.ctc_align_samples(utts, targets)   # (warm: arenas sized)
        wall = dict(greedy=[], align=[])
        legs = {}
        for _ in range(repeats):
            ms, _ = timed(lambda: model.offline_greedy_from_samples(utts))
            wall["greedy"].append(ms)
            legs["greedy"] = model.timing()
            ms, res = timed(lambda: model.ctc_align_samples(utts, targets))
            wall["align"].append(ms)
            legs["align"] = model.timing()
        for r, t in zip(res, targets):
            ts, en = r["timestamps"], r["end_frames"]
            if len(ts) != t.size or not all(a <= e for a, e in zip(ts, en)) or not all(e < a for e, a in zip(en, ts[1:])):
                raise SystemExit("ctc_align_samples returned a malformed alignment")
            if not r["best_logp"] <= r["total_logp"]:
                raise SystemExit("best_logp exceeds total_logp")
        out = {"preset": preset, "batch": B, "seconds": secs, "repeats": repeats,
               "mean_target_tokens": round(float(np.mean([t.size for t in targets])), 1)}
        for k in wall:
            out[f"{k}_wall_ms"] = round(float(np.median(wall[k])), 3)
            out[f"{k}_encoder_ms"] = round(float(legs[k]["encoder_ms"]), 3)
            out[f"{k}_search_ms"] = round(float(legs[k]["greedy_ms"]), 3)
        print(json.dumps(out))
        model.close()


if __name__ == "__main__":
    main()
