"""Cost of decoding a long recording by segment, by leg.

    python tools/vad_bench.py [preset] [minutes]   (defaults: zipformer2-large-en 10)

A synthetic recording of `minutes` minutes -- utterances of 3 to 12 s between pauses of 0.4 to 2 s of low noise -- is decoded with
Model.recognize_long (max_speech 2000 frames, batches of at most 32 segments and 32000 frames).  Per round the host milliseconds of its
three legs (k2hip_debug_long_timing): fbank over the whole recording with its upload, the detector with its flush, the batches; the
medians over the rounds, the segment and batch counts, and the real-time factor.  As far as the recording still fits in one row of the
offline path, the same recording is also decoded as ONE row with offline_greedy_from_samples and timed next to it (attention weights
grow with the square of the row: that leg is skipped, and named as skipped, once the call fails for lack of memory or beyond
--one-row-minutes, default 10).  One JSON line on stdout.  There is no time gate.  The legs are host clocks around work that ends in
a synchronise; DESIGN.md "Voice activity detection and long recordings" has the one run taken so far."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from k2transducerasr_amd import K2HipError, Model  # noqa: E402
from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model  # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
preset = argv[0] if len(argv) > 0 else "zipformer2-large-en"
minutes = float(argv[1]) if len(argv) > 1 else 10.0
one_row_minutes = float(opts.get("one-row-minutes", 10.0))
ROUNDS, WARMUP = 5, 1


def recording(seconds, rate=16000, seed=1):
    rng = np.random.default_rng(seed)
    parts, have, u = [], 0, 0
    while have < seconds * rate:
        gap = (1e-3 * rng.standard_normal(int(rng.uniform(0.4, 2.0) * rate))).astype(np.float32)
        utt = synth_utterance(1000 + u, float(rng.uniform(3.0, 12.0)), rate)
        parts += [gap, utt]
        have += len(gap) + len(utt)
        u += 1
    return np.concatenate(parts)[: int(seconds * rate)]


def main():
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"{preset}.k2w")
        write_synthetic_model(path, preset)
        model = Model(path, 0)
        x = recording(60.0 * minutes)
        cfg = model.vad_default_config()
        legs, walls, res = [], [], []
        for i in range(WARMUP + ROUNDS):
            t0 = time.perf_counter()
            res = model.recognize_long(x, config=cfg, max_batch=32, max_batch_frames=32000)
            wall = (time.perf_counter() - t0) * 1e3
            if i >= WARMUP:
                walls.append(wall)
                legs.append(model.long_timing())
        med = lambda v: float(np.median(v))
        out = dict(tool="vad_bench", preset=preset, minutes=minutes, samples=int(x.size), rounds=ROUNDS,
                   segments=len(res), forced=sum(g["forced"] for g in res), batches=len({g["batch"] for g in res}),
                   speech_frames=sum(g["end"] - g["start"] for g in res), tokens=sum(len(g["tokens"]) for g in res),
                   long_ms=med(walls), fbank_ms=med([g["fbank_ms"] for g in legs]), vad_ms=med([g["vad_ms"] for g in legs]),
                   batches_ms=med([g["batches_ms"] for g in legs]))
        out["x_real_time"] = 60e3 * minutes / out["long_ms"]
        # the same recording as one row of the offline path, while it fits
        if minutes <= one_row_minutes:
            try:
                row = []
                for i in range(WARMUP + ROUNDS):
                    t0 = time.perf_counter()
                    got = model.offline_greedy_from_samples([x])
                    if i >= WARMUP:
                        row.append((time.perf_counter() - t0) * 1e3)
                out["one_row_ms"] = med(row)
                out["one_row_tokens"] = len(got[0][0])
            except K2HipError as e:
                out["one_row_ms"] = None
                out["one_row_skipped"] = f"the call failed: {e}"
        else:
            out["one_row_ms"] = None
            out["one_row_skipped"] = f"{minutes} minutes exceed --one-row-minutes={one_row_minutes}"
        model.close()
        print(json.dumps(out))


if __name__ == "__main__":
    main()
