"""The offline batch with the encoder's half-precision switch off and on (Model.set_encoder_precision; csrc/gemm_f16.hip).

    python tools/encoder_half_bench.py [preset] [batch] [seconds]      (defaults: zipformer2-large-en 32 10)

A batch of `batch` synthetic utterances of `seconds` seconds is decoded from samples (offline_greedy_from_samples) ROUNDS times with
the switch off and on, interleaved round by round in one process after WARMUP rounds of each: "off_ms" / "on_ms" are the medians of
the calls' total_ms (device events around the whole call), with their [min, max] spread, and encoder_ms beside them.  Then one
instrumented call each way (every GEMM launch bracketed by events): the launch logs have the same rows in the same order, and the rows
whose kind carries the f16 family's bit when the switch is on are the covered launches.  "shapes" lists them grouped by (M, N, K, act,
residual): launches per call, microseconds summed over them in float32 and in f16, and the f16 tile.  "covered_f32_ms" / "covered_f16_ms"
sum those, "gemm_f32_ms" / "gemm_on_ms" are all GEMM launches of the call.  "same_tokens" counts the utterances whose token lists are
identical off and on.  One JSON line on stdout; there is no time gate (DESIGN.md "Half-precision operands in the encoder's linear
layers" has the runs taken so far)."""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from k2transducerasr_amd import Model  # noqa: E402
from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model  # noqa: E402

argv = sys.argv[1:]
preset = argv[0] if len(argv) > 0 else "zipformer2-large-en"
batch = int(argv[1]) if len(argv) > 1 else 32
seconds = float(argv[2]) if len(argv) > 2 else 10.0
ROUNDS, WARMUP = 9, 2
F16_BIT = 1 << 21


def main():
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "m.k2w")
        write_synthetic_model(path, preset)
        model = Model(path, 0)
        utts = [synth_utterance(u, seconds) for u in range(batch)]
        total = {False: [], True: []}
        enc = {False: [], True: []}
        tokens = {}
        for r in range(WARMUP + ROUNDS):
            for half in (False, True):
                model.set_encoder_precision(half)
                tokens[half] = model.offline_greedy_from_samples(utts)
                t = model.timing()
                if r >= WARMUP:
                    total[half].append(t["total_ms"])
                    enc[half].append(t["encoder_ms"])
        prof = {}
        model.set_instrument(True)
        for half in (False, True):
            model.set_encoder_precision(half)
            model.offline_greedy_from_samples(utts)
            prof[half] = model.gemm_profile().copy()
        model.set_instrument(False)
        stats = model.encoder_f16_stats()
        model.set_encoder_precision(False)
        model.close()
    off, on = prof[False], prof[True]
    assert off.shape == on.shape and np.array_equal(off[:, :6], on[:, :6]), "the two launch logs do not line up"
    shapes = {}
    for a, b in zip(off, on):
        if not int(b[6]) & F16_BIT:
            continue
        key = tuple(int(v) for v in b[:3]) + (int(b[4]), int(b[5]))
        s = shapes.setdefault(key, dict(M=key[0], N=key[1], K=key[2], act=key[3], res=key[4], launches=0, f32_us=0.0, f16_us=0.0,
                                        tile=f"{(int(b[6]) >> 8 & 15) * 32}x{(int(b[6]) >> 12 & 15) * 32}"))
        s["launches"] += 1
        s["f32_us"] += float(a[7])
        s["f16_us"] += float(b[7])
    rows = sorted(shapes.values(), key=lambda s: -s["f32_us"])
    for s in rows:
        s["f32_us"], s["f16_us"] = round(s["f32_us"], 1), round(s["f16_us"], 1)
    spread = lambda v: [round(float(np.min(v)), 3), round(float(np.max(v)), 3)]   # noqa: E731
    print(json.dumps(dict(
        preset=preset, batch=batch, seconds=seconds, rounds=ROUNDS,
        off_ms=round(float(np.median(total[False])), 3), off_spread=spread(total[False]),
        on_ms=round(float(np.median(total[True])), 3), on_spread=spread(total[True]),
        off_encoder_ms=round(float(np.median(enc[False])), 3), on_encoder_ms=round(float(np.median(enc[True])), 3),
        gemm_f32_ms=round(float(off[:, 7].sum()) / 1e3, 3), gemm_on_ms=round(float(on[:, 7].sum()) / 1e3, 3),
        covered_launches=int(sum(s["launches"] for s in rows)),
        covered_f32_ms=round(sum(s["f32_us"] for s in rows) / 1e3, 3), covered_f16_ms=round(sum(s["f16_us"] for s in rows) / 1e3, 3),
        panels=stats["panels"], panel_bytes=stats["panel_bytes"],
        same_tokens=int(sum(a == b for a, b in zip(tokens[False], tokens[True]))), utterances=batch, shapes=rows)), flush=True)


if __name__ == "__main__":
    main()
