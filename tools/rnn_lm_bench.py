"""Cost of rescoring a batch's N-best lists with a neural LM, by leg.

    python tools/rnn_lm_bench.py [preset] [batch] [seconds] [--lm=LxH ...]   (defaults: zipformer2-large-en 32 10, --lm=3x2048 --lm=2x512)

A batch of `batch` synthetic utterances of `seconds` seconds is decoded with modified beam search, beam 4, N-best 4
(OfflineRecognizer.get_results: the median wall milliseconds over the rounds is the leg the rescoring sits next to).  Its alternatives --
batch x 4 hypotheses, fewer where a stream kept fewer -- are then scored by synthetic LMs of L layers of width H (embedding H, the
model's vocabulary) through Model.rnn_lm_score with the leg timing on (k2hip_debug_rnn_lm_timing: events at the legs' borders): median
milliseconds of embed, GX (the time-parallel input products through the GEMM launcher), steps (one fused launch per layer and
position) and score (the output sweep and the totals), and of the whole call on the host clock.  The same tool times ONE recurrent
step at the call's widest shape (rows = the hypothesis count, H) both ways (k2hip_debug_rnn_lm_step_bench): the fused kernel, and the
step composed from the GEMM launcher and the cell kernel as the LSTM encoder's lstm_layer does.  One JSON line on stdout.  There is no
time gate: DESIGN.md "Neural LM rescoring" has the runs taken so far."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from k2transducerasr_amd import OfflineRecognizer, RnnLm  # noqa: E402
from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model, write_synthetic_rnn_lm  # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
lms = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--lm=")] or ["3x2048", "2x512"]
preset = argv[0] if len(argv) > 0 else "zipformer2-large-en"
batch = int(argv[1]) if len(argv) > 1 else 32
seconds = float(argv[2]) if len(argv) > 2 else 10.0
ROUNDS, WARMUP = 7, 2


def med(v):
    return float(np.median(v))


def main():
    out = dict(preset=preset, batch=batch, seconds=seconds, rounds=ROUNDS)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"{preset}.k2w")
        write_synthetic_model(path, preset)
        rec = OfflineRecognizer(path, 0, "modified_beam_search", 4, nbest=4)
        utts = [synth_utterance(u, seconds) for u in range(batch)]
        walls, hyps = [], []
        for i in range(WARMUP + ROUNDS):
            ss = [rec.create_offline_stream() for _ in utts]
            for s, u in zip(ss, utts):
                s.add_samples(u)
            t0 = time.perf_counter()
            rec.get_results(ss)
            if i >= WARMUP:
                walls.append((time.perf_counter() - t0) * 1e3)
            hyps = [a["tokens"] for s in ss for a in s.alternatives()]
            for s in ss:
                s.close()
        out.update(get_results_beam4_ms=med(walls), hypotheses=len(hyps), positions=sum(len(h) + 1 for h in hyps), longest=max(len(h) for h in hyps))
        V = rec.model.vocab_size
        out["lms"] = []
        for spec in lms:
            L, H = (int(x) for x in spec.split("x"))
            lp = os.path.join(d, f"lm_{spec}.k2w")
            write_synthetic_rnn_lm(lp, V, H, H, L, 1)
            lm = RnnLm(lp)
            rec.model.set_rnn_lm(lm, 0.0)
            lm.close()
            rec.model.rnn_lm_timing(True)
            legs, calls = [], []
            for i in range(WARMUP + ROUNDS):
                t0 = time.perf_counter()
                rec.model.rnn_lm_score(hyps, True)
                wall = (time.perf_counter() - t0) * 1e3
                if i >= WARMUP:
                    calls.append(wall)
                    legs.append(rec.model.rnn_lm_timing(True))
            rec.model.rnn_lm_timing(False)
            step = rec.model.rnn_lm_step_bench(len(hyps), H, 200)
            out["lms"].append(dict(lm=spec, call_ms=med(calls), **{k: med([g[k] for g in legs]) for k in legs[0]},
                                   step_fused_ms=step["fused_ms"], step_composed_ms=step["composed_ms"], step_rows=len(hyps), step_launches=200))
            rec.model.set_rnn_lm(None)
        rec.model.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
