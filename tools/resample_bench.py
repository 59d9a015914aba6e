"""Cost of feeding an offline batch at another sample rate, in the synchronous GetResults call shape.

    python tools/resample_bench.py [preset] [batch] [seconds]   (defaults: zipformer2-large-en 32 10)

One batch of `batch` synthetic utterances of `seconds` s is decoded with B x (create stream, feed, destroy) around one
OfflineRecognizer.get_results call, as bench.py's `value_sync_get_results` leg does.  The same audio is fed at 16 kHz through add_samples
(today's path) and, synthesised at 8, 44.1 and 48 kHz, through accept_waveform; the four legs are interleaved round by round so that
clock and cache state are shared.  Per leg: the median wall ms of the whole round (feeding included: the 48 kHz leg copies three times the
samples into the pinned queues), the median ms of the get_results call alone, and the median of the engine's front-end leg (timing()'s
fbank_ms: the table upload, the gather or the resampling gather over PCIe, and the fbank).  One JSON line on stdout.  There is no
time gate."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from k2transducerasr_amd import OfflineRecognizer  # noqa: E402
from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model  # noqa: E402

argv = sys.argv[1:]
preset = argv[0] if len(argv) > 0 else "zipformer2-large-en"
B = int(argv[1]) if len(argv) > 1 else 32
secs = float(argv[2]) if len(argv) > 2 else 10.0
RATES = (16000, 8000, 44100, 48000)
ROUNDS, WARMUP = 12, 3


def one_round(rec, rate, utts):
    t0 = time.perf_counter()
    ss = []
    for x in utts:
        s = rec.create_offline_stream()
        s.add_samples(x) if rate == 16000 else s.accept_waveform(rate, x)
        ss.append(s)
    t1 = time.perf_counter()
    res = rec.get_results(ss)
    t2 = time.perf_counter()
    fb = rec.model.timing()["fbank_ms"]
    for s in ss:
        s.close()
    t3 = time.perf_counter()
    return (t3 - t0) * 1e3, (t2 - t1) * 1e3, fb, sum(len(t) for t, _ in res)


def main():
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"{preset}.k2w")
        write_synthetic_model(path, preset)
        rec = OfflineRecognizer(path)
        utts = {r: [synth_utterance(u, secs, sample_rate=r) for u in range(B)] for r in RATES}
        legs = {r: [] for r in RATES}
        for i in range(WARMUP + ROUNDS):
            for r in RATES:
                got = one_round(rec, r, utts[r])
                if i >= WARMUP:
                    legs[r].append(got)
        out = {"preset": preset, "batch": B, "seconds": secs, "rounds": ROUNDS, "legs": {}}
        for r in RATES:
            a = np.array([g[:3] for g in legs[r]])
            out["legs"][str(r)] = {"round_ms": round(float(np.median(a[:, 0])), 3), "get_results_ms": round(float(np.median(a[:, 1])), 3),
                                   "front_end_ms": round(float(np.median(a[:, 2])), 3), "tokens": legs[r][0][3],
                                   "input_mb": round(sum(x.nbytes for x in utts[r]) / 1e6, 2)}
        print(json.dumps(out))


if __name__ == "__main__":
    main()
