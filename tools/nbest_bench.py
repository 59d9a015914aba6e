"""Offline batch time of the modified beam search with the N-best list off and on.

    python tools/nbest_bench.py [preset] [batch] [seconds] [beam] [nbest] [repeats]   (defaults: the bench.py preset, 32 10 4 4 12)

One GetResults batch of synthetic utterances through OfflineRecognizer, `repeats` times each way, interleaved; prints the median ms per
batch with Model.set_nbest(1) and with set_nbest(nbest), and checks that the results are the same and that entry 0 of every stream's
alternatives is its result.  One JSON line on stdout."""
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
beam = int(argv[3]) if len(argv) > 3 else 4
nbest = int(argv[4]) if len(argv) > 4 else 4
repeats = int(argv[5]) if len(argv) > 5 else 12


def batch(rec, utts):
    ss = [rec.create_offline_stream() for _ in utts]
    for s, u in zip(ss, utts):
        s.add_samples(u)
    t0 = time.perf_counter()
    res = rec.get_results(ss)
    ms = (time.perf_counter() - t0) * 1e3
    alts = [s.alternatives() for s in ss]
    for s in ss:
        s.close()
    return ms, res, alts


def main():
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"{preset}.k2w")
        write_synthetic_model(path, preset)
        rec = OfflineRecognizer(path, 0, "modified_beam_search", beam)
        utts = [synth_utterance(500 + u % 8, secs) for u in range(B)]
        batch(rec, utts)
        off, on = [], []
        for _ in range(repeats):
            rec.model.set_nbest(1)
            ms, res, _ = batch(rec, utts)
            off.append(ms)
            rec.model.set_nbest(nbest)
            ms, res_n, alts = batch(rec, utts)
            on.append(ms)
            if res_n != res:
                raise SystemExit("keeping the alternatives changed the results")
            for (tok, ts), a in zip(res, alts):
                if a[0]["tokens"] != tok[2 * B:] or a[0]["timestamps"] != ts[2 * B:]:
                    raise SystemExit("entry 0 of the alternatives is not the result")
        print(json.dumps({"preset": preset, "batch": B, "seconds": secs, "beam": beam, "nbest": nbest, "repeats": repeats,
                          "off_ms_per_batch": round(float(np.median(off)), 3), "off_min_max": [round(min(off), 3), round(max(off), 3)],
                          "on_ms_per_batch": round(float(np.median(on)), 3), "on_min_max": [round(min(on), 3), round(max(on), 3)],
                          "mean_alternatives": round(float(np.mean([len(a) for a in alts])), 2)}))


if __name__ == "__main__":
    main()
