"""Cost of hotword biasing in the offline modified beam search, at configs[2]'s shape.

    python tools/hotword_bench.py [steps] [warmup]      (defaults: 20 5)

zipformer2-large-en (synthetic weights), beam 4, one batch of 32 x 10 s resident on the device, decoded through the fused
samples -> tokens entry three ways in ONE process: no hotwords, an empty list (the tables exist, every bonus is 0), and 100 phrases
of 2 - 5 tokens drawn from what the unbiased run emitted (so matches really occur).  Reports the median ms per batch of each and how
many streams' results the list changed.  One JSON line on stdout.  For the search kernel's own time run it under
`rocprofv3 --kernel-trace --stats` in a run of its own and read the k_beam_loop rows (the `true` instantiation is the biased one)."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from k2transducerasr_amd import Hotwords, Model  # noqa: E402
from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
B, SECS, BEAM, PHRASES, SCORE = 32, 10.0, 4, 100, 1.5


def timed(m, ptr, n):
    for _ in range(warmup):
        res = m.offline_greedy_from_samples_dev(ptr, n, B)
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        res = m.offline_greedy_from_samples_dev(ptr, n, B)
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), res


def main():
    from hotword_twin import draw_phrases
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "large.k2w")
        write_synthetic_model(path, "zipformer2-large-en")
        m = Model(path, 0)
        m.set_decoding_method("modified_beam_search", BEAM)
        s = np.stack([synth_utterance(u, SECS) for u in range(B)])
        ptr = m.device_alloc(s.nbytes)
        try:
            m.device_upload(ptr, s)
            none_ms, unbiased = timed(m, ptr, s.shape[1])
            m.set_hotwords(Hotwords([], SCORE, m.vocab_size))
            empty_ms, empty = timed(m, ptr, s.shape[1])
            phrases = draw_phrases(unbiased, PHRASES, np.random.default_rng(100), min_len=2, max_len=5)
            hw = Hotwords(phrases, SCORE, m.vocab_size)
            m.set_hotwords(hw)
            biased_ms, biased = timed(m, ptr, s.shape[1])
            m.set_hotwords(None)
            again_ms, again = timed(m, ptr, s.shape[1])
            if empty != unbiased or again != unbiased:
                raise SystemExit("an empty list / cleared hotwords changed the results")
            print(json.dumps({"preset": "zipformer2-large-en", "B": B, "seconds": SECS, "beam": BEAM, "steps": steps,
                              "phrases": len(phrases), "states": hw.num_states, "score_per_token": SCORE,
                              "ms_no_hotwords": round(none_ms, 3), "ms_empty_list": round(empty_ms, 3), "ms_100_phrases": round(biased_ms, 3),
                              "ms_no_hotwords_again": round(again_ms, 3),
                              "streams_changed": sum(a != b for a, b in zip(biased, unbiased))}))
        finally:
            m.device_free(ptr)
            m.close()


if __name__ == "__main__":
    main()
