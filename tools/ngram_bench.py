"""Cost of n-gram LM shallow fusion in the offline modified beam search, at configs[2]'s shape.

    python tools/ngram_bench.py [steps] [warmup]      (defaults: 20 5)

zipformer2-large-en (synthetic weights), beam 4, one batch of 32 x 10 s resident on the device, decoded through the fused
samples -> tokens entry in ONE process: no LM, a seeded trigram (n-grams cut from what the plain run emitted, random ones besides;
tests/ngram_twin.draw_lm) at scale 0.5, and no LM again.  Reports the median ms per batch of each, the spread of the no-LM legs, and
how many streams' results the LM changed.  One JSON line on stdout.  For the search kernel's own time run it under
`rocprofv3 --kernel-trace --stats` in a run of its own and read the k_beam_loop rows (the `true` instantiation is the fused one)."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from k2transducerasr_amd import Model, NgramLm  # noqa: E402
from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
B, SECS, BEAM, SCALE = 32, 10.0, 4, 0.5


def timed(m, ptr, n):
    for _ in range(warmup):
        res = m.offline_greedy_from_samples_dev(ptr, n, B)
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        res = m.offline_greedy_from_samples_dev(ptr, n, B)
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms)), res


def main():
    from ngram_twin import draw_lm
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "large.k2w")
        write_synthetic_model(path, "zipformer2-large-en")
        m = Model(path, 0)
        m.set_decoding_method("modified_beam_search", BEAM)
        s = np.stack([synth_utterance(u, SECS) for u in range(B)])
        ptr = m.device_alloc(s.nbytes)
        try:
            m.device_upload(ptr, s)
            none_ms, none_lo, none_hi, plain = timed(m, ptr, s.shape[1])
            entries = draw_lm(plain, m.vocab_size, np.random.default_rng(100), n_cut=300, n_random=2000, n_no_unigram=5)
            lm = NgramLm(entries, m.vocab_size)
            m.set_ngram_lm(lm, SCALE)
            lm_ms, lm_lo, lm_hi, fused = timed(m, ptr, s.shape[1])
            m.set_ngram_lm(None)
            again_ms, again_lo, again_hi, again = timed(m, ptr, s.shape[1])
            if again != plain:
                raise SystemExit("a cleared LM changed the results")
            print(json.dumps({"preset": "zipformer2-large-en", "B": B, "seconds": SECS, "beam": BEAM, "steps": steps, "order": lm.order,
                              "states": lm.num_states, "arcs": lm.num_arcs, "scale": SCALE,
                              "ms_no_lm": round(none_ms, 3), "ms_no_lm_min_max": [round(none_lo, 3), round(none_hi, 3)],
                              "ms_trigram": round(lm_ms, 3), "ms_trigram_min_max": [round(lm_lo, 3), round(lm_hi, 3)],
                              "ms_no_lm_again": round(again_ms, 3), "ms_no_lm_again_min_max": [round(again_lo, 3), round(again_hi, 3)],
                              "streams_changed": sum(a != b for a, b in zip(fused, plain))}))
        finally:
            m.device_free(ptr)
            m.close()


if __name__ == "__main__":
    main()
