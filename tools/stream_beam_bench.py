"""Streaming tick under modified beam search next to greedy, on the same audio.

    python tools/stream_beam_bench.py [preset] [streams] [seconds] [beam] [--hotwords N] [--nbest N]   (defaults: zipformer2-streaming-zh 128 20 4)

N streams of the synthetic `preset` model each buffer an utterance of `seconds` s; the tool decodes all of them chunk by chunk
(one k2hip_online_step per tick over the whole group) once with greedy_search and once with modified_beam_search, reports the
median ms per tick of each, and holds the first few streams' beam results to the CPU oracle (k2o_modified_beam_search over the
oracle's own concatenated chunks; a difference is excused only where the oracle's margin at the first differing frame is below
LOGIT_TOL).  --hotwords N: two more beam runs with a hotword graph attached to EVERY stream -- an empty one (the biased kernels with
every bonus 0) and N phrases of 2 - 5 tokens drawn from the unbiased beam run's output (as tools/hotword_bench.py draws them) -- and a
second unbiased run behind them, their tick times printed beside the unbiased and the greedy one.  --nbest N: one more beam run with
Model.set_nbest(N) (alternatives and token log-probs kept per stream), its tick time beside the others and the results held equal to
the plain beam run's.  One JSON line on stdout."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from k2transducerasr_amd import OnlineRecognizer  # noqa: E402
from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model  # noqa: E402

argv = sys.argv[1:]
n_hotwords = None
if "--hotwords" in argv:
    i = argv.index("--hotwords")
    n_hotwords = int(argv[i + 1])
    del argv[i: i + 2]
n_best = None
if "--nbest" in argv:
    i = argv.index("--nbest")
    n_best = int(argv[i + 1])
    del argv[i: i + 2]
ngram_lm = "--ngram-lm" in argv      # also time the tick with a seeded trigram fused (tests/ngram_twin.draw_lm, scale 0.5)
if ngram_lm:
    argv.remove("--ngram-lm")
preset = argv[0] if len(argv) > 0 else "zipformer2-streaming-zh"
N = int(argv[1]) if len(argv) > 1 else 128
secs = float(argv[2]) if len(argv) > 2 else 20.0
beam = int(argv[3]) if len(argv) > 3 else 4
CHECK = 3
DISTINCT = 8


def run(rec, feats, method, k, hotwords=None):
    rec.model.set_decoding_method(method, k)
    hs = [rec.create_online_stream(hotwords=hotwords) for _ in feats]
    for h, f in zip(hs, feats):
        h.add_features(f)
    group = rec.batch(hs)
    ms = []
    while True:
        t0 = time.perf_counter()
        dec, _ = rec.get_results(group)
        dt = (time.perf_counter() - t0) * 1e3
        if not any(dec):
            break
        ms.append(dt)
    res = [(h.tokens[2:], h.timestamps) for h in hs]
    for h in hs:
        h.close()
    return ms, res


def main():
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"{preset}.k2w")
        write_synthetic_model(path, preset)
        rec = OnlineRecognizer(path)
        from oracle.online import OnlineOracle
        ora = OnlineOracle(path)
        base = [ora.fbank(synth_utterance(300 + u, secs)) for u in range(DISTINCT)]
        feats = [base[u % DISTINCT] for u in range(N)]
        run(rec, feats[: min(N, 8)], "greedy_search", 0)          # warm-up: arenas, decoder tables
        g_ms, _ = run(rec, feats, "greedy_search", 0)
        b_ms, b_res = run(rec, feats, "modified_beam_search", beam)
        hw_out = {}
        if n_hotwords is not None:
            from hotword_twin import SCORE, draw_phrases
            from k2transducerasr_amd import Hotwords
            V = rec.model.vocab_size
            phrases = draw_phrases(b_res[:DISTINCT], n_hotwords, np.random.default_rng(100), min_len=2, max_len=5)
            empty, full = Hotwords([], SCORE, V), Hotwords(phrases, SCORE, V)
            e_ms, e_res = run(rec, feats, "modified_beam_search", beam, empty)
            h_ms, h_res = run(rec, feats, "modified_beam_search", beam, full)
            b2_ms, _ = run(rec, feats, "modified_beam_search", beam)
            if e_res != b_res:
                raise SystemExit("an empty hotword graph changed the results")
            hw_out = {"hotword_phrases": len(phrases), "hotword_states": full.num_states,
                      "beam_empty_graph_ms_per_tick": round(float(np.median(e_ms)), 3),
                      "beam_hotwords_ms_per_tick": round(float(np.median(h_ms)), 3),
                      "beam_again_ms_per_tick": round(float(np.median(b2_ms)), 3),
                      "streams_moved_by_the_bias": int(sum(a != b for a, b in zip(h_res, b_res)))}
        if n_best is not None:
            rec.model.set_decoding_method("modified_beam_search", beam)
            rec.model.set_nbest(n_best)
            try:
                n_ms, n_res = run(rec, feats, "modified_beam_search", beam)
            finally:
                rec.model.set_nbest(1)
            if n_res != b_res:
                raise SystemExit("keeping the alternatives changed the results")
            hw_out["nbest"] = n_best
            hw_out["beam_nbest_ms_per_tick"] = round(float(np.median(n_ms)), 3)
        if ngram_lm:
            from k2transducerasr_amd import NgramLm
            from ngram_twin import draw_lm
            V = rec.model.vocab_size
            lm = NgramLm(draw_lm(b_res[:DISTINCT], V, np.random.default_rng(100), n_cut=300, n_random=2000, n_no_unigram=5), V)
            rec.model.set_ngram_lm(lm, 0.5)
            try:
                l_ms, l_res = run(rec, feats, "modified_beam_search", beam)
            finally:
                rec.model.set_ngram_lm(None)
            l2_ms, l2_res = run(rec, feats, "modified_beam_search", beam)
            if l2_res != b_res:
                raise SystemExit("a cleared LM changed the results")
            hw_out.update({"ngram_order": lm.order, "ngram_states": lm.num_states, "ngram_arcs": lm.num_arcs,
                           "beam_ngram_lm_ms_per_tick": round(float(np.median(l_ms)), 3),
                           "beam_no_lm_again_ms_per_tick": round(float(np.median(l2_ms)), 3),
                           "streams_moved_by_the_lm": int(sum(a != b for a, b in zip(l_res, b_res)))})
        import parity
        from test_online_beam_gpu import oracle_frames
        exact = excused = 0
        for u in range(min(CHECK, N)):
            enc, _ = oracle_frames(ora, base[u % DISTINCT])
            (want,), margins = ora.modified_beam_search(enc[None], beam, want_margins=True)
            got = b_res[u]
            if (list(got[0]), list(got[1])) == (want[0], want[1]):
                exact += 1
                continue
            t = min([a for a, (x, y) in enumerate(zip(got[1], want[1])) if x != y] + [min(len(got[1]), len(want[1]))])
            frame = want[1][t] if t < len(want[1]) else got[1][t]
            if margins[0, min(frame, margins.shape[1] - 1)] >= parity.LOGIT_TOL:
                raise SystemExit(f"stream {u}: beam result differs from the oracle at frame {frame} (margin {margins[0, frame]:.2e})")
            excused += 1
        # the first ticks include one-time work (pos-emb tables, arena growth): the median is the steady tick
        print(json.dumps({"preset": preset, "streams": N, "seconds": secs, "beam": beam, "ticks": len(b_ms),
                          "greedy_ms_per_tick": round(float(np.median(g_ms)), 3), "beam_ms_per_tick": round(float(np.median(b_ms)), 3),
                          "beam_over_greedy": round(float(np.median(b_ms) / np.median(g_ms)), 3),
                          "oracle_checked": min(CHECK, N), "oracle_exact": exact, "oracle_excused": excused, **hw_out}))


if __name__ == "__main__":
    main()
