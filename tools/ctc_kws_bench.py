"""Time of the CTC keyword spotter's chunk call next to the greedy streaming tick of the same streams.

    python tools/ctc_kws_bench.py [preset] [streams] [seconds] [--states N] [--vocab V]
                                                      (defaults: zipformer2-ctc-streaming-tiny-test 128 20; states 20, 100 and 400)

N streams of the synthetic streaming CTC `preset` each buffer an utterance of `seconds` s and are decoded chunk by chunk with the greedy
collapse (one k2hip_online_step per tick over the whole group).  For every trie size, N CTC keyword streams on one graph of random
three-token keywords take one CtcKeywordStream.search_chunk call over host log-probs [N, T', V] of the tick's shape (a log-softmax of
seeded normal values: the cost depends on them only through the number of events).  Every round runs the greedy tick and then one chunk
call per trie size, so all of them are interleaved and see the same clocks; the first rounds size the arenas and are dropped.  Prints
the median wall ms of each and the events found.  The chunk call includes the upload of the chunk's log-probs and of the graph's tables
and the download of the events and carried blocks.  --vocab V writes the preset with that vocabulary size.  One JSON line on stdout.
There is no time gate."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from k2transducerasr_amd import CtcKeywordStream, Keywords, OnlineRecognizer  # noqa: E402
from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model  # noqa: E402

argv = sys.argv[1:]
sizes, vocab = [20, 100, 400], None
if "--states" in argv:
    i = argv.index("--states")
    sizes = [int(argv[i + 1])]
    del argv[i: i + 2]
if "--vocab" in argv:
    i = argv.index("--vocab")
    vocab = int(argv[i + 1])
    del argv[i: i + 2]
preset = argv[0] if len(argv) > 0 else "zipformer2-ctc-streaming-tiny-test"
N = int(argv[1]) if len(argv) > 1 else 128
secs = float(argv[2]) if len(argv) > 2 else 20.0
DISTINCT, WARMUP = 8, 3


def main():
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"{preset}.k2w")
        write_synthetic_model(path, preset, meta_overrides={"vocab_size": str(vocab)} if vocab else None)
        rec = OnlineRecognizer(path)
        model = rec.model
        if model.meta("model_type") != "zipformer2ctc":
            raise SystemExit(f"{preset} is not a CTC model")
        base = [model.fbank(synth_utterance(300 + u, secs)) for u in range(DISTINCT)]
        hs = [rec.create_online_stream() for _ in range(N)]
        for u, h in enumerate(hs):
            h.add_features(base[u % DISTINCT])
        group = rec.batch(hs)
        Tc, V = rec.frames_per_chunk, model.vocab_size
        rng = np.random.default_rng(9)
        x = 2.0 * rng.standard_normal((N, Tc, V))
        lp = (x - np.log(np.exp(x).sum(axis=2, keepdims=True))).astype(np.float32)
        graphs, streams = {}, {}
        for want in sizes:
            words, prefixes = set(), set()   # (a small vocabulary shares prefixes: count the trie's states, not the words)
            while len(prefixes) + 1 < want - 1:
                w = tuple(int(v) for v in rng.integers(3, V, size=3))
                words.add(w)
                prefixes.update(w[:k] for k in (1, 2, 3))
            kw = Keywords(sorted(words), 0.35, V)
            graphs[want] = kw
            streams[want] = [CtcKeywordStream(model, kw) for _ in range(N)]
        g_ms, k_ms = [], {want: [] for want in sizes}
        rounds = 0
        while True:
            t0 = time.perf_counter()
            dec, _ = rec.get_results(group)
            dt = (time.perf_counter() - t0) * 1e3
            if not any(dec):
                break
            timed = rounds >= WARMUP and all(dec)
            if timed:
                g_ms.append(dt)
            for want in sizes:
                t0 = time.perf_counter()
                CtcKeywordStream.search_chunk(streams[want], lp)
                if timed:
                    k_ms[want].append((time.perf_counter() - t0) * 1e3)
            rounds += 1
        if len(g_ms) < 5:
            raise SystemExit(f"only {rounds} rounds: feed more seconds")
        out = {"preset": preset, "streams": N, "seconds": secs, "ticks_timed": len(g_ms), "chunk_frames": Tc, "vocab_size": V,
               "greedy_ms_per_tick": round(float(np.median(g_ms)), 3)}
        for want in sizes:
            S = graphs[want].num_states
            out[f"ctc_kws_S{S}_ms_per_chunk"] = round(float(np.median(k_ms[want])), 3)
            out[f"ctc_kws_S{S}_events"] = sum(len(s.events()) for s in streams[want])
            for s in streams[want]:
                s.close()
        for h in hs:
            h.close()
        print(json.dumps(out))


if __name__ == "__main__":
    main()
