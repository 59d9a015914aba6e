"""Time of the keyword spotter's chunk call next to the greedy streaming tick of the same streams.

    python tools/kws_bench.py [preset] [streams] [seconds] [--states N]   (defaults: zipformer2-streaming-zh 128 20; states 20, 100 and 400)

N streams of the synthetic `preset` model each buffer an utterance of `seconds` s and are decoded chunk by chunk with greedy_search
(one k2hip_online_step per tick over the whole group): the median ms per tick is the yardstick.  Then, for every trie size, N keyword
streams on one graph of random three-token keywords take one KeywordStream.search_chunk call per tick over a host encoder_out
[N, T', joiner_dim] of the tick's shape (seeded normal values: the cost does not depend on them); the median wall ms per call is
printed beside the greedy tick, with the events found.  The call includes the upload of the chunk's encoder_out and the download of the
events and carried blocks.  One JSON line on stdout.  There is no time gate."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from k2transducerasr_amd import Keywords, KeywordStream, OnlineRecognizer  # noqa: E402
from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model  # noqa: E402

argv = sys.argv[1:]
sizes = [20, 100, 400]
if "--states" in argv:
    i = argv.index("--states")
    sizes = [int(argv[i + 1])]
    del argv[i: i + 2]
preset = argv[0] if len(argv) > 0 else "zipformer2-streaming-zh"
N = int(argv[1]) if len(argv) > 1 else 128
secs = float(argv[2]) if len(argv) > 2 else 20.0
DISTINCT = 8


def greedy_ticks(rec, feats):
    rec.model.set_decoding_method("greedy_search", 0)
    hs = [rec.create_online_stream() for _ in feats]
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
    for h in hs:
        h.close()
    return ms


def main():
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"{preset}.k2w")
        write_synthetic_model(path, preset)
        rec = OnlineRecognizer(path)
        model = rec.model
        base = [model.fbank(synth_utterance(300 + u, secs)) for u in range(DISTINCT)]
        feats = [base[u % DISTINCT] for u in range(N)]
        greedy_ticks(rec, feats[: min(N, 8)])          # warm-up: arenas, decoder tables
        g_ms = greedy_ticks(rec, feats)
        ticks = len(g_ms)
        Tc = 16                                        # encoder frames per streaming chunk
        V, J = model.vocab_size, model.joiner_dim
        rng = np.random.default_rng(9)
        enc = (0.5 * rng.standard_normal((N, Tc, J))).astype(np.float32)
        out = {"preset": preset, "streams": N, "seconds": secs, "ticks": ticks, "chunk_frames": Tc, "vocab_size": V,
               "greedy_ms_per_tick": round(float(np.median(g_ms)), 3)}
        for want in sizes:
            words = set()
            while len(words) < max(1, (want - 1) // 3):
                words.add(tuple(int(x) for x in rng.integers(3, V, size=3)))
            kw = Keywords(sorted(words), 0.35, V)
            streams = [KeywordStream(model, kw) for _ in range(N)]
            KeywordStream.search_chunk(streams, enc)   # warm: the arena is sized
            ms = []
            for _ in range(max(ticks, 8)):
                t0 = time.perf_counter()
                KeywordStream.search_chunk(streams, enc)
                ms.append((time.perf_counter() - t0) * 1e3)
            events = sum(len(s.events()) for s in streams)
            out[f"kws_S{kw.num_states}_ms_per_chunk"] = round(float(np.median(ms)), 3)
            out[f"kws_S{kw.num_states}_events"] = events
            for s in streams:
                s.close()
        print(json.dumps(out))


if __name__ == "__main__":
    main()
