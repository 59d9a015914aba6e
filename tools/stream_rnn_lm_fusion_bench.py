"""Cost of carrying a neural LM through the streaming modified beam search: the streaming tick four ways, interleaved.

    python tools/stream_rnn_lm_fusion_bench.py [preset] [streams] [seconds] [beam] [--lm=LxH ...] [--rounds N]
    (defaults: zipformer2-streaming-zh 128 6 4, --lm=2x512 --lm=3x2048, 3 rounds)

N streams of the synthetic `preset` model each buffer an utterance of `seconds` s; the tool decodes all of them chunk by chunk (one
k2hip_online_step per tick over the whole group) under modified_beam_search, `rounds` times round-robin over the legs so that drift of
the device hits all of them alike, and reports the median ms per tick of each leg over all its ticks:
  plain            the unfused tick in the form the shape selects (the one-kernel search where it fits)
  plain_launches   the unfused tick under K2HIP_BEAM_LAUNCHES=1 (four launches per frame: the form a fused tick always takes)
  fused LxH        k2hip_set_rnn_lm_stream_fusion with a synthetic L x H LM of scale 0.5: per frame L k_nlm_advance launches and the LM
                   rows over all streams x beam slots, per tick the two movers (k_nlm_load_streams / k_nlm_store_streams)
and per fused leg lm_share_us_per_frame = (fused - plain_launches) / frames per tick, the block pool's bytes, and whether the fused
results differ from the plain ones.  One JSON line on stdout.  There is no time gate: DESIGN.md "Neural LM shallow fusion in the
streaming search" has the runs."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from k2transducerasr_amd import OnlineRecognizer, RnnLm, set_switch  # noqa: E402
from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model, write_synthetic_rnn_lm  # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
lms = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--lm=")] or ["2x512", "3x2048"]
rounds = next((int(a.split("=", 1)[1]) for a in sys.argv[1:] if a.startswith("--rounds=")), 3)
preset = argv[0] if len(argv) > 0 else "zipformer2-streaming-zh"
N = int(argv[1]) if len(argv) > 1 else 128
secs = float(argv[2]) if len(argv) > 2 else 6.0
beam = int(argv[3]) if len(argv) > 3 else 4
DISTINCT = 8


def run(rec, feats):
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
    res = [(h.tokens[2:], h.timestamps) for h in hs]
    for h in hs:
        h.close()
    return ms, res


def main():
    out = dict(preset=preset, streams=N, seconds=secs, beam=beam, rounds=rounds, slots=N * beam)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"{preset}.k2w")
        write_synthetic_model(path, preset)
        rec = OnlineRecognizer(path, 0, "modified_beam_search", beam)
        m = rec.model
        base = [np.ascontiguousarray(m.fbank(synth_utterance(300 + u, secs)), np.float32) for u in range(DISTINCT)]
        feats = [base[u % DISTINCT] for u in range(N)]
        handles = {}
        for spec in lms:
            L, H = (int(x) for x in spec.split("x"))
            lp = os.path.join(d, f"lm_{spec}.k2w")
            write_synthetic_rnn_lm(lp, m.vocab_size, H, H, L, 1)
            handles[spec] = RnnLm(lp)

        def leg(name):
            if name == "plain":
                return run(rec, feats)
            if name == "plain_launches":
                set_switch("K2HIP_BEAM_LAUNCHES", 1)
                try:
                    return run(rec, feats)
                finally:
                    set_switch("K2HIP_BEAM_LAUNCHES", 0)
            m.set_rnn_lm(handles[name], 0.5)
            m.set_rnn_lm_stream_fusion(True)
            try:
                return run(rec, feats)
            finally:
                m.set_rnn_lm_stream_fusion(False)
                m.set_rnn_lm(None)

        legs = ["plain", "plain_launches"] + lms
        run(rec, feats[: min(N, 8)])          # warm-up: arenas, decoder tables
        ms = {k: [] for k in legs}
        res = {}
        for _ in range(rounds):
            for k in legs:
                t, r = leg(k)
                ms[k] += t
                res[k] = r
        out["frames_per_tick"] = rec.frames_per_chunk
        out["ticks_per_leg"] = len(ms["plain"])
        out["plain_ms"] = float(np.median(ms["plain"]))
        out["plain_launches_ms"] = float(np.median(ms["plain_launches"]))
        assert res["plain"] == res["plain_launches"]
        out["lms"] = []
        for spec in lms:
            f = float(np.median(ms[spec]))
            out["lms"].append(dict(lm=spec, fused_ms=f, lm_share_us_per_frame=(f - out["plain_launches_ms"]) * 1e3 / rec.frames_per_chunk,
                                   streams_moved=sum(a != b for a, b in zip(res[spec], res["plain"]))))
        st = m.rnn_lm_stream_fusion_stats()
        out.update(chunk_calls=st["chunk_calls"], pool_bytes=st["pool_bytes"], live_blocks=st["live_blocks"])
        for h in handles.values():
            h.close()
        m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
