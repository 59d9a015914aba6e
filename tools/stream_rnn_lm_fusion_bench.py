"""Cost of carrying a neural LM through the streaming modified beam search: the streaming tick four ways, interleaved.

    python tools/stream_rnn_lm_fusion_bench.py [preset] [streams] [seconds] [beam] [--lm=LxH ...] [--rounds N] [--lodr]
    (defaults: zipformer2-streaming-zh 128 6 4, --lm=2x512 --lm=3x2048, 3 rounds)

N streams of the synthetic `preset` model each buffer an utterance of `seconds` s; the tool decodes all of them chunk by chunk (one
k2hip_online_step per tick over the whole group) under modified_beam_search, `rounds` times round-robin over the legs so that drift of
the device hits all of them alike, and reports the median ms per tick of each leg over all its ticks:
  plain            the unfused tick in the form the shape selects (the one-kernel search where it fits)
  plain_launches   the unfused tick under K2HIP_BEAM_LAUNCHES=1 (four launches per frame: the form a fused tick always takes)
  fused LxH        k2hip_set_rnn_lm_stream_fusion with a synthetic L x H LM of scale 0.5: per frame L k_nlm_advance launches and the LM
                   rows over all streams x beam slots, per tick the two movers (k_nlm_load_streams / k_nlm_store_streams)
  fused LxH +lodr  (--lodr) the same with a bi-gram LODR LM at weight -0.5 beside it (k2hip_set_lodr_lm): one more wave-walk per selected
                   candidate in the step and one more plane of carried states; reported as fused_lodr_ms next to fused_ms
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

from k2transducerasr_amd import NgramLm, OnlineRecognizer, RnnLm, set_switch  # noqa: E402
from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model, write_synthetic_rnn_lm  # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
lms = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--lm=")] or ["2x512", "3x2048"]
rounds = next((int(a.split("=", 1)[1]) for a in sys.argv[1:] if a.startswith("--rounds=")), 3)
preset = argv[0] if len(argv) > 0 else "zipformer2-streaming-zh"
N = int(argv[1]) if len(argv) > 1 else 128
secs = float(argv[2]) if len(argv) > 2 else 6.0
beam = int(argv[3]) if len(argv) > 3 else 4
DISTINCT = 8
LODR = "--lodr" in sys.argv[1:]


def bigram(V, seed=7):
    """a bi-gram over the model's tokens: unigrams for every real token and 400 random bigrams"""
    rng = np.random.default_rng(seed)
    real = [v for v in range(V) if v not in (0, 2)]
    ent = {(-1,): (-99.0, -0.5), (-3,): (-7.5, 0.0)}
    for v in real:
        ent[(v,)] = (float(rng.uniform(-6, -3)), float(rng.uniform(-1, -0.05)))
    for _ in range(400):
        ent.setdefault(tuple(int(x) for x in rng.choice(real, size=2)), (float(rng.uniform(-1.5, -0.1)), 0.0))
    return [(k, lp, bo) for k, (lp, bo) in sorted(ent.items(), key=lambda kv: (len(kv[0]), kv[0]))]


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
            with_lodr = name.endswith("+lodr")
            m.set_rnn_lm(handles[name[:-5] if with_lodr else name], 0.5)
            m.set_rnn_lm_stream_fusion(True)
            if with_lodr:
                m.set_lodr_lm(lodr, -0.5)
            try:
                return run(rec, feats)
            finally:
                m.set_lodr_lm(None)
                m.set_rnn_lm_stream_fusion(False)
                m.set_rnn_lm(None)

        lodr = NgramLm(bigram(m.vocab_size), m.vocab_size) if LODR else None
        legs = ["plain", "plain_launches"] + lms + ([s + "+lodr" for s in lms] if LODR else [])
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
            if LODR:
                g = float(np.median(ms[spec + "+lodr"]))
                out["lms"][-1].update(fused_lodr_ms=g, lodr_share_us_per_frame=(g - f) * 1e3 / rec.frames_per_chunk,
                                      streams_moved_by_lodr=sum(a != b for a, b in zip(res[spec + "+lodr"], res[spec])))
        st = m.rnn_lm_stream_fusion_stats()
        out.update(chunk_calls=st["chunk_calls"], pool_bytes=st["pool_bytes"], live_blocks=st["live_blocks"])
        for h in handles.values():
            h.close()
        if lodr:
            lodr.close()
        m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
