"""Cost of fusing a neural LM into the offline modified beam search, next to the plain search and to N-best rescoring.

    python tools/rnn_lm_fusion_bench.py [preset] [batch] [seconds] [--lm=LxH ...] [--lodr]   (defaults: zipformer2-large-en 32 10, --lm=2x512 --lm=3x2048)

The encoder output of `batch` synthetic utterances of `seconds` seconds is computed once; every leg is then the search operator on it
(Model.beam_search, beam 4: upload, search, download), median wall milliseconds over the rounds:
  plain_ms            the plain search in the form the shape selects (one kernel per batch)
  plain_launches_ms   the plain search under K2HIP_BEAM_LAUNCHES=1 (four launches per frame: the form a fused search always takes)
  fused_ms            the fused search (k2hip_set_rnn_lm_fusion): per frame L k_nlm_advance launches and the LM rows behind the step
  rescored_ms         the plain search with N-best 4 followed by Model.rnn_lm_score of all its alternatives with eos
  lm_share_us_per_frame   (fused_ms - plain_launches_ms) / T'
  swept / idle        per-layer LM launches of one fused search that read their weights / that only moved state
  fused_lodr_ms       (--lodr) the fused search with a bi-gram LODR LM at weight -0.5 (k2hip_set_lodr_lm), in the same run next to fused_ms:
                      one more wave-walk per selected candidate inside the step; lodr_share_us_per_frame = (fused_lodr_ms - fused_ms) / T'
and, per LM width H, ONE launch at 128 rows: k_nlm_advance (2 H products per gate: input and recurrent), the rescoring step
k_lm_lstm_step and the step composed from the GEMM launcher and the cell kernel (H products per gate: their input products are a
separate GEMM per time block).  One JSON line on stdout.  There is no time gate: DESIGN.md "Neural LM shallow fusion" has the runs."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from k2transducerasr_amd import Model, NgramLm, RnnLm, set_switch  # noqa: E402
from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model, write_synthetic_rnn_lm  # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
lms = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--lm=")] or ["2x512", "3x2048"]
preset = argv[0] if len(argv) > 0 else "zipformer2-large-en"
batch = int(argv[1]) if len(argv) > 1 else 32
seconds = float(argv[2]) if len(argv) > 2 else 10.0
ROUNDS, WARMUP, BEAM, ROWS = 5, 1, 4, 128
LODR = "--lodr" in sys.argv[1:]


def bigram(plain, V, seed=7):
    """a bi-gram over the model's tokens: unigrams for every real token, 400 bigrams cut from the plain search's output and random ones"""
    rng = np.random.default_rng(seed)
    real = [v for v in range(V) if v not in (0, 2)]
    ent = {(-1,): (-99.0, -0.5), (-3,): (-7.5, 0.0)}
    for v in real:
        ent[(v,)] = (float(rng.uniform(-6, -3)), float(rng.uniform(-1, -0.05)))
    seqs = [list(t) for t, _ in plain if len(t) >= 2]
    for i in range(400):
        if seqs and i % 2 == 0:
            s = seqs[rng.integers(len(seqs))]
            o = int(rng.integers(0, len(s) - 1))
            g = (int(s[o]), int(s[o + 1]))
        else:
            g = tuple(int(x) for x in rng.choice(real, size=2))
        if g[0] in (0, 2) or g[1] in (0, 2):
            continue
        ent.setdefault(g, (float(rng.uniform(-1.5, -0.1)), 0.0))
    return [(k, lp, bo) for k, (lp, bo) in sorted(ent.items(), key=lambda kv: (len(kv[0]), kv[0]))]


def timed(fn):
    walls = []
    for i in range(WARMUP + ROUNDS):
        t0 = time.perf_counter()
        fn()
        if i >= WARMUP:
            walls.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(walls))


def main():
    out = dict(preset=preset, batch=batch, seconds=seconds, beam=BEAM, rounds=ROUNDS)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"{preset}.k2w")
        write_synthetic_model(path, preset)
        m = Model(path, 0)
        feats = [m.fbank(synth_utterance(u, seconds)) for u in range(batch)]
        enc = m.encoder_proj(m.pad_sequence(feats).reshape(batch, -1, 80))
        Tp = enc.shape[1]
        out.update(frames=int(Tp), slots=batch * BEAM)
        out["plain_ms"] = timed(lambda: m.beam_search(enc, BEAM))
        plain_result = m.beam_search(enc, BEAM)
        set_switch("K2HIP_BEAM_LAUNCHES", 1)
        try:
            out["plain_launches_ms"] = timed(lambda: m.beam_search(enc, BEAM))
        finally:
            set_switch("K2HIP_BEAM_LAUNCHES", 0)
        out["lms"] = []
        for spec in lms:
            L, H = (int(x) for x in spec.split("x"))
            lp = os.path.join(d, f"lm_{spec}.k2w")
            write_synthetic_rnn_lm(lp, m.vocab_size, H, H, L, 1)
            lm = RnnLm(lp)
            m.set_rnn_lm(lm, 0.5)
            lm.close()
            r = dict(lm=spec)

            def rescored():
                alts = m.beam_search(enc, BEAM, nbest=4)
                m.rnn_lm_score([a["tokens"] for al in alts for a in al], True)

            r["rescored_ms"] = timed(rescored)
            m.set_rnn_lm_fusion(True)
            try:
                r["fused_ms"] = timed(lambda: m.beam_search(enc, BEAM))
                s0 = m.rnn_lm_fusion_stats()
                m.beam_search(enc, BEAM)
                s1 = m.rnn_lm_fusion_stats()
                if LODR:
                    lodr = NgramLm(bigram(plain_result, m.vocab_size), m.vocab_size)
                    m.set_lodr_lm(lodr, -0.5)
                    lodr.close()
                    try:
                        r["fused_lodr_ms"] = timed(lambda: m.beam_search(enc, BEAM))
                        r["fused_again_ms"] = timed(lambda: (m.set_lodr_lm(None), m.beam_search(enc, BEAM))[1])
                    finally:
                        m.set_lodr_lm(None)
                    r["lodr_share_us_per_frame"] = (r["fused_lodr_ms"] - r["fused_ms"]) * 1e3 / Tp
            finally:
                m.set_rnn_lm_fusion(False)
            r.update(swept=s1["swept"] - s0["swept"], idle=s1["idle"] - s0["idle"],
                     lm_share_us_per_frame=(r["fused_ms"] - out["plain_launches_ms"]) * 1e3 / Tp)
            step = m.rnn_lm_step_bench(ROWS, H, 200)
            r.update(rows=ROWS, launches=200, nlm_advance_ms=m.nlm_advance_bench(ROWS, H, 200), lm_lstm_step_ms=step["fused_ms"],
                     composed_step_ms=step["composed_ms"])
            m.set_rnn_lm(None)
            out["lms"].append(r)
        m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
