"""Generate tests/golden/encoder_bits_golden.json: SHA-1 digests of encoder outputs, taps and streaming caches, token lists and the
integer columns of the GEMM launch log, for the synthetic Zipformer2 / Zipformer v1 presets, offline and streaming.

Unlike tools/make_golden.py and tools/make_golden2.py this fixture is NOT independent of the HIP path: it is what the engine computed
on one MI355X at the commit that recorded it.  The encoder has no floating-point atomics, so its outputs are reproducible bit for bit;
tests/test_encoder_bits_gpu.py recomputes every entry with the functions below and asserts equality.  That pins a change that only
moves host orchestration (which launches, in which order, on which operands) from outside: re-record only with a change that is
meant to alter a kernel's arithmetic or the launch list, and say so.

Run it on the GPU twice, in two processes, and compare the two files before committing one (`--out` names the file).
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from k2transducerasr_amd import Model, OnlineProj, OnlineRecognizer, set_switch  # noqa: E402
from k2transducerasr_amd.k2w import read_k2w  # noqa: E402
from k2transducerasr_amd.synth import write_synthetic_model  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "encoder_bits_golden.json")
# K2HIP_FUSED_VPROJ_MIN_T's default (csrc/kernels.h, Tunables::fused_vproj_min_t)
FUSED_VPROJ_MIN_T = 4
JOIN_AT = (0, 2, 4)   # the call / tick at which each of the three streams joins
N_CALLS = 6


def sha(a) -> str:
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def feats(seed: int, B: int, T: int) -> np.ndarray:
    """fixed-seed log-mel-like features [B, T, 80]"""
    return (np.random.default_rng(seed).standard_normal((B, T, 80)) * 3.0 - 6.0).astype(np.float32)


def weight_checksum(path: str, name: str) -> float:
    _, t = read_k2w(path)
    return float(np.asarray(t[name], np.float64).sum())


def launch_rows(model) -> list:
    """(M, N, K, batch, act, residual, kind) of every GEMM launch of the last instrumented call"""
    return model.gemm_profile()[:, :7].astype(np.int64).tolist()


class switches:
    """process-global development switches, set for a block and put back after it"""

    def __init__(self, **on):
        self.on = on

    def __enter__(self):
        for k, v in self.on.items():
            set_switch(k, v)

    def __exit__(self, *exc):
        for k in self.on:
            set_switch(k, FUSED_VPROJ_MIN_T if k == "K2HIP_FUSED_VPROJ_MIN_T" else 0)


def offline_pass(m, x, taps, rows: bool) -> dict:
    out = {"encoder_proj": sha(m.encoder_proj(x))}
    for tap in taps:
        out[f"tap{tap}"] = sha(m.encoder_tap(x, tap))
    if rows:
        m.set_instrument(True)
        try:
            m.encoder_proj(x)
            out["rows"] = launch_rows(m)
        finally:
            m.set_instrument(False)
    return out


def case_a(path: str) -> dict:
    """zipformer2-tiny-test offline, B = 8, T = 77 (T50 = 35; stack 0 has M = 280 >= 256, the downsampled stacks fall below)"""
    m = Model(path, 0)
    x = feats(101, 8, 77)
    taps = [0, 1, 2, 3, 4, 100]
    out = {"default": offline_pass(m, x, taps, True)}
    with switches(K2HIP_NO_GLU_EPILOGUE=1, K2HIP_NO_FUSED_AV=1):
        out["no_glu_no_fused_av"] = offline_pass(m, x, taps, True)
    m.close()
    return out


def case_b(path: str) -> dict:
    """zipformer2-ctc-tiny-test offline, B = 2, T = 45: log_probs"""
    m = Model(path, 0)
    out = {"log_probs": sha(m.encoder_proj(feats(102, 2, 45)))}
    m.close()
    return out


def stream_feats(seed: int, T: int, S: int) -> np.ndarray:
    """three feature streams, each long enough for the chunks it decodes after joining"""
    return feats(seed, 3, T + (N_CALLS - 1) * S)


def proj_pass(path: str) -> dict:
    p = OnlineProj(path, 0)
    T, S = p.chunk_length, p.shift_length
    f = stream_feats(103, T, S)
    states, done, out = [], [], {"calls": []}
    try:
        for call in range(N_CALLS):
            for u, at in enumerate(JOIN_AT):
                if at == call:
                    states.append(p.get_encoder_init_states())
                    done.append(0)
            x = np.stack([f[u, done[u] * S : done[u] * S + T] for u in range(len(states))])
            if call == N_CALLS - 1:
                p.model.set_instrument(True)
            out["calls"].append(sha(p.encoder_proj(x, states)))
            done = [d + 1 for d in done]
        out["rows"] = launch_rows(p.model)
        out["processed_len"] = [p.processed_len(s) for s in states]
    finally:
        p.model.set_instrument(False)
        for s in states:
            p.free_states(s)
        p.model.close()
    return out


def case_c(path: str) -> dict:
    """zipformer2-streaming-tiny-test through OnlineProj.encoder_proj: 3 states over 6 calls, joining at calls 0, 2, 4"""
    out = {"default": proj_pass(path)}
    with switches(K2HIP_NO_FUSED_VPROJ=1, K2HIP_NO_FUSED_CONV=1, K2HIP_NO_GLU_EPILOGUE=1):
        out["unfused"] = proj_pass(path)
    m = Model(path, 0)
    # frames of a chunk at the embed's output rate, and what each stack makes of them
    chunk, dss = int(m.meta("decode_chunk_len")) // 2, [int(v) for v in m.meta("downsampling_factors").split(",")]
    m.close()
    if min(chunk // ds for ds in dss) < FUSED_VPROJ_MIN_T:   # a stack's chunk is below the default threshold: force the fused form there too
        with switches(K2HIP_FUSED_VPROJ_MIN_T=1):
            out["vproj_min_t_1"] = proj_pass(path)
    return out


def recognizer_pass(path: str, seed: int, rows: bool) -> dict:
    rec = OnlineRecognizer(path, 0)
    f = stream_feats(seed, rec.chunk_length, rec.shift_length)
    streams, out = [], {}
    try:
        for tick in range(N_CALLS):
            for u, at in enumerate(JOIN_AT):
                if at == tick:
                    s = rec.create_online_stream()
                    s.add_features(f[u, : f.shape[1] - at * rec.shift_length])
                    streams.append(s)
            if rows and tick == N_CALLS - 1:
                rec.model.set_instrument(True)
            dec, _ = rec.get_results(streams)
            assert dec == [1] * len(streams), (tick, dec)
        if rows:
            out["rows"] = launch_rows(rec.model)
        out["tokens"] = [s.tokens for s in streams]
        out["timestamps"] = [s.timestamps for s in streams]
        out["state"] = [{f"{layer}.{kind}": sha(s.state(layer, kind)) for layer in range(rec.num_layers) for kind in rec.state_kinds}
                        for s in streams]
    finally:
        rec.model.set_instrument(False)
        for s in streams:
            s.close()
        rec.model.close()
    return out


def case_d(path: str, path_ctc: str) -> dict:
    """the streaming Zipformer2 transducer and CTC models through OnlineRecognizer.get_results: 3 streams, staggered as in case c"""
    return {"transducer": recognizer_pass(path, 104, False), "ctc": recognizer_pass(path_ctc, 105, False)}


def case_e(path: str) -> dict:
    """zipformer-streaming-tiny-test (v1) through OnlineRecognizer, with the launch rows of the last tick"""
    return recognizer_pass(path, 106, True)


def case_f(path: str) -> dict:
    """zipformer-tiny-test (v1 offline): T50 divisible by 4 (T = 39 -> 16), and not (T = 45 -> 19: z1_group_rows)"""
    m = Model(path, 0)
    out = {f"T{T}": offline_pass(m, feats(107 + T, 2, T), [0, 1, 2, 3, 4], False) for T in (39, 45)}
    m.close()
    return out


# case -> (presets it loads, function)
CASES = {
    "a": (["zipformer2-tiny-test"], case_a),
    "b": (["zipformer2-ctc-tiny-test"], case_b),
    "c": (["zipformer2-streaming-tiny-test"], case_c),
    "d": (["zipformer2-streaming-tiny-test", "zipformer2-ctc-streaming-tiny-test"], case_d),
    "e": (["zipformer-streaming-tiny-test"], case_e),
    "f": (["zipformer-tiny-test"], case_f),
}


def checksum_tensor(preset: str) -> str:
    """the last product of the encoder call: a model with other weights cannot pass for this one"""
    return "ctc_output.1.weight" if "-ctc-" in preset else "joiner.encoder_proj.weight"


def run_case(name: str, tmpdir: str) -> dict:
    """{"weights": {preset: [tensor, float64 sum]}, "got": the case's digests}"""
    presets, fn = CASES[name]
    paths = []
    for p in presets:
        paths.append(os.path.join(tmpdir, p + ".k2w"))
        if not os.path.exists(paths[-1]):
            write_synthetic_model(paths[-1], p)
    return {"weights": {p: [checksum_tensor(p), weight_checksum(q, checksum_tensor(p))] for p, q in zip(presets, paths)}, "got": fn(*paths)}


if __name__ == "__main__":
    import argparse
    import tempfile

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        gold = {name: run_case(name, d) for name in CASES}
    with open(args.out, "w") as fh:
        json.dump(gold, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("encoder bits golden:", args.out, os.path.getsize(args.out), "bytes")
