"""The offline batch with the encoder's half-precision switch off and at levels 1, 2 and 3 (Model.set_encoder_precision;
csrc/gemm_f16.hip, csrc/convnext_f16.hip).

    python tools/encoder_half_bench.py [preset] [batch] [seconds] [conv route]      (defaults: zipformer2-large-en 32 10 0)

A batch of `batch` synthetic utterances of `seconds` seconds is decoded from samples (offline_greedy_from_samples) ROUNDS times with
the switch off, at 1 and at 2, interleaved round by round in one process after WARMUP rounds of each: "off_ms" / "on_ms" / "on2_ms" are
the medians of the calls' total_ms (device events around the whole call), with their [min, max] spread, and encoder_ms beside them.
Then one instrumented call each way (every GEMM launch bracketed by events): the launch logs have the same rows in the same order, and
the rows whose kind carries the f16 family's bit at level 1 are the covered launches.  "shapes" lists them grouped by (M, N, K, act,
residual): launches per call, microseconds summed over them in float32 and in f16, and the f16 tile.  "covered_f32_ms" / "covered_f16_ms"
sum those, "gemm_f32_ms" / "gemm_on_ms" / "gemm_on2_ms" are all GEMM launches of the call.  "shapes2" / "covered2_*" are the same for the
launches that carry the bit at level 2 only -- the newly covered ones (a conv module's fused launch counts its convolution on both
sides; where level 2 takes the gated f16 GEMM + dwconv1d_swoosh in place of a float32 fused launch the f16 side lacks the convolution's
launch, so such a route is judged by the batch figures).  `conv route` forces K2HIP_F16_CONV for the run (1 fused f16, 2 gated f16 GEMM
+ conv, 3 as level 1).  "same_tokens" / "same_tokens2" count the utterances whose token lists are identical off and on.  One JSON line on
stdout.  Level 3: "on3_ms" / "on3_encoder_ms" by convnext_f16_route's rule and "on3_two_ms" / "on3_two_encoder_ms" with the embed's ConvNeXt
pointwise pair forced to the two gemm_f16_mfma launches (K2HIP_F16_CONVNEXT=2), in the same interleaved rounds; "shapes3" are the embed's
launches that carry the bit at level 3 only, float32 against the two-launch f16 route, and "pair_us" the pointwise pair alone as float32
(two launches), two f16 launches and the fused launch (the row whose kind carries bit 22).  Level 4 (csrc/attn_f16.hip): "on4_ms" /
"on4_encoder_ms" by attn_f16_route's rule and "on4_r3_ms" / "on4_r3_encoder_ms" with K2HIP_F16_ATTN=3 (level 3's launches), in the same
rounds, and "same_tokens4".  The attention kernels are no GEMM launches and carry no events; their times come from a kernel trace:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/encoder_half_bench.py --attn-calls [preset] [batch] [seconds]
    python tools/encoder_half_bench.py --attn-table DIR/**/*_kernel_trace.csv

The first runs three calls at level 3 and three at level 4 and nothing else; the second prints, per attention kernel and grid (one grid
per stack: scores cdiv(T, 32) x B x H workgroups, apply cdiv(T, 16) x B x slices), the launches and the median microseconds.  There is no time gate (DESIGN.md "Half-precision operands in the encoder's linear layers" has the runs taken so far).

The offline Conformer's switch (Model.set_conformer_precision; csrc/conformer_f16.hip) has a leg of its own:

    python tools/encoder_half_bench.py --conformer [preset] [batch] [seconds]      (defaults: conformer-zh 8 30)

the batch at the levels 0, 1, 2 and 2 with the float32 attention core (K2HIP_F16_CONFORMER_ATTN=3), interleaved round by round: medians
of total_ms and encoder_ms with [min, max], the counters, the utterances with identical tokens at each level, and from one instrumented
call at level 1 the float32 value product's batched GEMM launches ("av_gemm_f32_us": count, microseconds summed).  The two new kernels
against the float32 scores kernel come from a kernel trace: --conformer-calls runs three calls at level 1 and three at level 2 and
nothing else, --attn-table lists the Conformer kernels too."""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from k2transducerasr_amd import Model, set_switch  # noqa: E402
from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model  # noqa: E402

argv = sys.argv[1:]
mode = argv.pop(0) if argv and argv[0].startswith("--") else ""
paths, argv = (argv, []) if mode == "--attn-table" else ([], argv)
conformer = mode.startswith("--conformer")
preset = argv[0] if len(argv) > 0 else ("conformer-zh" if conformer else "zipformer2-large-en")
batch = int(argv[1]) if len(argv) > 1 else (8 if conformer else 32)
seconds = float(argv[2]) if len(argv) > 2 else (30.0 if conformer else 10.0)
route = int(argv[3]) if len(argv) > 3 else 0
LEVELS = (0, 1, 2, 3, "3two", 4, "4r3")   # "3two": level 3 with the pointwise pair as two f16 launches; "4r3": level 4, float32 attention
ROUNDS, WARMUP = 9, 2
F16_BIT, PAIR_BIT = 1 << 21, 1 << 22


def set_level(model, half):
    set_switch("K2HIP_F16_CONVNEXT", 2 if half == "3two" else 0)
    set_switch("K2HIP_F16_ATTN", 3 if half == "4r3" else 0)
    model.set_encoder_precision(0)   # ("4r3" after 4 is the same level: the switch is read per call, the counters start here)
    model.set_encoder_precision({"3two": 3, "4r3": 4}.get(half, half))


def attn_calls():
    """three calls at level 3 and three at level 4 (the Conformer: at its levels 1 and 2), for a kernel trace"""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "m.k2w")
        write_synthetic_model(path, preset)
        model = Model(path, 0)
        utts = [synth_utterance(u, seconds) for u in range(batch)]
        switch = model.set_conformer_precision if conformer else model.set_encoder_precision
        for half in ((1, 2) if conformer else (3, 4)):
            switch(half)
            for _ in range(3):
                model.offline_greedy_from_samples(utts)
        switch(0)
        model.close()


def attn_table(paths):
    """median microseconds of the attention kernels of kernel-trace CSVs, by kernel and grid"""
    import csv
    rows = {}
    for p in paths:
        with open(p, newline="") as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"]
                if not any(k in name for k in ("k_attn_scores_softmax", "k_attn_av_out", "k_conformer_scores_softmax", "k_conformer_av")):
                    continue
                short = ("conformer_" if "k_conformer" in name else "") + ("scores" if "scores" in name else "apply") + ("_f16" if "_f16" in name else "_f32")
                grid = tuple(int(r[f"Grid_Size_{a}"]) // int(r[f"Workgroup_Size_{a}"]) for a in "XYZ")
                rows.setdefault((short, grid), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (short, grid), us in sorted(rows.items(), key=lambda kv: (kv[0][0].split("_")[0], -kv[0][1][0], kv[0][0])):
        print(json.dumps(dict(kernel=short, workgroups=grid, launches=len(us), median_us=round(float(np.median(us)), 2),
                              spread=[round(min(us), 2), round(max(us), 2)])))


def shape_table(off, on, skip):
    """the launches that are f16 in `on` and not in `skip`, grouped by shape: float32 (off) against f16 microseconds"""
    shapes = {}
    for a, b, c in zip(off, on, skip):
        if not int(b[6]) & F16_BIT or (skip is not off and int(c[6]) & F16_BIT):
            continue
        key = tuple(int(v) for v in b[:3]) + (int(b[4]), int(b[5]))
        s = shapes.setdefault(key, dict(M=key[0], N=key[1], K=key[2], act=key[3], res=key[4], launches=0, f32_us=0.0, f16_us=0.0,
                                        tile=f"{(int(b[6]) >> 8 & 15) * 32}x{(int(b[6]) >> 12 & 15) * 32}"))
        s["launches"] += 1
        s["f32_us"] += float(a[7])
        s["f16_us"] += float(b[7])
    rows = sorted(shapes.values(), key=lambda s: -s["f32_us"])
    for s in rows:
        s["f32_us"], s["f16_us"] = round(s["f32_us"], 1), round(s["f16_us"], 1)
    return rows


def conformer_main():
    levels = (0, 1, 2, "2r3")   # "2r3": level 2 with the float32 attention core
    spread = lambda v: [round(float(np.min(v)), 3), round(float(np.max(v)), 3)]   # noqa: E731

    def set_level(model, lv):
        set_switch("K2HIP_F16_CONFORMER_ATTN", 3 if lv == "2r3" else 0)
        model.set_conformer_precision(0)   # (the counters start here)
        model.set_conformer_precision(2 if lv == "2r3" else lv)

    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "m.k2w")
        write_synthetic_model(path, preset)
        model = Model(path, 0)
        utts = [synth_utterance(u, seconds) for u in range(batch)]
        total, enc, tokens, stats = {v: [] for v in levels}, {v: [] for v in levels}, {}, {}
        for r in range(WARMUP + ROUNDS):
            for lv in levels:
                set_level(model, lv)
                tokens[lv] = model.offline_greedy_from_samples(utts)
                t, stats[lv] = model.timing(), model.encoder_f16_stats()
                if r >= WARMUP:
                    total[lv].append(t["total_ms"])
                    enc[lv].append(t["encoder_ms"])
        model.set_instrument(True)
        set_level(model, 1)
        model.offline_greedy_from_samples(utts)
        prof = model.gemm_profile().copy()
        model.set_instrument(False)
        set_level(model, 0)
        model.close()
    av = prof[(prof[:, 3] > 1) & (prof[:, 1] < prof[:, 2])]   # batched launches with N = dk < K = T: the weights . values product
    out = dict(preset=preset, batch=batch, seconds=seconds, rounds=ROUNDS, utterances=batch,
               av_gemm_f32_us=dict(launches=int(len(av)), us=round(float(av[:, 7].sum()), 1)))
    for lv in levels:
        out[f"level{lv}"] = dict(total_ms=round(float(np.median(total[lv])), 3), total_spread=spread(total[lv]),
                                 encoder_ms=round(float(np.median(enc[lv])), 3), encoder_spread=spread(enc[lv]), **stats[lv],
                                 same_tokens=int(sum(a == b for a, b in zip(tokens[0], tokens[lv]))))
    print(json.dumps(out), flush=True)


def main():
    set_switch("K2HIP_F16_CONV", route)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "m.k2w")
        write_synthetic_model(path, preset)
        model = Model(path, 0)
        utts = [synth_utterance(u, seconds) for u in range(batch)]
        total = {v: [] for v in LEVELS}
        enc = {v: [] for v in LEVELS}
        tokens = {}
        for r in range(WARMUP + ROUNDS):
            for half in LEVELS:
                set_level(model, half)
                tokens[half] = model.offline_greedy_from_samples(utts)
                t = model.timing()
                if r >= WARMUP:
                    total[half].append(t["total_ms"])
                    enc[half].append(t["encoder_ms"])
        prof = {}
        model.set_instrument(True)
        stats = {}
        for half in LEVELS:
            set_level(model, half)
            model.offline_greedy_from_samples(utts)
            prof[half] = model.gemm_profile().copy()
            stats[half] = model.encoder_f16_stats()
        model.set_instrument(False)
        model.set_encoder_precision(False)
        model.close()
    off, on, on2, on3 = prof[0], prof[1], prof[2], prof["3two"]
    for p in (on, on2, on3):
        assert off.shape == p.shape and np.array_equal(off[:, :6], p[:, :6]), "the launch logs do not line up"
    rows, rows2, rows3 = shape_table(off, on, off), shape_table(off, on2, on), shape_table(off, on3, on2)
    pair = [s for s in rows3 if (s["N"], s["K"]) in ((384, 128), (128, 384))]
    fused = prof[3][(prof[3][:, 6].astype(np.int64) & PAIR_BIT) != 0]
    pair_us = dict(f32=round(sum(s["f32_us"] for s in pair), 1), two_f16=round(sum(s["f16_us"] for s in pair), 1),
                   fused=round(float(fused[:, 7].sum()), 1), fused_launches=int(len(fused)))
    spread = lambda v: [round(float(np.min(v)), 3), round(float(np.max(v)), 3)]   # noqa: E731
    print(json.dumps(dict(
        preset=preset, batch=batch, seconds=seconds, rounds=ROUNDS, conv_route=route,
        off_ms=round(float(np.median(total[0])), 3), off_spread=spread(total[0]),
        on_ms=round(float(np.median(total[1])), 3), on_spread=spread(total[1]),
        on2_ms=round(float(np.median(total[2])), 3), on2_spread=spread(total[2]),
        on3_ms=round(float(np.median(total[3])), 3), on3_spread=spread(total[3]),
        on3_two_ms=round(float(np.median(total["3two"])), 3), on3_two_spread=spread(total["3two"]),
        on3_encoder_ms=round(float(np.median(enc[3])), 3), on3_encoder_spread=spread(enc[3]),
        on3_two_encoder_ms=round(float(np.median(enc["3two"])), 3), on2_encoder_spread=spread(enc[2]),
        on4_ms=round(float(np.median(total[4])), 3), on4_spread=spread(total[4]),
        on4_encoder_ms=round(float(np.median(enc[4])), 3), on4_encoder_spread=spread(enc[4]),
        on4_r3_ms=round(float(np.median(total["4r3"])), 3), on4_r3_spread=spread(total["4r3"]),
        on4_r3_encoder_ms=round(float(np.median(enc["4r3"])), 3), on4_r3_encoder_spread=spread(enc["4r3"]),
        launches4=stats[4]["launches"], panels4=stats[4]["panels"], same_tokens4=int(sum(a == b for a, b in zip(tokens[0], tokens[4]))),
        pair_us=pair_us, panels3=stats[3]["panels"], panel_bytes3=stats[3]["panel_bytes"], launches3=stats[3]["launches"],
        same_tokens3=int(sum(a == b for a, b in zip(tokens[0], tokens[3]))), shapes3=rows3,
        off_encoder_ms=round(float(np.median(enc[0])), 3), on_encoder_ms=round(float(np.median(enc[1])), 3),
        on2_encoder_ms=round(float(np.median(enc[2])), 3),
        gemm_f32_ms=round(float(off[:, 7].sum()) / 1e3, 3), gemm_on_ms=round(float(on[:, 7].sum()) / 1e3, 3),
        gemm_on2_ms=round(float(on2[:, 7].sum()) / 1e3, 3),
        covered_launches=int(sum(s["launches"] for s in rows)),
        covered_f32_ms=round(sum(s["f32_us"] for s in rows) / 1e3, 3), covered_f16_ms=round(sum(s["f16_us"] for s in rows) / 1e3, 3),
        covered2_launches=int(sum(s["launches"] for s in rows2)),
        covered2_f32_ms=round(sum(s["f32_us"] for s in rows2) / 1e3, 3), covered2_f16_ms=round(sum(s["f16_us"] for s in rows2) / 1e3, 3),
        panels=stats[1]["panels"], panel_bytes=stats[1]["panel_bytes"], panels2=stats[2]["panels"], panel_bytes2=stats[2]["panel_bytes"],
        same_tokens=int(sum(a == b for a, b in zip(tokens[0], tokens[1]))),
        same_tokens2=int(sum(a == b for a, b in zip(tokens[0], tokens[2]))), utterances=batch, shapes=rows, shapes2=rows2)), flush=True)


if __name__ == "__main__":
    if mode == "--attn-table":
        attn_table(paths)
    elif mode in ("--attn-calls", "--conformer-calls"):
        attn_calls()
    elif mode == "--conformer":
        conformer_main()
    else:
        main()
