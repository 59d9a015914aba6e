#!/usr/bin/env python3
"""Benchmark of the K2TransducerAsr offline hot path on MI355X.

Default workload (BASELINE.json configs[1]): zipformer-large-en offline greedy, batch = 32
synthetic 10 s utterances per GPU.  One step = one pass of the whole path over the rank's shard
of utterances: fbank -> PadSequence (+19 frames, log-floor) -> Zipformer2-large encoder ->
on-device greedy search -> token arrays back in host memory.

Metric: RTFx = audio seconds / wall seconds (inverse of the reference's printed
`rtf = elapsed_ms / total_duration_ms`, K2TransducerAsr.Examples/OfflineRecognizer.cs:185-189),
whole job over all ranks.  `value` is timed with the samples already resident in HBM;
`value_from_host_memory` is the same K steps with the samples in page-locked host memory and
the H2D copy inside the pipeline (the reference's protocol: float[] in, text out).

Multi-GPU: one process per GPU, each rank decodes its own contiguous shard of the utterance list
exactly as the reference would decode that shard as its own GetResults batches; no collective on
the data path (RCCL / gloo carry the timing barrier, the max-over-ranks and the KB-sized gather
of the token lists).  `python bench.py --gpus N` with no WORLD_SIZE in the environment starts the
N ranks itself (before any GPU call); under torch.distributed.run it is one of the ranks.

A plain run times the headline leg only and prints its line.  `--full` adds everything else this
benchmark measures and checks: the host-memory and synchronous-GetResults legs, per-stage timings and
the GEMM roofline, the CPU baseline with `oracle_match`, and on one GPU the configs[2] / [3] / [4] legs.
`--dump-outputs DIR` writes the token ids and timestamps of the last timed step as .npy files.

    python bench.py --gpus 1 --steps 20 --warmup 3
    python bench.py --gpus 1 --steps 20 --warmup 3 --full
    python bench.py --gpus 8 --total-utts 256 --beam 4                              # configs[2]
    python bench.py --gpus 8 --preset conformer-zh --total-utts 64 --batch 8 --seconds 30   # configs[4]
    python bench.py --gpus 2 --dist-backend gloo                                    # rehearsal on one GPU
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PRESET = "zipformer2-large-en"
BATCH = 32
UTT_SECONDS = 10.0
F32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: Peak FP32 (matrix), dense


def _profile_file(pattern):
    """newest committed-profile summary matching `pattern`: from K2HIP_PROFILE_DIR when tools/refresh_profiles.sh is producing a new set (the
    bench record then cites the files of its OWN tag, under the names they are committed as), else from profiles/.  Returns
    (absolute path or None, the profiles/... name the record cites)."""
    import glob
    d = os.environ.get("K2HIP_PROFILE_DIR") or os.path.join(ROOT, "profiles")
    files = sorted(glob.glob(os.path.join(d, pattern)))
    if not files:
        return None, None
    return files[-1], "profiles/" + os.path.basename(files[-1])


def pmc_traffic():
    """HBM bytes per GEMM launch from the committed rocprofv3 PMC passes (cannot be read live:
    counters need their own profiler run).  Valid only for the default workload they were taken on."""
    path, cite = _profile_file("r*_gemm_traffic.json")
    if not path:
        return None, "no PMC summary under profiles/"
    with open(path) as f:
        d = json.load(f)
    return d["hbm_bytes_per_launch"], (f"bytes per launch (fetch {d['fetch_bytes_per_launch']} + write {d['write_bytes_per_launch']}), "
                                       f"from {cite}: {d['method']}")


def pmc_hbm_kernels():
    """per-kernel HBM-side bytes and achieved GB/s of the memory-bound kernels (tools/make_hbm_kernels.py over the same PMC passes)"""
    path, cite = _profile_file("r*_hbm_kernels.json")
    if not path:
        return None
    with open(path) as f:
        d = json.load(f)
    d["from"] = cite
    return d


def log(*a):
    print(*a, file=sys.stderr, flush=True)


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(d, results, first_id):
    """--dump-outputs: what a caller of the timed path receives for each utterance of the last timed step, its token ids and their
    frame timestamps, as [utterances, longest] float64 arrays padded with -1; beside them each row's token count and utterance id.
    Rows beyond the 64 MB budget are left out (the first utterances are kept)."""
    width = max([len(t) for t, _ in results] + [1])
    rows = min(len(results), max(1, DUMP_LIMIT_BYTES // (8 * (2 * width + 2))))
    tok = np.full((rows, width), -1.0)
    ts = np.full((rows, width), -1.0)
    for u, (t, s) in enumerate(results[:rows]):
        tok[u, :len(t)] = t
        ts[u, :len(s)] = s
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, "tokens.npy"), tok)
    np.save(os.path.join(d, "timestamps.npy"), ts)
    np.save(os.path.join(d, "token_counts.npy"), np.array([len(t) for t, _ in results[:rows]], np.float64))
    np.save(os.path.join(d, "utterance_ids.npy"), np.arange(first_id, first_id + rows, dtype=np.float64))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--preset", default=PRESET)
    ap.add_argument("--batch", type=int, default=BATCH, help="utterances per GetResults batch")
    ap.add_argument("--seconds", type=float, default=UTT_SECONDS)
    ap.add_argument("--total-utts", type=int, default=0,
                    help="utterances of the whole job, sharded contiguously over the ranks (strong scaling); "
                         "default = --batch per rank (weak scaling)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-host-leg", action="store_true", help="skip the second timing with samples in host memory")
    ap.add_argument("--no-pipeline", action="store_true", help="one synchronous call per batch (no batch overlap)")
    ap.add_argument("--cpu-utts", type=int, default=0, help="utterances of the CPU-baseline sample (default: one batch)")
    ap.add_argument("--no-secondary", action="store_true", help="skip the bounded configs[2] / [3] / [4] legs that follow the headline run on one GPU")
    ap.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL, one rank per GPU) or gloo (rehearsal of the N > 1 path on one GPU)")
    ap.add_argument("--beam", type=int, default=0, help="0 = greedy_search (headline metric); K = modified_beam_search with beam K (BASELINE configs[2])")
    ap.add_argument("--depth", type=int, default=0, help="batches in flight (0: 2; 3 is allowed with --beam)")
    ap.add_argument("--rotate", type=int, default=3,
                    help="distinct sets of utterances the timed steps cycle through (step s decodes set s %% R: other audio, other emission "
                         "pattern and search length from step to step; every set is checked once against the oracle sample)")
    ap.add_argument("--dump-results", default="", help="rank 0 writes every utterance's (tokens, timestamps) of the last step here (JSON)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline leg: the host-memory and synchronous legs, stage timings and GEMM roofline, the CPU baseline "
                         "and oracle match, and the secondary legs (each still subject to its --no-* switch)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="rank 0 writes the last timed step's token ids and timestamps of every utterance as float64 .npy files under DIR")
    ap.add_argument("--launch-check", action="store_true", help="rendezvous + shard bookkeeping only; no GPU work (CPU test of the launcher)")
    return ap.parse_args(argv)


# ------------------------------------------------------------------------------------------------
# launcher: `python bench.py --gpus N` starts its own ranks.  Nothing here may touch the GPU: the
# children are separate programs, started before any HIP call of this process.
# ------------------------------------------------------------------------------------------------
def launch_ranks(n: int, script: str = None) -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, script or os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    alive = set(range(n))
    while alive:
        for r in sorted(alive):
            code = procs[r].poll()
            if code is None:
                continue
            alive.discard(r)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 1
                log(f"[bench] rank {r} exited with {code}; stopping the other ranks")
                for o in alive:
                    procs[o].terminate()     # exactly the processes started above
        time.sleep(0.05)
    return rc


def ensure_weights(path, preset, rank, barrier):
    from k2transducerasr_amd.synth import write_synthetic_model

    if rank == 0 and not os.path.exists(path):
        tmp = path + f".tmp{os.getpid()}"
        t = time.time()
        write_synthetic_model(tmp, preset)
        os.replace(tmp, path)
        log(f"[bench] wrote synthetic {preset} weights to {path} in {time.time() - t:.1f}s")
    barrier()


def host_cores():
    """threads of the CPU leg: every core this process may USE (all host cores, count stated) unless OMP_NUM_THREADS says
    otherwise -- the affinity mask, cut to the cgroup's CPU quota where one is set, and to the GPU box's CPU share of 16 cores per visible
    GPU (a one-GPU lease of a many-core host shows the host's whole mask: 200 OpenMP threads spinning on a 16-core share do not finish)"""
    if int(os.environ.get("OMP_NUM_THREADS", "0")) > 0:
        return int(os.environ["OMP_NUM_THREADS"])
    n = len(os.sched_getaffinity(0))
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    try:
        import k2transducerasr_amd as pkg
        n_gpu = max(1, pkg.load_library().k2hip_device_count())
    except Exception:  # noqa: BLE001 -- no library / no GPU: the CPU container
        n_gpu = 1
    return max(1, min(n, 16 * n_gpu))


def cpu_model():
    """the host CPU's model string (/proc/cpuinfo; lscpu prints the same line)"""
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.lower().startswith("model name"):
                    return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(weights, n_utts, seconds, beam=0, extra_firsts=()):
    """The CPU restatement (oracle/, 'port') of the same path on this box's host cores, on a bounded sample of the same workload:
    the first `n_utts` utterances as ONE GetResults batch.  Returns the baseline record and the oracle's (tokens, timestamps) per
    utterance, which the caller holds against what the GPU returned for the same batch (`oracle_match`); `extra_firsts`: first
    utterance ids of further batches of the same size to decode as well (untimed: the other sets the timed steps rotate through)."""
    from k2transducerasr_amd.synth import synth_utterance
    from oracle import Oracle

    cores = host_cores()
    os.environ["OMP_NUM_THREADS"] = str(cores)
    ora = Oracle(weights)
    utts = [synth_utterance(u, seconds) for u in range(n_utts)]

    def run(us=None):
        feats = [ora.fbank(u) for u in (us if us is not None else utts)]
        if beam > 0:   # icefall modified_beam_search over the oracle's own encoder output (oracle/k2_oracle_beam.c)
            x = ora.pad_sequence(feats).reshape(len(feats), -1, ora.feature_dim)
            return ora.modified_beam_search(ora.encoder(x), beam)
        return ora.recognize_batch(feats)

    run_one = [synth_utterance(0, 1.0)]
    ora.recognize_batch([ora.fbank(run_one[0])])  # builds the transposed-weight cache
    t = time.time()
    res = run()
    dt = time.time() - t
    extra = [run([synth_utterance(f + i, seconds) for i in range(n_utts)]) for f in extra_firsts]
    # untimed: the oracle's encoder output and joiner logits of the sample batch, for `oracle_match.max_abs_logit_diff` (the caller runs
    # the same operator-level chain on the GPU: fbank -> PadSequence -> EncoderProj -> DecoderProj / JoinerProj)
    logits_ref = None
    if beam == 0 and ora.meta("model_type") not in ("zipformer2ctc",):
        try:
            feats = [ora.fbank(u) for u in utts]
            enc = ora.encoder(ora.pad_sequence(feats).reshape(len(feats), -1, ora.feature_dim))
            ys = np.array([[-1, 0], [5, 7]], np.int64)
            dec = ora.decoder(ys)
            rows = enc[:, ::4, :].reshape(-1, enc.shape[-1])
            logits_ref = {"enc": enc, "ys": ys, "logits": [ora.joiner(rows, np.repeat(dec[c : c + 1], rows.shape[0], 0)) for c in range(2)]}
        except Exception as e:  # noqa: BLE001 -- the record says why the figure is missing
            logits_ref = {"error": repr(e)}
    return {
        "value": round(n_utts * seconds / dt, 2),
        "unit": "x real-time (audio-sec/wall-sec)",
        "cores": cores,
        "cpu_model": cpu_model(),
        "kind": "port",
        "sample": f"{n_utts} x {seconds:g} s utterances of the same synthetic workload as one batch through oracle/ "
                  f"(C + OpenMP restatement{', modified beam search beam=%d' % beam if beam else ''}; the reference's ONNXRuntime path cannot run here), {dt:.2f} s wall",
    }, res, extra, logits_ref


def logit_diff(model, utts, ref):
    """max |GPU - oracle| of encoder_out and of the joiner logits on every 4th frame under two decoder contexts, through the operator-level
    entries (IOfflineProj: k2hip_fbank -> k2hip_pad_sequence -> k2hip_offline_encoder -> k2hip_decoder / k2hip_joiner); north_star: 1e-3."""
    if not ref or "error" in ref:
        return {"error": (ref or {}).get("error", "no reference")}
    feats = [model.fbank(u) for u in utts]
    enc = model.encoder_proj(model.pad_sequence(feats).reshape(len(feats), -1, model.feature_dim))
    dec = model.decoder_proj(ref["ys"])
    rows = enc[:, ::4, :].reshape(-1, enc.shape[-1])
    worst = 0.0
    for c in range(2):
        got = model.joiner_proj(rows, np.repeat(dec[c : c + 1], rows.shape[0], 0))
        worst = max(worst, float(np.abs(got - ref["logits"][c]).max()))
    return {"max_abs_logit_diff": round(worst, 7), "max_abs_encoder_out_diff": round(float(np.abs(enc - ref["enc"]).max()), 7),
            "logit_rows": int(2 * rows.shape[0]), "tolerance": 1e-3}


def dominant_kernel(rows):
    """The instantiation of the GEMM kernel that takes the most time in the instrumented pass, with ITS OWN algorithmic FLOPs and
    HIP-event time (k2hip_get_gemm_profile rows: M, N, K, batch, act, residual, kind, us; kind carries the pipelined kernel's tile)."""
    groups = {}
    for r in rows:
        M, N, K, bat, _, _, kind, us = (float(x) for x in r)
        kind = int(kind)
        if kind & (1 << 20):
            name = f"gemm_f32_mfma_p16<{32 * ((kind >> 8) & 15)}, {32 * ((kind >> 12) & 15)}>"
        elif kind & 128:
            name = f"gemm_f32_mfma_pipe<{32 * ((kind >> 8) & 15)}, {32 * ((kind >> 12) & 15)}>"
        elif kind & 64:
            name = "gemm_f32_mfma_ring"
        elif kind & 32:
            name = "gemm_f32_mfma_skinny"
        elif kind & 16:
            name = "gemm_f32_mfma_dma"
        else:
            name = "gemm_f32_mfma (register-staged: " + ("implicit conv" if (kind & 3) == 1 else "[K,N] operand" if (kind & 3) == 2 else "plain") + ")"
        g = groups.setdefault(name, [0, 0.0, 0.0])
        g[0] += 1
        g[1] += 2.0 * M * N * K * bat
        g[2] += us
    if not groups:
        return None
    name, (n, fl, us) = max(groups.items(), key=lambda kv: kv[1][2])
    ach = fl / (us * 1e-6) / 1e12 if us > 0 else 0.0
    return {"kernel": name, "launches_per_batch": n, "flops_per_batch": fl, "avg_launch_us": round(us / n, 2), "achieved": round(ach, 2),
            "peak": F32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / F32_MFMA_PEAK_TFLOPS, 4),
            "share_of_gemm_time": round(us / sum(g[2] for g in groups.values()), 3)}


def algorithmic_bytes(rows):
    """mean per launch: A + W read once, C written once, the residual read once (f32)"""
    tot = 0.0
    for r in rows:
        M, N, K, bat, _, res, _, _ = (float(x) for x in r)
        tot += 4.0 * bat * (M * K + N * K + M * N * (2.0 if res else 1.0))
    return int(tot / max(len(rows), 1))


def pmc_mfma_busy():
    """MFMA-pipe utilisation of the GEMM kernels from the committed rocprofv3 --pmc pass (SQ_VALU_MFMA_BUSY_CYCLES against
    SQ_BUSY_CU_CYCLES; counters need their own profiler run, so this cannot be read live)."""
    path, cite = _profile_file("r*_gemm_mfma_busy.json")
    if not path:
        return None, "no MFMA PMC summary under profiles/"
    with open(path) as f:
        d = json.load(f)
    return d["mfma_busy"], f"from {cite}: {d['method']}"


def run_secondary(timeout_s=240):
    """Bounded legs for BASELINE configs[2], [3], [4] (one GPU's share each), run as child programs AFTER the headline model has
    been closed, one at a time; each child prints its own JSON line (with its own cpu_baseline and oracle_match), condensed here.
    (16 timed steps each: the timed region ends with the last batch's search running alone, a 5 - 10 ms tail that 6 steps spread thinly.)"""
    here = os.path.dirname(os.path.abspath(__file__))
    legs = {
        "beam4_c2_shard": [sys.executable, os.path.join(here, "bench.py"), "--beam", "4", "--steps", "16", "--warmup", "2",
                           "--no-host-leg", "--no-secondary", "--full"],
        "conformer_zh_c4_shard": [sys.executable, os.path.join(here, "bench.py"), "--preset", "conformer-zh", "--batch", "8",
                                  "--seconds", "30", "--steps", "16", "--warmup", "2", "--no-host-leg", "--no-secondary", "--full"],
        "streaming_c3": [sys.executable, os.path.join(here, "bench_streaming.py"), "--check", "8"],
    }
    out = {}
    for name, cmd in legs.items():
        t = time.time()
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout_s, text=True)
            line = [l for l in p.stdout.splitlines() if l.startswith("{")]
            if not line:
                out[name] = {"error": f"exit {p.returncode}: {p.stderr[-400:]}"}
                continue
            d = json.loads(line[-1])
            out[name] = {
                "metric": d["metric"], "value": d["value"], "unit": d["unit"],
                "ms_per_step": d.get("ms_per_step", d.get("ms_per_chunk_step")),
                "workload": d["config"]["workload"],
                "roofline": {k: d["roofline"][k] for k in ("bound", "achieved", "peak", "unit", "frac") if k in d.get("roofline", {})},
                "cpu_baseline": d.get("cpu_baseline"),
                "oracle_match": d.get("oracle_match"),
                "emission_rate": d.get("emission_rate"),
                "exit_code": p.returncode,
                "wall_s": round(time.time() - t, 1),
            }
            if "tick" in d.get("roofline", {}):
                out[name]["roofline"]["tick_frac_of_mfma_peak"] = d["roofline"]["tick"]["frac_of_mfma_peak"]
        except subprocess.TimeoutExpired:
            out[name] = {"error": f"timed out after {timeout_s} s"}
    return out


def baseline_config_of(args, world, total):
    """which BASELINE.json config (if any) this invocation is"""
    if args.preset == PRESET and args.beam == 0 and args.batch == 32 and abs(args.seconds - 10.0) < 1e-9 and not args.total_utts:
        return "BASELINE.json configs[1]" + ("" if world == 1 else f" per GPU, x{world} GPUs")
    if args.preset == PRESET and args.beam == 4 and abs(args.seconds - 10.0) < 1e-9:
        if total == 256 and world == 8:
            return "BASELINE.json configs[2]"
        return f"BASELINE.json configs[2] at {total} utterances on {world} GPU(s) (the config is 256 on 8)"
    if args.preset == "conformer-zh" and args.beam == 0 and abs(args.seconds - 30.0) < 1e-9:
        if total == 64 and world == 8:
            return "BASELINE.json configs[4]"
        return f"BASELINE.json configs[4] at {total} utterances on {world} GPU(s) (the config is 64 on 8)"
    return "not a BASELINE.json config"


def main():
    args = parse_args()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        log(f"[bench] WORLD_SIZE={world} but --gpus {args.gpus}: refusing to report a line for a different job size")
        sys.exit(2)
    if os.environ.get("K2HIP_BENCH_FAIL_RANK") == str(rank):  # launcher test hook: this rank dies before the rendezvous
        sys.exit(3)
    dist = None
    if world > 1:
        import torch
        import torch.distributed as dist

        if args.dist_backend == "nccl" and not args.launch_check:
            if local_rank >= torch.cuda.device_count():
                log(f"[bench] rank {rank}: no GPU {local_rank} on this node ({torch.cuda.device_count()} visible); "
                    "use --dist-backend gloo to rehearse N ranks on fewer GPUs")
                sys.exit(4)
            torch.cuda.set_device(local_rank)
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend="gloo")

    def barrier():
        if dist is not None:
            dist.barrier()

    from k2transducerasr_amd.shard import batches_of, gather_results, max_over_ranks, shard_range

    B, secs = args.batch, args.seconds
    total = args.total_utts or B * world
    lo, hi = shard_range(total, world, rank)
    my_batches = batches_of(lo, hi, B)          # [(first utterance id, count)]: the GetResults batches of this rank
    if args.launch_check:
        got = gather_results(dist, [(rank, lo, hi, my_batches)], world, rank)
        barrier()
        if rank == 0:
            print(json.dumps({"launch_check": True, "n_gpus": world, "total_utts": total, "shards": got}), flush=True)
        if dist is not None:
            dist.destroy_process_group()
        return

    import k2transducerasr_amd as pkg
    from k2transducerasr_amd.synth import synth_utterance

    weights = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"k2hip_bench_{args.preset}.k2w")
    ensure_weights(weights, args.preset, rank, barrier)

    n_dev = pkg.load_library().k2hip_device_count()
    device = local_rank if args.dist_backend == "nccl" else local_rank % max(n_dev, 1)  # gloo rehearsal: ranks may share a GPU
    model = pkg.Model(weights, device)  # no fallback: raises without a GPU / library
    if args.beam > 0:
        model.set_decoding_method("modified_beam_search", args.beam)
    # batches in flight (k2hip.h K2HIP_MAX_BATCHES_IN_FLIGHT = 3): two for the greedy search (it hides under the next encoder); three for
    # the beam search, whose per-frame launches take longer than an encoder pass when they share the GPU with one
    # (with the beam search as one kernel per batch a third batch in flight no longer pays: 14.90 - 14.93 ms at depth 2, 14.95 - 15.01 at 3)
    depth = args.depth if args.depth > 0 else 2
    n_each = int(round(secs * 16000))
    # Step s decodes utterance SET s % R: set r holds the utterances u + r * total (u = the job's utterance ids), so consecutive steps
    # see other audio -- other emission patterns, search lengths and cache contents -- instead of one batch decoded over and over.
    # Utterance u is the same signal whichever rank decodes it (seed = u).
    R = max(1, min(args.rotate, args.steps))
    nb = len(my_batches)
    host = [[None] * nb for _ in range(R)]
    dev = [[None] * nb for _ in range(R)]
    for r in range(R):
        for i, (first, cnt) in enumerate(my_batches):
            h = model.host_alloc((cnt, n_each))
            for k in range(cnt):
                h[k] = synth_utterance(r * total + first + k, secs)
            d = model.device_alloc(h.nbytes)
            model.device_upload(d, h)
            host[r][i] = h
            dev[r][i] = d

    def submit(r, i, from_host):
        cnt = my_batches[i][1]
        return model.offline_submit_samples(host[r][i], None) if from_host else model.offline_submit_samples_dev(dev[r][i], n_each, cnt)

    def run_steps(n, from_host=False):
        """n passes over the rank's batches (pass s over utterance set s % R), software-pipelined `depth` deep: the next batch(es) are
        submitted before the oldest one's tokens are collected, so its encoder (and, from host memory, its H2D copy) overlaps that
        batch's search.  Every batch's tokens are back in host memory before this returns; returns the results of the last pass over
        each set, [set][batch] in utterance order."""
        last = [[None] * nb for _ in range(R)]
        if n == 0 or nb == 0:
            return last
        seq = [(s % R, i) for s in range(n) for i in range(nb)]
        if args.no_pipeline:
            for r, i in seq:
                last[r][i] = model.offline_wait(submit(r, i, from_host))
            return last
        pending = []  # ((set, batch index), ticket), oldest first: `depth` batches in flight
        for k in range(len(seq)):
            pending.append((seq[k], submit(seq[k][0], seq[k][1], from_host)))
            if len(pending) == depth:
                (r0, i0), tk = pending.pop(0)
                last[r0][i0] = model.offline_wait(tk)
        for (r0, i0), tk in pending:
            last[r0][i0] = model.offline_wait(tk)
        return last

    def timed(from_host):
        run_steps(args.warmup, from_host)
        model.synchronize()
        barrier()
        t0 = time.perf_counter()
        r = run_steps(args.steps, from_host)
        model.synchronize()
        barrier()
        el = time.perf_counter() - t0
        return r, max_over_ranks(dist, el, device="cuda" if (dist is not None and args.dist_backend == "nccl") else None)

    log(f"[bench] rank {rank}: timed leg, samples resident in HBM")
    res_sets, elapsed = timed(False)
    host_elapsed = None
    if args.full and not args.no_host_leg:
        log(f"[bench] rank {rank}: timed leg, samples in host memory (pipelined)")
        res_h, host_elapsed = timed(True)
        assert res_h == res_sets, "results from host memory and from device memory differ"
    # The call shape OfflineRecognizer.GetResults has today (OfflineRecognizer.cs:85-91 behind OfflineStream.AddSamples, OfflineStream.cs:43-57)
    # and the shipped C# binding produces (csharp/OfflineRecognizer.Hip.cs): per batch, B x CreateOfflineStream + AddSamples(host samples),
    # ONE synchronous GetResults (samples H2D, batched fbank, pad, encoder, search, tokens D2H -- nothing of the next batch overlaps it),
    # Tokens / Timestamps pulled into host lists.  Same utterance sets, same rotation; results must equal the pipelined legs'.
    sync_elapsed = None
    if args.full and not args.no_host_leg and not args.no_pipeline:
        import ctypes as C
        L = model._L

        def sync_steps(n):
            last = [[None] * nb for _ in range(R)]
            for s_ in range(n):
                r = s_ % R
                for i, (first, cnt) in enumerate(my_batches):
                    streams = [pkg.OfflineStream(model) for _ in range(cnt)]
                    for k, st in enumerate(streams):
                        st.add_samples(host[r][i][k])
                    arr = (C.c_void_p * cnt)(*[st._h for st in streams])
                    model._chk(L.k2hip_offline_recognizer_get_results(model.handle, arr, cnt))
                    last[r][i] = [(st.tokens[2 * cnt:], st.timestamps[2 * cnt:]) for st in streams]   # (behind the 2 x B blank prefix, :250-267)
                    for st in streams:
                        st.close()
            return last
        log(f"[bench] rank {rank}: timed leg, synchronous GetResults from host samples")
        sync_steps(min(args.warmup, 2))
        model.synchronize()
        barrier()
        t0 = time.perf_counter()
        res_s = sync_steps(args.steps)
        model.synchronize()
        barrier()
        sync_elapsed = max_over_ranks(dist, time.perf_counter() - t0, device="cuda" if (dist is not None and args.dist_backend == "nccl") else None)
        assert res_s == res_sets, "the synchronous GetResults route and the pipelined route give different results"
    res = res_sets[0]                                   # set 0 = the job's own utterance ids 0 .. total-1
    local = [r for batch in res for r in batch]
    allres = gather_results(dist, local, world, rank)   # rank order == utterance order
    other_sets = [gather_results(dist, [x for batch in res_sets[r] if batch is not None for x in batch], world, rank) for r in range(1, R)]

    # one synchronous pass over the first batch: per-stage HIP-event timings + pipelined == synchronous check
    stages = it = gemm_rows = None
    if args.full and nb:
        res_sync = model.offline_greedy_from_samples_dev(dev[0][0], n_each, my_batches[0][1])
        stages = model.timing()
        assert res_sync == res[0], "pipelined and synchronous results differ"
        # roofline of the dominant kernel (fp32 MFMA GEMM): one extra instrumented pass over the same batch, HIP events
        # recorded around every GEMM launch on the engine's own stream (no per-launch sync, launches stay back to back).
        model.set_instrument(True)
        model.offline_greedy_from_samples_dev(dev[0][0], n_each, my_batches[0][1])
        it = model.timing()
        gemm_rows = model.gemm_profile()
        model.set_instrument(False)

    bad_match = False
    if rank == 0:
        assert len(allres) == total, f"gathered {len(allres)} results for {total} utterances"
        audio = args.steps * total * secs
        value = audio / elapsed
        ach = it["gemm_flops"] / (it["gemm_ms"] * 1e-3) / 1e12 if it and it["gemm_ms"] > 0 else 0.0
        default_workload = args.preset == PRESET and B == BATCH and abs(secs - UTT_SECONDS) < 1e-9 and args.beam == 0 and not args.total_utts
        traffic, traffic_note = pmc_traffic() if default_workload else (None, "PMC passes exist for the default workload only")
        method = "greedy" if args.beam == 0 else f"modified-beam-search beam={args.beam}"
        tprime = max(1, model.encoder_out_frames(model.fbank_num_frames(n_each) + 19))
        n_tok = int(sum(len(r[0]) for r in allres))
        n_tok_sets = [n_tok] + [int(sum(len(r[0]) for r in s_)) for s_ in other_sets]
        out = {
            "metric": "RTFx (audio-sec/wall-sec) offline Zipformer greedy" if default_workload else f"RTFx (audio-sec/wall-sec) offline {args.preset} {method}",
            "value": round(value, 1),
            "unit": "audio-sec/wall-sec",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "strong" if args.total_utts else "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {
                "workload": f"{args.preset} offline {method}, {total} synthetic {secs:g} s utterances per step in GetResults batches of "
                            f"{B} ({baseline_config_of(args, world, total)}); samples resident in HBM, tokens returned to host",
                "batch": B,
                "total_utts_per_step": total,
                "utt_seconds": secs,
                "parallelism": f"utterance-sharded x{world} ({'one rank per GPU, RCCL' if args.dist_backend == 'nccl' else 'gloo rehearsal, ranks share GPUs'}), "
                               "no data-path collective",
                "pipeline": "synchronous" if args.no_pipeline else ("2 batches in flight (search of batch i overlaps encoder of i+1)" if depth == 2 else
                             "3 batches in flight (the beam searches of batches i and i+1 overlap each other and the encoder of i+2)"),
                "weights": f"seeded random init of the {args.preset} architecture (no checkpoints available)",
            },
            "tokens_emitted_per_step": n_tok,
            "emission_rate": round(n_tok / (total * tprime), 4),
            "results_sha1": hashlib.sha1(json.dumps(allres).encode()).hexdigest()[:16],
            "rotation": {"sets": R, "tokens_emitted_per_set": n_tok_sets,
                         "what": f"step s decodes utterance set s % {R}; set r holds the utterances r * {total} .. r * {total} + {total - 1} "
                                 "(other audio in consecutive steps); `results_sha1`, `tokens_emitted_per_step` and `emission_rate` are set 0's"},
        }
        out["value_note"] = ("`value` is the HBM-resident leg, as this build's measurement contract prescribes (inputs resident in HBM when the timed "
                             "region starts; a PCIe-inclusive rate is never `value`); SURVEY 8(d)'s host-memory definition is `value_from_host_memory` "
                             "(pipelined: k2hip_offline_submit_samples / wait, 2 batches in flight) and `value_sync_get_results` (the call shape "
                             "OfflineRecognizer.GetResults has and the shipped C# binding produces: one synchronous native GetResults per batch)")
        if host_elapsed is not None:
            out["value_from_host_memory"] = round(audio / host_elapsed, 1)
            out["ms_per_step_from_host_memory"] = round(host_elapsed / args.steps * 1e3, 3)
        if sync_elapsed is not None:
            out["value_sync_get_results"] = round(audio / sync_elapsed, 1)
            out["ms_per_step_sync_get_results"] = round(sync_elapsed / args.steps * 1e3, 3)
            out["sync_get_results_what"] = ("host samples -> B x (k2hip_offline_stream_create + accept_samples) -> k2hip_offline_recognizer_get_results "
                                            "(fbank on the GPU, one call per batch, nothing in flight beside it) -> Tokens / Timestamps in host lists; "
                                            "timed through the ctypes binding (7 calls per stream and batch: ~0.3 ms of interpreter time per batch that a "
                                            "P/Invoke host does not pay)")
        if it:
            out["roofline"] = {
                "kernel": "gemm_f32_mfma (all Linear / pointwise-conv / implicit-conv / attention-apply launches)",
                "bound": "mfma",
                "achieved": round(ach, 2),
                "peak": F32_MFMA_PEAK_TFLOPS,
                "unit": "TFLOP/s",
                "frac": round(ach / F32_MFMA_PEAK_TFLOPS, 4),
                "traffic": traffic,
                "traffic_note": traffic_note,
                "launches_per_batch": it["gemm_launches"],
                "flops_per_batch": it["gemm_flops"],
                "avg_launch_us": round(it["gemm_ms"] * 1e3 / max(it["gemm_launches"], 1), 2),
                "all_matrix_flops_per_batch": it["total_flops"],
                "algorithmic_bytes": algorithmic_bytes(gemm_rows),
                "algorithmic_bytes_note": "mean per launch over the same launches as `traffic`: A and W read once, C written once, a residual read once (f32); "
                                          "what `traffic` holds beyond it is the operands crossing the fabric once per XCD that needs them (8 private L2s: "
                                          "PN x A + (8 / PN) x W with the tile order's PN panels of N per launch), served by the memory-side cache (DESIGN 4)",
                "dominant": dominant_kernel(gemm_rows),
            }
            out["stages_ms_one_synchronous_batch"] = {k: round(stages[k], 3) for k in ("total_ms", "fbank_ms", "pad_ms", "encoder_ms", "greedy_ms", "d2h_ms")}
            # counters need their own profiler run: this is NOT measured by this process -- it is read from the committed profile named
            # in `source` and says so (a kernel change without a refreshed profile leaves it stale; `traffic` above is of the same kind)
            mb, mb_note = pmc_mfma_busy() if default_workload else (None, "PMC passes exist for the default workload only")
            out["roofline"]["committed_profile"] = {"mfma_busy": mb, "source": mb_note}
            # north_star: "rocprof HBM GB/s ... against gfx950 peak" -- the HBM-bound kernels of the batch, each against the 8 TB/s peak
            out["roofline"]["hbm_kernels"] = pmc_hbm_kernels() if default_workload else None
        if args.full and world == 1 and not args.no_cpu_baseline:
            n_cpu = args.cpu_utts or my_batches[0][1]
            whole = my_batches[0] == (0, n_cpu)
            log(f"[bench] CPU restatement on {host_cores()} host threads ({cpu_model()})")
            cb, ores, ores_extra, logits_ref = cpu_baseline(weights, n_cpu, secs, args.beam, [r * total for r in range(1, R)] if whole else [])
            out["cpu_baseline"] = cb
            # the oracle's results for the sample against what the timed legs returned for the same batch (outside the timed region);
            # and, untimed, the first batch of every other set the timed steps rotated through
            if whole:
                same = lambda g, w: [list(g[0]), list(g[1])] == [list(w[0]), list(w[1])]   # noqa: E731
                exact = sum(1 for g, w in zip(allres[:n_cpu], ores) if same(g, w))
                per_set = [exact] + [sum(1 for g, w in zip(s_[:n_cpu], o_) if same(g, w)) for s_, o_ in zip(other_sets, ores_extra)]
                out["oracle_match"] = {"streams": n_cpu * len(per_set), "exact": sum(per_set), "exact_per_set": per_set,
                                       "what": "tokens and timestamps of the timed legs' first batch of EVERY utterance set == oracle/ on the same batch"}
                # greedy: every set must be exact.  Beam search: set 0 must be; on other audio ~1 stream in 20 meets a frame whose candidates
                # are closer than the two encoders agree (tests/parity.py localises those frame by frame; this line only counts them)
                bad_match = per_set[0] < n_cpu or (args.beam == 0 and sum(per_set) < n_cpu * len(per_set))
                if logits_ref is not None:   # north_star: "fp32 logits within 1e-3" -- measured here, next to the token match
                    from k2transducerasr_amd.synth import synth_utterance as _su
                    ld = logit_diff(model, [_su(u, secs) for u in range(n_cpu)], logits_ref)
                    out["oracle_match"]["logits"] = ld
                    bad_match = bad_match or ld.get("max_abs_logit_diff", 1.0) > 1e-3
            else:
                out["oracle_match"] = {"streams": 0, "exact": 0, "what": "the CPU sample is not one of the timed batches"}
        if args.dump_results:
            with open(args.dump_results, "w") as f:
                json.dump({"results": allres, "batches_per_rank": nb, "n_gpus": world}, f)
        if args.dump_outputs:
            last = (args.steps - 1) % R                 # the utterance set the last timed step decoded
            dump_outputs(args.dump_outputs, ([allres] + other_sets)[last], last * total)
    for r in range(R):
        for h, d in zip(host[r], dev[r]):
            model.device_free(d)
            model.host_free(h)
    model.close()
    if rank == 0:
        if args.full and world == 1 and default_workload and not args.no_secondary:
            out["secondary"] = run_secondary()   # the GPU is free again: one child program per leg
            bad_match = bad_match or any(("error" in v) or v.get("exit_code") for v in out["secondary"].values())
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()
    if rank == 0 and bad_match:
        log("[bench] oracle_match failed (or a secondary leg failed): see the JSON line")
        sys.exit(5)


if __name__ == "__main__":
    main()
