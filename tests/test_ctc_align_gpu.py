"""CTC forced alignment and full-sum scoring on the GPU (csrc/ctc_align.hip through k2hip_ctc_align,
k2hip_offline_ctc_align_from_samples and the debug op "ctc_lattice"), against the float64 twin (tests/ctc_align_twin.py).

Bounds (none of them taken from what the engine gives):
  * the kernel alone on log_probs whose entries are multiples of 0.25: sums along a path are exact in float32, so best, the timestamps,
    the end frames and the token log-probs are exact; total is held to 1e-5 relative (float32 rounding of exp / log1p in the forward
    sums), the bound tests/test_align_gpu.py uses for the same kind of recursion;
  * end to end: the twin is fed the log_probs the encoder entry returns for the same padded batch, so the only difference is the
    recursion's arithmetic: total and best within 1e-5 relative of max(1, |value|), token log-probs exact;
  * against the search: the per-frame argmax path is the best of ALL labellings and spells the greedy result, so with that result as the
    target best_logp = the sum of the row maxima (1e-5 relative) and the timestamps are the greedy ones.

Worst differences seen on an MI355X are recorded in DESIGN.md "CTC forced alignment and full-sum scoring"."""
import ctypes as C

import numpy as np
import pytest

from ctc_align_twin import ctc_lattice, min_frames, path_score

pytestmark = pytest.mark.gpu

REL = 1e-5


def rel(got, want):
    return abs(float(got) - want) / max(1.0, abs(want))


@pytest.fixture(scope="module")
def ctc_path(tmp_path_factory):
    from k2transducerasr_amd.synth import write_synthetic_model
    p = str(tmp_path_factory.mktemp("ctcalign") / "ctc_tiny.k2w")
    write_synthetic_model(p, "zipformer2-ctc-tiny-test")
    return p


@pytest.fixture(scope="module")
def hip_ctc(ctc_path):
    from k2transducerasr_amd import Model
    return Model(ctc_path, 0)


@pytest.fixture(scope="module")
def oracle_ctc(ctc_path):
    from oracle import Oracle
    return Oracle(ctc_path)


@pytest.fixture(scope="module")
def device_log_probs(hip_ctc, utts):
    """log_probs [B, T', V] of the padded fixture batch from the existing encoder entry, on the engine's own features"""
    feats = [hip_ctc.fbank(u) for u in utts]
    return hip_ctc.encoder_proj(hip_ctc.pad_sequence(feats).reshape(len(utts), -1, 80))


@pytest.fixture(scope="module")
def greedy(hip_ctc, utts):
    return hip_ctc.offline_greedy_from_samples(utts)


@pytest.fixture(scope="module")
def untied(oracle_ctc, utts):
    """streams none of whose frames has a tied maximum, decided on the CPU with the oracle's log_probs; at most one in four is dropped"""
    f = [oracle_ctc.fbank(u) for u in utts]
    lp = oracle_ctc.encoder(oracle_ctc.pad_sequence(f).reshape(len(utts), -1, 80))
    top = np.sort(lp, axis=2)
    keep = [b for b in range(len(utts)) if np.all(top[b, :, -1] > top[b, :, -2])]
    assert 4 * (len(utts) - len(keep)) <= len(utts), keep
    return keep


def debug_op(model, name, iargs, bufs, outs):
    from k2transducerasr_amd import load_library
    L = load_library()
    L.k2hip_debug_op_run.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                     C.c_int32, C.c_uint32]
    n = len(bufs)
    ptrs = (C.c_void_p * n)(*[b.ctypes.data if b is not None and b.size else None for b in bufs])
    sizes = (C.c_int64 * n)(*[b.nbytes if b is not None else 0 for b in bufs])
    ia = (C.c_int64 * len(iargs))(*[int(v) for v in iargs])
    rc = L.k2hip_debug_op_run(model.handle, name.encode(), ia, len(iargs), ptrs, sizes, n, sum(1 << k for k in outs))
    assert rc == 0, (name, rc, L.k2hip_last_error())


# (row, T of that row, U, how the target is made).  Rows are shared through stream_of: (1,0) and (1,1); (70,31) and (70,32) -- S = 63 and
# 65, either side of a ballot word; (300,127) and (300,128) -- S = 255 and 257, either side of the workgroup loop.  (7,3) is `a a b`: the
# repeated token needs its blank.  (40,40) without repeats is the single-path trellis.
KERNEL_CASES = [(0, 1, 0, "random"), (0, 1, 1, "random"), (1, 2, 1, "random"), (2, 7, 3, "aab"), (3, 70, 31, "random"), (3, 70, 32, "random"),
                (4, 300, 127, "random"), (4, 300, 128, "random"), (5, 40, 40, "distinct")]
KERNEL_ROW_FRAMES = [1, 2, 7, 70, 300, 40]


def kernel_inputs(V):
    rng = np.random.default_rng(17)
    R, Tp = len(KERNEL_ROW_FRAMES), max(KERNEL_ROW_FRAMES)
    lp = (-0.25 * rng.integers(0, 13, size=(R, Tp, V))).astype(np.float32)
    for r in (3, 4):   # -inf cells where there are many paths
        lp[r][rng.random((Tp, V)) < 0.02] = -np.inf
    targets = []
    for _, T, U, how in KERNEL_CASES:
        if how == "aab":
            y = np.array([5, 5, 9], np.int64)
        elif how == "distinct":
            y = (1 + (np.arange(U) % (V - 1))).astype(np.int64)
        else:
            y = rng.integers(1, V, size=U).astype(np.int64)
        assert min_frames(y) <= T
        targets.append(y)
    return lp, targets


def test_kernel_alone_is_exact_on_quarters(hip_ctc):
    """"ctc_lattice" between guard pages on log_probs of multiples of 0.25 with -inf cells, nine targets in one call with ragged n_frames,
    three pairs of them sharing a row"""
    V = hip_ctc.vocab_size
    assert V == 37
    lp, targets = kernel_inputs(V)
    R, Tp, _ = lp.shape
    H = len(KERNEL_CASES)
    nf = np.array(KERNEL_ROW_FRAMES, np.int32)
    so = np.array([c[0] for c in KERNEL_CASES], np.int32)
    lens = np.array([t.size for t in targets], np.int32)
    ids = np.concatenate(targets).astype(np.int64)
    mt = int(lens.max())
    ts = np.full((H, mt), -7, np.int32)
    en = np.full((H, mt), -7, np.int32)
    yp = np.full((H, mt), -7, np.float32)
    sc = np.full((H, 2), -7, np.float32)
    debug_op(hip_ctc, "ctc_lattice", [R, Tp, H, mt], [lp, nf, so, ids, lens, ts, en, yp, sc], outs=(5, 6, 7, 8))
    worst = 0.0
    for h, (r, T, U, _) in enumerate(KERNEL_CASES):
        want = ctc_lattice(lp[r, :T].astype(np.float64), targets[h])
        assert np.isfinite(want["best"]), h
        assert sc[h, 1] == np.float32(want["best"]), (h, sc[h, 1], want["best"])
        assert ts[h, :U].tolist() == want["timestamps"], h
        assert en[h, :U].tolist() == want["end_frames"], h
        assert np.array_equal(yp[h, :U], want["token_log_probs"].astype(np.float32)), h
        worst = max(worst, rel(sc[h, 0], want["total"]))
        assert rel(sc[h, 0], want["total"]) <= REL, (h, sc[h, 0], want["total"])
        assert sc[h, 1] <= sc[h, 0]
        if U == T:
            assert sc[h, 0] == sc[h, 1] and want["timestamps"] == list(range(T))
    assert ts[3, :3].tolist()[1] > en[3, 0] + 1     # a a b: a blank frame between the repeated tokens
    print(f"ctc_lattice: worst relative difference of total {worst:.3g} (bound {REL:g})")


E2E_LENS = [6, 3, 0, 9, 2]


def e2e_targets(V, B):
    rng = np.random.default_rng(23)
    tg = [rng.integers(1, V, size=n).astype(np.int64) for n in E2E_LENS[:B]]
    tg[0][2] = tg[0][1]          # one repeated pair
    tg[1][0] = 2                 # unk is legal on the CTC path
    return tg


def test_end_to_end_against_the_twin(hip_ctc, utts, device_log_probs):
    B, Tp, V = device_log_probs.shape
    tg = e2e_targets(V, B)
    got = hip_ctc.ctc_align_samples(utts, tg)
    lp64 = device_log_probs.astype(np.float64)
    worst = dict(total=0.0, best=0.0, path=0.0, token=0.0)
    fails = []
    for b in range(B):
        g, w = got[b], ctc_lattice(lp64[b], tg[b])
        U = len(tg[b])
        ts, en = g["timestamps"], g["end_frames"]
        assert len(ts) == U == len(en) and all(0 <= a <= e < Tp for a, e in zip(ts, en)) and all(e < a for e, a in zip(en, ts[1:])), (b, ts, en)
        rescored = path_score(lp64[b], tg[b], ts, en)       # the engine's path under the twin's cells: no stream is excused
        d = dict(total=rel(g["total_logp"], w["total"]), best=rel(g["best_logp"], w["best"]), path=rel(rescored, w["best"]),
                 token=float(np.abs(g["token_log_probs"] - device_log_probs[b][ts, tg[b]]).max()) if U else 0.0)
        for k in worst:
            worst[k] = max(worst[k], d[k])
        if d["total"] > REL or d["best"] > REL or d["path"] > REL or d["token"] != 0.0 or not g["best_logp"] <= g["total_logp"]:
            fails.append((b, d))
    print("Model.ctc_align_samples against the twin, worst differences: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) +
          f" (bound {REL:g} relative, token exact)")
    assert not fails, fails


def test_best_path_of_the_greedy_result_is_the_argmax_path(hip_ctc, utts, device_log_probs, greedy, untied):
    tg = [np.array(tok, np.int64) for tok, _ in greedy]
    assert sum(t.size for t in tg) > 0
    got = hip_ctc.ctc_align_samples(utts, tg)
    worst = 0.0
    for b in untied:
        want = float(device_log_probs[b].astype(np.float64).max(axis=1).sum())
        worst = max(worst, rel(got[b]["best_logp"], want))
        assert rel(got[b]["best_logp"], want) <= REL, (b, got[b]["best_logp"], want)
        assert got[b]["timestamps"] == list(greedy[b][1]), (b, got[b]["timestamps"], greedy[b][1])
        assert got[b]["total_logp"] >= got[b]["best_logp"]
    print(f"best_logp of the greedy targets against the sum of the row maxima: worst relative difference {worst:.3g} (bound {REL:g})")


def test_rescoring_a_candidate_list_against_one_row(hip_ctc, utts, greedy, untied):
    b = next(b for b in untied if len(greedy[b][0]) >= 2)
    V = hip_ctc.vocab_size
    g = np.array(greedy[b][0], np.int64)
    sub = g.copy()
    sub[len(g) // 2] = 1 + (int(g[len(g) // 2]) % (V - 1))       # another id in [1, V)
    assert sub[len(g) // 2] != g[len(g) // 2]
    cands = [g, sub, np.delete(g, len(g) // 2)]
    got = hip_ctc.ctc_align_samples(utts, cands, stream_of=[b, b, b])
    for k, y in enumerate(cands):
        alone = hip_ctc.ctc_align_samples(utts, [y], stream_of=[b])[0]
        assert got[k]["timestamps"] == alone["timestamps"] and got[k]["end_frames"] == alone["end_frames"], k
        assert got[k]["total_logp"] == alone["total_logp"] and got[k]["best_logp"] == alone["best_logp"], k
        assert np.array_equal(got[k]["token_log_probs"], alone["token_log_probs"]), k
    assert got[0]["best_logp"] > got[1]["best_logp"] and got[0]["best_logp"] > got[2]["best_logp"], [x["best_logp"] for x in got]


def test_host_entry_equals_the_fused_one_and_the_recognizer_dispatches(hip_ctc, ctc_path, utts, device_log_probs):
    """Model.ctc_align on the encoder entry's log_probs gives what ctc_align_samples gives; OfflineRecognizer.align on a CTC model is the
    CTC form"""
    from k2transducerasr_amd import OfflineRecognizer
    B, Tp, V = device_log_probs.shape
    tg = e2e_targets(V, B)
    host = hip_ctc.ctc_align(device_log_probs, tg)
    fused = hip_ctc.ctc_align_samples(utts, tg)
    for h, f in zip(host, fused):
        assert h["timestamps"] == f["timestamps"] and h["end_frames"] == f["end_frames"]
        assert rel(f["total_logp"], h["total_logp"]) <= REL and rel(f["best_logp"], h["best_logp"]) <= REL
    short = hip_ctc.ctc_align(device_log_probs, tg, n_frames=np.full(B, Tp - 2, np.int32))
    assert all(e < Tp - 2 for s in short for e in s["end_frames"])
    rec = OfflineRecognizer(ctc_path)
    try:
        via = rec.align(utts, tg)
        assert [v["timestamps"] for v in via] == [f["timestamps"] for f in fused] and "end_frames" in via[0]
    finally:
        rec.model.close()


def test_errors_on_the_device_build(hip_ctc, hip_tiny, utts, device_log_probs):
    from k2transducerasr_amd import K2HipError
    B, Tp, V = device_log_probs.shape
    good = e2e_targets(V, B)
    ref = hip_ctc.ctc_align(device_log_probs, good)
    with pytest.raises(K2HipError) as e:                       # a transducer model has no CTC head
        hip_tiny.ctc_align(np.zeros((1, 4, hip_tiny.vocab_size), np.float32), [np.array([3], np.int64)])
    assert e.value.code == -6, (e.value.code, str(e.value))
    with pytest.raises(K2HipError) as e:
        hip_tiny.ctc_align_samples(utts[:1], [np.array([3], np.int64)])
    assert e.value.code == -6, (e.value.code, str(e.value))
    long = [t.copy() for t in good]
    long[1] = (1 + (np.arange(Tp + 1) % 2)).astype(np.int64)    # Tp + 1 tokens: one frame too long
    for fn in (lambda: hip_ctc.ctc_align(device_log_probs, long), lambda: hip_ctc.ctc_align_samples(utts, long)):
        with pytest.raises(K2HipError) as e:
            fn()
        assert e.value.code == -1 and "target 1" in str(e.value), (e.value.code, str(e.value))
    again = hip_ctc.ctc_align(device_log_probs, good)
    assert [(a["timestamps"], a["total_logp"], a["best_logp"]) for a in again] == [(a["timestamps"], a["total_logp"], a["best_logp"]) for a in ref]


def test_fused_align_changes_no_fused_search(hip_ctc, utts, greedy, untied):
    """offline_greedy_from_samples gives identical results before and after fused CTC align calls with more targets than streams (H = 7
    rows in the output block against B = 5) and with fewer (H = 1)"""
    before = hip_ctc.offline_greedy_from_samples(utts)
    assert len(utts) == 5
    b = next(b for b in untied if len(greedy[b][0]) >= 2)
    V = hip_ctc.vocab_size
    g = np.array(greedy[b][0], np.int64)
    cands = []
    for k in range(6):                                            # six substitutions of the greedy result, then the result itself
        sub = g.copy()
        sub[k % len(g)] = 1 + ((int(g[k % len(g)]) + k) % (V - 1))
        cands.append(sub)
    cands.append(g)
    many = hip_ctc.ctc_align_samples(utts, cands, stream_of=[b] * 7)
    assert [len(x["timestamps"]) for x in many] == [len(y) for y in cands]
    assert hip_ctc.offline_greedy_from_samples(utts) == before
    one = hip_ctc.ctc_align_samples(utts, [g], stream_of=[b])
    assert one[0]["timestamps"] == many[6]["timestamps"] and one[0]["best_logp"] == many[6]["best_logp"]
    assert hip_ctc.offline_greedy_from_samples(utts) == before
