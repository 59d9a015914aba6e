"""GPU tests of the sample-rate converter (csrc/resample.hip): the kernel alone through k2hip_debug_op_run "resample_gather" against the
float32 host reference bit for bit (the sign of a zero aside) and against the float64 twin within the dot product's own bound, the
state an OnlineStream carries across pushes, and accept_waveform end to end, offline and streaming, against accept_samples of the host
reference's output."""
import ctypes as C

import numpy as np
import pytest

from resample_twin import RefStream, Twin, bound, lib_plan, ref_resample, same_bits

pytestmark = pytest.mark.gpu

RATES = (8000, 11025, 44100, 48000)
FO = 16000
TILE = 1024   # kResampleTile (csrc/kernels.h)
KINDS = ("random", "impulse", "constant", "alternating")


@pytest.fixture(scope="module")
def twins():
    return {fi: Twin(fi, FO) for fi in RATES}


def make_input(kind, n, seed):
    if kind == "random":
        return np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(np.float32)
    if kind == "impulse":
        x = np.zeros(n, np.float32)
        x[n // 3] = 1.0
        return x
    if kind == "constant":
        return np.full(n, 0.75, np.float32)
    return np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(np.float32)   # full-scale alternating


def start(tw, k):
    return tw.first[k % tw.ou] + (k // tw.ou) * tw.iu


def end(tw, k):
    return start(tw, k) + tw.ntaps[k % tw.ou]


class Launch:
    """one "resample_gather" launch: rows over pieces of ONE samples buffer, outputs pre-filled with NaN"""

    def __init__(self, n_dst, nmax):
        self.n_dst, self.nmax, self.rows, self.chunks, self.pos = n_dst, nmax, [], [], 0

    def put(self, x, misalign=0):
        """x into the samples buffer, on a 16-byte boundary plus `misalign` floats; returns its float offset"""
        pad = (-self.pos) % 4 + misalign
        self.chunks.append(np.full(pad, np.nan, np.float32))   # (what lies between pieces must never reach an output)
        off = self.pos + pad
        self.chunks.append(np.asarray(x, np.float32))
        self.pos = off + len(x)
        return off

    def row(self, fi, head, tail, x0, k0, n_out, dst_row, mis_head=0, mis_tail=0):
        oh, ot = self.put(head, mis_head), self.put(tail, mis_tail)
        self.rows.append([fi, FO if fi else 0, oh, len(head), ot, len(tail), x0, k0, n_out, dst_row])

    def run(self, model):
        L = model._L
        L.k2hip_debug_op_run.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                         C.c_int32, C.c_uint32]
        samples = np.concatenate(self.chunks + [np.full(4, np.nan, np.float32)])
        dst = np.full((self.n_dst, self.nmax), np.nan, np.float32)
        ints = [len(self.rows), self.n_dst, self.nmax] + [v for r in self.rows for v in r]
        ia = (C.c_int64 * len(ints))(*ints)
        ptrs = (C.c_void_p * 2)(samples.ctypes.data, dst.ctypes.data)
        sizes = (C.c_int64 * 2)(samples.nbytes, dst.nbytes)
        rc = L.k2hip_debug_op_run(model.handle, b"resample_gather", ia, len(ints), ptrs, sizes, 2, 2)
        assert rc == 0, L.k2hip_last_error()
        return dst


def check_row(got, want32, want64, mag, nt, what):
    n = len(want32)
    assert same_bits(got[:n], want32), what
    assert np.all(got[n:] == 0), what   # zero-filled to nmax, nothing left of the NaN fill
    if n:
        err = np.abs(got[:n].astype(np.float64) - want64)
        assert np.all(err <= bound(mag, nt)), (what, err.max())


@pytest.mark.parametrize("fi", RATES)
def test_kernel_counts_and_inputs(hip_tiny, twins, fi):
    """output counts 0, 1, ou - 1, ou, ou + 1, tile - 1, tile, tile + 1 x the four inputs, one row each, in ONE launch per rate"""
    tw, w32 = twins[fi], lib_plan(fi, FO)["w"]
    counts = sorted({0, 1, max(tw.ou - 1, 0), tw.ou, tw.ou + 1, TILE - 1, TILE, TILE + 1})
    n_full = end(tw, TILE)   # inputs of TILE + 1 outputs
    assert n_full <= 4000
    nmax = TILE + 7
    la = Launch(len(counts) * len(KINDS), nmax)
    want = []
    for ki, kind in enumerate(KINDS):
        x = make_input(kind, n_full, 100 + ki)
        y32 = ref_resample(x, fi)
        y64, mag, nt = tw.apply(x, w32)
        assert len(y32) == len(y64) >= TILE + 1
        for c in counts:
            n_in = end(tw, c - 1) if c else end(tw, 0) - 1   # exactly the inputs of c outputs; one short of the first for none
            la.row(fi, x[:n_in], x[:0], 0, 0, c, len(want))
            want.append((y32[:c], y64[:c], mag[:c], nt[:c], f"{fi} {kind} {c} outputs"))
    got = la.run(hip_tiny)
    for r, w in enumerate(want):
        check_row(got[r], *w)


@pytest.mark.parametrize("fi", RATES)
def test_kernel_row_forms(hip_tiny, twins, fi):
    """rows in the middle of a stream (k0 > 0, x0 > 0): the head piece empty, the tail piece empty, the split inside a tap window, both
    pieces 1..3 floats off the 16-byte boundary"""
    tw, w32 = twins[fi], lib_plan(fi, FO)["w"]
    x = make_input("random", 3000, 9)
    y32 = ref_resample(x, fi)
    y64, mag, nt = tw.apply(x, w32)
    k0, n_out = next(k for k in range(1, 4000) if start(tw, k) >= 50) + 1, 300
    x0, x1 = max(start(tw, k0), 0), end(tw, k0 + n_out - 1)
    assert x0 > 0 and x1 <= len(x)
    blk = x[x0:x1]
    inside = max(start(tw, k0 + 1), 0) + 2 - x0   # a split between the taps of the row's second output
    forms = [(0, 0, 0), (len(blk), 0, 0), (inside, 0, 0), (inside, 1, 3), (len(blk) // 2, 2, 1), (len(blk) // 2 + 1, 3, 2), (0, 0, 1), (len(blk), 3, 0)]
    la = Launch(len(forms) + 1, n_out + 3)
    for r, (split, mh, mt) in enumerate(forms):
        la.row(fi, blk[:split], blk[split:], x0, k0, n_out, r, mh, mt)
    got = la.run(hip_tiny)
    for r, form in enumerate(forms):
        check_row(got[r], y32[k0:k0 + n_out], y64[k0:k0 + n_out], mag[k0:k0 + n_out], nt[k0:k0 + n_out], f"{fi} form {form}")
    assert np.all(np.isnan(got[len(forms)]))   # a destination row no row names is not touched
    # more input in front than the row needs (x0 below its first tap) is legal too
    lb = Launch(1, n_out)
    lb.row(fi, x[:7], x[7:x1], 0, k0, n_out, 0, 1, 2)
    check_row(lb.run(hip_tiny)[0], y32[k0:k0 + n_out], y64[k0:k0 + n_out], mag[k0:k0 + n_out], nt[k0:k0 + n_out], f"{fi} from 0")


def test_kernel_mixed_rates_and_pass_through(hip_tiny, twins):
    """ONE launch: four rows of four rates plus two pass-through rows, destination rows in another order"""
    nmax = 1300
    la = Launch(6, nmax)
    want = {}
    for r, fi in enumerate(RATES):
        tw = twins[fi]
        n_out = 900 + 100 * r
        x = make_input("random", end(tw, n_out - 1), 40 + r)
        y32 = ref_resample(x, fi)
        y64, mag, nt = tw.apply(x, lib_plan(fi, FO)["w"])
        assert len(y32) >= n_out
        la.row(fi, x[:len(x) // 3], x[len(x) // 3:], 0, 0, n_out, 5 - r, r % 4, (r + 1) % 4)
        want[5 - r] = (y32[:n_out], y64[:n_out], mag[:n_out], nt[:n_out], f"mixed {fi}")
    p = make_input("random", 1297, 77)
    la.row(0, p[:501], p[501:], 0, 0, 0, 0, 3, 1)     # both pieces off the boundary
    la.row(0, p[:400], p[:0], 0, 0, 0, 1)             # aligned: the float4 path, then zeros
    got = la.run(hip_tiny)
    for r, w in want.items():
        check_row(got[r], *w)
    assert np.array_equal(got[0, :1297].view(np.uint32), p.view(np.uint32)) and np.all(got[0, 1297:] == 0)
    assert np.array_equal(got[1, :400].view(np.uint32), p[:400].view(np.uint32)) and np.all(got[1, 400:] == 0)


def test_launcher_refuses_rows_that_read_outside(hip_tiny, twins):
    """a row whose outputs need more input than it holds never reaches the device"""
    tw = twins[48000]
    x = make_input("random", end(tw, 9) - 1, 3)
    la = Launch(1, 16)
    la.row(48000, x, x[:0], 0, 0, 10, 0)
    with pytest.raises(AssertionError, match="reads input"):
        la.run(hip_tiny)


def test_one_call_resample(hip_tiny):
    for fi in (8000, 44100, 48000):
        x = make_input("random", 3001, fi)
        y = hip_tiny.resample(x, fi)
        assert len(y) == hip_tiny.resample_num_out(fi, len(x)) and same_bits(y, ref_resample(x, fi))
    x = make_input("random", 500, 1)
    assert np.array_equal(hip_tiny.resample(x, FO), x) and hip_tiny.resample_num_out(FO, 500) == 500


# ---- streams ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rec(tmp_path_factory):
    from k2transducerasr_amd import OnlineRecognizer
    from k2transducerasr_amd.synth import write_synthetic_model
    p = str(tmp_path_factory.mktemp("rsmodels") / "stiny.k2w")
    write_synthetic_model(p, "zipformer2-streaming-tiny-test")
    return OnlineRecognizer(p)


def n_plans(model):
    n = C.c_int32(-1)
    model._L.k2hip_debug_resample_plans.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    model._chk(model._L.k2hip_debug_resample_plans(model.handle, C.byref(n)))
    return n.value


@pytest.mark.parametrize("fi", (48000, 44100))
def test_carried_state_of_an_online_stream(rec, fi):
    """~0.3 s pushed in pieces of 1, 160, 441 and random sizes: after every materialisation the stream's frames are those of
    accept_samples fed with the host reference's output of the whole input so far, bit for bit"""
    from k2transducerasr_amd.synth import synth_utterance
    x = synth_utterance(3, 0.3, sample_rate=fi)
    rng = np.random.default_rng(fi)
    for sizes in ([1] * 40 + [len(x)], [160] * 100, [441] * 40, rng.integers(1, 3000, 40).tolist()):
        s, r, ref = rec.create_online_stream(), rec.create_online_stream(), RefStream(fi, FO)
        pos = 0
        for i, n in enumerate(sizes):
            n = min(n, len(x) - pos)
            if n == 0:
                break
            s.accept_waveform(fi, x[pos:pos + n])
            r.add_samples(ref.push(x[pos:pos + n]))
            pos += n
            assert s.speech_length == r.speech_length
            if i % 7 == 0 or pos == len(x):
                a, b = s.speech, r.speech   # (materialises both)
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (fi, sizes[0], pos)
        assert pos == len(x) and s.speech_length == rec.model.fbank_num_frames(rec.model.resample_num_out(fi, len(x))) * 80 > 0
        s.close()
        r.close()


def test_stream_rules(rec, hip_tiny):
    from k2transducerasr_amd import K2HipError, OfflineStream
    x = make_input("random", 4000, 2)
    before = n_plans(rec.model)
    a, b = rec.create_online_stream(), rec.create_online_stream()
    a.accept_waveform(FO, x)          # the model's rate: exactly accept_samples, no plan
    b.add_samples(x)
    assert n_plans(rec.model) == before and np.array_equal(a.speech.view(np.uint32), b.speech.view(np.uint32))
    a.accept_waveform(FO, x[:100])
    a.add_samples(x[:100])
    with pytest.raises(K2HipError, match="16000 Hz.*48000 Hz") as e:
        a.accept_waveform(48000, x)
    assert e.value.code == -1
    c = rec.create_online_stream()
    c.accept_waveform(48000, x)
    with pytest.raises(K2HipError, match="48000 Hz.*8000 Hz"):
        c.accept_waveform(8000, x)
    with pytest.raises(K2HipError, match="48000 Hz.*16000 Hz") as e:
        c.add_samples(x)
    assert e.value.code == -1
    c.reset()                          # the rate goes with a reset
    c.accept_waveform(8000, x)
    assert c.speech_length == rec.model.fbank_num_frames(rec.model.resample_num_out(8000, len(x))) * 80
    for bad, code in ((0, -1), (-5, -1), (16001, -6)):
        d = rec.create_online_stream()
        with pytest.raises(K2HipError) as e:
            d.accept_waveform(bad, x)
        assert e.value.code == code
        d.add_samples(x)               # a refused rate leaves the stream as it was
    o = OfflineStream(hip_tiny)
    pos, total = 0, 0
    for n in (1, 37, 2999, 5000, 123):   # SpeechLength after each push: the frames of num_out
        o.accept_waveform(44100, make_input("random", n, n))
        total += n
        assert o.speech_length == max(hip_tiny.fbank_num_frames(hip_tiny.resample_num_out(44100, total)), 0) * 80
    with pytest.raises(K2HipError, match="44100 Hz.*16000 Hz"):
        o.add_samples(x)
    with pytest.raises(K2HipError, match="44100 Hz.*48000 Hz"):
        o.accept_waveform(48000, x)


def _offline(recog, feed):
    """feed: list of (rate or None, samples) -> (speech of a twin stream set, results)"""
    ss = []
    for rate, x in feed:
        s = recog.create_offline_stream()
        s.add_samples(x) if rate is None else s.accept_waveform(rate, x)
        ss.append(s)
    lens = [s.speech_length for s in ss]
    res = recog.get_results(ss)
    return lens, res, ss


@pytest.fixture(scope="module")
def utts_at():
    from k2transducerasr_amd.synth import synth_utterance
    return {fi: [synth_utterance(u, d, sample_rate=fi) for u, d in enumerate([1.3, 0.9, 1.1, 1.3, 0.7])] for fi in (8000, 16000, 48000)}


def test_offline_end_to_end(tiny_model_path, utts_at):
    """five utterances at 48 kHz and at 8 kHz through accept_waveform against accept_samples of the host reference's 16 kHz output:
    the same frames, tokens and timestamps, each rate's batch on its own; then a batch mixing 8, 16 and 48 kHz streams against the SAME
    batch fed with the references' outputs.  (Not against the three batches decoded apart: the reference's batch greedy search is
    defined per batch composition -- no length masking, and a stream's first decoder context changes when ANY stream of its batch
    emits (oracle/k2_oracle.c k2o_greedy_batch) -- so a stream's tokens differ between two batches at 16 kHz too.  On
    the device a 0.9 s stream decoded in a pair and in a batch of six with the same padded length gave different tokens.)"""
    from k2transducerasr_amd import OfflineRecognizer
    recog = OfflineRecognizer(tiny_model_path)
    apart = {}
    for fi in (48000, 8000):
        xs = utts_at[fi]
        ys = [ref_resample(x, fi) for x in xs]
        # the frames, stream by stream
        for x, y in list(zip(xs, ys))[:2]:
            a, b = recog.create_offline_stream(), recog.create_offline_stream()
            a.accept_waveform(fi, x[:1000])
            a.accept_waveform(fi, x[1000:])
            b.add_samples(y)
            assert np.array_equal(a.speech.view(np.uint32), b.speech.view(np.uint32))
        la, ra, sa = _offline(recog, [(fi, x) for x in xs])
        lb, rb, sb = _offline(recog, [(None, y) for y in ys])
        assert la == lb and ra == rb and sum(len(t) for t, _ in ra) > 10 * len(xs)
        assert [s.speech_length for s in sa] == [s.speech_length for s in sb]
        apart[fi] = ra
    # mixed: streams 0, 3 at 8 kHz, 1, 4 at 16 kHz, 2 at 48 kHz -- against the same streams fed with the references' outputs
    pick = [8000, 16000, 48000, 8000, 16000]
    mixed = [(None if fi == 16000 else fi, utts_at[fi][u]) for u, fi in enumerate(pick)]
    plain = [(None, utts_at[fi][u] if fi == 16000 else ref_resample(utts_at[fi][u], fi)) for u, fi in enumerate(pick)]
    lm, rm, _ = _offline(recog, mixed)
    lp, rp, _ = _offline(recog, plain)
    assert lm == lp and rm == rp
    recog.model.close()


def test_offline_end_to_end_ctc(tmp_path_factory, utts_at):
    from k2transducerasr_amd import OfflineRecognizer
    from k2transducerasr_amd.synth import write_synthetic_model
    p = str(tmp_path_factory.mktemp("rsctc") / "ctc_tiny.k2w")
    write_synthetic_model(p, "zipformer2-ctc-tiny-test")
    recog = OfflineRecognizer(p)
    xs = utts_at[48000][:3]
    la, ra, _ = _offline(recog, [(48000, x) for x in xs])
    lb, rb, _ = _offline(recog, [(None, ref_resample(x, 48000)) for x in xs])
    assert la == lb and ra == rb
    recog.model.close()


def test_streaming_greedy_over_three_chunks(rec):
    from k2transducerasr_amd.synth import synth_utterance
    fi = 48000
    x = synth_utterance(41, 1.2, sample_rate=fi)
    a, b, ref = rec.create_online_stream(), rec.create_online_stream(), RefStream(fi, FO)
    steps = 0
    for i in range(0, len(x), 2400 * 7):   # pushes of 350 ms
        a.accept_waveform(fi, x[i:i + 2400 * 7])
        b.add_samples(ref.push(x[i:i + 2400 * 7]))
        while True:
            dec, _ = rec.get_results([a, b])
            assert dec[0] == dec[1]
            if not dec[0]:
                break
            steps += 1
            assert a.tokens == b.tokens and a.timestamps == b.timestamps and a.hyp == b.hyp
    assert steps >= 3 and a.speech_length == b.speech_length
    assert a.is_finished(True) == b.is_finished(True) and a.speech_length == b.speech_length


def test_unchanged_without_a_resampling_stream(tiny_model_path, utts_at):
    """a batch without a resampling stream -- fed through accept_waveform at the model's own rate -- builds no plan, issues the GEMM
    launches of the accept_samples batch and gives its bits"""
    from k2transducerasr_amd import OfflineRecognizer
    recog = OfflineRecognizer(tiny_model_path)
    xs = utts_at[16000]
    _, ra, _ = _offline(recog, [(None, x) for x in xs])
    ta = recog.model.timing()
    _, rb, _ = _offline(recog, [(16000, x) for x in xs])
    tb = recog.model.timing()
    assert ra == rb and ta["gemm_launches"] == tb["gemm_launches"] > 0 and n_plans(recog.model) == 0
    recog.model.close()
