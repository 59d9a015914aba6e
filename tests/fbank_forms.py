"""Configurations, signals, float64 reference and per-element tolerance of tests/test_fbank_forms_gpu.py (csrc/fbank.hip through
Model.fbank).  Importable without a GPU: tests/test_outer_kernels_ref.py checks the reference's own FFT noise against a direct
long-double DFT under the same bound.

The reference is tests/torch_twin.py's fbank_np with the window, the mel weights, preemph_coeff and input_scale rounded to float32
first -- the model's tables (model.cpp) and FbankArgs hold exactly those values, and the kernel computes in float64 from there, as the
reference does.  What is left between the two, per element of log(max(e, FLT_EPSILON)):
  * the float32 cast of the energy: u = 2^-24 relative, i.e. u in the log (the floor is continuous: a bin next to it needs no
    exemption);
  * a mel weight whose float64 value sits on a float32 rounding boundary may round the other way in the model's libm: one float32
    ulp of one weight, at most 2 u of the energy;
  * logf: 3 ulp of the library's contract = 6 u |log e|;
  * the float64 arithmetic in front of the cast.  Each of the two implementations forms the frame (a 400-term mean, pre-emphasis,
    window) and a 512-point FFT of 9 stages in float64: every spectral value carries at most d = 2 * 2 * eps64 * 9 * ||frame||_2
    (both implementations, a factor 2 for the framing; ||frame||_2 the larger of the frame's norm as cut and as windowed).  A mel
    energy e = sum_k w_k |X_k|^2 then moves by at most 2 d sqrt(sum_k w_k) sqrt(e) + d^2 sum_k w_k (Cauchy-Schwarz), and the log by
    that over max(e, FLT_EPSILON).  For a bin far below its frame's energy (a pure tone's leakage) this term is the one that counts.
check() of test_kernels_gpu.py holds the sum under its 2e-5 ceiling for every compared element."""
import numpy as np

from torch_twin import fbank_energies, fbank_parts

U = 2.0 ** -24
EPS64 = 2.0 ** -53
FLT_EPSILON = float(np.finfo(np.float32).eps)

# (name, meta overrides of zipformer2-tiny-test)
CONFIGS = [
    ("defaults", {}),
    ("povey scale 32768", {"window_type": "povey", "input_scale": "32768"}),
    ("hanning no preemph no dc", {"window_type": "hanning", "preemph_coeff": "0", "remove_dc_offset": "0"}),
    ("rectangular 32 ms", {"window_type": "rectangular", "frame_length_ms": "32"}),
    ("20 ms shift 5 ms", {"frame_length_ms": "20", "frame_shift_ms": "5"}),
    ("low 100 high -400", {"low_freq": "100", "high_freq": "-400"}),
    ("22050 Hz 20 ms", {"sample_rate": "22050", "frame_length_ms": "20"}),
]


def frame_geometry(meta):
    sr = int(meta["sample_rate"])
    return sr * int(meta["frame_length_ms"]) // 1000, sr * int(meta["frame_shift_ms"]) // 1000


def signals(meta):
    """(name, float32 samples) for one configuration"""
    from k2transducerasr_amd.synth import synth_utterance
    N, S = frame_geometry(meta)
    rng = np.random.default_rng(N * 1000 + S)
    utt = synth_utterance(3, 0.5, int(meta["sample_rate"]))
    n = N + 3 * S
    imp = np.zeros(n, np.float32)
    imp[N // 2 + S] = 0.75
    alt = np.full(n, 0.99, np.float32)
    alt[1::2] = -0.99
    return [("utterance", utt), ("one frame", utt[:N].copy()), ("one sample short", utt[:N - 1].copy()),
            ("two frames less a sample", utt[:N + S - 1].copy()), ("two frames", utt[:N + S].copy()),
            ("zeros", np.zeros(n, np.float32)), ("constant 0.5", np.full(n, 0.5, np.float32)), ("impulse", imp),
            ("alternating 0.99", alt), ("noise 1e-5", (1e-5 * rng.standard_normal(n)).astype(np.float32))]


def num_frames(n, meta):
    N, S = frame_geometry(meta)
    return 1 + (n - N) // S if n >= N else 0


def reference(samples, meta, energies=fbank_energies):
    """log mel energies [nf, nb] in float64 and the per-element tolerance of the module docstring"""
    fr, W, raw = fbank_parts(samples, meta, f32_tables=True)
    nb = W.shape[0]
    if fr.shape[0] == 0:
        return np.zeros((0, nb)), np.zeros((0, nb))
    e = energies(fr, W)
    ec = np.maximum(e, FLT_EPSILON)
    want = np.log(ec)
    return want, U + 2.0 * U + 6.0 * U * np.abs(want) + fft_noise(fr, W, raw, e)


def fft_noise(fr, W, raw, e):
    norm = np.maximum(np.sqrt((fr * fr).sum(1)), np.sqrt((raw * raw).sum(1)))[:, None]
    d = 2 * 2 * EPS64 * 9 * norm
    sw = W.sum(1)[None, :]
    return (2.0 * d * np.sqrt(sw * np.maximum(e, 0.0)) + d * d * sw) / np.maximum(e, FLT_EPSILON)


def energies_longdouble(fr, W):
    """the same mel energies from a direct O(N^2) DFT in np.longdouble (exact twiddle angles: n k mod P)"""
    P = 2 * W.shape[1]
    N = fr.shape[1]
    nk = (np.arange(N)[:, None] * np.arange(P // 2)[None, :]) % P
    pi = 4 * np.arctan(np.longdouble(1))                 # (np.pi is a float64)
    ang = 2 * pi * nk.astype(np.longdouble) / np.longdouble(P)
    x = fr.astype(np.longdouble)
    re, im = x @ np.cos(ang), x @ np.sin(ang)
    return (re * re + im * im) @ W.T.astype(np.longdouble)
