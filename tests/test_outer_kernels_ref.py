"""The references of tests/test_outer_kernels_gpu.py and tests/test_fbank_forms_gpu.py, checked without a GPU.

  * every case of the GPU test with standin() -- the same formulas in float32 numpy -- in the kernel's place: the float64 reference and
    the stand-in must agree exactly where the kernel only moves data or produces integers, and within the derived per-element
    tolerance elsewhere; check() holds every tolerance under its 2e-5 ceiling.  The same run shows that the cases launch every op
    of outer_kernels.SIM.
  * every entry of outer_kernels.MUTANTS -- one op's stand-in made wrong in the way such a kernel goes wrong (a cache advanced by one
    row less, a floor left out, a float4 copied across a count, the other tie-break, a missing clamp ...) -- through its own case,
    which must fail: the cases have teeth before any kernel is involved.
  * every reference with arithmetic against an independent expression in torch float64 at 1e-12: log_softmax, conv0 + SwooshR (the
    twin's conv2d and swoosh_r), GLU, the tanh gates, tanh(enc + dec).
  * the fbank reference's own noise: fbank_np's float64 FFT against a direct O(N^2) DFT in np.longdouble on the same frames, for the
    full-scale (defaults) and the 32768-scaled (povey) configuration, every signal.  The bound is the float64 share of the GPU
    test's tolerance (fbank_forms.fft_noise, which budgets for two implementations' framing and FFT) plus the float64 log and
    mel sum (4 eps64 (1 + |log e|)).  Largest observed difference / bound: 0.26 (povey scale 32768, the utterance); 0.18 at full
    scale.  Every signal meets the 2e-5 ceiling at its amplitude: the largest tolerance of any element is 1.1e-5 (32768-scaled
    alternating signal)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fbank_forms as ff
import outer_kernels as ok
from torch_twin import swoosh_r

TOL = 1e-12


def r64(rng, *shape, scale=1.0):
    return rng.uniform(-1, 1, shape) * scale


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.abs(got - want).max() <= TOL * max(1.0, np.abs(want).max()), (what, np.abs(got - want).max())


@pytest.mark.parametrize("k", range(len(ok.CASES)), ids=[name.replace(" ", "_") for name, _ in ok.CASES])
def test_float32_standin_passes_every_case(k):
    ok.CASES[k][1](ok.Env(ok.standin, ok.null_switch))


def test_the_cases_launch_every_op():
    ok.CALLED.clear()
    for _, case in ok.CASES:
        case(ok.Env(ok.standin, ok.null_switch))
    assert ok.CALLED == set(ok.SIM), sorted(set(ok.SIM) - ok.CALLED)


def test_every_op_has_a_mutant_and_every_mutant_a_case():
    assert {m[1] for m in ok.MUTANTS} == set(ok.SIM), sorted(set(ok.SIM) - {m[1] for m in ok.MUTANTS})
    assert {m[0] for m in ok.MUTANTS} == {name for name, _ in ok.CASES}


@pytest.mark.parametrize("k", range(len(ok.MUTANTS)), ids=[f"{m[0]}: {m[1]} {m[2]}".replace(" ", "_") for m in ok.MUTANTS])
def test_each_case_rejects_its_wrong_standin(k):
    case_name, op, _, sim = ok.MUTANTS[k]
    wrong = ok.make_standin({**ok.SIM, op: sim})
    with pytest.raises(AssertionError):
        dict(ok.CASES)[case_name](ok.Env(wrong, ok.null_switch))


def test_arithmetic_references_are_torch():
    rng = np.random.default_rng(11)
    for M, V in ((3, 1), (4, 65), (2, 500)):
        x = r64(rng, M, V, scale=40.0)
        if V > 1:
            x[0, 1] = -np.inf
        b = [x.copy()]
        ok.sim_log_softmax_rows(np.float64, [M, V], b)
        want = torch.log_softmax(torch.from_numpy(x), dim=-1).numpy()
        assert np.array_equal(np.isneginf(b[0]), np.isneginf(want))
        fin = np.isfinite(want)
        close(b[0][fin], want[fin], f"log_softmax V={V}")
    for B, T, Fq in ((1, 3, 1), (2, 5, 7), (2, 9, 80)):
        xin, w, bias = r64(rng, B, T, Fq, scale=2.0), r64(rng, 8, 1, 3, 3), r64(rng, 8)
        y = swoosh_r(F.conv2d(torch.from_numpy(xin).unsqueeze(1), torch.from_numpy(w), torch.from_numpy(bias), padding=(0, 1)))
        b = [xin, w.reshape(72), bias, np.zeros((B, T - 2, Fq, 8))]
        ok.sim_conv0_swoosh(np.float64, [B, T, Fq], b)
        close(b[3], y.permute(0, 2, 3, 1).numpy(), f"conv0_swoosh T={T} F={Fq}")
    M, D = 5, 20
    x = r64(rng, M, 2 * D, scale=6.0)
    b = [x, np.zeros((M, D))]
    ok.sim_glu_sigmoid(np.float64, [M, D], b)
    close(b[1], F.glu(torch.from_numpy(x), dim=-1).numpy(), "glu_sigmoid")
    x = r64(rng, M, 3 * D, scale=12.0)
    b = [x, np.zeros((M, D))]
    ok.sim_tanh_gate(np.float64, [M, D], b)
    s, a, _ = torch.from_numpy(x).chunk(3, dim=-1)
    close(b[1], (a * torch.tanh(s)).numpy(), "tanh_gate")
    N, J = 5, 8
    for ds in (0, J):
        enc, dec = r64(rng, N, J, scale=6.0), r64(rng, (N - 1) * ds + J, scale=3.0)
        b = [enc, dec, np.zeros((N, J))]
        ok.sim_tanh_add(np.float64, [ds, N, J], b)
        d = torch.from_numpy(dec)
        rows = d.reshape(N, J) if ds else d.unsqueeze(0).expand(N, J)
        close(b[2], torch.tanh(torch.from_numpy(enc) + rows).numpy(), f"tanh_add dec_stride={ds}")
    # cat_shift's gated rows: NonlinAttention's x * tanh(s) of rows (s | x | ...), behind the old cache
    B, L, Tc, width, ldn = 2, 3, 4, 8, 20
    new, pool = r64(rng, B, Tc, ldn, scale=3.0), r64(rng, 2 * (L * width + 5))
    b = [pool.copy(), np.array([1, 0], np.int32), new, np.zeros((B, L + Tc, width))]
    ok.sim_cat_shift(np.float64, [L * width + 5, 2, ldn, B, L, Tc, width, 1], b)
    t = torch.from_numpy(new)
    gated = (t[..., width:2 * width] * torch.tanh(t[..., :width])).numpy()
    for s, slot in enumerate((1, 0)):
        old = pool[slot * (L * width + 5) + 2:][:L * width].reshape(L, width)
        cat = np.concatenate([old, gated[s]])
        close(b[3][s], cat, "cat_shift gated cat")
        close(b[0][slot * (L * width + 5) + 2:][:L * width].reshape(L, width), cat[Tc:], "cat_shift gated cache")


@pytest.mark.parametrize("name", ["defaults", "povey scale 32768"])
def test_fbank_reference_noise_against_a_long_double_dft(name):
    """(figures: module docstring)"""
    from k2transducerasr_amd.synth import preset
    meta = preset("zipformer2-tiny-test")
    meta.update(dict(ff.CONFIGS)[name])
    worst = 0.0
    for what, x in ff.signals(meta):
        fr, W, raw = ff.fbank_parts(x, meta, f32_tables=True)
        if fr.shape[0] == 0:
            continue
        e = ff.fbank_energies(fr, W)
        el = ff.energies_longdouble(fr, W).astype(np.float64)
        lg, lgl = np.log(np.maximum(e, ff.FLT_EPSILON)), np.log(np.maximum(el, ff.FLT_EPSILON))
        bound = ff.fft_noise(fr, W, raw, e) + 4 * ff.EPS64 * (1.0 + np.abs(lg))
        ratio = float((np.abs(lg - lgl) / bound).max())
        assert ratio <= 1.0, (name, what, ratio)
        worst = max(worst, ratio)
        want, tol = ff.reference(x, meta)
        assert tol.max() <= 2e-5 * max(1.0, np.abs(want).max()) and tol.max() <= 2e-5, (name, what, tol.max())
    print(f"fbank reference {name}: largest difference / bound {worst:.3f}")
    assert worst > 0.01          # the comparison is not vacuous


def test_fbank_signals_hit_the_floor_and_the_frame_counts():
    from k2transducerasr_amd.synth import preset
    for name, overrides in ff.CONFIGS:
        meta = preset("zipformer2-tiny-test")
        meta.update(overrides)
        N, S = ff.frame_geometry(meta)
        assert 256 < N <= 512, (name, N)
        sig = dict(ff.signals(meta))
        assert [ff.num_frames(sig[k].size, meta) for k in ("one frame", "one sample short", "two frames less a sample", "two frames")] == [1, 0, 1, 2]
        want, _ = ff.reference(sig["zeros"], meta)
        assert (want == np.log(ff.FLT_EPSILON)).all()
        want, _ = ff.reference(sig["noise 1e-5"], meta)
        floored = (want == np.log(ff.FLT_EPSILON)).mean()
        assert name == "povey scale 32768" or 0.05 < floored < 0.95, (name, floored)       # (scaled by 32768 the noise clears the floor)
