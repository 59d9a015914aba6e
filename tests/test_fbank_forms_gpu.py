"""csrc/fbank.hip through Model.fbank in every form model.cpp accepts -- the four window types, preemph_coeff and remove_dc_offset on
and off, input_scale, frame lengths of 320 .. 512 samples, another shift, other mel band edges, another sample rate -- on the
signals at the kernel's edges: exactly one frame of samples and one fewer, silence (every bin exactly logf(FLT_EPSILON)), a
constant, one impulse, a full-scale alternating signal (all its energy in the Nyquist bin, which no filter reaches), noise that
straddles the floor.  Each configuration is a zipformer2-tiny-test model with its metadata overridden, opened once per module.
The float64 reference (fbank_np on float32-rounded tables), the signals and the derivation of the per-element tolerance are in
tests/fbank_forms.py; no element is excluded and check() holds every tolerance under 2e-5.  The other tests run the default
configuration only, on utterances that avoid these edges."""
import numpy as np
import pytest

import fbank_forms as ff
from test_kernels_gpu import check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    from k2transducerasr_amd import Model
    from k2transducerasr_amd.synth import write_synthetic_model
    d = tmp_path_factory.mktemp("fbank_forms")
    out = {}
    for k, (name, overrides) in enumerate(ff.CONFIGS):
        path = str(d / f"cfg{k}.k2w")
        meta = write_synthetic_model(path, "zipformer2-tiny-test", meta_overrides=dict(overrides))
        out[name] = (Model(path, 0), meta)
    yield out
    for m, _ in out.values():
        m.close()


@pytest.mark.parametrize("name", [n for n, _ in ff.CONFIGS], ids=[n.replace(" ", "_") for n, _ in ff.CONFIGS])
def test_fbank_form(models, name):
    model, meta = models[name]
    N, S = ff.frame_geometry(meta)
    worst = 0.0
    for what, x in ff.signals(meta):
        nf = ff.num_frames(x.size, meta)
        assert model.fbank_num_frames(x.size) == nf, (name, what, x.size)
        got = model.fbank(x)
        want, tol = ff.reference(x, meta)
        assert got.shape == want.shape == (nf, 80), (name, what, got.shape, want.shape)
        if what == "one sample short":
            assert nf == 0
            continue
        assert nf == {"one frame": 1, "two frames less a sample": 1, "two frames": 2}.get(what, nf) and nf >= 1
        check(got, want, tol, f"fbank {name}: {what}")
        if what == "zeros":
            assert (got == np.log(np.float32(ff.FLT_EPSILON))).all(), (name, "silence is not exactly logf(FLT_EPSILON)")
        worst = max(worst, float((np.abs(got.astype(np.float64) - want) / tol).max()))
    print(f"fbank {name}: frame {N} shift {S}, largest error / tolerance {worst:.3f}")
