"""Level 3 of the encoder's half-precision switch on the device: gemm_f16_mfma's conv-gather form ("gemm_f16_gather") against float64 over
f16-rounded operands, the fused ConvNeXt pointwise pair ("convnext_f16", csrc/convnext_f16.hip) against the two gemm_f16_mfma launches
bit for bit and against float64, and the switch on the tiny models."""
import numpy as np
import pytest

from test_encoder_half_gpu import SENTINEL, covered_launches  # noqa: F401
from test_encoder_half_wide_gpu import TILES, launch, level2_launches
from test_gemm_gpu import ACT_SWOOSH_L, ACT_SWOOSH_R, act_f64
from test_kernels_gpu import U, act_tol, f64, nan, op, switch, uni  # noqa: F401  (op: the fixture)

pytestmark = pytest.mark.gpu

r16 = lambda a: a.astype(np.float16).astype(np.float64)   # noqa: E731


@pytest.mark.parametrize("cfg", [0, 1, 2])
@pytest.mark.parametrize("st,sf", [(1, 2), (2, 2)])
def test_gather_form_against_float64(op, st, sf, cfg):
    """3 x 3 windows over an NHWC input: K = 9 C in three segments of 3 C (288: an odd chunk count; 576)"""
    B = 2
    for C in (32, 64):
        for Tin in (3, 6):
            for Fin in (7, 10):
                for N in (32, 72):
                    rng = np.random.default_rng(1000 * C + 100 * Tin + 10 * Fin + N + st)
                    Tout, Fout, K = (Tin - 3) // st + 1, (Fin - 3) // sf + 1, 9 * C
                    M = B * Tout * Fout
                    x, W, bias = uni(rng, B * Tin * Fin * C), uni(rng, N, K), uni(rng, N)
                    r, k = np.arange(M)[:, None], np.arange(K)[None, :]
                    base = ((r // Fout // Tout * Tin + r // Fout % Tout * st) * Fin + r % Fout * sf) * C
                    h = r16(x[base + k // (3 * C) * (Fin * C) + k % (3 * C)]) @ r16(W).T + bias
                    Cb, plan = np.full((M, N + 5), SENTINEL, np.float32), np.zeros(3, np.int32)
                    op("gemm_f16_gather", [M, N, K, N + 5, ACT_SWOOSH_R, cfg, Fout, Tout, Tin, Fin, C, st, sf, 3 * C, Fin * C], [x, W, bias, Cb, plan], {3, 4})
                    assert (int(plan[0]), (int(plan[1]), int(plan[2]))) == (cfg, TILES[cfg])
                    assert np.all(Cb[:, N:] == SENTINEL), "written past the last output column"
                    err, tol = np.abs(f64(Cb[:, :N]) - act_f64(h, ACT_SWOOSH_R)), act_tol(h, 2e-5 * max(1.0, np.sqrt(K)))
                    assert (err <= tol).all(), (C, Tin, Fin, N, float((err - tol).max()))


def pair(op, dw, W1, b1, W2, b2, a3, M):
    """(the fused launch, the two gemm_f16_mfma launches, their float32 hidden tensor): C [M, 133] with the residual in place"""
    C0 = np.full((M, 133), SENTINEL, np.float32)
    C0[:, :128] = a3
    C1, C2 = C0.copy(), C0.copy()
    op("convnext_f16", [M, dw.shape[1], 133], [dw, W1, b1, W2, b2, C1], {5})
    hid = launch(op, dw, W1, b1, nan(M, 384), 1, M, 384, 128, act=ACT_SWOOSH_L)
    launch(op, hid, W2, b2, C2, 0, M, 128, 384, in_place=1)
    assert np.all(C1[:, 128:] == SENTINEL), "written past the last output column"
    return C1[:, :128], C2[:, :128], hid


@pytest.mark.parametrize("M", [1, 33, 128, 129, 257])
def test_fused_pair_equals_the_two_launches_and_float64(op, M):
    rng = np.random.default_rng(M)
    dw = nan(M + 3, 132)                                     # rows past M and the padding behind the 128 channels are NaN
    dw[:M, :128] = uni(rng, M, 128, scale=2.0)
    W1, b1, W2, b2, a3 = uni(rng, 384, 128, scale=0.3), uni(rng, 384), uni(rng, 128, 384, scale=0.2), uni(rng, 128), uni(rng, M, 128)
    got, two, hid = pair(op, dw, W1, b1, W2, b2, a3, M)
    assert np.isfinite(got).all(), "a NaN row or padding column of dw reached the output"
    assert np.array_equal(got.view(np.uint32), two.view(np.uint32))
    # the second product over f16 of the device's own hidden tensor: no rounding-boundary flips of the hidden value in the bound
    want = f64(a3) + r16(hid) @ r16(W2).T + b2
    err, tol = np.abs(f64(got) - want), 2e-5 * np.sqrt(384) + 2 * U * np.abs(want)
    print(f"convnext_f16 M={M}: max err {err.max():.3g} (tol {tol.min():.3g})")
    assert (err <= tol).all()


def test_one_lit_pixel_stays_in_its_row(op):
    """dw is zero but for one row and the residual rows are alike: every other output row is the same bit pattern per column"""
    M, lit, rng = 257, 130, np.random.default_rng(5)
    dw = np.zeros((M, 128), np.float32)
    dw[lit] = uni(rng, 128, scale=3.0)
    W1, b1, W2, b2 = uni(rng, 384, 128), uni(rng, 384), uni(rng, 128, 384), uni(rng, 128)
    got, two, _ = pair(op, dw, W1, b1, W2, b2, np.tile(uni(rng, 1, 128), (M, 1)), M)
    assert np.array_equal(got.view(np.uint32), two.view(np.uint32))
    dark = np.delete(got, lit, axis=0).view(np.uint32)
    assert (dark == dark[0]).all() and (got[lit].view(np.uint32) != dark[0]).sum() > 100


# max |level 3 - off| / max |off| of the encoder output: four times the worst value measured on an MI355X (DESIGN.md "Level 3")
DEVIATION_BOUND_3 = 4 * 3.64e-4   # measured: 3.632e-4 (zipformer2-tiny-test), 1.730e-4 (zipformer2-ctc-tiny-test)


@pytest.mark.parametrize("preset", ["zipformer2-tiny-test", "zipformer2-ctc-tiny-test"])
def test_level_3_on_the_tiny_models(tmp_path, utts, preset):
    from k2transducerasr_amd import Model
    from k2transducerasr_amd.synth import write_synthetic_model
    path = str(tmp_path / "m.k2w")
    meta = write_synthetic_model(path, preset)
    model = Model(path, 0)
    x = model.pad_sequence([model.fbank(u) for u in utts]).reshape(len(utts), -1, 80)
    out, stats = {}, {}
    for level in (0, 1, 2, 3):
        model.set_encoder_precision(level)
        out[level], stats[level] = model.encoder_proj(x), model.encoder_f16_stats()
    # level 2's plus conv.7, the fused pointwise pair, and encoder_embed.out where it is not a few columns over a long K (rule (d))
    want = level2_launches(meta, *x.shape[:2]) + 2 + (0 if int(meta["encoder_dims"].split(",")[0]) <= 96 else 1)
    assert stats[3]["launches"] == want and stats[3]["panels"] == stats[2]["panels"] + 4
    with switch("K2HIP_F16_CONVNEXT", 2):
        model.set_encoder_precision(0)
        model.set_encoder_precision(3)
        assert np.array_equal(model.encoder_proj(x).view(np.uint32), out[3].view(np.uint32)), "the two-launch route differs from the fused one"
        assert model.encoder_f16_stats()["launches"] == stats[3]["launches"] + 1
    dev = np.abs(out[3].astype(np.float64) - out[0]).max() / np.abs(out[0]).max()
    print(f"{preset}: level 3 max |on - off| / max |off| = {dev:.3e} (bound {DEVIATION_BOUND_3:.3e}), {stats[3]['launches']} launches")
    for level in (2, 1, 0):                                   # (a change of level packs anew: the counters start again)
        model.set_encoder_precision(level)
        assert np.array_equal(model.encoder_proj(x).view(np.uint32), out[level].view(np.uint32)), level
        assert model.encoder_f16_stats() == stats[level], level
    assert stats[0] == dict(launches=0, panels=0, panel_bytes=0)
    model.close()
    assert dev <= DEVIATION_BOUND_3


@pytest.mark.parametrize("name", ["encoder_embed.conv.7.weight", "encoder_embed.convnext.pointwise_conv2.weight"])
def test_an_embed_weight_beyond_f16_refuses_level_3(tmp_path, tiny_model_path, name):
    from k2transducerasr_amd import K2HipError, Model
    from k2transducerasr_amd.k2w import read_k2w, write_k2w
    meta, tensors = read_k2w(tiny_model_path)
    tensors = {k: np.array(v) for k, v in tensors.items()}
    tensors[name][3, 5] = 1e5
    path = str(tmp_path / "big.k2w")
    write_k2w(path, meta, tensors.items())
    model = Model(path, 0)
    model.set_encoder_precision(2)
    two = model.encoder_f16_stats()
    with pytest.raises(K2HipError) as e:
        model.set_encoder_precision(3)
    assert e.value.code == -1 and name in str(e.value) and "#" not in str(e.value)
    assert two["panels"] > 0 and model.encoder_f16_stats() == two      # stays at level 2
    model.close()
