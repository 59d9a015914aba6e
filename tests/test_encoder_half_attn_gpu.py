"""Level 4 of the encoder's half-precision switch on the device (csrc/attn_f16.hip): the f16 scores + softmax kernel
("attn_scores_softmax_f16") and the f16 attention apply ("attn_av_out_f16") against float64 over f16-rounded operands, and the switch on
the tiny models."""
import numpy as np
import pytest

from test_kernels_gpu import av_out_ref, check, f64, nan, op, random_weights, scores_case, scores_ref, softmax_tol, switch, uni  # noqa: F401

pytestmark = pytest.mark.gpu

r16 = lambda a: a.astype(np.float16).astype(np.float32)   # noqa: E731
MARK = 0x5a5a                                              # sentinel halves behind the last row of aw16


@pytest.mark.parametrize("T,B,H", [(1, 2, 2), (31, 2, 2), (33, 2, 2), (64, 2, 2), (100, 2, 2), (257, 2, 2), (1101, 1, 1)])
def test_scores_kernel_against_float64(op, T, B, H):
    """q and k rounded to f16, p and pos float32.  f16 x f16 products are exact in float32, so the scores differ from the float32
    kernel's only by the sum order: the softmax bound of test_kernels_gpu over the rounded operands, plus the final rounding of the
    weight: half an f16 ulp at the expected weight's upper end.  T = 1101: the in-place softmax branch (Tp > 1024)."""
    rng = np.random.default_rng(T)
    qkp, pp, ld, Tp, kargs, koff0, poff0 = scores_case(rng, B, T, H, 32, "z2")
    qkp[:, :poff0] = r16(qkp[:, :poff0])                   # the reference sees what the matrix pipe sees
    qkp[:, poff0 + 4 * H:] = np.nan                        # the row's padding
    pw, centred, eps, _ = scores_ref(qkp, pp, B, T, H, 32, koff0, poff0)
    Tp16 = (T + 7) // 8 * 8
    aw16 = np.full(H * B * T * Tp16 + 8, MARK, np.uint16)
    aw0 = np.full(B * T * Tp + 4, -7.625, np.float32)
    op("attn_scores_softmax_f16", [ld, B, T, Tp, H, *kargs], [qkp, pp, aw16.view(np.uint32), aw0], {2, 3})
    assert (aw16[-8:] == MARK).all() and (aw0[-4:] == -7.625).all(), "written past the last row"
    w16, w0 = aw16[:-8].reshape(H, B, T, Tp16), aw0[:-4].reshape(B, T, Tp)
    assert not w16[..., T:].any() and not w0[..., T:].view(np.uint32).any(), "pad columns are not +0"
    assert np.array_equal(w0[..., :T].astype(np.float16).view(np.uint16), w16[0, :, :, :T]), "aw0 is not head 0's float32 weights"
    tol32 = softmax_tol(pw, centred, eps)
    tol = tol32 + 0.5 * f64(np.spacing((pw + tol32).astype(np.float16)))
    err = np.abs(f64(w16[..., :T].view(np.float16)) - pw)
    print(f"scores f16 T={T}: max err {err.max():.3g}, max err / tol {(err / tol).max():.3g}")
    assert np.isfinite(err).all() and (err <= tol).all()
    check(w0[..., :T], pw[0], tol32[0], f"aw0 T={T}", large_operands=False)


@pytest.mark.parametrize("D", [16, 64, 96])                 # one column tile; a tile per blockIdx.z slice; slices of two tiles
@pytest.mark.parametrize("H,vh", [(4, 12), (8, 16)])
def test_apply_kernel_against_float64(op, H, vh, D):
    """the given f16 weights and f16-rounded values, float32 out_proj, bias and residual; both sums within 4 u sqrt(n) mag.  KL around
    the 64-key step and the 8-key operand, T around the 16-row strip; rows >= KL of the value buffer are NaN"""
    rng = np.random.default_rng(100 * H + D)
    B, HV = 2, H * vh
    for KL in (1, 31, 33, 64, 65, 130):
        for T in (5, 16, 37):
            Tp16 = (KL + 7) // 8 * 8
            aw = r16(random_weights(rng, H, B, T, KL, Tp16))
            v = nan(B * KL + 70, HV)
            v[:B * KL] = uni(rng, B * KL, HV)
            wout, bias, x = uni(rng, D, HV, scale=HV ** -0.5), uni(rng, D), uni(rng, B * T, D)
            want, tol = av_out_ref(aw, r16(v[:B * KL]), wout, bias, x, H, vh, KL)
            op("attn_av_out_f16", [B, T, KL, Tp16, H, vh, D], [aw.astype(np.float16).view(np.uint32), v, wout, bias, x], {4})
            check(x, want, tol, f"attn_av_out_f16 KL={KL} T={T} H={H} vh={vh} D={D}")


# max |level 4 - off| / max |off| of the encoder output: four times the worst value measured on an MI355X (DESIGN.md "Level 4")
DEVIATION_BOUND_4 = 4 * 3.81e-4   # measured: 3.807e-4 (zipformer2-tiny-test), 1.723e-4 (zipformer2-ctc-tiny-test)


@pytest.mark.parametrize("preset", ["zipformer2-tiny-test", "zipformer2-ctc-tiny-test"])
def test_level_4_on_the_tiny_models(tmp_path, utts, preset):
    from k2transducerasr_amd import Model
    from k2transducerasr_amd.synth import write_synthetic_model
    path = str(tmp_path / "m.k2w")
    meta = write_synthetic_model(path, preset)
    ints = lambda k: [int(v) for v in meta[k].split(",")]   # noqa: E731
    # every stack has query head dim 32 and a value projection attn_av_out takes (vh <= 16, H vh <= 128 and a multiple of 4, D % 16 == 0)
    assert set(ints("query_head_dims")) == {32}
    assert all(vh <= 16 and H * vh <= 128 and H * vh % 4 == 0 and D % 16 == 0 for H, vh, D in zip(ints("num_heads"), ints("value_head_dims"), ints("encoder_dims")))
    model = Model(path, 0)
    x = model.pad_sequence([model.fbank(u) for u in utts]).reshape(len(utts), -1, 80)
    out, stats = {}, {}
    for level in (0, 1, 2, 3, 4):
        model.set_encoder_precision(level)
        out[level], stats[level] = model.encoder_proj(x), model.encoder_f16_stats()
    # scores + the two applies of every layer; no new panels
    assert stats[4] == dict(stats[3], launches=stats[3]["launches"] + 3 * sum(ints("num_encoder_layers")))
    assert not np.array_equal(out[4].view(np.uint32), out[3].view(np.uint32))
    with switch("K2HIP_F16_ATTN", 3):
        model.set_encoder_precision(0)
        model.set_encoder_precision(4)
        assert np.array_equal(model.encoder_proj(x).view(np.uint32), out[3].view(np.uint32)), "level 4 on route 3 is not level 3"
        assert model.encoder_f16_stats() == stats[3]
    dev = np.abs(out[4].astype(np.float64) - out[0]).max() / np.abs(out[0]).max()
    print(f"{preset}: level 4 max |on - off| / max |off| = {dev:.3e} (bound {DEVIATION_BOUND_4:.3e}), {stats[4]['launches']} launches")
    for level in (3, 2, 1, 0):                                # (a change of level packs anew: the counters start again)
        model.set_encoder_precision(level)
        assert np.array_equal(model.encoder_proj(x).view(np.uint32), out[level].view(np.uint32)), level
        assert model.encoder_f16_stats() == stats[level], level
    model.set_encoder_precision(5)                            # values above 4 stay level 1
    assert np.array_equal(model.encoder_proj(x).view(np.uint32), out[1].view(np.uint32)) and model.encoder_f16_stats() == stats[1]
    model.close()
    assert dev <= DEVIATION_BOUND_4
