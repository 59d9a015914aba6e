"""Level 2 of the encoder's half-precision switch: gemm_f16_mfma's gated, act_cols and bypass forms and its conv tail, one launch each
("gemm_f16_form"), and the switch on the tiny models.  Sums within 2e-5 max(1, sqrt K) of float64 over f16-rounded operands; the gate and
the mix pass that on as tests/test_conv_fused_offline_gpu.py (GLU) and tests/gemm_forms.py (bypass) pass theirs."""
import numpy as np
import pytest

from test_conv_fused_offline_gpu import conv_module_ref, interleave
from test_encoder_half_gpu import SENTINEL, covered_launches
from test_gemm_gpu import ACT_NONE, ACT_SWOOSH_L, act_f64
from test_kernels_gpu import U, act_tol, f64, nan, op, sigmoid64, uni  # noqa: F401  (op: the fixture)

pytestmark = pytest.mark.gpu

TILES = {0: (128, 128), 1: (128, 64), 2: (64, 64)}

def launch(op, A, W, bias, C, cfg, M, N, K, act=ACT_NONE, act_cols=0, in_place=0, glu=0, glu_cols=0, orig=None, scale=None, wd=None, bd=None, T=0):
    plan = np.zeros(3, np.int32)
    ints = [M, N, K, A.shape[1], C.shape[1], C.shape[1], act, act_cols, 0, in_place, cfg, glu, glu_cols,
            0 if orig is None else orig.shape[1], 0 if wd is None else wd.shape[0], T]
    op("gemm_f16_form", ints, [A, W, bias, None, C, orig, scale, wd, bd, plan], {4, 9})
    assert (int(plan[0]), (int(plan[1]), int(plan[2]))) == (cfg, TILES[cfg])
    return C


def glu_ref(h, t, gc, tanh):
    """columns < gc in blocks of 32 = 16 values | their 16 gates -> 16 columns; the rest pass through behind them; and the bound"""
    blk = h[:, :gc].reshape(len(h), -1, 2, 16)
    val, gate = blk[:, :, 0].reshape(len(h), -1), blk[:, :, 1].reshape(len(h), -1)
    g, dg = (np.tanh(gate), 1.0) if tanh else (sigmoid64(gate), 0.25)
    tol = t * np.abs(g) + np.abs(val) * dg * t + np.abs(val * g) * (np.abs(gate) + 8) * U + 2e-6 * np.abs(val)
    return np.hstack([val * g, h[:, gc:]]), np.hstack([tol, np.full((len(h), h.shape[1] - gc), t)])


@pytest.mark.parametrize("cfg", [0, 1, 2])
@pytest.mark.parametrize("form", ["glu1_n64", "glu1_n160", "glu2_cols64", "act_cols32", "bypass_in_place"])
def test_forms_against_float64(op, form, cfg):
    N = dict(glu1_n64=64, glu1_n160=160, glu2_cols64=104, act_cols32=72, bypass_in_place=72)[form]
    for M in (33, 257):
        for K in (32, 96, 544):   # one chunk, a half-stage tail, an odd stage count
            rng = np.random.default_rng(M * 1000 + N + K)
            A = nan(M + 3, K + 4)                          # rows past M and the padding behind K are NaN
            A[:M, :K] = uni(rng, M, K)
            W, bias = uni(rng, N, K), uni(rng, N)
            h = A[:M, :K].astype(np.float16).astype(np.float64) @ W.astype(np.float16).astype(np.float64).T + bias
            t = 2e-5 * max(1.0, np.sqrt(K))
            kw = {}
            if form.startswith("glu"):
                gc = 64 if form == "glu2_cols64" else N
                kw = dict(glu=2 if form == "glu2_cols64" else 1, glu_cols=0 if gc == N else gc)
                want, tol = glu_ref(h, t, gc, form == "glu2_cols64")
            elif form == "act_cols32":
                kw = dict(act=ACT_SWOOSH_L, act_cols=32)
                want, tol = h.copy(), np.full(h.shape, t)
                want[:, :32], tol[:, :32] = act_f64(h[:, :32], ACT_SWOOSH_L), act_tol(h[:, :32], t)
            else:
                res, orig, scale = uni(rng, M, N), nan(M, N + 7), uni(rng, N)
                orig[:, :N] = uni(rng, M, N)
                kw = dict(in_place=1, orig=orig, scale=scale)
                v, o, s = h + res, f64(orig[:, :N]), f64(scale)
                want = o + (v - o) * s                      # tests/gemm_forms.py's propagation through the residual and the mix
                tol = (t + U * np.abs(v)) * np.abs(s) + 2 * U * (np.abs(o) + np.abs((v - o) * s)) + U * np.abs(v - o) * np.abs(s)
            C = np.full((M, want.shape[1] + 5), SENTINEL, np.float32)
            if form == "bypass_in_place":
                C[:, :N] = res
            launch(op, A, W, bias, C, cfg, M, N, K, **kw)
            assert np.all(C[:, want.shape[1]:] == SENTINEL), "written past the last output column"
            err = np.abs(f64(C[:, :want.shape[1]]) - want)
            assert (err <= tol).all(), (form, M, K, cfg, float((err - tol).max()))


def conv_pair(op, x, wg, bg, wd, bd, B, T, D, K, cfg):
    """(the fused launch, the gated f16 GEMM on the same tile + dwconv1d_swoosh)"""
    M, taps = B * T, wd.shape[0]
    y = launch(op, x, wg, bg, nan(M, D), cfg, M, 2 * D, K, glu=1, wd=wd, bd=bd, T=T)
    hid, y2 = launch(op, x, wg, bg, nan(M, D), cfg, M, 2 * D, K, glu=1), nan(M, D)
    op("dwconv1d_swoosh", [B, T, D, taps], [hid, wd, bd, y2], {3})
    return y, y2


@pytest.mark.parametrize("T", [1, 7, 62, 64, 127, 128])
@pytest.mark.parametrize("taps", [15, 31])
def test_conv_tail_equals_the_two_launches_and_float64(op, taps, T):
    rng = np.random.default_rng(taps * 1000 + T)
    for cfg in [c for c in (1, 2) if T <= TILES[c][0]]:
        for B in (2, 3):
            for D in (64, 96):          # two and three 64-column tiles
                for K in (32, 96, 160):
                    w, b = uni(rng, 2 * D, K, scale=1.5 / np.sqrt(K)), uni(rng, 2 * D)
                    wg, bg = interleave(w, b, D)
                    x, wd, bd = uni(rng, B * T, K, scale=0.1), uni(rng, taps, D, scale=0.3), uni(rng, D)
                    y, y2 = conv_pair(op, x, wg, bg, wd, bd, B, T, D, K, cfg)
                    what = f"conv tail B={B} T={T} D={D} taps={taps} K={K} tile {cfg}"
                    assert np.array_equal(y.view(np.uint32), y2.view(np.uint32)), what
                    r16 = lambda a: a.astype(np.float16).astype(np.float32)   # noqa: E731
                    want, tol = conv_module_ref(r16(x), r16(w), b, wd, bd, B, T, D, taps)
                    assert (np.abs(f64(y) - want) <= tol).all(), what


@pytest.mark.parametrize("B,T,cfg", [(2, 64, 2), (3, 127, 1), (3, 7, 2)])
def test_one_lit_frame_stays_in_its_stream(op, B, T, cfg):
    """GLU(in_proj(x)) is 1 at the last frame of stream 1, channel c0, else 0: that channel sees the taps reversed in time, its neighbours nothing"""
    D, K, taps, c0, rng = 64, 32, 15, 37, np.random.default_rng(3)
    x, w, b = np.zeros((B * T, K), np.float32), np.zeros((2 * D, K), np.float32), np.zeros(2 * D, np.float32)
    x[T + T - 1, 5], w[c0, 5], b[D:] = 1.0, 1.0, 30.0
    wg, bg = interleave(w, b, D)
    wd, bd = uni(rng, taps, D, scale=0.5), np.zeros(D, np.float32)
    y, y2 = conv_pair(op, x, wg, bg, wd, bd, B, T, D, K, cfg)
    z = np.zeros((B, T, D))
    for k in range(taps):
        if 0 <= T - 1 + taps // 2 - k < T:
            z[1, T - 1 + taps // 2 - k, c0] = float(wd[k, c0])
    z = z.reshape(B * T, D)
    assert np.array_equal(y.view(np.uint32), y2.view(np.uint32))
    assert (np.abs(f64(y) - (np.logaddexp(0.0, z - 1.0) - 0.08 * z - 0.313261687)) <= act_tol(z, 0.0)).all()
    dark = y[z == 0.0]
    assert (dark.view(np.uint32) == dark.view(np.uint32)[0]).all(), "an element that no tap reaches differs from SwooshR(0)"


# max |level 2 - off| / max |off| of the encoder output: four times the worst value measured on an MI355X (DESIGN.md "Level 2")
DEVIATION_BOUND_2 = 4 * 1.33e-4   # measured: 1.327e-4 (zipformer2-tiny-test), 8.72e-5 (zipformer2-ctc-tiny-test)

def level2_launches(meta, B, T):
    """level 1's plus, per layer: #ff1_attn_in, the gated in_proj launches where the engine issues them (M >= 256), feed_forward2.out_proj"""
    ints = lambda k: [int(v) for v in meta[k].split(",")]   # noqa: E731
    T50, n = (T - 7) // 2, covered_launches(meta, B, T)
    for D, F, nl, ds in zip(ints("encoder_dims"), ints("feedforward_dims"), ints("num_encoder_layers"), ints("downsampling_factors")):
        M, Hc, k32 = B * -(-T50 // ds), 3 * D // 4, lambda K: int(K % 32 == 0)   # noqa: E731
        n += nl * (k32(D) + (M >= 256 and Hc % 16 == 0) * k32(D) + 2 * (M >= 256) * k32(D) + k32(F))
    return n


@pytest.mark.parametrize("preset", ["zipformer2-tiny-test", "zipformer2-ctc-tiny-test"])
def test_level_2_on_the_tiny_models(tmp_path, utts, preset):
    from k2transducerasr_amd import Model
    from k2transducerasr_amd.synth import write_synthetic_model
    path = str(tmp_path / "m.k2w")
    meta = write_synthetic_model(path, preset)
    model = Model(path, 0)
    x = model.pad_sequence([model.fbank(u) for u in utts]).reshape(len(utts), -1, 80)
    off = model.encoder_proj(x)
    model.set_encoder_precision(1)
    one = model.encoder_proj(x)
    model.set_encoder_precision(2)
    two = model.encoder_proj(x)
    n2 = model.encoder_f16_stats()["launches"]
    assert n2 == level2_launches(meta, *x.shape[:2]) and n2 > covered_launches(meta, *x.shape[:2])
    dev = np.abs(two.astype(np.float64) - off).max() / np.abs(off).max()
    print(f"{preset}: level 2 max |on - off| / max |off| = {dev:.3e} (bound {DEVIATION_BOUND_2:.3e}), {n2} launches")
    model.set_encoder_precision(1)
    assert np.array_equal(model.encoder_proj(x).view(np.uint32), one.view(np.uint32))
    assert model.encoder_f16_stats()["launches"] == covered_launches(meta, *x.shape[:2])
    model.set_encoder_precision(2)
    model.set_encoder_precision(0)
    assert model.encoder_f16_stats() == dict(launches=0, panels=0, panel_bytes=0)
    assert np.array_equal(model.encoder_proj(x).view(np.uint32), off.view(np.uint32))
    model.close()
    assert dev <= DEVIATION_BOUND_2


@pytest.mark.parametrize("suffix,level1_ok", [("feed_forward1.in_proj.weight", True), ("conv_module2.in_proj.weight", False)])
def test_a_newly_covered_weight_beyond_f16_refuses_level_2(tmp_path, tiny_model_path, suffix, level1_ok):
    from k2transducerasr_amd import K2HipError, Model
    from k2transducerasr_amd.k2w import read_k2w, write_k2w
    name = "encoder.encoders.1.layers.0." + suffix
    meta, tensors = read_k2w(tiny_model_path)
    tensors = {k: np.array(v) for k, v in tensors.items()}
    tensors[name][3, 5] = 1e5
    path = str(tmp_path / "big.k2w")
    write_k2w(path, meta, tensors.items())
    model = Model(path, 0)
    for level, ok in ((2, False), (1, level1_ok)):
        if ok:
            model.set_encoder_precision(level)
            assert model.encoder_f16_stats()["panels"] > 0
        else:
            with pytest.raises(K2HipError) as e:
                model.set_encoder_precision(level)
            assert e.value.code == -1 and name in str(e.value)
            assert model.encoder_f16_stats()["panels"] == 0
    model.close()
