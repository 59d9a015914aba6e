"""The encoder's half-precision switch on the device (k2hip_set_encoder_precision): gemm_f16_mfma alone (csrc/gemm_f16.hip, through
k2hip_debug_op_run "gemm_f16") against a float64 product of the f16-rounded operands, its rounding of A against numpy's, and the
switch on the tiny Zipformer2 models."""
import ctypes as C

import numpy as np
import pytest

from test_gemm_gpu import ACT_NONE, ACT_SWOOSH_L, ACT_TANH, act_f64

pytestmark = pytest.mark.gpu

# (M, N, K, epilogue): M 1 / 33 / 129 (second row tile of the small tiles) / 257; N 8 (less than a block) / 32 / 72 (ragged third
# block) / 136 (ragged second 128-tile); K 32 (one chunk: the prologue is the whole loop) / 64 / 96 (a half stage as tail) / 160 / 544
# (17 chunks: an odd stage count through the double buffer)
CASES = [(1, 8, 32, "none"), (33, 32, 64, "swoosh"), (129, 72, 96, "act_cols"), (257, 136, 160, "res_in_place"),
         (129, 136, 544, "tanh_after_res"), (257, 72, 544, "res_in_place"), (33, 8, 160, "tanh_after_res")]
SENTINEL = np.float32(-12345.0)


@pytest.fixture(scope="module")
def gemm_f16(hip_tiny):
    L = hip_tiny._L
    L.k2hip_debug_op_run.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                     C.c_int32, C.c_uint32]

    def run(ints, bufs, out):
        ptrs = (C.c_void_p * len(bufs))(*[b.ctypes.data if b is not None else None for b in bufs])
        sizes = (C.c_int64 * len(bufs))(*[b.nbytes if b is not None else 0 for b in bufs])
        rc = L.k2hip_debug_op_run(hip_tiny.handle, b"gemm_f16", (C.c_int64 * len(ints))(*ints), len(ints), ptrs, sizes, len(bufs),
                                  sum(1 << k for k in out))
        assert rc == 0, (rc, L.k2hip_last_error(), ints)
    return run


@pytest.mark.parametrize("cfg", [-1, 0, 1, 2])
@pytest.mark.parametrize("M,N,K,epi", CASES)
def test_kernel_against_float64(gemm_f16, M, N, K, epi, cfg):
    rng = np.random.default_rng(M * 1000 + N + K)
    lda, ldc, ldr = K + 4, N + 5, N + 3
    A = np.full((M + 3, lda), np.nan, np.float32)          # rows past M and the padding behind K are NaN
    A[:M, :K] = rng.uniform(-1, 1, (M, K))
    W = rng.uniform(-1, 1, (N, K)).astype(np.float32)
    bias = rng.uniform(-1, 1, N).astype(np.float32)
    res = rng.uniform(-1, 1, (M, ldr)).astype(np.float32)
    Cbuf = np.full((M, ldc), SENTINEL, np.float32)
    acc = A[:M, :K].astype(np.float16).astype(np.float64) @ W.astype(np.float16).astype(np.float64).T
    act, act_cols, after, in_place, b, r = ACT_NONE, 0, 0, 0, bias, None
    if epi == "none":
        b, want = None, acc
    elif epi == "swoosh":
        act, want = ACT_SWOOSH_L, act_f64(acc + bias, ACT_SWOOSH_L)
    elif epi == "act_cols":
        act, act_cols, want = ACT_SWOOSH_L, 32, acc + bias
        want[:, :32] = act_f64(want[:, :32], ACT_SWOOSH_L)
    elif epi == "res_in_place":
        in_place, ldr = 1, ldc
        Cbuf[:, :N] = res[:, :N]
        want = acc + bias + res[:, :N]
    else:
        act, after, r, want = ACT_TANH, 1, res, np.tanh(acc + bias + res[:, :N])
    plan = np.zeros(3, np.int32)
    gemm_f16([M, N, K, lda, ldc, ldr, act, act_cols, after, in_place, cfg], [A, W, b, r, Cbuf, plan], out=[4, 5])
    if cfg >= 0:
        assert plan[0] == cfg
    assert (plan[1], plan[2]) in [(128, 128), (128, 64), (64, 64)]
    assert np.all(Cbuf[:, N:] == SENTINEL), "written past column N"
    err = np.abs(Cbuf[:, :N].astype(np.float64) - want).max()
    tol = 2e-5 * max(1.0, np.sqrt(K))   # f16 x f16 products are exact in float32: only the float32 summation differs (test_gemm_gpu.py's bound)
    print(f"gemm_f16 {M}x{N}x{K} {epi} cfg {cfg} -> tile {plan[1]}x{plan[2]}: max err {err:.3g} (tol {tol:.3g})")
    assert err <= tol


def test_rounding_of_a_is_numpys(gemm_f16):
    """W = the first N rows of an identity, so C = f16(A)[:, :N]: exact ties, the f16 subnormal range, the largest finite value, the
    first value that rounds to infinity, an overflow, -0.0 and a NaN.  A truncating conversion fails on the ties."""
    M, N, K = 33, 72, 96
    rng = np.random.default_rng(7)
    A = (rng.standard_normal((M, K)) * np.exp2(rng.integers(-26, 10, (M, K)))).astype(np.float32)
    A[0, :8] = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 2049.0, 65504.0, 6e-8, 2.0 ** -25, -3.1e-8]
    A[1, :3] = [-0.0, 3e-6, 65519.0]
    A[5, 70], A[6, 3], A[7, 71] = 65520.0, 1e5, np.nan    # (each non-finite entry in a row of its own: inf x 0 fills its row with NaN)
    W = np.eye(K, dtype=np.float32)[:N].copy()
    Cbuf = np.full((M, N), SENTINEL, np.float32)
    gemm_f16([M, N, K, K, N, 0, 0, 0, 0, 0, -1], [A, W, None, None, Cbuf, np.zeros(3, np.int32)], out=[4])
    with np.errstate(over="ignore"):
        want = A.astype(np.float16).astype(np.float32)[:, :N]
    fin = np.all(np.isfinite(want), axis=1) & ~np.isin(np.arange(M), [5, 6, 7])
    assert fin.sum() == M - 3
    # bit-equal, but for the sign of zero: a sum that starts from +0 returns +0 for -0
    assert np.array_equal(Cbuf[fin].view(np.uint32), (want[fin] + np.float32(0)).view(np.uint32))
    with np.errstate(invalid="ignore", over="ignore"):
        ref = A.astype(np.float16).astype(np.float64) @ W.astype(np.float64).T
    for row in (5, 6, 7):
        assert np.array_equal(np.isnan(Cbuf[row]), np.isnan(ref[row])) and np.array_equal(np.isinf(Cbuf[row]), np.isinf(ref[row]))
    assert np.isinf(Cbuf[5, 70]) and np.isinf(Cbuf[6, 3]) and np.isnan(Cbuf[7]).all()


# max |on - off| / max |off| of the encoder output: four times the worst value measured on an MI355X over the fixture utterances of
# both presets (DESIGN.md "Half-precision operands in the encoder's linear layers": the line "measured deviation")
DEVIATION_BOUND = 4 * 8.14e-5   # measured: 8.14e-5 (zipformer2-tiny-test), 4.56e-5 (zipformer2-ctc-tiny-test)


def covered_launches(meta, B, T):
    """the linear() calls of one offline encoder pass that run on gemm_f16_mfma: plain launches over a packed weight with K % 32 == 0"""
    ints = lambda k: [int(v) for v in meta[k].split(",")]   # noqa: E731
    T50, n = (T - 7) // 2, 0
    for D, F, H, vh, nl, ds in zip(ints("encoder_dims"), ints("feedforward_dims"), ints("num_heads"), ints("value_head_dims"),
                                   ints("num_encoder_layers"), ints("downsampling_factors")):
        M, Hc, k32 = B * -(-T50 // ds), 3 * D // 4, lambda K: int(K % 32 == 0)   # noqa: E731
        assert (H * vh) % 32 != 0        # (self_attn out_proj: K = H vh stays float32 in these presets, fused or not)
        plain_nonlin, plain_conv = M < 256 or Hc % 16 != 0, M < 256    # else their in_proj carries a gated epilogue: float32
        n += nl * (k32(3 * F // 4) + plain_nonlin * k32(D) + k32(Hc) + 2 * k32(D) + 2 * plain_conv * k32(D) + 2 * k32(D) + 2 * k32(D) + k32(5 * F // 4))
    return n


@pytest.mark.parametrize("preset", ["zipformer2-tiny-test", "zipformer2-ctc-tiny-test"])
def test_switch_on_the_tiny_models(tmp_path, utts, preset):
    from k2transducerasr_amd import Model
    from k2transducerasr_amd.synth import write_synthetic_model
    path = str(tmp_path / "m.k2w")
    meta = write_synthetic_model(path, preset)
    model = Model(path, 0)
    x = model.pad_sequence([model.fbank(u) for u in utts]).reshape(len(utts), -1, 80)
    off = model.encoder_proj(x)
    model.set_encoder_precision(True)
    assert model.encoder_f16_stats()["panels"] > 0
    on = model.encoder_proj(x)
    assert model.encoder_f16_stats()["launches"] == covered_launches(meta, *x.shape[:2])
    assert not np.array_equal(on.view(np.uint32), off.view(np.uint32))
    dev = np.abs(on.astype(np.float64) - off).max() / np.abs(off).max()
    print(f"{preset}: max |on - off| / max |off| = {dev:.3e} (bound {DEVIATION_BOUND:.3e})")
    model.set_encoder_precision(False)
    assert model.encoder_f16_stats() == dict(launches=0, panels=0, panel_bytes=0)
    assert np.array_equal(model.encoder_proj(x).view(np.uint32), off.view(np.uint32))
    model.close()
    assert dev <= DEVIATION_BOUND


@pytest.mark.parametrize("preset", ["zipformer2-streaming-tiny-test", "conformer-tiny-test", "zipformer-tiny-test", "lstm-tiny-test"])
def test_other_families_are_unsupported(tmp_path, preset):
    from k2transducerasr_amd import K2HipError, Model
    from k2transducerasr_amd.synth import write_synthetic_model
    path = str(tmp_path / "m.k2w")
    write_synthetic_model(path, preset)
    model = Model(path, 0)
    with pytest.raises(K2HipError) as e:
        model.set_encoder_precision(True)
    assert e.value.code == -6
    model.close()


def test_a_weight_beyond_f16_refuses_the_switch(tmp_path, tiny_model_path, utts):
    from k2transducerasr_amd import K2HipError, Model
    from k2transducerasr_amd.k2w import read_k2w, write_k2w
    name = "encoder.encoders.1.layers.1.feed_forward3.in_proj.weight"
    meta, tensors = read_k2w(tiny_model_path)
    tensors = {k: np.array(v) for k, v in tensors.items()}
    tensors[name][3, 5] = 1e5
    path = str(tmp_path / "big.k2w")
    write_k2w(path, meta, tensors.items())
    model = Model(path, 0)
    want = model.offline_greedy_from_samples(utts)
    with pytest.raises(K2HipError) as e:
        model.set_encoder_precision(True)
    assert e.value.code == -1 and name in str(e.value)
    assert model.encoder_f16_stats()["panels"] == 0
    assert model.offline_greedy_from_samples(utts) == want     # goes on decoding in float32
    model.close()
