"""The offline conv module's in_proj + GLU + depthwise conv + SwooshR in ONE launch (csrc/gemm.hip gemm_f32_mfma_pipe<.., DWK>,
gemm_glu_dwconv1d) through the debug op "gemm_glu_dwconv1d", which runs what the layer body runs for the shape: the fused launch where
glu_dwconv_pipe_entry has one, else the GLU GEMM + dwconv1d_swoosh (from 256 rows on), else the plain in_proj + glu_dwconv1d_swoosh.

Every case runs twice, as the engine would run it and with K2HIP_NO_FUSED_CONV=1 (the two launches):
  * the two outputs are equal bit for bit -- the fused launch takes the tile of the GLU GEMM it replaces and forms the convolution's
    sums in k_glu_dwconv1d's order;
  * both are within the float64 reference's tolerance: test_kernels_gpu.dwconv1d_ref's, restated here for an input that is itself a
    rounded product -- the in_proj sums carry sum_tol(|x| |W|^T + |b|, D + 1), which the GLU passes on (|sigmoid| <= 1 on the value,
    |value| sigmoid' <= |value| / 4 on the gate).

Shapes.  The grid the change was specified with -- K 15 / 31, T 1, K/2, K-1, K, 63, 64, 65, 127, 128, B 1 / 3, D 64 / 192 (the
in_proj's K is D), and T = 129 with B = 2 -- has at most 384 rows, and a GLU GEMM that small runs on a ring tile with the K step
split over wave groups, not on a pipe tile: there the predicate says "two launches" and the op must report that (entry -1) and be
right.  The fused launch itself is reached from ~2000 rows on, so FUSED below adds the smallest shapes that reach each of its three
tiles with both tap counts: a full tile (T = BM), one dead row (T = BM - 1: the next stream's first row sits in the tile), many
dead rows, and a last stream whose tile hangs over the end of the tensor (every case: rows m0 + T .. m0 + BM - 1 of the last tile).
The op's report is asserted for each, so no case can pass by quietly taking the other path."""
import numpy as np
import pytest

from test_kernels_gpu import (U, act_tol, check, f64, nan, op, sigmoid64, sum_tol, switch, swoosh_r64, uni)  # noqa: F401  (op: the fixture)

pytestmark = pytest.mark.gpu

# (B, T, D, K, pipe table entry): 5 = 64 x 64, 1 = 128 x 64, 8 = 128 x 128
FUSED = [(32, 64, 192, 15, 5), (33, 63, 192, 31, 5), (40, 52, 192, 15, 5),
         (17, 128, 256, 31, 1), (17, 127, 256, 15, 1), (22, 100, 256, 31, 1),
         (32, 127, 512, 15, 8), (32, 128, 512, 31, 8)]


def interleave(w, b, D):
    """model.cpp's "#glu" order: row 32 q + p = value of channel 16 q + p, row 32 q + 16 + p = its gate"""
    ch = np.arange(D)
    rv = 32 * (ch // 16) + ch % 16
    wg, bg = np.empty_like(w), np.empty_like(b)
    wg[rv], wg[rv + 16] = w[:D], w[D:]
    bg[rv], bg[rv + 16] = b[:D], b[D:]
    return wg, bg


def conv_module_ref(x, w, b, wd, bd, B, T, D, K):
    """SwooshR(bd + sum_k wd[k] g[t + k - K/2]), g = GLU(x w^T + b) (value | gate halves), zero outside [0, T): float64, and the bound"""
    X, W = f64(x), f64(w)
    h = X @ W.T + f64(b)
    htol = sum_tol(np.abs(X) @ np.abs(W).T + np.abs(f64(b)), D + 1)
    val, gate = h[:, :D], h[:, D:]
    sg = sigmoid64(gate)
    g = (val * sg).reshape(B, T, D)
    gtol = (np.abs(val * sg) * (np.abs(gate) + 8) * U + htol[:, :D] * sg + np.abs(val) * 0.25 * htol[:, D:]).reshape(B, T, D)
    Wd = f64(wd)
    gp = np.zeros((B, T + K - 1, D))
    gp[:, K // 2:K // 2 + T] = g
    gm = np.abs(gp)
    z = np.broadcast_to(f64(bd), (B, T, D)).copy()
    zm = np.abs(z)
    for k in range(K):
        z += Wd[k] * gp[:, k:k + T]
        zm += np.abs(Wd[k]) * gm[:, k:k + T]
    ztol = sum_tol(zm, K + 1) + gtol.max() * np.sqrt((Wd ** 2).sum(0))
    return swoosh_r64(z).reshape(B * T, D), act_tol(z, ztol).reshape(B * T, D)


def run_both(op, x, wg, bg, wd, bd, B, T, D, K):
    """(y fused-or-whatever-the-engine-runs, its entry, y of the two launches)"""
    out = []
    for off in (0, 1):
        y, entry = nan(B * T, D), np.full(1, -7, np.int32)
        with switch("K2HIP_NO_FUSED_CONV", off):
            op("gemm_glu_dwconv1d", [B, T, D, K], [x, wg, bg, wd, bd, y, entry], {5, 6})
        out.append((y, int(entry[0])))
    assert out[1][1] == -1, ("K2HIP_NO_FUSED_CONV must keep the two launches", B, T, D, K, out[1][1])
    return out[0][0], out[0][1], out[1][0]


def case(op, rng, B, T, D, K, want_entry):
    # operands scaled so that the bound, which grows with sqrt(D) |x| |W|^T and passes through K taps, stays below check()'s 2e-5 at
    # D = 512 and K = 31 too: hidden values O(1) through the bias, the x term ~0.05 -- thousands of times the bound
    w, b = uni(rng, 2 * D, D, scale=1.5 / np.sqrt(D)), uni(rng, 2 * D)
    wg, bg = interleave(w, b, D)
    x, wd, bd = uni(rng, B * T, D, scale=0.1), uni(rng, K, D, scale=0.3), uni(rng, D)
    y, entry, y2 = run_both(op, x, wg, bg, wd, bd, B, T, D, K)
    what = f"gemm_glu_dwconv1d B={B} T={T} D={D} K={K}"
    assert entry == want_entry, (what, "entry", entry, "expected", want_entry)
    want, tol = conv_module_ref(x, w, b, wd, bd, B, T, D, K)
    check(y2, want, tol, what + " (two launches)")
    check(y, want, tol, what + f" (entry {entry})")
    assert np.array_equal(y.view(np.uint32), y2.view(np.uint32)), (what, "fused and two-launch outputs differ in",
                                                                   int((y.view(np.uint32) != y2.view(np.uint32)).sum()), "elements")


@pytest.mark.parametrize("K", [15, 31])
def test_specified_grid_reports_the_two_launches_and_is_right(op, K):
    """the grid of the specification: every shape has fewer than ~400 rows, so none has the fused form (module docstring); the op
    says so, and both runs are the same launches -- equal bit for bit and within the bound"""
    rng = np.random.default_rng(1500 + K)
    for T in sorted({1, K // 2, K - 1, K, 63, 64, 65, 127, 128}):
        for B in (1, 3):
            for D in (64, 192):
                case(op, rng, B, T, D, K, -1)
    case(op, rng, 2, 129, 192, K, -1)   # a stream longer than any tile


@pytest.mark.parametrize("B,T,D,K,entry", FUSED)
def test_fused_launch_equals_the_two_launches(op, B, T, D, K, entry):
    case(op, np.random.default_rng(B * 1000 + T), B, T, D, K, entry)


def test_longer_stream_than_the_tile_falls_back(op):
    """T = 129 at a size whose GLU GEMM does run on a 128-row pipe tile: not fused, still right"""
    case(op, np.random.default_rng(129), 17, 129, 256, 15, -1)


@pytest.mark.parametrize("B,T,D,K,entry", FUSED[:2] + FUSED[3:5] + FUSED[6:] + [(3, 40, 64, 15, -1)])
def test_one_lit_frame_comes_out_as_the_taps_reversed_in_time(op, B, T, D, K, entry):
    """x, in_proj and gate bias chosen so that GLU(in_proj(x)) is exactly 1 at one (stream, frame, channel) and exactly 0 elsewhere
    (one unit input row, one unit weight, gate bias 30: sigmoid = 1 in float32); conv bias 0.  Then the pre-activation output of that
    channel at frame t0 + K/2 - k is tap k exactly (one product by 1), every other element is 0: row, stream or channel misindexing
    that random data could hide moves or drops a tap."""
    rng = np.random.default_rng(7)
    wd, bd = uni(rng, K, D, scale=0.5), np.zeros(D, np.float32)
    half = K // 2
    for b0, t0, c0 in ((0, 0, 0), (B - 1, T - 1, D - 1), (B // 2, T // 2, 17), (B - 1, 0, 33), (1, T - 1, 16)):
        j = (5 * c0 + 3) % D
        x = np.zeros((B * T, D), np.float32)
        x[b0 * T + t0, j] = 1.0
        w, b = np.zeros((2 * D, D), np.float32), np.zeros(2 * D, np.float32)
        w[c0, j] = 1.0
        b[D:] = 30.0
        wg, bg = interleave(w, b, D)
        y, got_entry, y2 = run_both(op, x, wg, bg, wd, bd, B, T, D, K)
        assert got_entry == entry
        z = np.zeros((B, T, D))
        for k in range(K):
            t = t0 + half - k
            if 0 <= t < T:
                z[b0, t, c0] = float(wd[k, c0])
        z = z.reshape(B * T, D)
        check(y, swoosh_r64(z), act_tol(z, 0.0), f"lit frame ({b0}, {t0}, {c0}) B={B} T={T} D={D} K={K}")
        assert np.array_equal(y.view(np.uint32), y2.view(np.uint32))
        dark = y[z == 0.0]
        assert (dark.view(np.uint32) == dark.view(np.uint32)[0]).all(), "an element that no tap reaches differs from SwooshR(0)"
