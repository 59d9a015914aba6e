"""Every operand form and epilogue term GemmArgs (csrc/kernels.h) can express, one gemm() launch at a time, against float64.

tests/test_gemm_gpu.py holds the plain Linear form of every kernel family to a host product; the engines launch much more than that
form -- the [K,N] operand batched over streams and heads, the implicit-conv gather, the output gate, the bypass mix over an in-place
residual, activations on the first columns only, the joiner's tanh(enc[row / K] + dec), skip flags, layer-batched and split-K
launches -- and until here those reached a kernel only inside an engine, judged by token parity.  Each launch below goes through
k2hip_debug_op_run's "gemm" / "gemm_glu_causal_conv" ops (include/k2hip_debug.h): operands made here between NaN guards, leading
dimensions wider than the rows and pointers inside their buffers as the engines pass them, outputs pre-filled with NaN, every
element the launch writes compared with the float64 reference of tests/gemm_forms.py within its derived tolerance and every other
float of the output buffer bit-unchanged.  The hook reports the plan gemm() took; every test ends by asserting the number of
launches it made and the (family, index) plans it was written to reach, so a moved dispatcher threshold cannot empty a case.
tests/test_gemm_forms_ref.py runs the same cases on the CPU with a float32 product in the kernel's place.

That the cases bite was shown with single value-only mutations of csrc/gemm.hip, the file run once on each (first failing test):
  `col < act_cols` -> `<=`: test_act_cols_and_the_in_place_residual;  act_after_res ignored: test_skinny_families_by_automatic_dispatch;
  sW1 dropped in the [K,N] form, and mul read with ldc for ldm: test_kn_operand_batched_over_streams_and_heads;
  sBias0 dropped: test_batched_plain_form;  byp_scale[col] -> [0]: test_bypass_epilogue_over_an_in_place_residual;
  skinny reduction over red[0..2]: test_skinny_families_by_automatic_dispatch;  conv gather cv_sf -> 1: test_conv_gather.
(Residual row `row / res_div` -> `row` was not run: it reads up to res_div times past the residual buffer.  Its cases are those
of test_res_div_and_act_after_res and the joiner launches.)"""
import numpy as np
import pytest

import gemm_forms as gf
from test_kernels_gpu import ERR_UNSUPPORTED, Ring, check, glu_causal_conv_ref, nan, op, sum_tol, uni  # noqa: F401 (op: a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gemm(op):
    def run(launch, expect=0):
        """one gemm() launch through the hook: C's buffer after it and the plan the hook reports"""
        C = launch.C0.copy()
        plan = np.full(5, -1, np.int32)
        skip = None if launch.skip is None else np.array([launch.skip], np.int32)
        bufs = [launch.A, launch.W, launch.bias, None if launch.res_is_C else launch.res, C, skip, launch.mul, launch.orig, launch.scale, plan]
        op("gemm", launch.iargs(), bufs, {4, 9}, expect=expect)
        return C, gf.plan_name(plan)
    return run


def test_skinny_families_by_automatic_dispatch(gemm):
    """case 1: SKINNY3 / SKINNY6 / SKINNY6_8 with a wave's K slice of 16 / 32 / 48 / 80 floats (the masked look-ahead groups), M 1 /
    15 / 16 / 17 / 300, N 4 / 36 / 48 / 50 / 96, and the beam search's joiner launch tanh(A W^T + b + enc[row // beam]) with N = 500 /
    512 / 100 (second grid dimension, a last column chunk of 20 / 32 / 4 columns)"""
    gf.run_case(gf.case_skinny, 1, gemm, check)


def test_res_div_and_act_after_res(gemm):
    """case 2: the shared residual row and the activation behind the residual, each alone and both, on the skinny kernel and on the
    register-staged one (K % 64 != 0; M > 4096)"""
    gf.run_case(gf.case_res_div, 2, gemm, check)


def test_kn_operand_batched_over_streams_and_heads(gemm):
    """case 3: the [K,N] operand with the stride patterns of the Zipformer2 attention apply, NonlinAttention (mul / ldm / sM0) and the
    Conformer, K = T in 1 .. 250 with A's rows zero-padded to a multiple of 4, N 4 .. 288.  (GemmArgs::wz_map is gone: MODE_WKN
    reads z0 * sW0 like the other modes, which these launches check.)"""
    gf.run_case(gf.case_wkn, 3, gemm, check)


def test_conv_gather(gemm):
    """case 4: encoder_embed's two implicit-conv layouts (tests/test_gemm_forms_ref.py holds the gather reference to conv2d)"""
    gf.run_case(gf.case_conv, 4, gemm, check)


def test_bypass_epilogue_over_an_in_place_residual(gemm):
    """case 5: byp_orig / byp_scale / ld_orig with C == res on every forced family and the automatic choice"""
    gf.run_case(gf.case_bypass, 5, gemm, check)


def test_act_cols_and_the_in_place_residual(gemm):
    """case 6: SwooshL on the first act_cols columns only, the boundary inside and at the edge of a 16-column group"""
    gf.run_case(gf.case_act_cols, 6, gemm, check)


def test_batched_plain_form(gemm):
    """case 7: sBias0 over layers on LDS-DMA tiles 20 / 21, in place, split-K partials through nb1, the Conformer's score products"""
    gf.run_case(gf.case_batched, 7, gemm, check)


def test_skip_if_zero(gemm):
    """case 8: flag 0 leaves every float of C at its NaN prefill, flag 1 computes, in every kernel family"""
    gf.run_case(gf.case_skip, 8, gemm, check)


def test_relu_and_double_swish(gemm):
    """case 9: the two activations tests/test_gemm_gpu.py defines and never launches, in every kernel family"""
    gf.run_case(gf.case_relu_dswish, 9, gemm, check)


def glu_conv_operands(rng, B, Tc, D, K):
    """x, the "#glu"-interleaved in_proj, the conv module's filters, and the streams' caches in a non-identity subset of a larger pool"""
    pad, Kc = K // 2, (K + 1) // 2
    rg = Ring(rng, B, 1, 1, D * pad, [0] * B, nslots=B + 3)
    x, wg, bg = uni(rng, B * Tc, D), uni(rng, 2 * D, D, scale=2.0 / D), uni(rng, 2 * D, scale=0.5)
    wc, bc, ww, bw = uni(rng, D, Kc, scale=0.4), uni(rng, D), uni(rng, D, K, scale=0.3), uni(rng, D)
    sc = uni(rng, 2, D, K, scale=0.5)
    return rg, x, wg, bg, wc, bc, ww, bw, sc


def glu_conv_reference(rg, x, wg, bg, wc, bc, ww, bw, sc, B, Tc, D, K, dt=np.float64):
    """x Wg^T + bg over the interleaved rows (in precision dt), de-interleaved to (value | gate) halves, then the float64 GLU +
    chunk-causal convolution of tests/test_kernels_gpu.py"""
    z = x.astype(dt) @ wg.astype(dt).T + bg.astype(dt)
    ztol = sum_tol(np.abs(x.astype(np.float64)) @ np.abs(wg.astype(np.float64)).T + np.abs(bg.astype(np.float64)), D + 1)
    val, gate = gf.glu_interleave(D)
    x2, x2tol = np.concatenate([z[:, val], z[:, gate]], 1), np.concatenate([ztol[:, val], ztol[:, gate]], 1)
    cache0 = np.stack([rg.ring(rg.pool0, b).astype(np.float64).reshape(D, K // 2) for b in range(B)])
    want, tol, newcache = glu_causal_conv_ref(x2, cache0, wc, bc, ww, bw, sc, B, Tc, D, K, x2tol if dt == np.float64 else 0.0)
    # the cached frames are GLU outputs value * sigmoid(gate): the value's bound, a quarter of the gate's per unit of value, the exp
    ctol = x2tol.max() * (1.0 + 0.25 * np.abs(x2[:, :D]).max()) + np.abs(newcache).max() * 16 * gf.U
    return want, tol, newcache, ctol


def test_gemm_glu_causal_conv_against_float64(op):
    """case 10: in_proj + GLU + chunk-causal conv + cache advance in one ring launch, on entries 16 / 17 / 12 / 8, conv kernels 7 / 15 /
    31, Tc 2 .. 32, B Tc ragged against the tile: y, the named slots' advanced caches, every other float of the pool bit-unchanged.
    Shapes without a fused form come back UNSUPPORTED with nothing launched."""
    rng = np.random.default_rng(10)
    entries = {}
    for B, Tc, D, K, want_entry in gf.CONV_SHAPES:
        rg, x, wg, bg, wc, bc, ww, bw, sc = glu_conv_operands(rng, B, Tc, D, K)
        y, entry = nan(B * Tc, D), np.full(1, -7, np.int32)
        op("gemm_glu_causal_conv", [*rg.ints(), B, Tc, D, K], [x, wg, bg, rg.pool, rg.slots, wc, bc, ww, bw, sc, y, entry], {3, 10, 11})
        want, tol, newcache, ctol = glu_conv_reference(rg, x, wg, bg, wc, bc, ww, bw, sc, B, Tc, D, K)
        what = f"gemm_glu_causal_conv B={B} Tc={Tc} D={D} K={K}"
        assert int(entry[0]) == want_entry, (what, int(entry[0]))
        check(y, want, tol, what)
        newcache = newcache.reshape(B, 1, D * (K // 2))
        want_pool, _ = rg.after(newcache)
        rg.check_pool(rg.pool, want_pool, ctol, "cache " + what)
        entries[want_entry] = entries.get(want_entry, 0) + 1
    for B, Tc, D, K in gf.CONV_REFUSED:
        rg, x, wg, bg, wc, bc, ww, bw, sc = glu_conv_operands(rng, B, Tc, D, K)
        y, entry = nan(B * Tc, D), np.full(1, -7, np.int32)
        op("gemm_glu_causal_conv", [*rg.ints(), B, Tc, D, K], [x, wg, bg, rg.pool, rg.slots, wc, bc, ww, bw, sc, y, entry], {3, 10, 11},
           expect=ERR_UNSUPPORTED)
        assert np.isnan(y).all() and np.array_equal(rg.pool, rg.pool0)
    print(f"gemm_glu_causal_conv: {sum(entries.values())} launches, ring entries {dict(sorted(entries.items()))}")
    assert sum(entries.values()) >= 13 and set(entries) == {16, 17, 12, 8}
