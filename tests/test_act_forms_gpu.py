"""Swoosh's softplus has two forms in csrc/act.h: softplus_ge1, which every GEMM epilogue and elementwise kernel uses (v_log_f32 and
the extended-precision product with ln 2, nothing else), and softplus_libm, the library's general log it replaced.  The contract is
bit identity for every input: the "act_forms" op of k2hip_debug_op_run evaluates both in one plain kernel and the outputs are
compared here as uint32, NaN to NaN.  A second test runs the activations through one kernel of every GEMM family against a float64
product on the host, as tests/test_gemm_gpu.py does."""
import numpy as np
import pytest

from test_gemm_gpu import ACT_SWOOSH_L, ACT_SWOOSH_R, act_f64, gemm_run, operands  # noqa: F401  (gemm_run: fixture)
from test_kernels_gpu import act_tol, op  # noqa: F401  (op: fixture)

pytestmark = pytest.mark.gpu


def _f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def _around(x, ulps=32768):
    """every bit pattern within +-ulps of x"""
    c = int(np.float32(x).view(np.uint32))
    return np.arange(c - ulps, c + ulps + 1, dtype=np.int64).astype(np.uint32)


@pytest.fixture(scope="module")
def patterns():
    walk = np.arange(0, 1 << 32, 1021, dtype=np.int64).astype(np.uint32)           # all 2^32 patterns at stride 1021
    # z = 15 (the select) is x = 19 for SwooshL and 16 for SwooshR; e^z overflows near z = 88.7 (x = 92 / 89) and goes denormal
    # near z = -87 (x = -83)
    near = [_around(x) for x in (19.0, 16.0, 92.0, 89.0, -83.0)]
    fmin = np.float32(np.finfo(np.float32).tiny)
    special = np.concatenate([np.array([0.0, -0.0, fmin, -fmin, np.inf, -np.inf, np.nan], np.float32).view(np.uint32),
                              np.array([1, 2, 3, 0x80000001, 0x80000002, 0x80000003], np.uint32)])   # the smallest denormals
    return np.ascontiguousarray(np.concatenate([walk, *near, special]))


@pytest.mark.parametrize("act", [ACT_SWOOSH_L, ACT_SWOOSH_R])
def test_lean_and_library_softplus_agree_bit_for_bit(op, patterns, act):  # noqa: F811
    x = _f32(patterns).copy()
    n = x.size
    assert 4.2e6 < n < 4.7e6
    y_lean, y_libm = np.full(n, np.nan, np.float32), np.full(n, np.nan, np.float32)
    op("act_forms", [act, n], [x, y_lean, y_libm], {1, 2})
    a, b = y_lean.view(np.uint32), y_libm.view(np.uint32)
    both_nan = np.isnan(y_lean) & np.isnan(y_libm)
    diff = (a != b) & ~both_nan
    assert not diff.any(), (act, int(diff.sum()), [(hex(int(patterns[i])), hex(int(a[i])), hex(int(b[i]))) for i in np.flatnonzero(diff)[:4]])
    # and the outputs are the activation: inputs of moderate size against float64 within tests/test_kernels_gpu.py's bound for
    # the hardware exp / log, so a kernel that wrote the same wrong value twice cannot pass
    fin = np.isfinite(x) & (np.abs(x) < 64.0)
    z = x[fin].astype(np.float64)
    assert (np.abs(y_lean[fin] - act_f64(z, act)) <= act_tol(z, 0.0)).all()
    assert np.isnan(y_lean[np.isnan(x)]).all()


GEMM_SHAPES = [(130, 96, 64), (65, 70, 32)]
GEMM_CFGS = [-1, 2001, 3000, 105]      # the dispatcher's choice, pipe 128x64, p16 64x96, ring 64x64: one per family
_MIN_K = {-1: 4, 2001: 64, 3000: 64, 105: 32}   # gemm_plan.cpp: three pipeline stages need two K steps; ring entry 5 has no K split


def test_swoosh_epilogue_of_every_gemm_family_against_float64(gemm_run):  # noqa: F811
    ran = 0
    for si, (M, N, K) in enumerate(GEMM_SHAPES):
        A, W, bias, _ = operands(M, N, K, 900 + si)
        z = A.astype(np.float64) @ W.astype(np.float64).T + bias.astype(np.float64)
        tol = 2e-5 * max(1.0, K ** 0.5)            # tests/test_gemm_gpu.py's bound
        for cfg in GEMM_CFGS:
            if K < _MIN_K[cfg]:
                continue
            for act in (ACT_SWOOSH_L, ACT_SWOOSH_R):
                got = gemm_run(A, W, bias, None, act, cfg)
                assert np.isfinite(got).all(), (cfg, M, N, K, act, "an element was not written")
                err = np.abs(got.astype(np.float64) - act_f64(z, act))
                assert err.max() <= tol, (cfg, M, N, K, act, float(err.max()), tol, np.unravel_index(err.argmax(), err.shape))
                ran += 1
    assert ran == 12
