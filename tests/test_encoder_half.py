"""Host side of the encoder's half-precision switch (k2hip_set_encoder_precision): the form predicate and tile rule of gemm_f16_mfma
(csrc/gemm_plan.cpp gemm_f16_form / plan_gemm_f16) and the panel packer (csrc/gemm_f16_layout.h), through k2hip_debug_gemm_f16_plan /
k2hip_debug_gemm_f16_pack: no model, no device."""
import ctypes as C

import numpy as np
import pytest

FIELDS = ["M", "N", "K", "lda", "ldc", "glu", "mul", "byp_orig", "w_kn", "cv_Fout", "nb0", "nb1", "res_div", "skip_if_zero", "cf_pool", "dw_w"]
COVERED = dict(M=4064, N=512, K=512, lda=512, ldc=512, glu=0, mul=0, byp_orig=0, w_kn=0, cv_Fout=0, nb0=1, nb1=1, res_div=1,
               skip_if_zero=0, cf_pool=0, dw_w=0)


@pytest.fixture(scope="module")
def lib():
    from k2transducerasr_amd import load_library
    L = load_library()
    L.k2hip_debug_gemm_f16_plan.argtypes = [C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.k2hip_debug_gemm_f16_pack.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]
    return L


def plan(L, force=-1, **over):
    f = dict(COVERED, **over)
    if "lda" not in over:
        f["lda"] = f["K"]
    form, out = C.c_int32(-1), (C.c_int32 * 3)()
    rc = L.k2hip_debug_gemm_f16_plan((C.c_int64 * 16)(*[f[k] for k in FIELDS]), 16, force, C.byref(form), out)
    assert rc == 0, L.k2hip_last_error()
    return form.value, tuple(out)


@pytest.mark.parametrize("over", [dict(glu=1), dict(glu=2), dict(mul=1), dict(byp_orig=1), dict(w_kn=1), dict(cv_Fout=8), dict(nb0=2), dict(nb1=3),
                                  dict(res_div=4), dict(skip_if_zero=1), dict(cf_pool=1), dict(dw_w=1), dict(K=48), dict(K=16), dict(K=100),
                                  dict(lda=514), dict(N=96, K=256), dict(N=48, K=512)], ids=str)
def test_each_uncovered_term_alone_is_refused(lib, over):
    assert plan(lib, **over) == (0, (-1, -1, -1))


@pytest.mark.parametrize("M,N,K,tile", [
    (4064, 512, 512, (1, 128, 64)),     # 32 x 4 = 128 tiles of 128 x 128, 32 x 8 = 256 of 128 x 64: exactly one per CU
    (3968, 512, 512, (2, 64, 64)),      # 31 x 8 = 248 of 128 x 64: one short of the rule -> 64 x 64
    (8000, 2048, 512, (0, 128, 128)),   # 63 x 16 tiles
    (2048, 2048, 768, (0, 128, 128)),   # 16 x 16 = 256
    (2048, 1920, 768, (1, 128, 64)),   # 16 x 15 = 240 of 128 x 128, 16 x 30 of 128 x 64
    (2048, 768, 2560, (2, 64, 64)),     # 96 / 192 large tiles
    (1, 8, 32, (2, 64, 64)),
    (16160, 48, 192, (2, 64, 64)),      # few columns stay covered while K < 256 ...
    (4064, 128, 512, (2, 64, 64)),      # ... and a long K from 97 columns on
])
def test_tile_by_workgroup_count(lib, M, N, K, tile):
    assert plan(lib, M=M, N=N, K=K, ldc=N) == (1, tile)
    for idx, bm, bn in [(0, 128, 128), (1, 128, 64), (2, 64, 64)]:
        assert plan(lib, force=idx, M=M, N=N, K=K, ldc=N) == (1, (idx, bm, bn))


def test_panels_hold_the_rounded_matrix():
    """N = 40 (a ragged second column block), K = 96 (three chunks): element (n, k) of W.astype(float16) sits, bit for bit, at
    block n // 32, chunk k // 32, [j = k % 16 // 8][hh = k % 32 // 16][n % 32][e = k % 8]; the padding columns are zero"""
    from k2transducerasr_amd import load_library
    L = load_library()
    L.k2hip_debug_gemm_f16_pack.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]
    N, K = 40, 96
    rng = np.random.default_rng(5)
    W = (rng.standard_normal((N, K)) * np.exp2(rng.integers(-20, 12, (N, K)))).astype(np.float32)
    W[3, 5], W[39, 95], W[0, 0] = 65504.0, -6e-8, 1 + 2.0 ** -11
    out = np.full(64 * K, 0xffff, np.uint16)
    fin = C.c_int32(-1)
    assert L.k2hip_debug_gemm_f16_pack(W.ctypes.data, N, K, out.ctypes.data, out.size, C.byref(fin)) == 0 and fin.value == 1
    p = out.reshape(2, K // 32, 2, 2, 32, 8)   # [block][chunk][j][hh][column][e]
    n, k = np.meshgrid(np.arange(64), np.arange(K), indexing="ij")
    got = p[n // 32, k // 32, k % 16 // 8, k % 32 // 16, n % 32, k % 8]
    want = np.zeros((64, K), np.uint16)
    want[:N] = W.astype(np.float16).view(np.uint16)
    assert np.array_equal(got, want)
    W[7, 9] = 1e5   # not finite in f16: reported
    assert L.k2hip_debug_gemm_f16_pack(W.ctypes.data, N, K, out.ctypes.data, out.size, C.byref(fin)) == 0 and fin.value == 0
