"""Host side of level 2 of the encoder's half-precision switch: the form predicate at both levels (csrc/gemm_plan.cpp gemm_f16_form), the
conv-tail rule (glu_dwconv_f16_entry / glu_dwconv_f16_route) and the panels of a "#glu"-interleaved weight: no model, no device."""
import ctypes as C

import numpy as np
import pytest

from test_encoder_half import COVERED, FIELDS

GLU = dict(M=4064, N=1024, K=512, ldc=512, glu=1)
FORMS = {"glu": GLU, "tanh_glu_cols": dict(N=1152, ldc=768, glu=2, glu_cols=768), "bypass": dict(K=1536, byp_orig=1),
         "conv_tail": dict(GLU, M=3968, dw_w=1, dw_K=31, dw_T=124)}

@pytest.fixture(scope="module")
def lib():
    from k2transducerasr_amd import load_library
    L = load_library()
    L.k2hip_debug_gemm_f16_plan.argtypes = [C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.k2hip_debug_conv_f16_plan.argtypes = [C.c_int32] * 4 + [C.POINTER(C.c_int32)] * 2
    L.k2hip_debug_gemm_f16_pack.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]
    return L


def form(L, level, **over):
    f = {**COVERED, "level": level, "glu_cols": 0, "dw_K": 0, "dw_T": 0, **over}
    f["lda"] = f["K"]
    got, plan = C.c_int32(-1), (C.c_int32 * 3)()
    assert L.k2hip_debug_gemm_f16_plan((C.c_int64 * 20)(*[f[k] for k in FIELDS + ["level", "glu_cols", "dw_K", "dw_T"]]), 20, -1, C.byref(got), plan) == 0
    return got.value


@pytest.mark.parametrize("name", FORMS)
def test_level_2_accepts_what_level_1_rejects(lib, name):
    assert (form(lib, 1, **FORMS[name]), form(lib, 2, **FORMS[name])) == (0, 1)
    assert form(lib, 1) == form(lib, 2) == 1            # the plain form (with it #ff1_attn_in's: act_cols is no field of the predicate)
    assert form(lib, 2, **dict(FORMS[name], mul=1)) == 0


@pytest.mark.parametrize("over", [dict(glu=3), dict(glu_cols=48), dict(dw_w=1, dw_K=31, dw_T=124, glu=0), dict(dw_w=1, dw_K=7, dw_T=124),
                                  dict(dw_w=1, dw_K=31, dw_T=129, M=4128), dict(dw_w=1, dw_K=31, dw_T=100), dict(dw_w=1, dw_K=31, dw_T=124, N=1056)], ids=str)
def test_level_2_still_refuses(lib, over):
    assert form(lib, 2, **{**GLU, "M": 3968, **over}) == 0


@pytest.mark.parametrize("B,T,D,K,entry", [(32, 64, 512, 31, 2), (32, 63, 512, 15, 2), (32, 65, 512, 31, 1), (32, 128, 768, 15, 1), (32, 129, 512, 31, -1),
                                           (32, 124, 528, 31, -1), (32, 124, 512, 7, -1), (32, 124, 512, 33, -1), (1, 1, 32, 15, 2)])
def test_conv_tail_rule(lib, B, T, D, K, entry):
    e, route = C.c_int32(-9), C.c_int32(-9)
    assert lib.k2hip_debug_conv_f16_plan(B, T, D, K, C.byref(e), C.byref(route)) == 0
    assert e.value == entry and route.value in ((1, 2, 3) if entry >= 0 else (2, 3))


def test_panels_of_an_interleaved_weight(lib):
    """the conv module's in_proj [2 D, D], value rows | gate rows, interleaved as model.cpp's "#glu" copy is and packed: unpacked, the
    panels are numpy's interleave of the f16-rounded original"""
    D = 48
    W = np.random.default_rng(11).standard_normal((2 * D, D)).astype(np.float32)[:, :32].copy()   # K = 32
    ch = np.arange(D)
    rv = 32 * (ch // 16) + ch % 16
    Wg = np.empty_like(W)
    Wg[rv], Wg[rv + 16] = W[:D], W[D:]
    out, fin = np.full(2 * D * 32, 0xffff, np.uint16), C.c_int32(-1)
    assert lib.k2hip_debug_gemm_f16_pack(Wg.ctypes.data, 2 * D, 32, out.ctypes.data, out.size, C.byref(fin)) == 0 and fin.value == 1
    n, k = np.meshgrid(np.arange(2 * D), np.arange(32), indexing="ij")
    got = out.reshape(3, 1, 2, 2, 32, 8)[n // 32, 0, k % 16 // 8, k // 16, n % 32, k % 8]    # [block][chunk][j][hh][column][e]
    W16 = W.astype(np.float16).view(np.uint16)
    assert np.array_equal(got[rv], W16[:D]) and np.array_equal(got[rv + 16], W16[D:])
