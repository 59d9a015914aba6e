"""Host side of level 3 of the encoder's half-precision switch: the conv-gather form in the predicate (csrc/gemm_plan.cpp gemm_f16_fits),
the route of the ConvNeXt pointwise pair (convnext_f16_route) and the panels of an "#ohwi" conv weight: no model, no device."""
import ctypes as C

import numpy as np
import pytest

from test_encoder_half import COVERED, FIELDS
from test_encoder_half_wide import lib  # noqa: F401  (the fixture)

MORE = ["level", "glu_cols", "dw_K", "dw_T", "seg_len", "seg_stride", "cv_C", "pair_npix"]
CONV7 = dict(M=19 * 222, N=128, K=288, ldc=128, cv_Fout=19, seg_len=96, seg_stride=39 * 32, cv_C=32)   # encoder_embed.conv.7


def ask(L, level, **over):
    f = {**COVERED, **dict.fromkeys(MORE, 0), "level": level, **over}
    f["lda"] = 0 if f["cv_Fout"] else f["K"]
    got, plan = C.c_int32(-1), (C.c_int32 * 3)()
    assert L.k2hip_debug_gemm_f16_plan((C.c_int64 * 24)(*[f[k] for k in FIELDS + MORE]), 24, -1, C.byref(got), plan) == 0
    return got.value


def test_the_gather_form_is_level_3s(lib):
    assert [ask(lib, level, **CONV7) for level in (1, 2, 3)] == [0, 0, 1]
    assert ask(lib, 3) == 1 and ask(lib, 3, glu=1, N=1024) == 1           # levels 1 and 2's forms stay


@pytest.mark.parametrize("over", [dict(seg_len=24), dict(K=240, seg_len=80), dict(mul=1), dict(seg_stride=1250), dict(cv_C=6), dict(glu=1)], ids=str)
def test_level_3_refuses_a_gather_it_cannot_run(lib, over):
    assert ask(lib, 3, **{**CONV7, **over}) == 0


@pytest.mark.parametrize("npix,route", [(1, 1), (100, 1), (128, 1), (129, 1), (300960, 1), ((1 << 29) // 384, 1), ((1 << 29) // 384 + 1, 3)])
def test_route_of_the_pointwise_pair(lib, npix, route):
    """fused wherever the launches' 32-bit offsets hold (below a tile too: one workgroup); K2HIP_F16_CONVNEXT unset"""
    assert ask(lib, 3, pair_npix=npix) == route


def test_panels_of_an_ohwi_weight(lib):
    """a 3 x 3 conv filter [Co, Ci, 3, 3] repacked as model.cpp's "#ohwi" copy is ([Co][kt][kf][ci], K = 9 Ci) and packed: unpacked, the
    panels are numpy's f16 rounding of the repacked matrix"""
    Co, Ci = 40, 32
    W = np.random.default_rng(12).standard_normal((Co, Ci, 3, 3)).astype(np.float32)
    Wr = np.ascontiguousarray(W.transpose(0, 2, 3, 1).reshape(Co, 9 * Ci))
    out, fin = np.full(64 * 9 * Ci, 0xffff, np.uint16), C.c_int32(-1)
    assert lib.k2hip_debug_gemm_f16_pack(Wr.ctypes.data, Co, 9 * Ci, out.ctypes.data, out.size, C.byref(fin)) == 0 and fin.value == 1
    n, k = np.meshgrid(np.arange(64), np.arange(9 * Ci), indexing="ij")
    got = out.reshape(2, 9, 2, 2, 32, 8)[n // 32, k // 32, k % 16 // 8, k % 32 // 16, n % 32, k % 8]    # [block][chunk][j][hh][column][e]
    assert np.array_equal(got[:Co], Wr.astype(np.float16).view(np.uint16)) and not got[Co:].any()
