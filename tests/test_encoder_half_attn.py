"""Host side of level 4 of the encoder's half-precision switch: the route of a layer's attention core (csrc/gemm_plan.cpp attn_f16_route)
through k2hip_debug_gemm_f16_plan's 7-value form: no model, no device."""
import ctypes as C

import pytest

from test_encoder_half_wide import lib  # noqa: F401  (the fixture)

LAYER = dict(level=4, streaming=0, T=505, H=4, qh=32, vh=12, D=192)   # zipformer2-large-en's first stack on the headline batch


def route(L, **over):
    f = {**LAYER, **over}
    got, plan = C.c_int32(-1), (C.c_int32 * 3)()
    assert L.k2hip_debug_gemm_f16_plan((C.c_int64 * 7)(*[f[k] for k in LAYER]), 7, -1, C.byref(got), plan) == 0
    return got.value


@pytest.mark.parametrize("over,want", [
    (dict(), 1), (dict(level=3), 3), (dict(level=5), 3),
    (dict(streaming=1), 3),                      # the streaming tick never takes the route
    (dict(qh=24), 3),                            # the scores kernel is the head dim 32 one
    (dict(vh=20), 3), (dict(vh=16, H=8), 1),     # attn_av_out's fit: vh <= 16, H vh <= 128
    (dict(T=1276), 1), (dict(T=1277), 3),        # 32 rows of Tp + 4 floats in 160 KiB of LDS: Tp <= 1276
    (dict(H=16, vh=8), 1), (dict(H=20, vh=4), 3),   # heads w, w + 4, .. of four waves: at most 4 each
], ids=str)
def test_route_of_the_attention_core(lib, over, want):
    assert route(lib, **over) == want
