"""The predicate and tile rule of the offline conv module's fused launch (csrc/gemm_plan.cpp glu_dwconv_pipe_entry) through
k2hip_debug_conv_fused_plan: host only, no model, no device.

The rule: the fused launch exists where the GLU in_proj GEMM it replaces (M = B T rows >= 256, N = 2 D, K = D) runs on one of the pipe
tiles 128 x 64 (entry 1), 64 x 64 (5), 128 x 128 (8), a stream's T frames fit the tile's rows, and one tile per stream does not add a
round of the 256 CUs.  It takes that tile, which is what makes it bit-identical to the two launches."""
import ctypes as C

import pytest

DIMS = [192, 256, 512, 768, 512, 256]      # zipformer2-large-en (config.py)
KERNELS = [31, 31, 15, 15, 15, 31]
DS = [1, 2, 4, 8, 4, 2]
TILE_ROWS = {1: 128, 5: 64, 8: 128}
TILE_COLS = {1: 64, 5: 64, 8: 128}


@pytest.fixture(scope="module")
def plan():
    from k2transducerasr_amd import load_library
    L = load_library()
    L.k2hip_debug_conv_fused_plan.argtypes = [C.c_int32] * 5 + [C.POINTER(C.c_int32)]

    def run(B, T, D, K, streaming=0):
        e = C.c_int32(-99)
        rc = L.k2hip_debug_conv_fused_plan(B, T, D, K, streaming, C.byref(e))
        assert rc == 0, (rc, L.k2hip_last_error())
        return e.value
    return run


def stack_frames(seconds):
    """frames per utterance in each of the six stacks: fbank frames (25 ms / 10 ms, snip edges) + PadSequence's 19, the embed's
    (n - 7) // 2, then each stack's downsampling, rounded up"""
    t0 = ((1 + (16000 * seconds - 400) // 160) + 19 - 7) // 2
    return [-(-t0 // d) for d in DS]


def test_headline_batch_fuses_the_three_low_rate_stacks(plan):
    """32 x 10 s: T = 505, 253, 127, 64, 127, 253.  The T = 127 stacks (D = 512) run their GLU GEMM 4064 x 1024 x 512 on 128 x 128
    tiles, the T = 64 stack (D = 768) 2048 x 1536 x 768 on 64 x 64 tiles: one stream per tile in both.  The others do not fit a tile."""
    assert stack_frames(10) == [505, 253, 127, 64, 127, 253]
    got = [plan(32, T, D, K) for T, D, K in zip(stack_frames(10), DIMS, KERNELS)]
    assert got == [-1, -1, 8, 5, 8, -1]


def test_longer_utterances(plan):
    """20 s: only the 6.25 Hz stack still holds a stream in a tile (T = 126; its GEMM 4032 x 1536 x 768 runs on 128 x 64 tiles);
    30 s: none (T >= 189).  Whatever the entry, it is a tile that holds the stream and divides the columns."""
    assert [plan(32, T, D, K) for T, D, K in zip(stack_frames(20), DIMS, KERNELS)] == [-1, -1, -1, 1, -1, -1]
    assert [plan(32, T, D, K) for T, D, K in zip(stack_frames(30), DIMS, KERNELS)] == [-1] * 6
    for secs in (10, 20, 30):
        for B in (1, 8, 32, 64):
            for T, D, K in zip(stack_frames(secs), DIMS, KERNELS):
                e = plan(B, T, D, K)
                assert e in (-1, 1, 5, 8)
                if e >= 0:
                    assert T <= TILE_ROWS[e] and (2 * D) % TILE_COLS[e] == 0 and B * T >= 256


def test_fewer_than_256_rows_keep_the_plain_in_proj(plan):
    assert plan(2, 127, 512, 15) == -1      # 254 rows
    assert plan(1, 128, 512, 15) == -1
    assert plan(3, 64, 768, 15) == -1
    assert plan(1, 1, 64, 15) == -1


def test_small_batches_whose_gemm_runs_on_another_kernel_are_not_fused(plan):
    """a GLU GEMM of a few hundred rows runs on a ring tile with the K step split over wave groups (other sums): two launches"""
    assert plan(3, 127, 192, 15) == -1
    assert plan(3, 128, 64, 31) == -1
    assert plan(4, 127, 512, 15) == -1


def test_tile_rule(plan):
    assert plan(32, 128, 512, 15) == 8      # a full tile
    assert plan(17, 129, 256, 15) == -1     # a stream longer than its GEMM's tile
    assert plan(32, 65, 512, 15) == -1      # 2080 x 1024 x 512 runs on 64 x 64 tiles: T = 65 does not fit
    assert plan(32, 127, 512, 7) == -1      # tap counts without an instantiation
    assert plan(32, 127, 512, 16) == -1
    assert plan(32, 127, 512, 33) == -1
    assert plan(0, 127, 512, 15) == -1 and plan(32, 0, 512, 15) == -1
    # half-empty tiles may not add a round of the chip: 2560 x 1536 x 768 is 40 x 24 = 960 tiles of 64 x 64 (4 rounds); a tile per
    # stream of 16 frames would be 160 x 24 = 3840 (15 rounds)
    assert plan(160, 16, 768, 15) == -1


def test_the_cases_of_the_gpu_test(plan):
    """tests/test_conv_fused_offline_gpu.py's FUSED list names the tile each case must reach"""
    for B, T, D, K, e in [(32, 64, 192, 15, 5), (33, 63, 192, 31, 5), (40, 52, 192, 15, 5), (17, 128, 256, 31, 1), (17, 127, 256, 15, 1),
                          (22, 100, 256, 31, 1), (32, 127, 512, 15, 8), (32, 128, 512, 31, 8), (17, 129, 256, 15, -1), (3, 40, 64, 15, -1)]:
        assert plan(B, T, D, K) == e, (B, T, D, K)


def test_streaming_site_and_switch(plan):
    from k2transducerasr_amd import set_switch
    assert plan(32, 127, 512, 15, streaming=1) == -1
    assert plan(32, 64, 768, 15, streaming=1) == -1
    set_switch("K2HIP_NO_FUSED_CONV", 1)
    try:
        assert plan(32, 127, 512, 15) == -1 and plan(32, 64, 768, 15) == -1
    finally:
        set_switch("K2HIP_NO_FUSED_CONV", 0)
    assert plan(32, 127, 512, 15) == 8
    set_switch("K2HIP_NO_GLU_EPILOGUE", 1)      # no GLU GEMM to extend
    try:
        assert plan(32, 127, 512, 15) == -1
    finally:
        set_switch("K2HIP_NO_GLU_EPILOGUE", 0)
