"""Hand-written cases of the voice activity detector's segmentation machine, shared by the CPU tests (tests/test_vad.py: the float32
host reference and the float64 twin) and the GPU tests (tests/test_vad_gpu.py: the kernels).

A case is a decision string written as runs (value, length), every run at least 3 frames long.  features() turns it into a feature
matrix that produces exactly that string: one band bin holds s_t = d*[t + 2] (0.0 or 1.0, the ends repeated), margin is -1e30 and
abs_floor 0.5, so d_t = (m_t > 0.5) = "at least 3 of d*[t - 2 .. t + 2] are 1" = d*[t] for runs of 3 or more, and
m_t = (ones among d*[t - 2 .. t + 2]) / 5: the values the forced cut's argmin sees.  The expected segments are worked out by hand in
the comments, frame by frame where it matters."""
import numpy as np

NUM_BINS = 4


def config(max_speech):
    """W = 24, min_silence 6, min_speech 5, speech_pad 2; the band is bin 1 alone"""
    from k2transducerasr_amd import VadConfig
    return VadConfig(band_lo=1, band_hi=2, floor_window=24, rise=0.0, margin=-1e30, abs_floor=0.5, min_silence=6, min_speech=5, speech_pad=2,
                     max_speech=max_speech)


def decisions(runs):
    return np.concatenate([np.full(n, v, np.uint8) for v, n in runs])


def features(runs):
    d = decisions(runs)
    T = len(d)
    x = np.full((T, NUM_BINS), 7.0, np.float32)   # (the bins outside the band must not matter)
    x[:, 1] = d[np.minimum(np.arange(T) + 2, T - 1)]
    return x


# name -> (max_speech, runs, segments [(start, end, forced)] after a flush, is_speech before the flush)
CASES = {
    # a pause of min_silence - 1 = 5 frames does not end the segment: speech 4 .. 25 is one raw segment [4, 25), closed at t = 30
    # (30 + 1 - 25 = 6), reported [4 - 2, 25 + 2)
    "silence_run_one_short": (48, [(0, 4), (1, 8), (0, 5), (1, 8), (0, 10)], [(2, 27, 0)], False),
    # a pause of 6 does: [4, 12) closes at t = 17, [18, 26) at t = 31; the second start is 18 - 2 = 16 >= the first end 12 + 2 = 14
    "silence_run_exact": (48, [(0, 4), (1, 8), (0, 6), (1, 8), (0, 10)], [(2, 14, 0), (16, 28, 0)], False),
    # a speech run of min_speech - 1 = 4 frames is dropped
    "speech_run_one_short": (48, [(0, 4), (1, 4), (0, 10)], [], False),
    # ... of 5 frames is kept: [4, 9) -> [2, 11)
    "speech_run_exact": (48, [(0, 4), (1, 5), (0, 10)], [(2, 11, 0)], False),
    # speech from frame 0: the front padding is clipped by frame 0
    "padding_clipped_by_frame_0": (48, [(1, 6), (0, 10)], [(0, 8, 0)], False),
    # max_speech = 16, the cut looks at the last 8 frames.  start = 3, forced at t = 18 (18 + 1 - 3 = 16), window [11, 18]; the pause
    # d* = 0 at 12, 13, 14 gives m = 0.6, 0.4, 0.4, 0.4, 0.6, 0.8, 1, 1 over the window: the cut is 12, the first of the three 0.4.
    # The segment that follows starts at the cut: its front padding is clipped by the previous segment's end (12 - 2 < 12).  It ends
    # with the speech at 21, closed at t = 26: [12, 21 + 2)
    "forced_cut_inside_a_pause": (16, [(0, 3), (1, 9), (0, 3), (1, 6), (0, 10)], [(1, 12, 1), (12, 23, 0)], False),
    # constant speech: m = 1.0 over the whole window [11, 18], an exact tie: the earliest frame, 11.  Then start = 11 and the next cut
    # is due at t = 26, a silent frame (silence since 23, only 4 frames of it): window [19, 26] holds m = 1, 1, .8, .6, .4, .2, 0, 0,
    # the cut is 25 (the first of the two zeros), te = max(23, 25) = 25, start = 25.  The silence then closes at t = 30 with te - start
    # = 0 frames: dropped.  Two forced cuts in a row.
    "forced_cut_tie_then_silent_frame": (16, [(0, 3), (1, 20), (0, 10)], [(1, 11, 1), (11, 25, 1)], False),
    # the same up to the second cut (silence 23 .. 28, so m at 25 and 26 is still 0), but speech resumes at 29.  With te = max(te, c) =
    # 25 the silence has lasted 4 frames at t = 28 and the segment from 25 goes on (with te = 23 kept it would have closed at t = 28 and
    # a new one would start at 29).  It is cut again at t = 40 (40 + 1 - 25 = 16): silence since 38, window [33, 40] holds m = 1, 1, 1,
    # .8, .6, .4, .2, 0: the cut is 40, te = max(38, 40), and what is left is dropped at t = 45.
    "forced_cut_te_is_max_of_te_and_cut": (16, [(0, 3), (1, 20), (0, 6), (1, 9), (0, 10)], [(1, 11, 1), (11, 25, 1), (25, 40, 1)], False),
    # end of audio 3 frames into a pause: the segment ends where the pause began, [4, 12) -> [2, 14), 14 <= T = 15
    "flush_inside_a_pause": (48, [(0, 4), (1, 8), (0, 3)], [(2, 14, 0)], True),
    # end of audio in speech: the segment ends at T = 12 and its padding is clipped to T
    "flush_inside_speech": (48, [(0, 4), (1, 8)], [(2, 12, 0)], True),
    # nothing open at the end of audio: the flush reports nothing more
    "flush_with_nothing_open": (48, [(0, 4), (1, 5), (0, 10)], [(2, 11, 0)], False),
    "flush_of_silence": (48, [(0, 12)], [], False),
}
