"""The inputs of the biased streaming CTC prefix beam search tests (helper of test_ctc_prefix_stream_bias.py, which checks them on the
CPU, and test_ctc_prefix_stream_bias_gpu.py, which runs them on the device).  Nothing new is drawn: the rows, phrase lists and LMs are
those of ctc_prefix_bias_cases.py, the chunkings those of ctc_prefix_stream_cases.py.

What a chunk boundary has to carry shows only where the inputs cross it in the ways that matter; test_ctc_prefix_stream_bias.py counts,
with the float64 twin at the ends of 16-frame chunks, the boundaries with a live slot whose match is pending and those whose final
order differs from the slot order, per group, and asserts each count non-zero.

The flip row of ctc_prefix_bias_cases.py in chunks of one frame (every value a multiple of 0.25, exact in float32 and float64):
    after frame 0   slots [a] (hs 1, ctx 1.5, pending 1.5 -> final -1.5), [b] (final -1.25): the result is [b], score -1.25
    after frame 1   slots [a, b] (ctx 3.0, the phrase committed, final 1.0), [b]:            the result is [a, b], score 1.0
    after frame 2   the result is [a, b], score 0.75
A carry that returns hs to the start state at a boundary never sees the phrase end: [a, b] keeps ctx 1.5 and ends at -2.25 + 1.5 = -0.75.
A carry that passes ctx on with the pending bonus subtracted gives [a] ctx 0 and [a, b] ctx 1.5: -0.75 again.  A carry in final order
puts [b] in slot 0 after frame 0, where the search over the row has [a]."""
import ctc_prefix_bias_cases as bc
import ctc_prefix_stream_cases as scases

CHUNK, SHORT_CHUNK = scases.CHUNK, 7
A, B = 1, 3       # the flip row's tokens
FLIP_STEPS = [([B], -1.25), ([A, B], 1.0), ([A, B], 0.75)]
FLIP_SLOTS_AFTER_FRAME_0 = [dict(tokens=[A], hs=1, ctx=1.5), dict(tokens=[B], hs=0, ctx=0.0)]
FLIP_WEAK_FINAL = -0.75
FLIP_CHUNKINGS = [[1, 1, 1], [1, 2], [2, 1]]
LEFT_OUT_LIMIT = 0.02     # of a chunking's intermediate chunk ends, at most this share may have a final gap below G


def group_of(name):
    return name.split()[0]


def chunkings(T):
    """the two chunkings every strict case runs in: 16 frames, and 7 with a ragged last chunk"""
    return [scases.uniform(T, CHUNK), scases.uniform(T, SHORT_CHUNK)]


def respelled_cases():
    """(name, row, beam, graph, lm, G) of the re-spelled row, per table kind"""
    return [(n, lp, beams[0], g, lm, G) for n, lp, beams, g, lm, G in bc.strict_cases() if n.startswith("re-spelled")]


def respelled_splits():
    return [ch for ch in scases.respelled_chunkings() if len(ch) == 2]
