"""The inputs of the streaming hotword tests (helper of test_hotwords_stream.py / test_hotwords_stream_gpu.py): the streaming tiny
model's oracle frames with phrases drawn from its unbiased result, and the prefix lengths the GPU tests check.  The reference is
chunk-invariant by construction: after a step a stream must hold what hotword_twin.twin_beam_search gives over the frames so far,
so the twin over every checked PREFIX is the whole definition -- the chunking does not enter it."""
import functools

import numpy as np

from hotword_twin import SCORE, TwinGraph, draw_phrases, twin_beam_search

STREAM_PRESET = "zipformer2-streaming-tiny-test"
STREAM_UTT = (7, 2.4)           # synth_utterance(seed, seconds): the utterance of test_online_beam_gpu.py's operator-level test
STREAM_BEAMS = (1, 2, 4, 8)
STREAM_PHRASES, STREAM_PHRASE_SEED = 8, 5
STEPS = (1, 8, 13, None)        # chunkings of the operator-level test (None: all frames in one call)
SCORE_TOL = 2e-3                # the streaming beam tests' figure


def prefix_ends(n_frames, steps):
    """the prefix lengths at which a stream fed in chunks of `step` frames is checked, over all steps"""
    ends = set()
    for step in steps:
        step = n_frames if step is None else step
        ends |= set(range(step, n_frames, step)) | {n_frames}
    return sorted(ends)


def stream_phrases(unbiased):
    """unbiased: (tokens, timestamps) of the unbiased beam-4 search over the whole utterance"""
    return draw_phrases([unbiased], STREAM_PHRASES, np.random.default_rng(STREAM_PHRASE_SEED))


_TWIN = {}


def twin_prefix(key, oracle, enc, n, beam, phrases):
    """twin_beam_search over enc[:n], cached per (key, n, beam) -- `key` names (model, utterance, phrase set)"""
    k = (key, n, beam)
    if k not in _TWIN:
        _TWIN[k] = twin_beam_search(oracle, enc[:n], beam, TwinGraph(phrases, SCORE, oracle.vocab_size))
    return _TWIN[k]


def twin_final_states(oracle, enc, beam, graph):
    """the hypotheses the twin holds after each frame n = 1 .. len(enc): {n: [(ys, raw log-prob, pending(state), len incl. the ctx
    blanks)]} in insertion order (one pass: the hypotheses after frame n do not depend on the frames behind it).  A restatement
    of twin_beam_search's frame loop WITHOUT its final pick, used only to show that the finalize rule decides something
    (test_hotwords_stream.py, item 1 b); the reference stays twin_beam_search."""
    import torch
    cs = oracle.context_size
    ys0 = [0] * cs
    B = {tuple(ys0): dict(ys=ys0, lp=torch.zeros(1), st=0)}
    out = {}
    for t in range(enc.shape[0]):
        A = list(B.values())
        B = {}
        dec = oracle.decoder(np.array([h["ys"][-cs:] for h in A], np.int64))
        lg = torch.from_numpy(oracle.joiner(np.repeat(enc[t: t + 1], len(A), 0), dec)).log_softmax(-1)
        lg = (lg + torch.cat([h["lp"].reshape(1, 1) for h in A])).reshape(-1)
        V = lg.numel() // len(A)
        tv, ti = lg.topk(min(2 * beam, lg.numel()))
        order = np.lexsort((ti.numpy(), -tv.numpy()))
        tv, ti = tv[order], ti[order]
        for k in range(min(beam, lg.numel())):
            h, tok = A[int(ti[k]) // V], int(ti[k]) % V
            ys, st, lp = h["ys"][:], h["st"], tv[k].reshape(1)
            if tok not in (0, 2):
                ys.append(tok)
                st, bonus, _ = graph.step(st, tok)
                lp = lp + torch.tensor([bonus], dtype=torch.float32)
            key = tuple(ys)
            if key in B:
                B[key]["lp"] = torch.logaddexp(B[key]["lp"], lp)
            else:
                B[key] = dict(ys=ys, lp=lp, st=st)
        out[t + 1] = [(h["ys"][cs:], float(h["lp"]), float(graph.pending(h["st"])), len(h["ys"])) for h in B.values()]
    return out


@functools.lru_cache(maxsize=None)
def stream_case(path):
    """(oracle, enc [N, J], unbiased (tokens, timestamps) at beam 4, phrases) of the streaming tiny model written at `path`"""
    from k2transducerasr_amd.synth import synth_utterance
    from oracle.online import OnlineOracle
    from test_online_beam_gpu import oracle_frames
    ora = OnlineOracle(path)
    enc, _ = oracle_frames(ora, ora.fbank(synth_utterance(*STREAM_UTT)))
    (res,) = ora.modified_beam_search(enc[None], 4)
    unbiased = (res[0], res[1])
    return ora, enc, unbiased, stream_phrases(unbiased)
