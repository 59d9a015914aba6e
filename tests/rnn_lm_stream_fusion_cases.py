"""The cases of the streaming neural LM shallow fusion tests (test_rnn_lm_stream_fusion.py on the CPU, test_rnn_lm_stream_fusion_gpu.py
on the device).

THE DEFINITION needs no streaming twin: after any chunking a stream holds what the offline fused search gives over all frames so far,
so the twin of prefix n is rnn_lm_fusion_twin.twin_beam_search(enc[:n], .., nbest=4).

CASES.  The accepted operator cases of rnn_lm_fusion_cases.SEEDS and both TOGETHER cases, unchanged.  Their per-frame gaps (the top
beam + 1 candidates of every frame) do not depend on the prefix: a frame's candidates are the same whatever follows.  The adjacent gaps
of the FINAL normalised scores do: the offline cases were accepted on the gaps at n = T' alone, and a stream is looked at after every
chunk.  A prefix end (stream, n) is NEAR-TIED when the twin's norm_gap over enc[:n] is below parity.LOGIT_TOL; there the order of the
alternatives (and, where the top two are the close pair, the pick) may legitimately differ between the float32 device and the twin.
NEAR_TIED records those ends per case (`python tests/rnn_lm_stream_fusion_cases.py` prints the tables); the CPU test recomputes them
and holds them to the record and to CAP; the GPU test excuses order and pick against the twin there and nowhere else.  Against the
ENGINE'S OWN offline fused search nothing is excused anywhere: both sides issue the same per-frame launches on the same M.

THE SCORE BOUND is rnn_lm_fusion_cases.score_bound at the prefix's own frame count n.

DROPPED names a recorded case, stream and prefix end at which the fused search's final beam holds a token sequence that the unfused
search's final beam over the same frames does not (the unfused search dropped it; rescoring could not bring it back), and the fused
pick at the end of the utterance differs from the unfused one: the case on which the GPU test shows that state is really carried."""
import numpy as np

import parity
import rnn_lm_fusion_cases as oc

NBEST = oc.NBEST
SCALE = oc.SCALE
YP_TOL = oc.YP_TOL
CHUNKINGS = (1, 3, 7, 0)      # frames per call; 0: the whole utterance in one call
CAP = 10                      # near-tied prefix ends a case may have, of 60 (3 streams x 20 frames)
score_bound = oc.score_bound

# (LM name, beam) -> sorted [(stream, n)] with the twin's norm_gap over enc[:n] below parity.LOGIT_TOL
NEAR_TIED = {
    ("A", 1): [],   # 0 of 60, pick within tolerance at 0
    ("A", 2): [],   # 0 of 60, pick within tolerance at 0
    ("A", 4): [(2, 5), (2, 14)],   # 2 of 60, pick within tolerance at 2
    ("A", 8): [(0, 3), (0, 6), (0, 7), (1, 16), (1, 17), (2, 9), (2, 13)],   # 7 of 60, pick within tolerance at 0
    ("B", 1): [],   # 0 of 60, pick within tolerance at 0
    ("B", 2): [],   # 0 of 60, pick within tolerance at 0
    ("B", 4): [(2, 5), (2, 14), (2, 19)],   # 3 of 60, pick within tolerance at 3
    ("B", 8): [(0, 1), (0, 9), (1, 18), (2, 19)],   # 4 of 60, pick within tolerance at 0
    ("C", 1): [],   # 0 of 60, pick within tolerance at 0
    ("C", 2): [],   # 0 of 60, pick within tolerance at 0
    ("C", 4): [(0, 14), (0, 15), (1, 7), (1, 14)],   # 4 of 60, pick within tolerance at 1
    ("C", 8): [(0, 8), (0, 13), (0, 14), (0, 16), (0, 18), (1, 7), (2, 7), (2, 16)],   # 8 of 60, pick within tolerance at 0
}
# what -> the same for the TOGETHER cases (LM A, beam 4)
NEAR_TIED_TOGETHER = {
    "hotwords": [(2, 5)],   # 1, pick within tolerance at 1
    "ngram": [],   # 0, pick within tolerance at 0
}
# prefix ends at which the twin's PICK itself is within tolerance (margins[n] < LOGIT_TOL): a subset of the above, at most 3 of 60
PICK_TIED_MAX = 3

DROPPED = dict(name="A", beam=4, stream=0, n=12, tokens=[35])   # (the first of 34 such (prefix end, hypothesis) pairs of that stream)


def case_inputs(tmpdir, oras, name, beam):
    """(oracle, enc [3, T', J], FusionLm) of the operator case (name, beam); oras: which -> Oracle"""
    base, seed, _ = oc.SEEDS[(name, beam)]
    ora = oras[oc.OPERATOR[name]]
    _, nlm, _ = oc.make_lm(tmpdir, name, seed)
    return ora, oc.encode(ora, oc.utterances(base)), nlm


def prefix_runs(ora, enc_b, beam, nlm, nbest=NBEST, **kw):
    """the twin over enc_b[:n] for n = 1 .. T' (index n - 1)"""
    from rnn_lm_fusion_twin import twin_beam_search
    return [twin_beam_search(ora, enc_b[:n], beam, nlm=nlm, nscale=SCALE if nlm is not None else 0.0, nbest=nbest, **kw) for n in range(1, enc_b.shape[0] + 1)]


def near_tied(runs_by_stream):
    """(sorted [(stream, n)] near-tied, how many of them have the pick itself within tolerance)"""
    out, picks = [], 0
    for b, runs in enumerate(runs_by_stream):
        for n, r in enumerate(runs, 1):
            if r.get("norm_gap", np.inf) < parity.LOGIT_TOL:
                out.append((b, n))
                picks += bool(r["margins"][n] < parity.LOGIT_TOL)
    return out, picks


def dropped_and_kept(ora, enc_b, beam, nlm):
    """[(n, tokens)] of the fused final beam over enc_b[:n] that the unfused final beam over the same frames does not hold"""
    fused = prefix_runs(ora, enc_b, beam, nlm, nbest=8)
    plain = prefix_runs(ora, enc_b, beam, None, nbest=8)
    out = []
    for n, (f, p) in enumerate(zip(fused, plain), 1):
        have = {tuple(a["tokens"]) for a in p["alts"]}
        out += [(n, list(a["tokens"])) for a in f["alts"] if tuple(a["tokens"]) not in have]
    return out, fused[-1]["ys"] != plain[-1]["ys"]


if __name__ == "__main__":   # the search that filled the tables above
    import sys
    import tempfile
    only = sys.argv[1:] or ["near", "together", "dropped"]
    with tempfile.TemporaryDirectory() as d:
        oras = {w: oc.make_oracle(d, w)[1] for w in ("tiny", "tiny165")}
        if "near" in only:
            for (name, beam) in sorted(oc.SEEDS):
                ora, enc, nlm = case_inputs(d, oras, name, beam)
                nt, picks = near_tied([prefix_runs(ora, enc[b], beam, nlm) for b in range(enc.shape[0])])
                print(f'    ("{name}", {beam}): {nt},   # {len(nt)} of {enc.shape[0] * enc.shape[1]}, pick within tolerance at {picks}', flush=True)
        if "together" in only:
            for what in sorted(oc.TOGETHER):
                base, seed, _ = oc.TOGETHER[what]
                enc = oc.encode(oras["tiny"], oc.utterances(base))
                ex = oc.together_extras(oras["tiny"], enc, what)
                _, nlm, _ = oc.make_lm(d, "A", seed)
                kw = dict(lm=ex.get("lm"), scale=ex.get("scale", 0.0), graph=ex.get("graph"))
                nt, picks = near_tied([prefix_runs(oras["tiny"], enc[b], 4, nlm, **kw) for b in range(enc.shape[0])])
                print(f'    "{what}": {nt},   # {len(nt)}, pick within tolerance at {picks}', flush=True)
        if "dropped" in only:
            for (name, beam) in sorted(oc.SEEDS):
                if beam < 2:
                    continue
                ora, enc, nlm = case_inputs(d, oras, name, beam)
                for b in range(enc.shape[0]):
                    dk, moved = dropped_and_kept(ora, enc[b], beam, nlm)
                    if dk and moved:
                        print(f'DROPPED = dict(name="{name}", beam={beam}, stream={b}, n={dk[0][0]}, tokens={dk[0][1]})   # {len(dk)} such (prefix end, hypothesis) pairs', flush=True)
