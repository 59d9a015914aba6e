"""The CTC prefix beam search on inputs that tie on purpose (tests/ctc_prefix_tie_cases.py): exact ties inside a thread's list, across the
lanes, rows and waves of the selection, across slots, between a stay candidate and an extension, through folds, at the beam cut and in
the final order -- through every form of csrc/ctc_prefix.hip: the offline kernel ("ctc_prefix_beam"), the resumed one
("ctc_prefix_resume") under three chunkings, the biased instantiation ("ctc_prefix_beam_bias") and the public entry.

Bounds (none taken from what the engine gives; tests/test_ctc_prefix_tie_cases_ref.py checks every row on the CPU):
  * tokens, timestamps, n_hyps, the order of the entries and the token log-probs are EXACT on every row at every beam 1 .. 8, nbest =
    beam.  Nothing is excused: a row is in the suite only if every decision of the float64 twin is a tie between equally formed (or
    exact) scores or at least G = 8 E apart (G from 3.7e-6 to 8.9e-6; the smallest gap that is no tie is 0.031);
  * mirrored scores are within 1e-5 relative to max(1, |value|), the bound of tests/test_ctc_prefix_gpu.py; dyadic scores are BIT-EQUAL
    to the twin's (every sum is exact, every logaddexp has a -inf operand);
  * the resumed kernel, the biased instantiation with tables that cannot fire and the public entry are bit-equal to the offline op.
Outputs are pre-filled with -7.  Worst differences seen on an MI355X are recorded in DESIGN.md "The CTC prefix beam search on exact
ties, folds and the beam cut"."""
import numpy as np
import pytest

import ctc_prefix_bias_cases as bc
import ctc_prefix_tie_cases as tc
from ctc_prefix_bias_twin import biased_prefix_beam_search
from hotword_twin import TwinGraph
from test_ctc_prefix_bias_gpu import run_op as run_biased
from test_ctc_prefix_gpu import run_op
from test_ctc_prefix_stream_gpu import against_twin, stream_rows

pytestmark = pytest.mark.gpu

REL = 1e-5
KEYS = ("tokens", "timestamps", "token_log_probs", "n_tokens", "n_hyps", "scores")
FAMILIES = [("mirrored", V) for V in tc.MIRRORED_VS] + [("dyadic", V) for V in tc.DYADIC_VS]


@pytest.fixture(scope="module")
def hip_ctc(tmp_path_factory):
    from k2transducerasr_amd import Model
    from k2transducerasr_amd.synth import write_synthetic_model
    p = str(tmp_path_factory.mktemp("ctcprefixties") / "ctc_tiny.k2w")
    write_synthetic_model(p, "zipformer2-ctc-tiny-test")
    m = Model(p, 0)
    assert m.vocab_size == 37
    return m


def check_row(out, r, lp_row, want, family):
    """row r of a kernel result against the twin: everything exact; the score within REL (mirrored) or bit-equal (dyadic).  Returns the
    worst relative score difference."""
    hyps = want["hyps"]
    nbest = out["scores"].shape[1]
    assert out["n_hyps"][r] == len(hyps), (r, out["n_hyps"][r], len(hyps))
    worst = 0.0
    for i in range(nbest):
        if i >= len(hyps):
            assert out["n_tokens"][r, i] == -7 and out["scores"][r, i] == -7 and np.all(out["tokens"][r, i] == -7), (r, i)
            continue
        h = hyps[i]
        n = len(h["tokens"])
        assert out["n_tokens"][r, i] == n, (r, i, out["n_tokens"][r, i], n)
        assert out["tokens"][r, i, :n].tolist() == h["tokens"], (r, i, out["tokens"][r, i, :n].tolist(), h["tokens"])
        assert out["timestamps"][r, i, :n].tolist() == h["timestamps"], (r, i, out["timestamps"][r, i, :n].tolist(), h["timestamps"])
        assert np.array_equal(out["token_log_probs"][r, i, :n], np.asarray([lp_row[t, v] for t, v in zip(h["timestamps"], h["tokens"])], np.float32)), (r, i)
        assert np.all(out["tokens"][r, i, n:] == -7) and np.all(out["timestamps"][r, i, n:] == -7) and np.all(out["token_log_probs"][r, i, n:] == -7)
        got = float(out["scores"][r, i])
        if family == "dyadic":
            assert got == h["score"], (r, i, got, h["score"])
        else:
            d = abs(got - h["score"]) / max(1.0, abs(h["score"]))
            worst = max(worst, d)
            assert d <= REL, (r, i, got, h["score"])
    return worst


def same(a, b, what):
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


# ---- 1. the offline kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,V", FAMILIES)
def test_offline_kernel(hip_ctc, family, V):
    """every row, beams 1 .. 8, nbest = beam, the rows of a family and V in one call"""
    rows = tc.rows_of(family, V)
    worst = 0.0
    for beam in tc.BEAMS:
        out = run_op(hip_ctc, rows, None, beam, beam, tc.T)
        assert out["flag"] == 0
        for r in range(rows.shape[0]):
            worst = max(worst, check_row(out, r, rows[r], tc.reference(family, V, r, beam)[0], family))
    print(f"{family} V={V}: worst relative score difference {worst:.3g} (bound {REL:g}" + ("; bit-equal required)" if family == "dyadic" else ")"))


# ---- 2. the resumed kernel ---------------------------------------------------------------------------------------------------------------
def cut(pattern, T):
    """chunk lengths following `pattern` until T frames are covered, the last one shortened"""
    out = []
    while sum(out) < T:
        out.append(min(pattern[len(out) % len(pattern)], T - sum(out)))
    return out


@pytest.mark.parametrize("family,V", FAMILIES)
def test_resumed_kernel(hip_ctc, family, V):
    """the same rows as streams of "ctc_prefix_resume": one frame per chunk, 3 / 1 / 5 / 3, and one chunk; with ragged n_frames (12, 9, 5)
    the rows leave the batch early.  stream_rows asserts after EVERY step that each stream equals the offline op over its frames so far
    bit for bit, scores and slot order included -- tied slots crossing a chunk boundary are the point; the whole rows also meet the twin."""
    rows = tc.rows_of(family, V)
    R = rows.shape[0]
    ragged = (12, 9, 5)[:R]
    for beam in tc.BEAMS:
        for pattern, lens, Tc in (((1,), (tc.T,) * R, 1), ((3, 1, 5, 3), (tc.T,) * R, 5), ((3, 1, 5, 3), ragged, 5), ((tc.T,), ragged[::-1], tc.T)):
            carries = stream_rows(hip_ctc, [(rows[r, : lens[r]], cut(pattern, lens[r])) for r in range(R)], beam, Tc)
            for r in range(R):
                if lens[r] == tc.T:
                    against_twin(carries[r], tc.reference(family, V, r, beam)[0], rows[r])


# ---- 3. the biased instantiation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,V", FAMILIES)
def test_biased_instantiation_with_tables_that_cannot_fire(hip_ctc, family, V):
    """k_ctc_prefix<false, true> with null tables, with a graph without phrases, with phrases that earn 0.0 and with an LM of <s> and <unk>
    alone at scale 0.0: the plain op bit for bit on every tie row"""
    rows = tc.rows_of(family, V)
    empty_lm = bc.TwinLm([((-1,), -99.0, 0.0), ((-3,), -7.5, 0.0)], V).scaled(0.0)
    tables = ((None, None), (TwinGraph([], bc.SCORE, V), None), (TwinGraph([[5, 7], [9]], 0.0, V), None), (TwinGraph([], bc.SCORE, V), empty_lm))
    for beam in tc.BEAMS:
        want = run_op(hip_ctc, rows, None, beam, beam, tc.T)
        for i, (graph, lm) in enumerate(tables):
            got = run_biased(hip_ctc, rows, None, beam, beam, tc.T, graph, lm)
            assert got["flag"] == want["flag"] == 0
            same(got, want, (family, V, beam, i))


def test_biased_key_tie(hip_ctc):
    """the dyadic row with the dyadic bonus of ctc_prefix_tie_cases.py: a biased key ties with an unbiased candidate of another slot and
    another acoustic total, in both frames and in the final order.  Exact, scores included."""
    lp = tc.bias_row()
    graph = TwinGraph(tc.BIAS_PHRASES, tc.BIAS_SCORE, tc.BIAS_V)
    for beam in tc.BIAS_BEAMS:
        want = biased_prefix_beam_search(lp.astype(np.float64), beam, graph, None)
        assert [(h["tokens"], h["score"]) for h in want["hyps"]] == tc.BIAS_WANT[beam]
        out = run_biased(hip_ctc, lp[None], None, beam, beam, 2, graph, None)
        assert out["flag"] == 0
        check_row(out, 0, lp, want, "dyadic")


# ---- 4. the public entry -----------------------------------------------------------------------------------------------------------------
def test_public_entry(tmp_path):
    """Model.ctc_prefix_beam_search (k2hip_ctc_prefix_beam_search) of a CTC model with a vocabulary of 65 on the mirrored and the dyadic
    rows of V = 65: the op's result bit for bit"""
    from k2transducerasr_amd import Model
    from k2transducerasr_amd.synth import write_synthetic_model
    p = str(tmp_path / "ctc_v65.k2w")
    write_synthetic_model(p, "zipformer2-ctc-tiny-test", meta_overrides={"vocab_size": "65"})
    m = Model(p, 0)
    try:
        assert m.vocab_size == 65
        for family in ("mirrored", "dyadic"):
            rows = tc.rows_of(family, 65)
            for beam in (1, 3, 8):
                op = run_op(m, rows, None, beam, beam, tc.T)
                got = m.ctc_prefix_beam_search(rows, beam=beam, nbest=beam)
                for r in range(rows.shape[0]):
                    assert len(got[r]) == op["n_hyps"][r]
                    for i, a in enumerate(got[r]):
                        n = op["n_tokens"][r, i]
                        assert a["tokens"] == op["tokens"][r, i, :n].tolist() and a["timestamps"] == op["timestamps"][r, i, :n].tolist(), (family, beam, r, i)
                        assert np.float32(a["score"]).tobytes() == op["scores"][r, i].tobytes(), (family, beam, r, i)
                        assert np.asarray(a["token_log_probs"], np.float32).tobytes() == op["token_log_probs"][r, i, :n].tobytes()
                    check_row(op, r, rows[r], tc.reference(family, 65, r, beam)[0], family)
    finally:
        m.close()


# ---- 5. independence ---------------------------------------------------------------------------------------------------------------------
def test_a_tie_rows_result_does_not_depend_on_the_other_rows(hip_ctc):
    for family, V, beam in (("mirrored", 600, 8), ("mirrored", 65, 3), ("dyadic", 257, 5)):
        rows = tc.rows_of(family, V)
        three = np.stack([rows[1], rows[0], rows[1][::-1]])
        batch = run_op(hip_ctc, three, None, beam, beam, tc.T)
        alone = run_op(hip_ctc, rows[:1], None, beam, beam, tc.T)
        for k in KEYS:
            assert alone[k][0].tobytes() == batch[k][1].tobytes(), (family, V, k)
        check_row(alone, 0, rows[0], tc.reference(family, V, 0, beam)[0], family)
