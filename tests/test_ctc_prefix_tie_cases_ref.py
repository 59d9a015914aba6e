"""Host-side checks of tests/ctc_prefix_tie_cases.py, the inputs tests/test_ctc_prefix_ties_gpu.py puts through the CTC prefix beam
search: the acceptance rule and the coverage on every committed row at every beam 1 .. 8, the float32 twin against the float64 one
(picks, tokens, timestamps, order; E re-measured against the recorded G), csrc/ctc_prefix_ref.h -- the C text of the tie and fold rule
-- run on these rows as its own program, and the sensitivity of the cases: every deliberately wrong variant of the search
(ctc_prefix_twin.RULES) is told from the reference, so each of these mistakes in a kernel would fail the device test."""
import os
import subprocess

import numpy as np
import pytest

import ctc_prefix_tie_cases as tc
from ctc_prefix_bias_twin import biased_prefix_beam_search
from ctc_prefix_twin import RULES, prefix_beam_search
from hotword_twin import TwinGraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-5          # the score bound of tests/test_ctc_prefix_gpu.py
FAMILIES = [("mirrored", V) for V in tc.MIRRORED_VS] + [("dyadic", V) for V in tc.DYADIC_VS]
# what a family can tell apart: the dyadic one has neither folds nor a stay beside an extension, and V = 2 has one candidate per frame
DYADIC_RULES = ("higher_index", "column_before_slot", "thread_keeps_later", "thread_list_short", "final_last_first")


def different(got, ref):
    """tokens, timestamps or order differ, or a score by more than the device test's bound"""
    if [(h["tokens"], h["timestamps"]) for h in got["hyps"]] != [(h["tokens"], h["timestamps"]) for h in ref["hyps"]]:
        return True
    return any(abs(a["score"] - b["score"]) > REL * max(1.0, abs(b["score"])) for a, b in zip(got["hyps"], ref["hyps"]))


@pytest.mark.parametrize("family,V", FAMILIES)
def test_acceptance_coverage_and_the_float32_twin(family, V):
    """every committed row passes check_case at every beam 1 .. 8 with the recorded G; coverage() raises nowhere; the float32 twin's
    picks, tokens, timestamps and order are the float64 twin's; 8 E re-measured is at most G; the dyadic scores are EQUAL; the
    committed seed is the first one accepted"""
    rows, G = tc.rows_of(family, V), tc.g_of(family, V)
    assert rows.shape[0] <= 3 and rows.shape[1] == tc.T == 12 and rows.dtype == np.float32
    worst_e, worst_fin, gap = 0.0, 0.0, np.inf
    for r in range(rows.shape[0]):
        for beam in tc.BEAMS:
            run, F = tc.reference(family, V, r, beam)
            why = tc.check_run(run, F, G)
            assert why is None, (family, V, r, beam, why)
            e, same, fin = tc.measured_e(rows[r], beam)
            assert same, (family, V, r, beam)
            worst_e, worst_fin, gap = max(worst_e, e), max(worst_fin, fin), min(gap, tc.smallest_non_tie_gap(run))
    print(f"{family} V={V}: E {worst_e:.3g}, G {G:.3g}, smallest gap that is no tie {gap:.3g}, float32 against float64 final scores {worst_fin:.3g}")
    assert 8 * worst_e <= G < gap
    if family == "dyadic":
        assert worst_e == 0 and worst_fin == 0 and gap >= 0.125
        fin = rows[np.isfinite(rows)]
        assert np.all(fin * 8 == np.round(fin * 8)) and fin.min() >= -3 and fin.max() <= 0
    for beam in tc.BEAMS:
        c = tc.coverage(family, V, beam)
        print(f"  beam {beam}: " + " ".join(f"{k}={v}" for k, v in c.items() if v))
    assert tc.find_seed(family, V) == (tc.MIRRORED_SEEDS if family == "mirrored" else tc.DYADIC_SEEDS)[V]


def test_the_rows_are_what_the_docstring_says():
    for V in tc.MIRRORED_VS:
        rows = tc.rows_of("mirrored", V)
        groups = tc.groups_of(V)
        assert all(b < V for g in groups for b in g) and {g for g in groups if g in tc.SEAMS} == {s for s in tc.SEAMS if s[1] < V}
        assert ((5, 261, 517) in groups) == (V > 517) and ((100, 300) in groups) == (V > 300) and (17, 18) in groups
        assert any(V - 1 in g for g in groups)
        for g in groups:                                            # duplicates: equal in EVERY frame of every row
            assert all(np.array_equal(rows[:, :, g[0]], rows[:, :, c]) for c in g[1:]), g
        assert np.array_equal(rows[:, 0], rows[:, 1]) and np.all(rows[1, 0] == tc.FLOOR)
        assert np.all(rows[2, 0, list(tc.LEVEL_GROUP)] == rows[2, 0, 0]) and rows[2, 0, 0] > tc.FLOOR
        assert np.all(rows >= tc.FLOOR) and np.all(rows[rows > tc.FLOOR] >= -5) and rows.max() <= np.float32(-0.3)
        assert (rows == tc.FLOOR).mean() > 0.8                      # most columns sit on the floor
        for t in range(2, tc.T):                                    # the designated group is the frame's top
            for r in range(3):
                top = np.flatnonzero(rows[r, t] == rows[r, t].max())
                assert tuple(top) in groups + [(40,)] and rows[r, t].max() >= np.float32(-0.8) and np.sort(rows[r, t])[-len(top) - 1] <= -2
    # the floor alone: the stay, then v = 1, 2, ... by flat index
    for V in tc.MIRRORED_VS:
        assert tc.reference("mirrored", V, 1, 8)[0]["picks"][0] == list(range(8))
    for V in tc.DYADIC_VS:
        rows = tc.rows_of("dyadic", V)
        assert np.all(rows[:, 0::2, 0] == -np.inf) and np.all(rows[:, 1::2, 1:] == -np.inf) and np.all(np.isfinite(rows[:, 1::2, 0]))
        for r in range(rows.shape[0]):
            run = tc.reference("dyadic", V, r, 8)[0]
            assert not any(fr["folds"] for fr in run["frames"])     # no folds in this family
            cut_ties = sum(len(fr["tot"]) > fr["n_sel"] and fr["tot"][fr["n_sel"] - 1] == fr["tot"][fr["n_sel"]] for fr in run["frames"])
            assert V == 2 or cut_ties >= 3, (V, r, cut_ties)


@pytest.mark.parametrize("family,V", FAMILIES)
def test_the_c_reference_on_the_tie_rows(family, V, tmp_path):
    """csrc/ctc_prefix_ref.h through `san_ctc_prefix_driver row <file>` (make san_ctc_prefix: its own program under AddressSanitizer /
    UBSan, nothing preloaded): every frame's picks, the tokens, timestamps, order and token log-probs equal the float64 twin's; the
    scores are within the device test's bound, and bit-equal on the dyadic family"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "k2transducerasr_amd", "csrc"), "-s", "san_ctc_prefix"])
    exe = os.path.join(ROOT, "tests", "native", "k2hip_san_ctc_prefix_driver")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    rows = tc.rows_of(family, V)
    worst = 0.0
    for r in range(rows.shape[0]):
        for beam in (1, 2, 3, 5, 8):
            path = str(tmp_path / f"row_{r}_{beam}.bin")
            with open(path, "wb") as f:
                f.write(f"{V} {tc.T} {beam}\n".encode())
                f.write(np.ascontiguousarray(rows[r], np.float32).tobytes())
            p = subprocess.run([exe, "row", path], capture_output=True, text=True, env=env, timeout=120)
            assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-3000:]
            assert p.returncode == 0 and "san_ctc_prefix_driver row ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
            ref = tc.reference(family, V, r, beam)[0]
            lines = p.stdout.splitlines()
            picks = [[int(x) for x in ln.split()[2:]] for ln in lines if ln.startswith("picks ")]
            assert picks == ref["picks"], (family, V, r, beam, next(t for t in range(tc.T) if picks[t] != ref["picks"][t]))
            hyps = [ln for ln in lines if ln.startswith("hyp ")]
            assert len(hyps) == len(ref["hyps"])
            for ln, h in zip(hyps, ref["hyps"]):
                head, ts, yp = ln.split("|")
                head = head.split()
                score = np.array([int(head[2])], np.uint32).view(np.float32)[0]
                assert [int(x) for x in head[4:]] == h["tokens"] and int(head[3]) == len(h["tokens"]) and [int(x) for x in ts.split()] == h["timestamps"]
                assert np.array_equal(np.array([int(x) for x in yp.split()], np.uint32).view(np.float32), h["token_log_probs"].astype(np.float32))
                if family == "dyadic":
                    assert float(score) == h["score"], (family, V, r, beam, score, h["score"])
                else:
                    worst = max(worst, abs(float(score) - h["score"]) / max(1.0, abs(h["score"])))
                    assert abs(float(score) - h["score"]) <= REL * max(1.0, abs(h["score"])), (family, V, r, beam, score, h["score"])
    print(f"{family} V={V}: ctc_prefix_ref.h against the float64 twin, worst relative score difference {worst:.3g} (bound {REL:g})")


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("family,V", [(f, V) for f, V in FAMILIES if V > 2])
def test_every_wrong_search_is_told_from_the_reference(family, V, rule):
    """the twin with one rule broken differs from the reference (tokens, timestamps, order, or a score by more than the device test's
    bound) on at least one committed (row, beam) -- at EVERY V of the mirrored family for every rule, and at every V > 2 of the dyadic
    family for the rules it can show (it has no folds and never a stay beside an extension; V = 2 has one candidate per frame)"""
    if family == "dyadic" and rule not in DYADIC_RULES:
        rows = tc.rows_of(family, V)
        for r in range(rows.shape[0]):                              # (and the rule changes nothing there, as said)
            assert not different(prefix_beam_search(rows[r].astype(np.float64), 4, rule=rule), tc.reference(family, V, r, 4)[0])
        return
    rows = tc.rows_of(family, V)
    caught = [(r, beam) for r in range(rows.shape[0]) for beam in tc.BEAMS
              if different(prefix_beam_search(rows[r].astype(np.float64), beam, rule=rule), tc.reference(family, V, r, beam)[0])]
    print(f"{family} V={V} {rule}: told apart by {len(caught)} of {rows.shape[0] * len(tc.BEAMS)} (row, beam) runs")
    assert caught


def test_tracking_changes_nothing():
    """the twin with a Forms table returns what it returns without one"""
    lp = tc.rows_of("mirrored", 65)[0]
    for beam in (1, 4, 8):
        a, b = prefix_beam_search(lp.astype(np.float64), beam), tc.reference("mirrored", 65, 0, beam)[0]
        assert a["picks"] == b["picks"] and a["cut_gaps"] == b["cut_gaps"] and a["rank_gaps"] == b["rank_gaps"]
        assert [(h["tokens"], h["timestamps"], h["score"], h["pb"], h["pnb"]) for h in a["hyps"]] == [
            (h["tokens"], h["timestamps"], h["score"], h["pb"], h["pnb"]) for h in b["hyps"]]


def test_the_biased_key_tie():
    """the hand derivation in ctc_prefix_tie_cases.py against tests/ctc_prefix_bias_twin.py, float64 and float32 alike: exact"""
    lp = tc.bias_row()
    graph = TwinGraph(tc.BIAS_PHRASES, tc.BIAS_SCORE, tc.BIAS_V)
    for beam in tc.BIAS_BEAMS:
        for dt in (np.float64, np.float32):
            got = biased_prefix_beam_search(lp, beam, graph, None, dt)
            assert [(h["tokens"], h["score"]) for h in got["hyps"]] == tc.BIAS_WANT[beam], (beam, dt, got["hyps"])
            assert got["picks"][0][:2] == [3, 4] and got["picks"][1][:2] == [6, tc.BIAS_V + 7]
            assert [h["tot"] for h in got["hyps"]][:2] == [-2.25, -1.75]                 # one key, two acoustic totals
        plain = prefix_beam_search(lp.astype(np.float64), beam)
        assert plain["picks"][0][:2] == [4, 3]                                           # without the phrase the order is the other one
