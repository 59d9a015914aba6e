"""CPU tests of the CTC prefix beam search: the numpy twin (tests/ctc_prefix_twin.py) against brute-force enumeration of every frame
labelling and against the alignment twin, the tie rules, `a a`, the re-spelled prefix, the inputs of the GPU tests (their gaps against
G, see tests/ctc_prefix_cases.py), and the host side of the feature (csrc/ctc_prefix_ref.h, the ABI entries' argument checks over the
engine stand-ins) as its own program under AddressSanitizer / UBSan."""
import os
import subprocess

import numpy as np
import pytest

import ctc_prefix_cases as cases
from ctc_align_twin import ctc_lattice
from ctc_prefix_twin import brute_force, min_gap, prefix_beam_search, seeded_log_probs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def close(got, want, tol=1e-12):
    if want == -np.inf:
        return got == -np.inf
    return abs(got - want) <= tol * max(1.0, abs(want))


@pytest.mark.parametrize("T", range(1, 7))
def test_twin_equals_brute_force(T):
    """V = 3, nothing pruned: the survivors are exactly the prefixes with a finite full sum, in score order, and every score, pb and pnb
    is the sum over all 3^T labellings (within 1e-12); every fifth trial has -inf cells"""
    rng = np.random.default_rng(300 + T)
    for trial in range(5):
        lp = -rng.random((T, 3)) * 6
        if trial == 4:
            lp[rng.random(lp.shape) < 0.25] = -np.inf
        got = prefix_beam_search(lp, 1000)
        want = {k: v for k, v in brute_force(lp).items() if v[0] > -np.inf}
        if not want:
            assert len(got["hyps"]) == 1 and got["hyps"][0]["score"] == -np.inf
            continue
        assert sorted(tuple(h["tokens"]) for h in got["hyps"]) == sorted(want), (T, trial)
        assert got["respelled_folds"] == 0
        for h in got["hyps"]:
            tot, pb, pnb = want[tuple(h["tokens"])]
            assert close(h["score"], tot) and close(h["pb"], pb) and close(h["pnb"], pnb), (T, trial, h, want[tuple(h["tokens"])])
            ts = h["timestamps"]
            assert all(0 <= a < T for a in ts) and all(a < b for a, b in zip(ts, ts[1:]))
            assert np.array_equal(h["token_log_probs"], [lp[t, v] for t, v in zip(ts, h["tokens"])])
        assert all(a["score"] >= b["score"] for a, b in zip(got["hyps"], got["hyps"][1:]))


def test_pruned_scores_never_exceed_the_alignment_twins_total():
    """with a beam that prunes, a hypothesis' score is a sum over SOME of its paths: <= tests/ctc_align_twin.py's total for the same
    tokens; with nothing pruned the two are equal"""
    for seed, T, V, beam in [(1, 12, 5, 3), (2, 20, 6, 4), (3, 9, 4, 8), (4, 6, 3, 1000)]:
        lp = seeded_log_probs(seed, T, V).astype(np.float64)
        for h in prefix_beam_search(lp, beam)["hyps"]:
            total = ctc_lattice(lp, h["tokens"])["total"]
            assert h["score"] <= total + 1e-12 * max(1.0, abs(total)), (seed, h["tokens"], h["score"], total)
            if beam == 1000:
                assert close(h["score"], total)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_tie_rules_on_hand_built_rows(dtype):
    lp, beam = cases.TIE_LOWER_ID               # equal tokens: the lower id wins
    got = prefix_beam_search(lp, beam, dtype)
    assert [h["tokens"] for h in got["hyps"]] == [[1], [2]] and got["hyps"][0]["score"] == got["hyps"][1]["score"] == -0.5
    lp, beam = cases.TIE_STAY                   # stay against extension: stay wins
    got = prefix_beam_search(lp, beam, dtype)
    assert [h["tokens"] for h in got["hyps"]] == [[]] and got["hyps"][0]["score"] == -0.5
    lp, beam = cases.TIE_LOWER_SLOT             # equal candidates of two slots: the lower slot wins
    got = prefix_beam_search(lp, beam, dtype)
    assert got["picks"][0] == [0, 1] and got["picks"][1] == [2, 3 + 2]
    assert [h["tokens"] for h in got["hyps"]] == [[2], [1, 2]] and got["hyps"][0]["score"] == got["hyps"][1]["score"] == -1.25
    assert [h["timestamps"] for h in got["hyps"]] == [[1], [0, 1]]


def test_a_a():
    got = prefix_beam_search(cases.PEAKY_A_BLANK_A, 4)["hyps"][0]
    assert got["tokens"] == [1, 1] and got["timestamps"] == [0, 2]
    got = prefix_beam_search(cases.PEAKY_A_A_A, 4)["hyps"][0]
    assert got["tokens"] == [1] and got["timestamps"] == [0] and got["token_log_probs"][0] == 0.0


def test_respelled_prefix_folds_into_the_old_descendant():
    """the committed seeded input (V = 3, T = 10, beam 4): the twin counts a fold into a slot whose history parent is NOT the folded
    slot's node -- a parent_node == node check would miss it -- and the N-best stays pairwise distinct; so does every frame's beam on a
    sweep of small inputs"""
    got = prefix_beam_search(cases.respelled_row(), cases.RESPELLED_BEAM)
    assert got["respelled_folds"] >= 1
    toks = [tuple(h["tokens"]) for h in got["hyps"]]
    assert len(set(toks)) == len(toks) == cases.RESPELLED_BEAM
    found = 0
    for seed in range(40):
        r = prefix_beam_search(seeded_log_probs(seed, 10, 3, 2.0), 4)
        found += r["respelled_folds"]
        toks = [tuple(h["tokens"]) for h in r["hyps"]]
        assert len(set(toks)) == len(toks), seed
    assert found >= 2


def measured_e(lp, beam):
    """the worst difference between the float32 and the float64 twin's gaps while their selections agree, and the float64 run"""
    a, b = prefix_beam_search(lp, beam, np.float64), prefix_beam_search(lp, beam, np.float32)
    e = 0.0
    for t, (pa, pb) in enumerate(zip(a["picks"], b["picks"])):
        if pa != pb:
            return e, a, False
        if np.isfinite(a["cut_gaps"][t]) and np.isfinite(b["cut_gaps"][t]):
            e = max(e, abs(a["cut_gaps"][t] - b["cut_gaps"][t]))
    for ga, gb in zip(a["rank_gaps"], b["rank_gaps"]):
        e = max(e, abs(ga - gb))
    return e, a, True


def test_inputs_of_the_gpu_tests_clear_their_gap():
    """every seeded case the GPU tests assert exactly: 8 E <= G with E re-measured here, and every gap of the float64 twin >= G"""
    for name, lp, beams, G in cases.strict_cases():
        for beam in beams:
            e, run, agree = measured_e(lp, beam)
            print(f"{name} beam {beam}: E {e:.3g}, smallest gap {min_gap(run):.3g}, G {G:.3g}")
            assert agree and 8 * e <= G <= min_gap(run), (name, beam, e, min_gap(run), G)
    ex, _ = cases.exhaustive_rows()
    assert len(prefix_beam_search(ex[1], 8)["hyps"]) == 5 and len(prefix_beam_search(ex[0, :1], 8)["hyps"]) == 3
    assert prefix_beam_search(cases.respelled_row(), cases.RESPELLED_BEAM)["respelled_folds"] >= 1


def test_fixture_utterances_stay_within_the_cap(tmp_path, utts):
    """the end-to-end GPU test leaves out streams whose smallest twin gap is below G_FIXTURE, at most one in four: with the oracle's
    log_probs of the fixture batch none is; E of the table in ctc_prefix_cases.py is re-measured"""
    from k2transducerasr_amd.synth import write_synthetic_model
    from oracle import Oracle
    p = str(tmp_path / "ctc.k2w")
    write_synthetic_model(p, "zipformer2-ctc-tiny-test")
    o = Oracle(p)
    lp = o.encoder(o.pad_sequence([o.fbank(u) for u in utts]).reshape(len(utts), -1, 80)).astype(np.float32)
    out = 0
    for b in range(len(utts)):
        e, run, agree = measured_e(lp[b], 4)
        print(f"stream {b}: E {e:.3g}, smallest gap {min_gap(run):.3g}")
        assert 8 * e <= cases.G_FIXTURE
        out += not (agree and min_gap(run) >= cases.G_FIXTURE)
    assert 4 * out <= len(utts), out


def test_host_side_under_the_sanitizers(tiny_model_path, tmp_path):
    """tests/native/san_ctc_prefix_driver.cpp (make san_ctc_prefix): ctc_prefix_ref.h against brute force with nothing pruned, the tie and
    fold rules, a re-spelled prefix, and the argument checks of k2hip_ctc_prefix_beam_search / k2hip_set_decoding_method /
    k2hip_set_nbest over the CPU stand-in of the engine, a transducer handle refusing both entries.  Its own program, built with ASan /
    UBSan."""
    from k2transducerasr_amd.synth import write_synthetic_model
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "k2transducerasr_amd", "csrc"), "-s", "san_ctc_prefix"])
    ctc = str(tmp_path / "ctc.k2w")
    write_synthetic_model(ctc, "zipformer2-ctc-tiny-test")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "native", "k2hip_san_ctc_prefix_driver"), ctc, tiny_model_path], capture_output=True, text=True,
                       env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "san_ctc_prefix_driver ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


def test_surface_exists():
    import inspect

    from k2transducerasr_amd import Model, OfflineRecognizer, load_library
    sig = inspect.signature(Model.ctc_prefix_beam_search)
    assert [p for p in sig.parameters][:7] == ["self", "log_probs", "beam", "n_frames", "nbest", "want_scores", "want_token_log_probs"]
    assert sig.parameters["beam"].default == 4
    assert callable(Model.set_decoding_method) and "nbest" in inspect.signature(OfflineRecognizer.__init__).parameters
    assert hasattr(load_library(), "k2hip_ctc_prefix_beam_search")
    with open(os.path.join(ROOT, "include", "k2hip.h")) as f:
        text = f.read()
    assert "k2hip_ctc_prefix_beam_search" in text and "PREFIX IDENTITY IS SEQUENCE IDENTITY" in text
