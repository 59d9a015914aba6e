"""CPU tests of the CTC forced alignment: the float64 twin (tests/ctc_align_twin.py) against brute-force enumeration of every frame
labelling that collapses to the target, the tie rules on hand-built cases, and the host side of the feature (csrc/ctc_lattice_ref.h, the
two ABI entries' argument checks over the engine stand-ins) as its own program under AddressSanitizer / UBSan."""
import os
import subprocess

import numpy as np
import pytest

from ctc_align_twin import all_targets, brute_force, ctc_lattice, min_frames, path_score

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("T", range(1, 7))
def test_twin_equals_brute_force(T):
    """total and best of the twin's recursions = the enumeration of all 3^T labellings, for every T <= 6, V = 3 and every target up to
    length 3 (repeats included) that fits, on random log_probs (every fifth trial with -inf cells); the backtraced path scores `best`
    and timestamps[u] <= end_frames[u] < timestamps[u+1]"""
    rng = np.random.default_rng(200 + T)
    V = 3
    seen = 0
    for y in all_targets(V, 3):
        if min_frames(y) > T:
            continue
        for trial in range(5):
            lp = -rng.random((T, V)) * 6
            if trial == 4:
                lp[rng.random(lp.shape) < 0.2] = -np.inf
            got = ctc_lattice(lp, y)
            total, best = brute_force(lp, y)
            seen += 1
            if best == -np.inf:
                assert got["total"] == -np.inf and got["best"] == -np.inf
                continue
            assert abs(got["total"] - total) <= 1e-12 * max(1.0, abs(total)), (T, y, trial)
            assert abs(got["best"] - best) <= 1e-12 * max(1.0, abs(best)), (T, y, trial)
            assert got["best"] <= got["total"] + 1e-12
            ts, en = got["timestamps"], got["end_frames"]
            assert all(0 <= a <= b < T for a, b in zip(ts, en)) and all(b < a for b, a in zip(en, ts[1:])), (T, y, ts, en)
            assert abs(path_score(lp, y, ts, en) - best) <= 1e-12 * max(1.0, abs(best))
            assert np.array_equal(got["token_log_probs"], [lp[ts[u], y[u]] for u in range(len(y))])
            if not y:
                assert abs(got["total"] - lp[:, 0].sum()) <= 1e-12 * T * 6 and got["best"] == got["total"]
    assert seen >= 5


def test_twin_sums_to_one_over_all_label_sequences():
    """for one random log-softmaxed lp with T = 4, V = 3: sum over every label sequence of length <= T of exp(total) = 1"""
    rng = np.random.default_rng(7)
    T, V = 4, 3
    x = rng.standard_normal((T, V)) * 2
    lp = x - np.log(np.exp(x).sum(axis=1, keepdims=True))
    mass = sum(np.exp(ctc_lattice(lp, y)["total"]) for y in all_targets(V, T) if min_frames(y) <= T)
    assert abs(mass - 1.0) <= 1e-12, mass


def test_twin_tie_rules():
    """hand-built cases on multiples of 0.25 (columns: blank, a, b)"""
    inf = np.inf
    # s-2 against s-1: y = a b, T = 3.  Into b's state at frame 2 the paths (a a b) and (a - b) tie at -0.5: s-2 wins, a lasts through frame 1
    got = ctc_lattice([[-4, 0, -4], [-0.5, -0.5, -1], [-4, -4, 0]], [1, 2])
    assert got["best"] == -0.5 and got["timestamps"] == [0, 2] and got["end_frames"] == [1, 2] and got["states"] == [1, 1, 3]
    # s-1 against s: y = a, T = 2.  Into a's state at frame 1 (blank a) and (a a) tie at -0.75: s-1 wins, a starts at frame 1
    got = ctc_lattice([[-0.25, -0.25, -4], [-4, -0.5, -4]], [1])
    assert got["best"] == -0.75 and got["timestamps"] == [1] and got["end_frames"] == [1] and got["token_log_probs"][0] == -0.5
    # the end: y = a, T = 2.  (a a) ends in S-2, (a -) in S-1, both -0.5: S-2 wins; (- a) is blocked, so total = -0.5 + log 2
    got = ctc_lattice([[-inf, -0.25, -4], [-0.25, -0.25, -4]], [1])
    assert got["best"] == -0.5 and got["timestamps"] == [0] and got["end_frames"] == [1] and got["states"] == [1, 1]
    assert abs(got["total"] - (-0.5 + np.log(2.0))) < 1e-15
    # a repeated token needs its blank: y = a a, T = 3 has the single path a - a
    got = ctc_lattice([[-1, -0.25, -4], [-0.5, 0, -4], [-1, -0.25, -4]], [1, 1])
    assert got["states"] == [1, 2, 3] and got["best"] == got["total"] == -1.0


def test_host_side_under_the_sanitizers(tiny_model_path, tmp_path):
    """tests/native/san_ctc_align_driver.cpp (make san_ctc_align): ctc_lattice_ref.h against brute force (U = 0, T = 1, targets that need
    exactly T frames because of repeats, -inf cells) and the tie rules; k2hip_ctc_align / k2hip_offline_ctc_align_from_samples argument
    checks over the CPU stand-in of the engine -- blank and out-of-range ids, a target one frame too long, a bad stream_of, a bad
    n_frames, lens > max_tokens with nothing written, a transducer model, NULL outputs, a valid call after every refused one.  Its own
    program, built with ASan / UBSan."""
    from k2transducerasr_amd.synth import write_synthetic_model
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "k2transducerasr_amd", "csrc"), "-s", "san_ctc_align"])
    ctc = str(tmp_path / "ctc.k2w")
    write_synthetic_model(ctc, "zipformer2-ctc-tiny-test")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "native", "k2hip_san_ctc_align_driver"), ctc, tiny_model_path], capture_output=True, text=True,
                       env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "san_ctc_align_driver ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


def test_python_surface_exists():
    from k2transducerasr_amd import Model, OfflineRecognizer
    assert callable(Model.ctc_align) and callable(Model.ctc_align_samples) and callable(OfflineRecognizer.align)
