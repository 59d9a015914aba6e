"""CPU tests of the CTC keyword spotter: the float64 twin (tests/ctc_kws_twin.py) against an explicit enumeration of frame labellings, the
hand-built cases against their written-down answers, the float32 host reference (csrc/ctc_kws_ref.h, through k2hip_debug_ctc_kws_ref_dp)
against the twin, the decision gaps of the end-to-end fixture from the twin alone, and the host side of the feature as its own program
under AddressSanitizer / UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ctc_kws_cases import HOST_S, HOST_T, KEYWORDS, THRESHOLDS, hand_cases, host_cases, tables
from ctc_kws_twin import brute_force_frame, build_trie, fresh_state, root_children, token_passing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The float32 error of a cell of the fixture: a cell is a sum of at most 35 log-probs (one per frame), every partial sum is at most
# MAX_SUM in magnitude, every addition rounds once (2^-24 relative).  Crude: every term is charged the largest magnitude.
FIXTURE_FRAMES, MAX_SUM = 35, 52.0
F32_BOUND = FIXTURE_FRAMES * 2.0 ** -24 * MAX_SUM     # 1.1e-4
MIN_RATIO = 4.0


def ref_dp(case, lp, v=None, st=None):
    """csrc/ctc_kws_ref.h on one stream -> (events, v [2][S], st [2][S])"""
    from k2transducerasr_amd import load_library
    L = load_library()
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    L.k2hip_debug_ctc_kws_ref_dp.argtypes = [ip, ip, ip, ip, fp, ip, C.c_int32, fp, C.c_int32, C.c_int32, fp, ip, ip, ip, ip, fp, C.c_int32, ip]
    S, (T, V) = len(case["parent"]), lp.shape
    if v is None:
        v64, s64 = fresh_state(S)
        v, st = v64.astype(np.float32), s64.astype(np.int32)
    v, st = np.ascontiguousarray(v, dtype=np.float32).copy(), np.ascontiguousarray(st, dtype=np.int32).copy()
    lp = np.ascontiguousarray(lp, dtype=np.float32)
    cap = max(T, 1)
    ek, es, ee = (np.zeros(cap, np.int32) for _ in range(3))
    em = np.zeros(cap, np.float32)
    n = C.c_int32(0)
    p = lambda x, t: x.ctypes.data_as(t)
    rc = L.k2hip_debug_ctc_kws_ref_dp(p(case["parent"], ip), p(case["tok"], ip), p(case["depth"], ip), p(case["kw"], ip), p(case["bar"], fp),
                                      p(case["rc"], ip), S, p(lp, fp), V, T, p(v, fp), p(st, ip), p(ek, ip), p(es, ip), p(ee, ip), p(em, fp), cap,
                                      C.byref(n))
    assert rc == 0, L.k2hip_last_error()
    return [(int(ek[i]), int(es[i]), int(ee[i]), float(em[i])) for i in range(n.value)], v, st


def trie_of(case):
    return dict(parent=case["parent"], tok=case["tok"], depth=case["depth"], kw=case["kw"], bar=case["bar"].astype(np.float64))


def start_block(case, b):
    blk = case.get("blocks", [None] * len(case["streams"]))[b]
    return (None, None) if blk is None else blk


@pytest.mark.parametrize("T", range(1, 7))
def test_twin_equals_brute_force(T):
    """the twin's n[c] and b[c] after every frame = the maximum over explicitly enumerated frame labellings (from a start frame over the
    symbols {path tokens, blank}, collapsing to path(c), ending on the token or on a blank), on tiny tries with -inf cells: values, the
    entered flag under ties, the start frames, the events, the reset and the hold.  The tries include a keyword with an adjacent repeated
    token and one that is a proper prefix of another."""
    rng = np.random.default_rng(700 + T)
    tries = [([[1]], 0.5), ([[1, 3]], 0.4), ([[1, 1]], 0.4), ([[1], [1, 3], [3], [3, 1]], 0.45), ([[1, 3, 3]], 0.5), ([[3, 1, 3], [3, 1]], 0.5)]
    fired = 0
    for words, th in tries:
        trie = build_trie(words, th)
        trie["bar"] = np.round(trie["bar"] * 4) / 4     # multiples of 0.25: n == bar happens
        rc = root_children(trie)
        S = len(trie["parent"])
        for trial in range(4):
            lp = -0.25 * rng.integers(0, 6, size=(T, 5)).astype(np.float64)
            if trial >= 2:
                lp[rng.random(lp.shape) < 0.2] = -np.inf
            v, st = fresh_state(S)
            R, hold, closed = -1, -1, []
            for t in range(T):
                # the hold, restated: which root arc is closed at frame t
                if hold >= 0 and not lp[t, trie["tok"][hold]] >= lp[t, 0]:
                    hold = -1
                closed.append(hold)
                ev, v, st = token_passing(trie, lp[t: t + 1], v, st)
                want = brute_force_frame(trie, lp, t, R, closed)
                cand = [c for c, w in want.items() if trie["kw"][c] >= 0 and w[1] and w[0] >= trie["bar"][c]]
                if cand:
                    win = min(cand, key=lambda c: (-trie["depth"][c], -want[c][0], trie["kw"][c]))
                    assert len(ev) == 1 and ev[0][0] == trie["kw"][win] and ev[0][2] == t and ev[0][3] == want[win][0], (words, trial, t)
                    assert ev[0][1] in want[win][2]
                    assert np.all(v[:, 1:] == -np.inf) and np.all(st[:, 1:] == -1)
                    R, hold = t, int(rc[win])
                    fired += 1
                else:
                    assert ev == [], (words, trial, t, ev)
                    for c, (n, _, sn, b, sb) in want.items():
                        assert v[0, c] == n and v[1, c] == b, (words, trial, t, c, v[:, c], n, b)
                        assert (st[0, c] in sn) if n > -np.inf else st[0, c] == -1
                        assert (st[1, c] in sb) if b > -np.inf else st[1, c] == -1
                assert st[0, 0] == t + 1 and v[0, 0] == 0 and st[1, 0] == hold and v[1, 0] == -np.inf
    assert fired > 0


def test_hand_built_cases():
    """every tie (the three-way tie for n, the tie for b), n == bar exactly, two and three terminals in one frame (depth, then value, then
    keyword index), the reset after an event, the hold (a one-token keyword over a three-frame run fires once; released by a blank frame,
    then a second event; both log-probs -inf; after a longer keyword), rc = -1, a repeated token that must pass through b: the twin and
    the host reference both give the written-down events and cells"""
    for case in hand_cases():
        trie = trie_of(case)
        for b, lp in enumerate(case["streams"]):
            v0, s0 = start_block(case, b)
            tev, tv, ts = token_passing(trie, lp, None if v0 is None else v0.astype(np.float64), None if s0 is None else s0.astype(np.int64))
            rev, rv, rs = ref_dp(case, lp, v0, s0)
            for who, ev, v, st in (("twin", tev, tv, ts), ("ref", rev, rv, rs)):
                assert ev == case["expect"][b], (case["name"], b, who, ev)
                for (pl, c), (x, s) in case.get("states", [{}] * (b + 1))[b].items():
                    assert v[pl, c] == x and st[pl, c] == s, (case["name"], b, who, pl, c, v[pl, c], st[pl, c])


def test_host_reference_against_the_twin():
    """csrc/ctc_kws_ref.h (float32) = the twin (float64) on planes of multiples of 0.25 with -inf cells, where both are exact: events, sums
    and carried blocks exactly equal, S in {1, 2, 65, 257, 1024} x T in {1, 2, 17, 64}; any chunking gives one call's result"""
    rng = np.random.default_rng(11)
    cases = host_cases()
    assert {(len(c["parent"]), c["streams"][0].shape[0]) for c in cases} == {(S, T) for S in HOST_S for T in HOST_T}
    n_events = n_held = 0
    for case in cases + hand_cases():
        trie = trie_of(case)
        for b, lp in enumerate(case["streams"]):
            v0, s0 = start_block(case, b)
            ev, v, st = ref_dp(case, lp, v0, s0)
            trace = []
            tev, tv, ts = token_passing(trie, lp, None if v0 is None else v0.astype(np.float64), None if s0 is None else s0.astype(np.int64),
                                        trace=trace)
            assert ev == tev, (case["name"], b, ev[:3], tev[:3])
            assert np.array_equal(v, tv.astype(np.float32)) and st.tolist() == ts.tolist(), (case["name"], b)
            n_events += len(ev)
            n_held += sum(1 for r in trace if r >= 0)
            T = lp.shape[0]
            cv, cs, cev, t = v0, s0, [], 0
            while t < T:
                n = min(T - t, int(rng.integers(1, 6)))
                e2, cv, cs = ref_dp(case, lp[t: t + n], cv, cs)
                cev += e2
                t += n
            assert cev == ev and cv.tobytes() == v.tobytes() and cs.tobytes() == st.tobytes(), (case["name"], b)
    assert n_events > 100 and n_held > 20   # the random cases do fire, and the hold does close arcs


@pytest.fixture(scope="module")
def oracle_log_probs(tmp_path_factory, utts):
    """the oracle's log-probs of the `utts` fixture on zipformer2-ctc-tiny-test"""
    from k2transducerasr_amd.synth import write_synthetic_model
    from oracle import Oracle
    p = str(tmp_path_factory.mktemp("ctckws") / "ctc_tiny.k2w")
    write_synthetic_model(p, "zipformer2-ctc-tiny-test")
    ora = Oracle(p)
    f = [ora.fbank(u) for u in utts]
    return np.asarray(ora.encoder(ora.pad_sequence(f).reshape(len(utts), -1, 80)), np.float32)


def fixture_run(lp, hold_rule=True):
    """the twin over a [B][T][V] batch with the fixture's keywords -> (events per stream, gaps, frames closed by the hold, largest |cell|)"""
    trie = build_trie(KEYWORDS, THRESHOLDS)
    trie["bar"] = tables(trie)["bar"].astype(np.float64)   # the float32 bars the engine compares with
    events, gaps, held, top = [], [], 0, 0.0
    for b in range(lp.shape[0]):
        v, st = fresh_state(len(trie["parent"]))
        trace, evs = [], []
        for t in range(lp.shape[1]):
            ev, v, st = token_passing(trie, lp[b, t: t + 1], v, st, hold_rule=hold_rule, gaps=gaps, trace=trace)
            evs += ev
            top = max(top, float(np.abs(v[np.isfinite(v)]).max()))
        events.append(evs)
        held += sum(1 for r in trace if r >= 0)
    return events, gaps, held, top


def test_fixture_decisions_clear_their_error_bounds(oracle_log_probs):
    """the end-to-end input of tests/test_ctc_kws_gpu.py, from the twin alone: EVERY comparison between finite values that the recursion
    makes on this input -- predecessor choices, the b choice, threshold tests of entered terminals, choices among candidates, hold tests
    -- has a gap of at least MIN_RATIO = 4 times F32_BOUND = 35 additions x 2^-24 x 52 = 1.1e-4, the float32 error of a cell, so float32
    arithmetic on the same log-probs takes the same decisions.  (Exact ties between -inf cells are decided by rule, not by rounding.)
    Measured on the oracle's log-probs: 32 events (6 of two tokens, 26 of three), the hold closes the root arc on 25 frames, 43 events
    with the hold rule off, smallest gap 1.44e-3 = 13 x the bound.  No winning path on this random model uses a self loop or a blank
    cell (end - start + 1 is the keyword's length for every event); those are covered by the plane cases."""
    lp = oracle_log_probs
    assert lp.shape == (5, 35, 37)
    events, gaps, held, top = fixture_run(lp)
    flat = [e for evs in events for e in evs]
    no_hold = [e for evs in fixture_run(lp, hold_rule=False)[0] for e in evs]
    by_len = {n: sum(1 for e in flat if len(KEYWORDS[e[0]]) == n) for n in (1, 2, 3)}
    print(f"{len(flat)} events {by_len}, {held} frames closed by the hold, {len(no_hold)} events without the hold rule, "
          f"{len(gaps)} comparisons, smallest gap {min(gaps):.3g} = {min(gaps) / F32_BOUND:.1f} x {F32_BOUND:.3g}, largest |cell| {top:.1f}")
    assert top <= MAX_SUM
    assert len(flat) == 32 and by_len == {1: 0, 2: 6, 3: 26}
    assert held == 25
    assert len(no_hold) == 43 and no_hold != flat
    assert all(e[2] - e[1] + 1 == len(KEYWORDS[e[0]]) for e in flat)
    assert min(gaps) >= MIN_RATIO * F32_BOUND


def test_host_side_under_the_sanitizers(tiny_model_path, tmp_path):
    """tests/native/san_ctc_kws_driver.cpp (make san_ctc_kws): ctc_kws_ref.h against an explicit enumeration of alignments, every refusal
    of the new entries followed by a valid call, the streams' life cycle (the graph destroyed before its stream) and the fused entry's
    capacity rule over the CPU stand-in of the engine.  Its own program, built with ASan / UBSan."""
    from k2transducerasr_amd.synth import write_synthetic_model
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "k2transducerasr_amd", "csrc"), "-s", "san_ctc_kws"])
    ctc = str(tmp_path / "ctc.k2w")
    write_synthetic_model(ctc, "zipformer2-ctc-tiny-test")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "native", "k2hip_san_ctc_kws_driver"), ctc, tiny_model_path], capture_output=True, text=True,
                       env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "san_ctc_kws_driver ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


def test_python_surface_exists():
    import k2transducerasr_amd as k
    assert callable(k.Model.ctc_spot_keywords) and callable(k.Model.ctc_spot_keywords_samples) and callable(k.OfflineRecognizer.spot_keywords)
    assert all(callable(getattr(k.CtcKeywordStream, m)) for m in ("search_chunk", "events", "reset", "num_frames", "state", "close"))
    assert "CtcKeywordStream" in k.__all__
