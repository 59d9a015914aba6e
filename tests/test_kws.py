"""CPU tests of the keyword spotter: the graph builder against a Python restatement and every refusal with its message, the float32 host
reference of the token passing (csrc/kws_ref.h, through k2hip_debug_kws_ref_dp) against the float64 twin (tests/kws_twin.py), the twin
against brute force over all paths on tiny tries, the decision margins of the end-to-end fixture from the twin alone, the keyword file
loader, and the host side of the feature as its own program under AddressSanitizer / UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import parity
from kws_cases import KEYWORDS, THRESHOLD, hand_cases, random_cases, wide_keywords
from kws_twin import brute_force_frame, build_trie, fresh_state, token_passing, trie_cells

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELL_TOL = 2 * parity.LOGIT_TOL / 10   # tests/test_align_gpu.py


def ref_dp(parent, depth, kw, bar, stay, emit, a=None, start=None):
    """csrc/kws_ref.h on one stream -> (events, a, start)"""
    from k2transducerasr_amd import load_library
    L = load_library()
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    L.k2hip_debug_kws_ref_dp.argtypes = [ip, ip, ip, fp, C.c_int32, fp, fp, C.c_int32, fp, ip, ip, ip, ip, fp, C.c_int32, ip]
    S, T = len(parent), stay.shape[0]
    if a is None:
        a64, s64 = fresh_state(S)
        a, start = a64.astype(np.float32), s64.astype(np.int32)
    a, start = a.copy(), start.copy()
    arr = [np.ascontiguousarray(x, dtype=np.int32) for x in (parent, depth, kw)]
    bar = np.ascontiguousarray(bar, dtype=np.float32)
    stay, emit = np.ascontiguousarray(stay, dtype=np.float32), np.ascontiguousarray(emit, dtype=np.float32)
    cap = max(T, 1)
    ek, es, ee = (np.zeros(cap, np.int32) for _ in range(3))
    em = np.zeros(cap, np.float32)
    n = C.c_int32(0)
    p = lambda x, t: x.ctypes.data_as(t)
    rc = L.k2hip_debug_kws_ref_dp(p(arr[0], ip), p(arr[1], ip), p(arr[2], ip), p(bar, fp), S, p(stay, fp), p(emit, fp), T, p(a, fp), p(start, ip),
                                  p(ek, ip), p(es, ip), p(ee, ip), p(em, fp), cap, C.byref(n))
    assert rc == 0, L.k2hip_last_error()
    return [(int(ek[i]), int(es[i]), int(ee[i]), float(em[i])) for i in range(n.value)], a, start


def test_trie_and_bar_against_the_restatement():
    from k2transducerasr_amd import Keywords
    thr = [0.9, 0.5, 0.25, 1.0, 0.05, 0.5, 0.5, 0.35, 0.5]
    for words, th, V in ((KEYWORDS, thr, 37), (KEYWORDS, THRESHOLD, 41), (wide_keywords(), 0.3, 3000), ([], 0.5, 37), ([[1], [1, 1]], 0.5, 3)):
        kw = Keywords(words, th, V)
        want = build_trie(words, np.broadcast_to(np.asarray(th, np.float32), (len(words),)).astype(np.float64))
        got = kw.tables()
        assert kw.num_states == len(want["parent"]) and kw.num_keywords == len(words)
        for k in ("parent", "tok", "depth", "kw"):
            assert got[k].tolist() == want[k].tolist(), k
        assert all(got["parent"][s] < s for s in range(1, kw.num_states))
        # bar is ONE float32 product of depth and logf(threshold): logf is within an ulp, the product rounds once (1.5 x 2^-23 < 2e-7)
        assert np.all(np.abs(got["bar"] - want["bar"]) <= 2e-7 * np.abs(want["bar"])) and got["bar"].dtype == np.float32
        assert np.all(np.isfinite(got["bar"]))
    assert Keywords(KEYWORDS, THRESHOLD, 37).num_states == 18
    assert len({w[0] for w in wide_keywords()}) == 70


def test_every_refusal_names_the_keyword():
    from k2transducerasr_amd import K2HipError, Keywords

    def refused(words, th, V, *parts):
        with pytest.raises(K2HipError) as e:
            Keywords(words, th, V)
        assert e.value.code == -1 and all(p in str(e.value) for p in parts), str(e.value)

    refused([[5, 6], []], 0.5, 37, "keyword 1", "empty")
    refused([[5], [6, 37]], 0.5, 37, "keyword 1", "37")
    refused([[5, -1]], 0.5, 37, "keyword 0")
    refused([[5], [6, 0, 7]], 0.5, 37, "keyword 1", "blank")
    refused([[2]], 0.5, 37, "keyword 0", "unk")
    refused([[5, 6], [7], [5, 6]], 0.5, 37, "keyword 2", "duplicates", "keyword 0")
    for bad in (0.0, -0.1, 1.0001, float("nan"), float("inf")):
        refused([[5], [6]], [0.5, bad], 37, "keyword 1", "threshold")
    chains = [[3 + p] + [3 + (p + i) % 300 for i in (1, 2, 3)] for p in range(256)]
    assert Keywords(chains[:255], 0.5, 400).num_states == 1021
    refused(chains, 0.5, 400, "keyword 255", "1024")


def test_keyword_file_loader(tmp_path):
    from k2transducerasr_amd import K2HipError, Keywords, TokenTable
    toks = tmp_path / "tokens.txt"
    toks.write_text("".join(f"{s} {i}\n" for i, s in enumerate(["<blk>", "<sos/eos>", "<unk>", "▁HE", "LLO", "▁WORLD", ":x"])))
    tab = TokenTable(str(toks))
    f = tmp_path / "kw.txt"
    f.write_text("▁HE LLO :0.35\n\n▁WORLD\n▁HE :x\n")
    kw = Keywords.load(tab, str(f), 0.5)
    t = kw.tables()
    assert kw.num_keywords == 3 and t["tok"].tolist() == [-1, 3, 4, 5, 6] and t["kw"].tolist() == [-1, -1, 0, 1, 2]   # ":x" is a token
    assert abs(t["bar"][2] - 2 * np.log(0.35)) < 1e-6 and abs(t["bar"][3] - np.log(0.5)) < 1e-6
    for text, parts in (("▁HE NOPE\n", ("line 1", "NOPE")), ("▁HE\n▁HE :1.5\n", ("line 2", "threshold")), ("▁HE :abc\n", ("line 1", "threshold")),
                        ("▁WORLD\n\n▁WORLD\n", ("line 3", "duplicates", "line 1")), ("<unk>\n", ("line 1", "unk"))):
        f.write_text(text)
        with pytest.raises(K2HipError) as e:
            Keywords.load(tab, str(f), 0.5)
        assert e.value.code == -1 and all(p in str(e.value) for p in parts), str(e.value)
    with pytest.raises(K2HipError) as e:
        Keywords.load(tab, str(tmp_path / "missing.txt"), 0.5)
    assert e.value.code == -2


@pytest.mark.parametrize("T", range(1, 7))
def test_twin_equals_brute_force(T):
    """the twin's token passing = the enumeration of every path on tiny tries (S <= 5, T <= 6) with -inf cells: values, the emit-wins
    rule, the start frames, the events and the reset"""
    rng = np.random.default_rng(300 + T)
    tries = [([[5]], 0.5), ([[5, 6, 7]], 0.4), ([[5, 6], [7, 8]], 0.3), ([[5], [5, 6], [7], [7, 8]], 0.45), ([[5, 6, 7, 8]], 0.6)]
    for words, th in tries:
        trie = build_trie(words, th)
        trie["bar"] = np.round(trie["bar"] * 4) / 4     # multiples of 0.25: a == bar happens
        S = len(trie["parent"])
        assert S <= 5
        for trial in range(8):
            stay = -0.25 * rng.integers(0, 8, size=(T, S)).astype(np.float64)
            emit = -0.25 * rng.integers(0, 8, size=(T, S)).astype(np.float64)
            if trial >= 4:
                stay[rng.random(stay.shape) < 0.2] = -np.inf
                emit[rng.random(emit.shape) < 0.2] = -np.inf
            a, start = fresh_state(S)
            R = -1
            for t in range(T):
                ev, a, start = token_passing(trie, stay[t: t + 1], emit[t: t + 1], a, start)
                want = brute_force_frame(trie, stay, emit, t, R)
                cand = [c for c, (v, by, _) in want.items() if trie["kw"][c] >= 0 and by and v >= trie["bar"][c]]
                if cand:
                    win = min(cand, key=lambda c: (-trie["depth"][c], -want[c][0], trie["kw"][c]))
                    assert len(ev) == 1 and ev[0][0] == trie["kw"][win] and ev[0][2] == t and ev[0][3] == want[win][0], (words, trial, t)
                    assert ev[0][1] in want[win][2]
                    assert np.all(a[1:] == -np.inf) and np.all(start[1:] == -1)
                    R = t
                else:
                    assert ev == []
                    for c, (v, _, starts) in want.items():
                        assert a[c] == v, (words, trial, t, c)
                        assert (start[c] in starts) if v > -np.inf else start[c] == -1
                assert start[0] == t + 1 and a[0] == 0


def all_cases():
    return hand_cases() + random_cases()


def test_host_reference_against_the_twin():
    """csrc/kws_ref.h (float32) = the twin (float64) on planes of multiples of 0.25, where both are exact: events, sum_logp and the carried
    block bit for bit; the hand-built cases also against their written-down answers; any chunking gives one call's result"""
    rng = np.random.default_rng(7)
    n_events = 0
    for case in all_cases():
        trie = dict(parent=case["parent"], depth=case["depth"], kw=case["kw"], bar=case["bar"].astype(np.float64))
        for b, (stay, emit) in enumerate(case["streams"]):
            ev, a, start = ref_dp(case["parent"], case["depth"], case["kw"], case["bar"], stay, emit)
            tev, ta, ts = token_passing(trie, stay.astype(np.float64), emit.astype(np.float64))
            assert ev == tev, (case["name"], b)
            assert np.array_equal(a, ta.astype(np.float32)) and start.tolist() == ts.tolist(), (case["name"], b)
            n_events += len(ev)
            if "expect" in case:
                assert ev == case["expect"][b], (b, ev)
                for c, (va, vs) in case["states"][b].items():
                    assert a[c] == va and start[c] == vs, (b, c, a[c], start[c])
            # chunked
            T = stay.shape[0]
            ca, cs, cev, t = None, None, [], 0
            while t < T:
                n = min(T - t, int(rng.integers(1, 6)))
                e2, ca, cs = ref_dp(case["parent"], case["depth"], case["kw"], case["bar"], stay[t: t + n], emit[t: t + n], ca, cs)
                cev += e2
                t += n
            assert cev == ev and ca.tobytes() == a.tobytes() and cs.tobytes() == start.tobytes(), (case["name"], b)
    assert n_events > 100   # the random cases do fire


@pytest.fixture(scope="module")
def fixture_cells(oracle_tiny, utts):
    f = [oracle_tiny.fbank(u) for u in utts]
    enc = oracle_tiny.encoder(oracle_tiny.pad_sequence(f).reshape(len(utts), -1, 80))
    trie = build_trie(KEYWORDS, THRESHOLD)
    return trie, enc, [trie_cells(oracle_tiny, enc[b], trie) for b in range(enc.shape[0])]


def test_fixture_decisions_clear_their_error_bounds(fixture_cells):
    """the end-to-end input of tests/test_kws_gpu.py, from the twin alone: every decision an event depends on (threshold tests,
    predecessor choices at qualifying terminals and along the winning paths, choices among candidates) clears its own error bound --
    the arcs involved x CELL_TOL -- at least 10 times, so a device whose cells are within CELL_TOL takes the same decisions"""
    trie, enc, cells = fixture_cells
    assert enc.shape[:2] == (5, 35) and len(trie["parent"]) == 18
    ratios, events = [], []
    for stay, emit in cells:
        ev, _, _ = token_passing(trie, stay, emit, ratios=ratios, tol=CELL_TOL)
        events += ev
    print(f"{len(events)} events of {len({e[0] for e in events})} keywords, {len(ratios)} decisions, smallest margin / bound {min(ratios):.1f}")
    # 17 events; keywords 0 (three tokens), 1, 2 and 7 occur
    assert len(events) == 17 and {e[0] for e in events} == {0, 1, 2, 7}
    assert all(e[2] - e[1] + 1 == len(KEYWORDS[e[0]]) for e in events)     # no winning path holds a stay arc on this model
    assert min(ratios) >= 10


def test_host_side_under_the_sanitizers(tiny_model_path, tmp_path):
    """tests/native/san_kws_driver.cpp (make san_kws): the graph builder and its refusals, kws_ref.h against the enumeration of every
    path, the entries' argument checks and the streams' life cycle over the CPU stand-in of the engine.  Its own program, built with
    ASan / UBSan."""
    from k2transducerasr_amd.synth import write_synthetic_model
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "k2transducerasr_amd", "csrc"), "-s", "san_kws"])
    ctc = str(tmp_path / "ctc.k2w")
    write_synthetic_model(ctc, "zipformer2-ctc-tiny-test")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "native", "k2hip_san_kws_driver"), tiny_model_path, ctc], capture_output=True, text=True,
                       env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "san_kws_driver ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
