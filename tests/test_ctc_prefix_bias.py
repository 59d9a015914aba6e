"""CPU tests of the hotword / n-gram LM biasing of the CTC prefix beam search: the numpy twin (tests/ctc_prefix_bias_twin.py) against the
unbiased twin with no and with empty tables, against brute force where nothing is pruned, the walk invariant, the hand-built flip, the
conditions the committed inputs (tests/ctc_prefix_bias_cases.py) were picked for, their gaps against G, and csrc/ctc_prefix_bias_ref.h
against the float32 twin bit for bit (through tests/native/san_ctc_prefix_bias_driver.cpp's `case` mode, its own program)."""
import ctypes
import ctypes.util
import os
import subprocess

import numpy as np
import pytest

import ctc_prefix_bias_cases as bc
import ctc_prefix_cases as base
from ctc_prefix_bias_twin import (HW_EVENTS, LM_EVENTS, biased_prefix_beam_search, dense_graph, lm_tables, measured_e, min_gap, walk)
from ctc_prefix_twin import brute_force, prefix_beam_search
from hotword_twin import TwinGraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_runs = {}


def run(name, lp, beam, graph, lm, dtype):
    """a twin run of a committed case, computed once and shared"""
    key = (name, beam, np.dtype(dtype).name)
    if key not in _runs:
        _runs[key] = biased_prefix_beam_search(lp, beam, graph, lm, dtype)
    return _runs[key]


def listing(res):
    return [(h["tokens"], h["timestamps"]) for h in res["hyps"]]


def test_no_tables_and_empty_tables_are_the_plain_search():
    """null tables, an empty graph and score_per_token = 0 add nothing: picks, gaps, scores, histories equal prefix_beam_search exactly"""
    lp, nf = base.ragged_rows()
    phrases = [[5, 7], [9]]
    for dtype in (np.float64, np.float32):
        for r in range(len(base.RAGGED_SEEDS)):
            for beam in base.RAGGED_BEAMS:
                want = prefix_beam_search(lp[r, : nf[r]], beam, dtype)
                for graph in (None, TwinGraph([], bc.SCORE, 37), TwinGraph(phrases, 0.0, 37)):
                    got = biased_prefix_beam_search(lp[r, : nf[r]], beam, graph, None, dtype)
                    assert got["picks"] == want["picks"] and got["cut_gaps"] == want["cut_gaps"] and got["final_gaps"] == want["rank_gaps"]
                    assert [h["slot"] for h in got["hyps"]] == list(range(len(want["hyps"])))
                    for a, b in zip(got["hyps"], want["hyps"]):
                        assert (a["tokens"], a["timestamps"], a["score"], a["tot"]) == (b["tokens"], b["timestamps"], b["score"], b["score"])
                        assert np.array_equal(a["token_log_probs"], b["token_log_probs"]) and a["ctx"] == 0


@pytest.mark.parametrize("kind", bc.KINDS)
def test_unpruned_rows_against_brute_force(kind):
    """V = 3, T <= 2, beam 8: every entry's final is the brute-force full sum plus the walk over its tokens minus pending (float64)"""
    ex, nf = base.exhaustive_rows()
    graph, lm = bc.pick(kind, bc.small_graph(bc.EXHAUSTIVE_PHRASES), bc.small_lm())
    for r, T in enumerate(nf):
        got = biased_prefix_beam_search(ex[r, :T], 8, graph, lm)
        bf = {k: v for k, v in brute_force(ex[r, :T]).items() if v[0] > -np.inf}
        assert sorted(tuple(h["tokens"]) for h in got["hyps"]) == sorted(bf)
        for h in got["hyps"]:
            ctx, hs, _ = walk(h["tokens"], graph, lm)
            want = bf[tuple(h["tokens"])][0] + float(ctx) - (float(graph.pending(hs)) if graph else 0.0)
            assert abs(h["score"] - want) <= 1e-12 * max(1.0, abs(want)), (r, h, want)
        assert all(a["score"] >= b["score"] for a, b in zip(got["hyps"], got["hyps"][1:]))


def test_slot_state_is_the_walk_over_the_tokens_bit_for_bit():
    """float32, every committed case: each surviving slot's (ctx, hs, ls) equals the walk over its tokens -- also where the sequence was
    re-spelled or received folds"""
    for name, lp, beams, graph, lm, _ in bc.strict_cases():
        for beam in beams:
            for h in run(name, lp, beam, graph, lm, np.float32)["hyps"]:
                ctx, hs, ls = walk(h["tokens"], graph, lm, np.float32)
                assert (np.float32(h["ctx"]).tobytes(), h["hs"], h["ls"]) == (np.float32(ctx).tobytes(), hs, ls), (name, beam, h)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_hand_built_flip(dtype):
    """the derivation in ctc_prefix_bias_cases.py: [b] without the phrase, [a, b] with it, best score 0.75 exactly"""
    plain = prefix_beam_search(bc.FLIP_ROWS, bc.FLIP_BEAM, dtype)["hyps"][0]
    assert (plain["tokens"], plain["timestamps"]) == bc.FLIP_UNBIASED
    got = biased_prefix_beam_search(bc.FLIP_ROWS, bc.FLIP_BEAM, bc.flip_graph(), None, dtype)
    best = got["hyps"][0]
    assert (best["tokens"], best["timestamps"], best["score"]) == bc.FLIP_BIASED
    assert (best["ctx"], best["hs"], best["tot"]) == (3.0, 0, -2.25) and got["events"]["committed"] == 1
    assert got["hyps"][1]["tokens"] == [3] and abs(got["hyps"][1]["score"] + 1.99945) < 1e-5


def test_the_committed_inputs_show_what_they_were_picked_for():
    events = {k: 0 for k in HW_EVENTS + LM_EVENTS}
    moved = reordered = weaker_differs = 0
    for name, lp, beams, graph, lm, _ in bc.strict_cases():
        for beam in beams:
            got = run(name, lp, beam, graph, lm, np.float64)
            for k in events:
                events[k] += got["events"][k]
            moved += got["hyps"][0]["tokens"] != prefix_beam_search(lp, beam)["hyps"][0]["tokens"]
            reordered += [h["slot"] for h in got["hyps"]] != list(range(len(got["hyps"])))
            if graph is not None and "wide" not in name and "long" not in name:
                weaker_differs += listing(biased_prefix_beam_search(lp, beam, graph, lm, bonus_after_selection=True)) != listing(got)
    print(events, moved, reordered, weaker_differs)
    assert all(v > 0 for v in events.values()), events
    assert moved > 0 and reordered > 0 and weaker_differs > 0
    for kind in ("hw", "both"):   # a re-spelled fold with a graph over the re-spelled row's tokens
        graph, lm = bc.pick(kind, bc.small_graph(bc.RESPELLED_PHRASES), bc.small_lm())
        assert run(f"re-spelled {kind}", base.respelled_row(), base.RESPELLED_BEAM, graph, lm, np.float64)["respelled_folds"] >= 1
    graph, lm = bc.wide_tables()   # the hub: more than 64 arcs, and the result walks on from it
    tab = lm_tables(lm)
    hub_state = lm.state_of[(bc.wide_hub(),)]
    assert tab["states"][hub_state, 1] - tab["states"][hub_state, 0] > 64
    best = run("wide lm", base.wide_row(), 4, None, lm, np.float64)["hyps"][0]["tokens"]
    assert any(a == bc.wide_hub() for a in best[:-1])


def test_inputs_of_the_gpu_tests_clear_their_gap():
    """every case the GPU tests assert exactly: 8 E <= G with E re-measured here, and every gap of the float64 twin >= G"""
    for name, lp, beams, graph, lm, G in bc.strict_cases():
        for beam in beams:
            a, b = run(name, lp, beam, graph, lm, np.float64), run(name, lp, beam, graph, lm, np.float32)
            assert a["picks"] == b["picks"] and [h["slot"] for h in a["hyps"]] == [h["slot"] for h in b["hyps"]], (name, beam)
            e = max([abs(x - y) for x, y in zip(a["cut_gaps"], b["cut_gaps"]) if np.isfinite(x) and np.isfinite(y)] +
                    [abs(x - y) for x, y in zip(a["final_gaps"], b["final_gaps"]) if np.isfinite(x) and np.isfinite(y)] + [0.0])
            print(f"{name} beam {beam}: E {e:.3g}, smallest gap {min_gap(a):.3g}, G {G:.3g}")
            assert 8 * e <= G <= min_gap(a), (name, beam, e, min_gap(a), G)


def test_fixture_batch_clears_its_gap(tmp_path, utts):
    """the end-to-end GPU test's streams, on the oracle's log-probs of the fixture batch: every stream, every table kind clears G_FIXTURE,
    8 E <= G_FIXTURE with E re-measured, and the biasing moves some result"""
    from k2transducerasr_amd.synth import write_synthetic_model
    from oracle import Oracle
    p = str(tmp_path / "ctc.k2w")
    write_synthetic_model(p, "zipformer2-ctc-tiny-test")
    o = Oracle(p)
    lp = o.encoder(o.pad_sequence([o.fbank(u) for u in utts]).reshape(len(utts), -1, 80)).astype(np.float32)
    graph, lm = bc.fixture_tables(lp)
    moved = 0
    for kind in bc.KINDS:
        g, m = bc.pick(kind, graph, lm)
        for b in range(len(utts)):
            e, a, agree = measured_e(lp[b], bc.FIXTURE_BEAM, g, m)
            print(f"stream {b} {kind}: E {e:.3g}, smallest gap {min_gap(a):.3g}")
            assert agree and 8 * e <= bc.G_FIXTURE <= min_gap(a), (kind, b, e, min_gap(a))
            moved += a["hyps"][0]["tokens"] != prefix_beam_search(lp[b], bc.FIXTURE_BEAM)["hyps"][0]["tokens"]
    assert moved > 0


def write_case(path, lp, beam, graph, lm):
    """the `case` file of tests/native/san_ctc_prefix_bias_driver.cpp"""
    lp = np.ascontiguousarray(lp, np.float32)
    T, V = lp.shape
    words = [lp.view(np.int32).ravel()]
    S = S_lm = A = start = 0
    if graph is not None:
        nxt, bonus, pending = dense_graph(graph)
        S = nxt.shape[0]
        words += [nxt.ravel(), bonus.view(np.int32).ravel(), pending.view(np.int32)]
    if lm is not None:
        t = lm_tables(lm)
        S_lm, A, start = t["states"].shape[0], len(t["arc_tok"]), t["start"]
        words += [t["states"].ravel(), t["arc_tok"], t["arc_lp"].view(np.int32), t["arc_next"], t["uni_lp"].view(np.int32), t["uni_next"]]
    np.concatenate([np.array([T, V, beam, S, S_lm, A, start], np.int32)] + words).astype(np.int32).tofile(path)


def libm_lae():
    """logaddexp in float32 with the C library's expf / log1pf: the operations csrc/ctc_prefix_ref.h's ctc_prefix_logaddexp makes (numpy
    rounds its own float32 exp / log1p differently in the last place on a few arguments)"""
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    for f in (m.expf, m.log1pf):
        f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float]

    def lae(a, b, dt):
        assert dt is np.float32
        hi, lo = (a, b) if a > b else (b, a)
        if lo == -np.inf:
            return np.float32(hi)
        return np.float32(np.float32(hi) + np.float32(m.log1pf(m.expf(np.float32(np.float32(lo) - np.float32(hi))))))
    return lae


def test_host_reference_equals_the_float32_twin_bit_for_bit(tmp_path):
    """csrc/ctc_prefix_bias_ref.h (its own program under ASan / UBSan) on every committed case at its widest beam against the float32
    twin run with the C library's expf / log1pf: the entries' order, slots, tokens, timestamps, hs, ls and the bits of final, tot and
    ctx are equal"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "k2transducerasr_amd", "csrc"), "-s", "san_ctc_prefix_bias"])
    exe = os.path.join(ROOT, "tests", "native", "k2hip_san_ctc_prefix_bias_driver")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    lae = libm_lae()
    for name, lp, beams, graph, lm, _ in bc.strict_cases():
        beam = max(beams)
        want = biased_prefix_beam_search(lp, beam, graph, lm, np.float32, lae=lae)
        path = str(tmp_path / "case.bin")
        write_case(path, lp, beam, graph, lm)
        r = subprocess.run([exe, "case", path], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (name, r.stderr[-2000:])
        lines = r.stdout.strip().split("\n")
        assert lines[0] == f"respelled {want['respelled_folds']}", name
        assert len(lines) - 1 == len(want["hyps"]), name
        for line, h in zip(lines[1:], want["hyps"]):
            head, ts = line.split("|")
            f = head.split()
            got = (int(f[1]), int(f[2]), int(f[3]), [int(x) for x in f[7:]], [int(x) for x in ts.split()])
            assert got == (h["slot"], h["hs"], h["ls"], h["tokens"], h["timestamps"]), (name, line, h)
            bits = [np.array([v], np.float32).view(np.uint32)[0] for v in (h["score"], h["tot"], h["ctx"])]
            assert [int(x, 16) for x in f[4:7]] == bits, (name, line, h)


def test_surface_exists():
    import inspect

    from k2transducerasr_amd import Model, OfflineRecognizer, load_library
    assert callable(Model.set_ctc_prefix_biasing)
    assert inspect.signature(OfflineRecognizer.__init__).parameters["ctc_prefix_biasing"].default is False
    assert hasattr(load_library(), "k2hip_set_ctc_prefix_biasing")
    with open(os.path.join(ROOT, "include", "k2hip.h")) as f:
        text = f.read()
    assert "k2hip_set_ctc_prefix_biasing" in text and "Hotword and n-gram LM biasing of the CTC prefix beam search" in text
    with open(os.path.join(ROOT, "include", "k2hip_debug.h")) as f:
        assert '"ctc_prefix_beam_bias"' in f.read()
