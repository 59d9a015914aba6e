"""CPU tests of the streaming CTC prefix beam search (prefixes carried across chunks): the numpy restatement of the carry
(tests/ctc_prefix_stream_twin.py) against the whole-row twin (tests/ctc_prefix_twin.py) in float32 and float64, the figures of the new
small-vocabulary case, the power of the inputs to tell a correct carry from two weaker ones, and the host side of the feature
(csrc/ctc_prefix_hist.h, the resumed reference step, the ABI entries' argument rules over the engine stand-ins) as its own program under
AddressSanitizer / UBSan."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ctc_prefix_cases as cases
import ctc_prefix_stream_cases as scases
from ctc_prefix_stream_twin import chunked_search, same_hyps
from ctc_prefix_twin import min_gap, prefix_beam_search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_whole = {}


def whole(key, lp, beam, dtype=np.float64):
    k = (key, beam, np.dtype(dtype).name)
    if k not in _whole:
        _whole[k] = prefix_beam_search(lp, beam, dtype)
    return _whole[k]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_respelled_row_at_every_split_and_chunking(dtype):
    """V = 3, T = 10, beam 4: all nine two-chunk splits and uniform chunks of 1, 2, 3, 4 give the whole search's slots -- tokens,
    timestamps, token log-probs, (pb, pnb, score) in the dtype's own bits, and the same picks in every frame"""
    row = cases.respelled_row()
    want = whole("respelled", row, cases.RESPELLED_BEAM, dtype)
    chunkings = scases.respelled_chunkings()
    assert len(chunkings) == 13
    for ch in chunkings:
        tw = chunked_search(row, cases.RESPELLED_BEAM, ch, dtype)
        assert same_hyps(tw.hyps(), want["hyps"]), ch
        assert tw.picks == want["picks"] and tw.respelled_folds == want["respelled_folds"] >= 1, ch
        assert tw.boundary_folds >= 1, ch         # every chunking has a fold decided through the relation tables


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_strict_cases_in_chunks_of_16(dtype):
    crossing = 0
    for name, lp, beams, _ in cases.strict_cases():
        for beam in beams:
            tw = chunked_search(lp, beam, scases.CHUNK, dtype)
            assert same_hyps(tw.hyps(), whole(name, lp, beam, dtype)["hyps"]), (name, beam)
            if lp.shape[1] == 37:
                crossing += tw.boundary_folds
    # the V = 37 seeded cases have no fold relation crossing a 16-frame boundary at all: alone they would pass a broken carry
    assert crossing == 0


@pytest.mark.parametrize("beam", scases.SMALL4_BEAMS)
def test_small_vocabulary_case_and_its_figures(beam):
    """seeded_log_probs(3000, 48, 4, 2.0) in chunks of 16: equal to the whole search in both dtypes; the twin's smallest gap, the gaps at
    the boundary frames, E re-measured the way test_ctc_prefix.py measures it, gap >= 8 E, the re-spelled folds of beam 8"""
    lp = scases.small4_row()
    a, b = whole("small4", lp, beam), whole("small4", lp, beam, np.float32)
    for dtype, want in ((np.float64, a), (np.float32, b)):
        tw = chunked_search(lp, beam, scases.SMALL4_CHUNK, dtype)
        assert same_hyps(tw.hyps(), want["hyps"]) and tw.picks == want["picks"]
        assert tw.boundary_folds >= 1
    assert a["picks"] == b["picks"]               # float32 and float64 selections agree
    e = 0.0
    for t in range(scases.SMALL4_T):
        if np.isfinite(a["cut_gaps"][t]) and np.isfinite(b["cut_gaps"][t]):
            e = max(e, abs(a["cut_gaps"][t] - b["cut_gaps"][t]))
    for ga, gb in zip(a["rank_gaps"], b["rank_gaps"]):
        e = max(e, abs(ga - gb))
    gap = min_gap(a)
    boundary = [a["cut_gaps"][t] for t in (15, 16, 31, 32)]
    print(f"small4 beam {beam}: E {e:.3g}, smallest gap {gap:.3g}, gaps at frames 15/16/31/32 {boundary}, re-spelled folds {a['respelled_folds']}")
    assert gap >= scases.SMALL4_MIN_GAP[beam] and e <= scases.SMALL4_E[beam] and gap >= 8 * e
    assert min(boundary) >= scases.SMALL4_MIN_GAP[beam]
    assert a["respelled_folds"] == (2 if beam == 8 else 0)


def test_the_inputs_tell_a_correct_carry_from_a_weaker_one():
    """a stand-in that sees a fold relation only inside the chunk (same carried origin, non-empty suffix) differs from the whole search at
    every split and chunking of the re-spelled row and on the V = 4 case at both beams; one that decides by node identity fails on the
    re-spelled row"""
    row = cases.respelled_row()
    want = whole("respelled", row, cases.RESPELLED_BEAM)["hyps"]
    for ch in scases.respelled_chunkings():
        assert not same_hyps(chunked_search(row, cases.RESPELLED_BEAM, ch, carry="in_chunk").hyps(), want), ch
        assert not same_hyps(chunked_search(row, cases.RESPELLED_BEAM, ch, carry="node").hyps(), want), ch
    lp = scases.small4_row()
    for beam in scases.SMALL4_BEAMS:
        assert not same_hyps(chunked_search(lp, beam, scases.SMALL4_CHUNK, carry="in_chunk").hyps(), whole("small4", lp, beam)["hyps"]), beam


def test_ragged_chunk_capacity_does_not_matter():
    """a chunk of n frames inside a capacity Tc > n (the relation tables' cap) gives the same slots"""
    lp = scases.small4_row()
    want = whole("small4", lp, 8)["hyps"]
    assert same_hyps(chunked_search(lp, 8, [7] * 6 + [6], Tc=16).hyps(), want)
    assert same_hyps(chunked_search(lp, 8, [7] * 6 + [6]).hyps(), want)


def write_cases(path):
    """the driver's cases.bin: int32 n, then per case int32 T, V, beam, n_chunks, chunk lengths, float32 lp[T][V]"""
    out = []
    row = cases.respelled_row()
    for ch in scases.respelled_chunkings():
        out.append((row, cases.RESPELLED_BEAM, ch))
    for _, lp, beams, _ in cases.strict_cases():
        for beam in beams:
            out.append((lp, beam, scases.uniform(lp.shape[0], scases.CHUNK)))
    for beam in scases.SMALL4_BEAMS:
        out.append((scases.small4_row(), beam, scases.uniform(scases.SMALL4_T, scases.SMALL4_CHUNK)))
        out.append((scases.small4_row(), beam, [7] * 6 + [6]))
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(out)))
        for lp, beam, ch in out:
            lp = np.ascontiguousarray(lp, np.float32)
            f.write(struct.pack(f"<{4 + len(ch)}i", lp.shape[0], lp.shape[1], beam, len(ch), *ch))
            f.write(lp.tobytes())
    return len(out)


def test_host_side_under_the_sanitizers(tiny_model_path, tmp_path):
    """tests/native/san_ctc_prefix_stream_driver.cpp (make san_ctc_prefix_stream): every case above chunked through CtcPrefixHistory and
    the float32 reference of the resumed step, after every chunk bit for bit ctc_prefix_ref.h over the frames so far and the live tree
    nodes at most beam * (longest live prefix + 1) + 1; then the argument rules of the new entries over the CPU stand-in of the engine.
    Its own program, built with ASan / UBSan."""
    from k2transducerasr_amd.synth import write_synthetic_model
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "k2transducerasr_amd", "csrc"), "-s", "san_ctc_prefix_stream"])
    ctc = str(tmp_path / "ctc.k2w")
    write_synthetic_model(ctc, "zipformer2-ctc-tiny-test")
    ctc_streaming = str(tmp_path / "ctc_streaming.k2w")
    write_synthetic_model(ctc_streaming, "zipformer2-ctc-streaming-tiny-test")
    n = write_cases(str(tmp_path / "cases.bin"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "native", "k2hip_san_ctc_prefix_stream_driver"), str(tmp_path / "cases.bin"), ctc, tiny_model_path, ctc_streaming],
                       capture_output=True, text=True, env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and f"san_ctc_prefix_stream_driver ok ({n} cases)" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


NEW_SYMBOLS = ["k2hip_ctc_prefix_stream_create", "k2hip_ctc_prefix_stream_destroy", "k2hip_ctc_prefix_stream_reset", "k2hip_ctc_prefix_stream_num_frames",
               "k2hip_ctc_prefix_beam_search_chunk", "k2hip_ctc_prefix_stream_num_tokens", "k2hip_ctc_prefix_stream_get_tokens",
               "k2hip_ctc_prefix_stream_get_timestamps", "k2hip_ctc_prefix_stream_get_token_log_probs", "k2hip_ctc_prefix_stream_get_score",
               "k2hip_ctc_prefix_stream_num_alternatives", "k2hip_ctc_prefix_stream_get_alternative", "k2hip_online_stream_set_ctc_prefix_beam"]


def test_surface_exists():
    import inspect

    from k2transducerasr_amd import CtcPrefixStream, Model, OnlineRecognizer, OnlineStream, load_library
    lib = load_library()
    with open(os.path.join(ROOT, "include", "k2hip.h")) as f:
        text = f.read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name + "(" in text, name
    with open(os.path.join(ROOT, "include", "k2hip_debug.h")) as f:
        assert "ctc_prefix_resume" in f.read()
    assert "prefixes carried across chunks" in text
    assert [p for p in inspect.signature(Model.create_ctc_prefix_stream).parameters] == ["self", "beam", "nbest"]
    assert inspect.signature(Model.create_ctc_prefix_stream).parameters["nbest"].default == 1
    assert [p for p in inspect.signature(Model.ctc_prefix_beam_search_chunk).parameters] == ["self", "streams", "log_probs", "n_frames"]
    assert [p for p in inspect.signature(OnlineStream.set_ctc_prefix_beam).parameters] == ["self", "beam", "nbest"]
    sig = inspect.signature(OnlineRecognizer.create_online_stream)
    assert sig.parameters["ctc_prefix_beam"].default == 0 and sig.parameters["nbest"].default == 1
    for attr in ("tokens", "timestamps", "token_log_probs", "score", "num_frames", "alternatives", "reset", "close"):
        assert hasattr(CtcPrefixStream, attr), attr
