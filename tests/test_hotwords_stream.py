"""Per-stream hotword biasing of the STREAMING modified beam search, the part that needs no GPU: the reference (hotword_twin) on
the inputs test_hotwords_stream_gpu.py uses -- chunk-invariant by construction, since it is run on prefixes -- is decisive there;
the setters' argument errors that are decided before any device work; the sanitizer builds of the host layer."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import parity
from hotword_stream_cases import STEPS, STREAM_BEAMS, STREAM_PRESET, prefix_ends, stream_case, twin_final_states, twin_prefix
from hotword_twin import SCORE, TINY_BEAMS, WIDE_BEAMS, WIDE_VOCAB, TwinGraph, tiny_phrases, wide_enc, wide_phrases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "k2transducerasr_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")


def _decisive(what, key, ora, enc, beams, phrases, steps):
    """item 1 of the issue for one stream: events occur, the finalize rule decides at some prefix end, the smallest margin"""
    graph = TwinGraph(phrases, SCORE, ora.vocab_size)
    ends = prefix_ends(enc.shape[0], steps)
    events = dict(bonus=0, broken=0, committed=0)
    smallest, rule_decides = np.inf, 0
    for beam in beams:
        whole = twin_prefix(key, ora, enc, enc.shape[0], beam, phrases)
        for k in events:
            events[k] += int(whole["events"][k])
        states = twin_final_states(ora, enc, beam, graph)
        for n in ends:
            run = twin_prefix(key, ora, enc, n, beam, phrases)
            m = run["margins"]
            smallest = min(smallest, float(m[np.isfinite(m)].min()) if np.isfinite(m).any() else np.inf)
            hyps = states[n]
            raw = int(np.argmax([lp / ln for _, lp, _, ln in hyps]))
            fin = int(np.argmax([(lp - pend) / ln for _, lp, pend, ln in hyps]))
            assert hyps[fin][0] == run["ys"], (what, beam, n)      # (the restated loop agrees with the twin's own pick)
            if hyps[raw][2] > 0 and raw != fin:
                rule_decides += 1
    print(f"{what}: events {events}, {rule_decides} prefix ends decided by the finalize rule, smallest margin {smallest:.6g} over "
          f"{len(ends) * len(beams)} (beam, prefix) checks")
    return events, rule_decides, smallest


def test_reference_is_decisive_on_the_streaming_tiny_frames(tmp_path_factory):
    from k2transducerasr_amd.synth import write_synthetic_model
    p = str(tmp_path_factory.mktemp("hw_stream_ref") / "stream.k2w")
    write_synthetic_model(p, STREAM_PRESET, blank_bias=0.0)
    ora, enc, unbiased, phrases = stream_case(p)
    assert len(phrases) >= 4
    ev, decides, smallest = _decisive("streaming tiny", "stream", ora, enc, STREAM_BEAMS, phrases, STEPS)
    assert min(ev.values()) >= 1, ev
    assert decides >= 1, "no prefix end falls on an unfinished leading match: the finalize rule decides nothing on these inputs"
    # (c) the smallest margin is RECORDED, not asserted: over ~10^4 top-k decisions (224 (beam, prefix) runs x up to 60 frames, the
    # beam-th against the (beam + 1)-th candidate of a 37-token vocabulary) some gap is always far below parity.LOGIT_TOL -- 5.5e-6
    # on this utterance, and no utterance / phrase seed tried gave a figure above it.  The GPU file therefore grants NO excuse at
    # all: every (stream, prefix) check there is exact.
    assert np.isfinite(smallest) and smallest >= 0


def test_reference_is_decisive_on_the_tiny_and_wide_batches(oracle_tiny, utts, tmp_path_factory):
    from kat_model import write_wide_model
    from oracle import Oracle
    f = [oracle_tiny.fbank(u) for u in utts]
    enc = oracle_tiny.encoder(oracle_tiny.pad_sequence(f).reshape(len(utts), -1, 80))
    total, smallest = dict(bonus=0, broken=0, committed=0), np.inf
    for beam in TINY_BEAMS:
        phrases = tiny_phrases(oracle_tiny.modified_beam_search(enc, beam))
        for b in range(enc.shape[0]):
            ev, _, sm = _decisive(f"tiny beam={beam} stream {b}", ("tiny", beam, b), oracle_tiny, enc[b], (beam,), phrases, (8,))
            smallest = min(smallest, sm)
            for k in total:
                total[k] += ev[k]
    assert min(total.values()) >= 1, total
    p = str(tmp_path_factory.mktemp("hw_stream_wide") / "wide.k2w")
    write_wide_model(p, WIDE_VOCAB)
    ora = Oracle(p)
    wenc = wide_enc()
    wtotal = dict(bonus=0, broken=0, committed=0)
    for beam in WIDE_BEAMS:
        phrases = wide_phrases(ora.modified_beam_search(wenc, beam))
        for b in range(wenc.shape[0]):
            ev, _, sm = _decisive(f"wide beam={beam} stream {b}", ("wide", beam, b), ora, wenc[b], (beam,), phrases, (13,))
            smallest = min(smallest, sm)
            for k in wtotal:
                wtotal[k] += ev[k]
    assert min(wtotal.values()) >= 1, wtotal
    print(f"tiny + wide batches: smallest margin {smallest:.6g}")
    assert np.isfinite(smallest) and smallest >= 0      # (recorded, not asserted: see above)


def test_null_stream_is_an_argument_error():
    from k2transducerasr_amd import Hotwords, load_library
    L = load_library()
    L.k2hip_online_stream_set_hotwords.argtypes = [C.c_void_p, C.c_void_p]
    L.k2hip_beam_stream_set_hotwords.argtypes = [C.c_void_p, C.c_void_p]
    hw = Hotwords([[4, 5]], SCORE, 37)
    for f in (L.k2hip_online_stream_set_hotwords, L.k2hip_beam_stream_set_hotwords):
        assert f(None, hw._h) == -1
        assert b"null argument" in L.k2hip_last_error()
        assert f(None, None) == -1
    hw.close()


def _make(target):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_hotword_streams_under_asan_ubsan(tiny_model_path, tmp_path):
    from k2transducerasr_amd.synth import write_synthetic_model
    _make("san")
    stream = str(tmp_path / "stream.k2w")
    write_synthetic_model(stream, STREAM_PRESET)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(NATIVE, "k2hip_san_hotwords_driver"), tiny_model_path, stream], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "OK" in r.stdout


def test_hotword_streams_under_tsan(tiny_model_path, tmp_path):
    from k2transducerasr_amd.synth import write_synthetic_model
    _make("tsan")
    stream = str(tmp_path / "stream.k2w")
    write_synthetic_model(stream, STREAM_PRESET)
    r = subprocess.run([os.path.join(NATIVE, "k2hip_tsan_hotwords_driver"), tiny_model_path, stream], capture_output=True, text=True,
                       env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "OK" in r.stdout
