"""N-best hypotheses and token log-probs of the modified beam search, without a GPU: the Python twin (tests/nbest_twin.py) against the
CPU oracle and against a hand-derived merge case, and the host layer's argument checks of the new entry points."""
import numpy as np
import pytest

from hotword_twin import SCORE, tiny_phrases
from kat_model import frames, write_kat_model
from nbest_twin import KAT_MERGE, TwinGraph, kat_merge_logp, nbest_twin_batch, nbest_twin_search


@pytest.fixture(scope="module")
def enc_tiny(oracle_tiny, utts):
    f = [oracle_tiny.fbank(u) for u in utts]
    return oracle_tiny.encoder(oracle_tiny.pad_sequence(f).reshape(len(utts), -1, 80))


def _check_lists(runs, beam):
    for r in runs:
        alts = r["alts"]
        assert 1 <= len(alts) <= beam
        seqs = [tuple(a["tokens"]) for a in alts]
        assert len(set(seqs)) == len(seqs)                              # pairwise distinct sequences
        norms = [a["norm"] for a in alts]
        assert norms == sorted(norms, reverse=True)
        for a in alts:
            assert len(a["tokens"]) == len(a["timestamps"]) == len(a["token_log_probs"])
            assert (a["token_log_probs"] <= 0).all()
            assert a["timestamps"] == sorted(a["timestamps"])


@pytest.mark.parametrize("beam", [1, 2, 4, 8])
def test_twin_entry0_is_the_oracle(oracle_tiny, enc_tiny, beam):
    want, sc = oracle_tiny.modified_beam_search(enc_tiny, beam, want_scores=True)
    runs = nbest_twin_batch(oracle_tiny, enc_tiny, beam)
    assert [(r["alts"][0]["tokens"], r["alts"][0]["timestamps"]) for r in runs] == want
    np.testing.assert_allclose([r["alts"][0]["score"] for r in runs], sc, atol=1e-4, rtol=0)
    _check_lists(runs, beam)
    if beam > 1:
        assert max(len(r["alts"]) for r in runs) > 1


@pytest.mark.parametrize("beam", [1, 2, 4, 8])
def test_twin_entry0_is_the_oracle_with_hotwords(oracle_tiny, enc_tiny, beam):
    """The oracle has no hotwords: with c = 0 the graph is walked and earns nothing, so entry 0 must still be the oracle's result;
    with the committed score the biased entry 0 must be what tests/hotword_twin.py's search returns."""
    from hotword_twin import twin_batch
    want, sc = oracle_tiny.modified_beam_search(enc_tiny, beam, want_scores=True)
    phrases = tiny_phrases(oracle_tiny.modified_beam_search(enc_tiny, max(beam, 2)))
    V = oracle_tiny.vocab_size
    runs = nbest_twin_batch(oracle_tiny, enc_tiny, beam, TwinGraph(phrases, 0.0, V))
    assert [(r["alts"][0]["tokens"], r["alts"][0]["timestamps"]) for r in runs] == want
    np.testing.assert_allclose([r["alts"][0]["score"] for r in runs], sc, atol=1e-4, rtol=0)
    _check_lists(runs, beam)
    g = TwinGraph(phrases, SCORE, V)
    runs = nbest_twin_batch(oracle_tiny, enc_tiny, beam, g)
    res, bsc, _, _, _ = twin_batch(oracle_tiny, enc_tiny, beam, g)
    assert [(r["alts"][0]["tokens"], r["alts"][0]["timestamps"]) for r in runs] == res
    np.testing.assert_allclose([r["alts"][0]["score"] for r in runs], bsc, atol=1e-4, rtol=0)
    _check_lists(runs, beam)


def test_kat_merge_keeps_the_first_inserted_token_log_probs(tmp_path):
    """nbest_twin.KAT_MERGE (derivation there): [5] + blank and [] + 5 merge at t1; the survivor keeps timestamp 0 and log p_t0(5); the
    hotword bonus of the phrase [5] is in the score and not in the token log-probs."""
    from oracle import Oracle
    p = str(tmp_path / "kat.k2w")
    write_kat_model(p)
    ora = Oracle(p)
    enc = frames(KAT_MERGE["rows"])
    kept, dropped = kat_merge_logp(0, 5, 0.1 * (0.5 + 0.5)), kat_merge_logp(1, 5, 0.1 * (0.5 + 0.5))
    assert abs(kept - dropped) > 0.04                                    # the case discriminates
    plain = nbest_twin_search(ora, enc, KAT_MERGE["beam"])
    by_seq = {tuple(a["tokens"]): a for a in plain["alts"]}
    assert set(by_seq) == {(), (5,), (5, 5)}
    a5 = by_seq[(5,)]
    assert a5["timestamps"] == [0]
    assert abs(float(a5["token_log_probs"][0]) - kept) < 1e-5
    # its score is the logaddexp of both paths
    both = np.logaddexp(kat_merge_logp(0, 5, 0.1) + kat_merge_logp(1, 0, 0.1 * (0.5 + 5)), kat_merge_logp(0, 0, 0.1) + kat_merge_logp(1, 5, 0.1))
    assert abs(a5["score"] - both) < 1e-5
    # entry 0 is the oracle's result
    assert (plain["alts"][0]["tokens"], plain["alts"][0]["timestamps"]) == ora.modified_beam_search(enc[None], KAT_MERGE["beam"])[0]
    biased = nbest_twin_search(ora, enc, KAT_MERGE["beam"], TwinGraph(KAT_MERGE["phrases"], SCORE, 8))
    b5 = {tuple(a["tokens"]): a for a in biased["alts"]}[(5,)]
    assert b5["timestamps"] == [0]
    assert abs(b5["score"] - (both + SCORE)) < 1e-5                      # the bonus is in the score ...
    assert np.array_equal(b5["token_log_probs"], a5["token_log_probs"])  # ... and not in the token log-probs


# ---- the host layer through the C ABI (no GPU: everything below fails before a device is needed, or needs none) -------------------
def test_null_and_range_arguments():
    import ctypes as C
    from k2transducerasr_amd import load_library
    L = load_library()
    L.k2hip_set_nbest.argtypes = [C.c_void_p, C.c_int32]
    assert L.k2hip_set_nbest(None, 2) == -1
    for fn in ("k2hip_offline_stream_num_alternatives", "k2hip_online_stream_num_alternatives", "k2hip_beam_stream_num_alternatives"):
        getattr(L, fn).argtypes = [C.c_void_p]
        assert getattr(L, fn)(None) == -1
    for fn in ("k2hip_offline_stream_get_token_log_probs", "k2hip_online_stream_get_token_log_probs", "k2hip_beam_stream_get_token_log_probs"):
        getattr(L, fn).argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        assert getattr(L, fn)(None, None, 0) == -1
    L.k2hip_beam_search_nbest.argtypes = [C.c_void_p] * 2 + [C.c_int32] * 4 + [C.c_void_p] * 6 + [C.c_int32]
    assert L.k2hip_beam_search_nbest(None, None, 1, 1, 4, 2, None, None, None, None, None, None, 1) == -1


def test_beam_history_nbest_under_the_sanitizers():
    """tests/native/san_nbest_driver.cpp: BeamHistory::nbest and the materialised token log-probs against a whole-sequence model, over
    several chunks with a pruned-then-respelled prefix, a tie, a pending table and a reset -- built with ASan / UBSan"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "k2transducerasr_amd", "csrc"), "-s", "san"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(root, "tests", "native", "k2hip_san_nbest_driver")], capture_output=True, text=True, env=env, timeout=300)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])


def test_host_layer_of_the_new_entry_points_under_the_sanitizers(tiny_model_path, tmp_path):
    """tests/native/san_nbest_api_driver.cpp: csrc/api.cpp over the CPU stand-in of the engine, under ASan / UBSan -- a bad nbest, a
    small cap (nothing written), greedy / CTC rejection, the pipelined route's (submit and wait) and GetResult's refusal, the start
    state before a result, after a reset and after a failed GetResults, a greedy stream's accessors"""
    import os
    import subprocess
    from k2transducerasr_amd.synth import write_synthetic_model
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "k2transducerasr_amd", "csrc"), "-s", "san"])
    stream, ctc = str(tmp_path / "stream.k2w"), str(tmp_path / "ctc.k2w")
    write_synthetic_model(stream, "zipformer2-streaming-tiny-test")
    write_synthetic_model(ctc, "zipformer2-ctc-tiny-test")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(root, "tests", "native", "k2hip_san_nbest_api_driver"), tiny_model_path, stream, ctc], capture_output=True,
                       text=True, env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "OK" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
