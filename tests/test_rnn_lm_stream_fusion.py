"""CPU side of the streaming neural LM shallow fusion tests: the recorded near-tied prefix ends of tests/rnn_lm_stream_fusion_cases.py
recomputed on the twin and held to the record and to the cap, the "dropped hypothesis" case that gives the GPU test its meaning, and
the rules of the new switch through the CPU stand-in engine (the refusals, reset, the offline switch alone)."""
import numpy as np
import pytest

import parity
import rnn_lm_fusion_cases as oc
import rnn_lm_stream_fusion_cases as cases


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    d = tmp_path_factory.mktemp("rnn_lm_stream_fusion_cpu")
    return d, {w: oc.make_oracle(d, w)[1] for w in ("tiny", "tiny165")}


@pytest.mark.parametrize("name,beam", sorted(oc.SEEDS))
def test_near_tied_prefix_ends_are_the_recorded_ones(world, name, beam):
    """the twin over every prefix of every stream: the ends whose adjacent final normalised scores are closer than LOGIT_TOL equal the
    record, no case has more than CAP of 60 (what the GPU test may excuse against the twin), the pick itself is that close at no more
    than PICK_TIED_MAX -- and the per-frame gaps of a prefix are those of the whole utterance's first n frames"""
    d, oras = world
    ora, enc, nlm = cases.case_inputs(d, oras, name, beam)
    assert enc.shape[0] * enc.shape[1] == 60
    runs = [cases.prefix_runs(ora, enc[b], beam, nlm) for b in range(enc.shape[0])]
    got, picks = cases.near_tied(runs)
    print(f"LM {name} beam {beam}: near-tied prefix ends {got}, pick within tolerance at {picks}")
    assert got == cases.NEAR_TIED[(name, beam)]
    assert len(got) <= cases.CAP and picks <= cases.PICK_TIED_MAX
    for rs in runs:
        whole = rs[-1]["gaps"]
        assert float(np.min(whole)) >= parity.LOGIT_TOL
        for n, r in enumerate(rs, 1):
            assert np.array_equal(r["gaps"], whole[:n])


@pytest.mark.parametrize("what", sorted(oc.TOGETHER))
def test_near_tied_prefix_ends_together(world, what):
    d, oras = world
    base, seed, _ = oc.TOGETHER[what]
    ora = oras["tiny"]
    enc = oc.encode(ora, oc.utterances(base))
    ex = oc.together_extras(ora, enc, what)
    _, nlm, _ = oc.make_lm(d, "A", seed)
    got, picks = cases.near_tied([cases.prefix_runs(ora, enc[b], 4, nlm, lm=ex.get("lm"), scale=ex.get("scale", 0.0), graph=ex.get("graph"))
                                  for b in range(enc.shape[0])])
    assert got == cases.NEAR_TIED_TOGETHER[what]
    assert len(got) <= cases.CAP and picks <= cases.PICK_TIED_MAX


def test_a_recorded_case_keeps_a_hypothesis_the_unfused_search_drops(world):
    """without this the GPU test's "carry really happens" shows nothing: at the recorded prefix end the fused beam holds a token sequence
    the unfused beam over the same frames has dropped, and the fused pick at the end of the utterance is not the unfused one"""
    d, oras = world
    c = cases.DROPPED
    assert (c["name"], c["beam"]) in oc.SEEDS
    ora, enc, nlm = cases.case_inputs(d, oras, c["name"], c["beam"])
    found, moved = cases.dropped_and_kept(ora, enc[c["stream"]], c["beam"], nlm)
    assert moved and found and found[0] == (c["n"], c["tokens"])


def test_rules_through_the_cpu_stand_in_engine(tiny_model_path, tmp_path):
    """the setting changed mid-stream and the LM replaced while a stream carries state (K2HIP_ERR_INVALID, nothing moves), reset, the
    offline switch alone enabling nothing on a streaming entry, a call that fails after its blocks were staged: the native driver's
    checks over the stand-in engine (tests/native/san_rnn_lm_stream_fusion_driver.cpp; a failed CHECK names its line)"""
    from test_rnn_lm_stream_fusion_sanitizers import run_driver
    r = run_driver(tiny_model_path, tmp_path)
    assert r.returncode == 0 and "san_rnn_lm_stream_fusion_driver ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
