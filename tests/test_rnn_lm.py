"""Neural LM rescoring without a GPU: the container and its loader, the importer, the host reference (csrc/rnn_lm_ref.h) against torch's
own LSTM in float64 (tests/rnn_lm_twin.py), the row plan (csrc/rnn_lm_plan.cpp) against its restatement, the measured bound, and the
conditions the recognizer tests of test_rnn_lm_gpu.py rest on."""
import numpy as np
import pytest
import torch

import rnn_lm_cases as cases
from rnn_lm_twin import Twin, plan_restated, rescored_order, restate32

from k2transducerasr_amd import K2HipError, RnnLm
from k2transducerasr_amd.binding import rnn_lm_plan
from k2transducerasr_amd.k2w import read_k2w, write_k2w
from k2transducerasr_amd.rnn_lm_import import import_state_dict
from k2transducerasr_amd.synth import rnn_lm_state_dict, write_rnn_lm, write_synthetic_rnn_lm

INVALID, UNSUPPORTED, IO = -1, -6, -2


@pytest.fixture(scope="module")
def lms(tmp_path_factory):
    """name -> (path, state dict, RnnLm, Twin)"""
    d = tmp_path_factory.mktemp("rnn_lm")
    out = {}
    for name, (V, E, H, L, seed) in cases.LMS.items():
        p = str(d / f"{name}.k2w")
        sd = write_synthetic_rnn_lm(p, V, E, H, L, seed)
        out[name] = (p, sd, RnnLm(p), Twin(sd, L))
    return out


def test_error_codes_are_the_headers():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "k2hip.h")).read()
    for name, v in (("K2HIP_ERR_INVALID", INVALID), ("K2HIP_ERR_UNSUPPORTED", UNSUPPORTED), ("K2HIP_ERR_IO", IO)):
        assert int(re.search(name + r" \((-?\d+)\)", src).group(1)) == v


def test_round_trip_and_getters(lms):
    for name, (V, E, H, L, _) in cases.LMS.items():
        p, sd, lm, _ = lms[name]
        assert (lm.vocab_size, lm.embedding_dim, lm.hidden_dim, lm.num_layers, lm.sos_id, lm.eos_id) == (V, E, H, L, 1, 1)
        meta, t = read_k2w(p)
        assert meta["model_type"] == "rnn_lm" and set(t) == set(sd)
        for k in sd:
            assert np.array_equal(t[k], sd[k])


def test_importer_from_a_torch_module(tmp_path):
    class M(torch.nn.Module):   # icefall's RnnLmModel by its attribute names
        def __init__(self):
            super().__init__()
            self.input_embedding = torch.nn.Embedding(37, 32)
            self.rnn = torch.nn.LSTM(32, 64, 2, batch_first=True)
            self.output_linear = torch.nn.Linear(64, 37)

    torch.manual_seed(3)
    m = M()
    hyps = [[5, 9, 36, 0], [], [7]]
    for wrapped in (False, True):
        p = str(tmp_path / f"imp{int(wrapped)}.k2w")
        sd = m.state_dict()
        dims = import_state_dict({"model": sd, "epoch": 3} if wrapped else sd, p)
        assert dims == dict(vocab_size=37, embedding_dim=32, hidden_dim=64, num_layers=2)
        tot, _ = RnnLm(p).score_host(hyps)
        with torch.no_grad():   # the module itself, float64
            md = M().double()
            md.load_state_dict({k: v.double() for k, v in sd.items()})
            for h, got in zip(hyps, tot):
                x = torch.tensor([[1] + h])
                lp = torch.log_softmax(md.output_linear(md.rnn(md.input_embedding(x))[0][0]), -1)
                want = float(lp[torch.arange(len(h) + 1), torch.tensor(h + [1])].sum())
                assert abs(got - want) <= cases.total_bound(len(h) + 1)
    with pytest.raises(ValueError):
        import_state_dict({k: v for k, v in m.state_dict().items() if k != "rnn.bias_hh_l1"}, str(tmp_path / "bad.k2w"))


def test_tie_weights(tmp_path):
    sd = rnn_lm_state_dict(37, 64, 64, 1, 4, tie_weights=True)
    hyps = [[3, 4, 5], [36]]
    want, _ = Twin(sd, 1).score_all(hyps)
    for keep in (False, True):
        p = str(tmp_path / f"tied{int(keep)}.k2w")
        write_rnn_lm(p, sd, 1, tie_weights=True, keep_tied_output=keep)
        assert ("output_linear.weight" in read_k2w(p)[1]) == keep
        got, _ = RnnLm(p).score_host(hyps)
        assert all(abs(g - w) <= cases.total_bound(len(h) + 1) for g, w, h in zip(got, want, hyps))
    bad = rnn_lm_state_dict(37, 32, 64, 1, 4)
    p = str(tmp_path / "tied_bad.k2w")
    write_rnn_lm(p, bad, 1, tie_weights=True)   # E != H and no output matrix in the file
    with pytest.raises(K2HipError) as e:
        RnnLm(p)
    assert e.value.code == INVALID and "tie_weights" in str(e.value)


def _rewrite(path, sd, meta_changes=None, drop=None, replace=None):
    meta = {"model_type": "rnn_lm", "vocab_size": "37", "embedding_dim": "64", "hidden_dim": "64", "num_layers": "1", "sos_id": "1", "eos_id": "1",
            "tie_weights": "0"}
    meta.update(meta_changes or {})
    t = {k: v for k, v in sd.items() if k != drop}
    t.update(replace or {})
    write_k2w(path, meta, list(t.items()))


def test_every_load_refusal(tmp_path):
    sd = rnn_lm_state_dict(37, 64, 64, 1, 2)
    p = str(tmp_path / "x.k2w")

    def refused(code, *words, **kw):
        _rewrite(p, sd, **kw)
        with pytest.raises(K2HipError) as e:
            RnnLm(p)
        assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)

    _rewrite(p, sd)
    RnnLm(p)
    for name in sd:                                                                   # a missing tensor, named
        refused(INVALID, name, "missing", drop=name)
    refused(INVALID, "rnn.weight_hh_l0", "shape", replace={"rnn.weight_hh_l0": sd["rnn.weight_hh_l0"][:, :32].copy()})
    refused(INVALID, "rnn.bias_ih_l0", "shape", replace={"rnn.bias_ih_l0": sd["rnn.bias_ih_l0"].reshape(4, 64)})
    refused(INVALID, "output_linear.weight", "shape", replace={"output_linear.weight": sd["output_linear.weight"].T.copy()})
    refused(INVALID, "input_embedding.weight", "float32", replace={"input_embedding.weight": np.zeros((37, 64), np.int64)})
    for bad in (np.nan, np.inf):
        w = sd["rnn.weight_ih_l0"].copy()
        w[200, 7] = bad
        refused(INVALID, "rnn.weight_ih_l0", "non-finite", replace={"rnn.weight_ih_l0": w})
    refused(INVALID, "sos_id", meta_changes={"sos_id": "37"})
    refused(INVALID, "eos_id", meta_changes={"eos_id": "-1"})
    refused(INVALID, "num_layers", meta_changes={"num_layers": "9"})
    refused(INVALID, "model_type", meta_changes={"model_type": "zipformer2"})
    # H % 32 != 0 / E % 4 != 0
    for E, H in ((64, 48), (30, 64)):
        q = str(tmp_path / f"u{E}_{H}.k2w")
        write_rnn_lm(q, rnn_lm_state_dict(37, E, H, 1, 2), 1)
        with pytest.raises(K2HipError) as e:
            RnnLm(q)
        assert e.value.code == UNSUPPORTED
    # a truncated file
    _rewrite(p, sd)
    raw = open(p, "rb").read()
    for cut in (10, len(raw) // 2, len(raw) - 4):
        open(p, "wb").write(raw[:cut])
        with pytest.raises(K2HipError) as e:
            RnnLm(p)
        assert e.value.code in (IO, INVALID)
    with pytest.raises(K2HipError) as e:
        RnnLm(str(tmp_path / "absent.k2w"))
    assert e.value.code == IO


def test_score_host_against_the_twin_and_the_bound(lms):
    """every LM x every set, with and without eos: the host reference within the bound of the float64 twin per token and per total; the
    float32 restatement's error re-measured against the recorded E32"""
    e32 = ehost = 0.0
    for name, (V, E, H, L, _) in cases.LMS.items():
        _, sd, lm, tw = lms[name]
        for sname, hyps in cases.hyp_sets(V).items():
            for eos in (True, False):
                tot, tlp = lm.score_host(hyps, eos)
                wt, wl = tw.score_all(hyps, eos)
                for i, h in enumerate(hyps):
                    P = len(h) + int(eos)
                    assert len(tlp[i]) == len(wl[i]) == P
                    r_tot, r32 = restate32(sd, L, h, eos)
                    if P:
                        e32 = max(e32, float(np.abs(r32 - wl[i]).max()))
                        ehost = max(ehost, float(np.abs(tlp[i] - wl[i]).max()))
                        assert np.abs(tlp[i] - wl[i]).max() <= cases.token_bound(), (name, sname, eos, i)
                    else:
                        assert tot[i] == 0.0 and r_tot == 0.0
                    assert abs(tot[i] - wt[i]) <= cases.total_bound(P), (name, sname, eos, i)
                    assert tot[i] == np.float32(sum(tlp[i], np.float32(0)))   # the float32 sum in position order
    print(f"e32 = {e32:.4g} (recorded {cases.E32:.4g}), host reference error {ehost:.4g}, token bound {cases.token_bound():.4g}")
    # the recorded constant is this measurement (numpy's matrix product may sum in another order on another machine: a factor of two)
    assert e32 <= 2 * cases.E32 and cases.E32 <= 4 * max(e32, 1e-9)


def test_host_checks(lms):
    _, _, lm, _ = lms["A"]
    for hyps, word in (([[1, 2], [3, 37]], "hypothesis 1"), ([[-1]], "hypothesis 0")):
        with pytest.raises(K2HipError) as e:
            lm.score_host(hyps)
        assert e.value.code == INVALID and word in str(e.value)
    import ctypes as C
    tok, off, tot = np.zeros(4, np.int64), np.array([0, 3, 2], np.int64), np.zeros(2, np.float32)
    rc = lm._L.k2hip_rnn_lm_score_host(lm._h, tok.ctypes.data_as(C.POINTER(C.c_int64)), off.ctypes.data_as(C.POINTER(C.c_int64)), 2, 1, None,
                                       tot.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == INVALID and b"hypothesis 1" in lm._L.k2hip_last_error() and b"decrease" in lm._L.k2hip_last_error()
    assert lm._L.k2hip_rnn_lm_vocab_size(None) == -1 and lm._L.k2hip_rnn_lm_eos_id(None) == -1
    tot, tlp = lm.score_host([], True)
    assert len(tot) == 0 and tlp == []


def test_plan_against_its_restatement():
    rng = np.random.default_rng(7)
    sets = [[], [0], [0, 0, 0], [5] * 9, list(range(12, 0, -1)), list(range(6))]
    sets += [rng.choice([0, 1, 2, 31, 32, 33], size=int(n)).tolist() for n in rng.integers(1, 80, size=30)]
    sets += [rng.integers(0, 50, size=int(n)).tolist() for n in rng.integers(1, 40, size=20)]
    blocked = 0
    for lens in sets:
        for eos in (True, False):
            for H, cap in ((32, 0), (64, 4 * 64 * 40), (32, 1)):
                got, want = rnn_lm_plan(lens, eos, H, cap), plan_restated(lens, eos, H, cap or 1 << 26)
                assert got == want, (lens, eos, H, cap)
                P = [n + int(eos) for n in lens]
                assert sorted(got["order"]) == list(range(len(lens))) and [P[i] for i in got["order"]] == sorted(P, reverse=True)
                assert got["base"][-1] == sum(P) and all(a >= b for a, b in zip(got["active"], got["active"][1:]))
                blocked += len(got["block"]) > 2
    assert blocked > 0


@pytest.mark.parametrize("kind", ["transducer", "ctc"])
def test_recognizer_case_conditions_on_the_twins(kind, tmp_path, utts):
    """what test_rnn_lm_gpu.py's recognizer tests rest on, on the twins' own N-best lists of the five fixture utterances: with the
    recorded LM seed and scale no two adjacent keys of a stream fall inside KEY_GAP, and at least two streams change their top entry"""
    from oracle import Oracle
    from k2transducerasr_amd.synth import write_synthetic_model
    rc = cases.RECOGNIZER[kind]
    p = str(tmp_path / "m.k2w")
    write_synthetic_model(p, rc["preset"])
    ora = Oracle(p)
    enc = ora.encoder(ora.pad_sequence([ora.fbank(u) for u in utts]).reshape(len(utts), -1, 80))
    if kind == "ctc":
        from ctc_prefix_twin import prefix_beam_search
        lists = [[(h["tokens"], h["score"]) for h in prefix_beam_search(enc[b], 4)["hyps"][:4]] for b in range(len(utts))]
    else:
        from nbest_twin import nbest_twin_batch
        lists = [[(a["tokens"], a["score"]) for a in r["alts"][:4]] for r in nbest_twin_batch(ora, enc, 4)]
    V, E, H, L, _ = cases.LMS["A"]
    tw = Twin(rnn_lm_state_dict(V, E, H, L, rc["seed"]), L)
    changed, gap = 0, np.inf
    for l in lists:
        lm = [tw.score(t)[0] for t, _ in l]
        order, keys = rescored_order([s for _, s in l], [len(t) for t, _ in l], lm, rc["scale"], kind == "ctc")
        changed += order[0] != 0
        ks = sorted(keys, reverse=True)
        gap = min([gap] + [a - b for a, b in zip(ks, ks[1:])])
    print(f"{kind}: {changed} of {len(lists)} tops change, smallest adjacent key gap {gap:.4g}")
    assert changed >= 2 and gap >= cases.KEY_GAP
