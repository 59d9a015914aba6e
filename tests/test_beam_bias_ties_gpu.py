"""The BIASED modified beam search -- k_beam_loop<1, true>, k_beam_loop<2, true>, k_beam_step<true>, the final picks of k_beam_final and
k_beam_resume_final on lp - pending(state), the wave walk of lm_walk.h -- on exact ties, merges and the beam cut: hotword bonuses that
are earned, handed back, committed and left through a failure link, n-gram LM terms of every kind, both together, at V in {200, 400,
600, 1021, 1029} and beams 1, 2, 4, 5 and 8.  Inputs, float64 reference, the extended bound and the promises that make the comparison
exact: tests/beam_bias_cases.py, checked on the host by tests/test_beam_bias_cases_ref.py.  Rig and forms: tests/test_beam_ties_gpu.py.

Held in every form, plain and then with nbest = 8 on one handle: tokens, timestamps, number and ORDER of the alternatives equal the
float64 twin's exactly -- nothing excused: every decision is an exact tie of equally formed scores or 10 x the bound wide -- scores
within beam_bias_cases.score_bound, token log-probs within beam_cases.noise_terms, entry 0 equal to the plain call bit for bit, the
k_beam_loop forms bit-equal among themselves, the launch counter showing that the biased kernels ran, and the plain bits back once the
bias is cleared.  The resumed search walks graph A in stream 0, none in stream 1 and graph B in stream 2 of ONE call with the LM on the
model: after the last chunk the alternatives are the twin's and bit-equal to the offline call made with that stream's graph, and at the
inner chunk ends the stream's pick is the twin's pick on that prefix -- the pick loses pending, the carried block keeps it."""
import contextlib
import functools

import numpy as np
import pytest

import beam_bias_cases as bb
import beam_cases as bc
from test_beam_ties_gpu import K_BEAM_LOOP, SWITCHES, forms_for, launch_counts, retries, run_form, same_bits, splits, table_rows
from test_search_ties_gpu import switch

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def reference(V, config, case, stream, beam, n=None):
    """(float64 twin's result over the first n frames, score bound) -- computed once, shared by every test of the module"""
    m = bb.cases(V)
    c = next(x for x in m.cases if x.name == case)
    bias = bb.biases(V)[config]
    enc = c.enc[stream][:n]
    ref = bb.twin(m.W, m.b, enc, beam, np.float64, bias.graph, bias.lm)
    return ref, bb.score_bound(m.W, m.b, ref, enc.shape[0])


@functools.lru_cache(maxsize=None)
def prefix_ok(V, case, stream, beam, n):
    m = bb.cases(V)
    c = next(x for x in m.cases if x.name == case)
    return bb.prefix_ok(m, c.enc[stream], beam, bb.resumed_bias(V, stream), n)


@pytest.fixture(scope="module", params=bb.VS, ids=lambda V: f"V{V}")
def rig(request, tmp_path_factory):
    """the V model twice (with the all-contexts decoder table, and loaded without it), the two hotword lists and the LM"""
    from k2transducerasr_amd import Hotwords, Model, NgramLm
    V = request.param
    m = bb.cases(V)
    path = str(tmp_path_factory.mktemp("beam_bias_ties") / f"v{V}.k2w")
    m.write(path)
    table = Model(path, 0)
    with switch("K2HIP_DECODER_TABLE_MB", 0, 1024):
        bare = Model(path, 0)
        assert table_rows(bare) == 0
    assert table_rows(table) == (V + 1) * V, "the one-kernel forms need the all-contexts decoder table"
    b = bb.biases(V)
    tools = dict(A=Hotwords(b["hw"].phrases, bb.SCORE, V), B=Hotwords(b["bothB"].phrases, bb.SCORE, V), lm=NgramLm(b["lm"].entries, V))
    yield m, table, bare, tools
    with switch("K2HIP_DECODER_TABLE_MB", 0, 1024):
        assert table_rows(bare) == 0, "the no_table form ran with a table"
    table.close()
    bare.close()
    for t in tools.values():
        t.close()


@contextlib.contextmanager
def biased(model, tools, config):
    """the model-level bias of a configuration, cleared again on the way out"""
    try:
        if config != "lm":
            model.set_hotwords(tools["B" if config == "bothB" else "A"])
        if config != "hw":
            model.set_ngram_lm(tools["lm"], bb.SCALE)
        yield
    finally:
        model.set_hotwords(None)
        model.set_ngram_lm(None)


def unbiased(model, bare, enc, beam):
    """the plain call (on the model without a table: under the switch it was loaded with)"""
    with switch("K2HIP_DECODER_TABLE_MB", 0, 1024) if model is bare else contextlib.nullcontext():
        return model.beam_search(enc, beam, want_scores=True)


def against_twin(m, config, case, beam, alts, what, worst):
    """every stream's alternatives against the float64 twin: content and order exact, numbers within the derived bounds"""
    e_u = bc.noise_terms(m.W, m.b)[0]
    for s, got in enumerate(alts):
        ref, bound = reference(m.V, config, case, s, beam)
        want = ref["alts"][:8]
        assert len(got) == len(want), (what, s, len(got), len(want))
        assert [(a["tokens"], a["timestamps"]) for a in got] == [(a["tokens"], a["timestamps"]) for a in want], (what, s, got, want)
        for g, w in zip(got, want):
            d = abs(g["score"] - w["score"])
            worst[0] = max(worst[0], d)
            worst[2] = max(worst[2], d / bound)
            assert d <= bound, (what, s, g["score"], w["score"], bound)
            assert len(g["token_log_probs"]) == len(g["tokens"])
            if len(g["tokens"]):
                d = float(np.abs(g["token_log_probs"] - w["token_log_probs"]).max())
                worst[1] = max(worst[1], d)
                assert d <= e_u, (what, s, d, e_u)


@pytest.mark.parametrize("beam", bb.BEAMS)
@pytest.mark.parametrize("config", ("hw", "lm", "both"))
def test_every_form_returns_the_float64_order(rig, config, beam):
    m, table, bare, tools = rig
    worst = [0.0, 0.0, 0.0]
    forms = forms_for(m.V, beam) if config == "both" else ("loop", "launches")
    for c in m.cases:
        out = {}
        before = {model: unbiased(model, bare, c.enc, beam) for model in (table, bare)}
        for form in forms:
            model = bare if form == "no_table" else table
            r0 = retries(table)
            p0, h0 = launch_counts()
            with biased(model, tools, config):
                plain, psc, alts = out[form] = run_form(form, table, bare, c.enc, beam)
            p1, h1 = launch_counts()
            what = f"V={m.V} {config} beam={beam} {c.name} {form}"
            assert (p1 - p0, h1 - h0) == (0, 2), (what, "the biased kernels did not run", p1 - p0, h1 - h0)
            assert retries(table) - r0 == (2 if form == "repeat" else 0), (what, retries(table) - r0)
            against_twin(m, config, c.name, beam, alts, what, worst)
            for s, a in enumerate(alts):      # entry 0 is the plain call's result, bit for bit
                assert (a[0]["tokens"], a[0]["timestamps"]) == plain[s], (what, s)
                assert np.float32(a[0]["score"]) == psc[s], (what, s)
            # the bias cleared: the plain bits again, from the plain kernels
            after = unbiased(model, bare, c.enc, beam)
            assert launch_counts() == (p1 + 1, h1), what
            assert after[0] == before[model][0] and after[1].tobytes() == before[model][1].tobytes(), what
        for form in K_BEAM_LOOP[1:]:
            if form in out:
                assert out[form][0] == out["loop"][0] and out[form][1].tobytes() == out["loop"][1].tobytes(), (m.V, config, beam, c.name, form)
                same_bits(out[form][2], out["loop"][2])
    bound = max(reference(m.V, config, c.name, s, beam)[1] for c in m.cases for s in range(c.enc.shape[0]))
    print(f"V={m.V} {config} beam={beam}: worst score diff {worst[0]:.3g} ({worst[2]:.3f} of its bound; largest bound {bound:.3g}), "
          f"worst token log-prob diff {worst[1]:.3g} ({worst[1] / bc.noise_terms(m.W, m.b)[0]:.3f} of its bound {bc.noise_terms(m.W, m.b)[0]:.3g})")


@pytest.mark.parametrize("beam", bb.BEAMS)
def test_the_resumed_search_walks_each_streams_own_graph(rig, beam):
    """BeamStream.search_chunk with graph A on stream 0, none on stream 1, graph B on stream 2 and the LM on the model, over the same
    frames in chunks of one frame, as 3 / 1 / 5 / 3 and as one chunk.  A stream that read its neighbour's tables, a pick that kept
    its pending bonus, or a carried block that lost it, ends elsewhere than the twin."""
    from k2transducerasr_amd import BeamStream
    m, table, _, tools = rig
    configs = ("both", "lm", "bothB")
    graphs = (tools["A"], None, tools["B"])
    table.set_decoding_method("modified_beam_search", beam)
    table.set_nbest(8)
    table.set_ngram_lm(tools["lm"], bb.SCALE)
    compared = total = 0
    worst = 0.0
    try:
        for c in m.cases:
            B, T, _ = c.enc.shape
            assert B == len(graphs)
            for form in ("loop", "launches"):
                sw = SWITCHES[form]
                with switch(sw, 1) if sw else contextlib.nullcontext():
                    off = []                  # stream s of the offline call made with stream s's graph
                    for s, g in enumerate(graphs):
                        table.set_hotwords(g)
                        off.append(table.beam_search(c.enc, beam, nbest=8)[s])
                    table.set_hotwords(None)
                for name, chunks in splits(T).items():
                    what = f"V={m.V} beam={beam} {c.name} {form} {name}"
                    ss = [BeamStream(table, beam) for _ in range(B)]
                    for st, g in zip(ss, graphs):
                        st.set_hotwords(g)
                    p0, h0 = launch_counts()
                    n = 0
                    with switch(sw, 1) if sw else contextlib.nullcontext():
                        for k in chunks:
                            BeamStream.search_chunk(ss, c.enc[:, n: n + k])
                            n += k
                            if name != "uneven" or n == T:
                                continue
                            assert n in bb.ENDS
                            for s, st in enumerate(ss):
                                total += 1
                                if not prefix_ok(m.V, c.name, s, beam, n):      # (decided on the host, from the twin alone)
                                    continue
                                compared += 1
                                ref, bound = reference(m.V, configs[s], c.name, s, beam, n)
                                pick = ref["alts"][0]
                                assert (st.tokens, st.timestamps) == (pick["tokens"], pick["timestamps"]), (what, s, n)
                                worst = max(worst, abs(st.score - pick["score"]) / bound)
                                assert abs(st.score - pick["score"]) <= bound, (what, s, n, st.score, pick["score"], bound)
                    p1, h1 = launch_counts()
                    assert n == T and p1 == p0 and h1 > h0, (what, "the biased kernels did not run", p1 - p0, h1 - h0)
                    for s, st in enumerate(ss):
                        ref, bound = reference(m.V, configs[s], c.name, s, beam)
                        alts = st.alternatives()
                        assert [(a["tokens"], a["timestamps"]) for a in alts] == [(a["tokens"], a["timestamps"]) for a in ref["alts"][:8]], (what, s)
                        for a, w in zip(alts, ref["alts"]):
                            assert abs(a["score"] - w["score"]) <= bound, (what, s, a["score"], w["score"], bound)
                        same_bits([alts], [off[s]])
                        assert st.tokens == off[s][0]["tokens"] and st.timestamps == off[s][0]["timestamps"], (what, s)
                        assert np.float32(st.score) == np.float32(off[s][0]["score"]), (what, s, st.score, off[s][0]["score"])
                        st.close()
    finally:
        table.set_hotwords(None)
        table.set_ngram_lm(None)
        table.set_nbest(1)
        table.set_decoding_method("greedy_search")
    print(f"V={m.V} beam={beam}: {compared} of {total} inner chunk ends compared with the twin's pick on the prefix, worst score diff {worst:.3f} of its bound")
    assert compared > 0
