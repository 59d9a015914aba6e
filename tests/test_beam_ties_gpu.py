"""The modified beam search (csrc/beam.hip) on exact ties, merges and the beam cut: one model per V in {200, 400, 600, 1021, 1029} -- one
256-column chunk with NE = 8 and out-of-range elements; two chunks (the two-slab exchange at beam <= 4, the two-chunk single pass under
K2HIP_BEAM_PARTS=1); NE = 16 in three passes; NE = 16 with a padded tail; the re-reading path with its excl list -- at beams 1, 2, 4, 5
and 8 (5: k_beam_loop<2> with a beam that is no power of two).  Inputs, float64 reference, bound and the promises that make the
comparison exact: tests/beam_cases.py, checked on the host by tests/test_beam_cases_ref.py.

Held in every form: tokens, timestamps, number and ORDER of the alternatives equal the float64 twin's exactly -- no excuse, no margin
argument: every decision is an exact tie or 10 x the bound wide -- scores within beam_cases.score_bound and token log-probs within
beam_cases.noise_terms (not the 2e-3 other tests allow), entry 0 of the N-best equal to the plain call bit for bit, and the forms that
run k_beam_loop (default, one workgroup per stream, hypotheses in device memory, the one-slab repeat) bit-equal among themselves.

FORMS: "loop" (default: two slabs at V = 400 and beam <= 4), "parts1" (K2HIP_BEAM_PARTS=1), "hyp_global" (K2HIP_BEAM_HYP_GLOBAL),
"launches" (K2HIP_BEAM_LAUNCHES: k_beam_step, logits from the GEMM), "no_table" (a second model object loaded and run with
K2HIP_DECODER_TABLE_MB=0, which has only the launch form: the engine reads the switch when a search first asks for the table, so it
stays 0 around every call on that object, and k2hip_debug_decoder_table_check shows that it never got one), "repeat" (K2HIP_TEST_GREEDY_TIMEOUT: the two-slab launch reports a timeout
and the one-slab repeat's output is returned; k2hip_debug_search_retries moves by one per call exactly where two slabs run).

Every form is called twice in a row on one handle, plain and then with nbest = 8.  That order found a sizing bug: the
arena's counting pass saw null N-best pointers and left the token log-prob array out, so the second call ran out of arena wherever
the first call's 12.5 % slack did not cover it -- the launch form at V = 600, beam 4 and 5, the resumed search at V >= 1021, beam 8."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import beam_cases as bc
from test_search_ties_gpu import switch

pytestmark = pytest.mark.gpu

K_BEAM_LOOP = ("loop", "parts1", "hyp_global", "repeat")
SWITCHES = {"loop": None, "parts1": "K2HIP_BEAM_PARTS", "hyp_global": "K2HIP_BEAM_HYP_GLOBAL", "launches": "K2HIP_BEAM_LAUNCHES", "no_table": None,
            "repeat": "K2HIP_TEST_GREEDY_TIMEOUT"}


@functools.lru_cache(maxsize=None)
def built(V):
    return bc.build(V)


@functools.lru_cache(maxsize=None)
def reference(V, case, stream, beam):
    """(float64 twin's result, score bound) -- computed once, shared by every test of the module"""
    m = built(V)
    c = next(x for x in m.cases if x.name == case)
    ref = bc.twin(m.W, m.b, c.enc[stream], beam)
    return ref, bc.score_bound(m.W, m.b, ref, c.enc.shape[1])


@pytest.fixture(scope="module", params=bc.VS, ids=lambda V: f"V{V}")
def rig(request, tmp_path_factory):
    """the V model twice: with the all-contexts decoder table (the one-kernel forms), and loaded without it"""
    from k2transducerasr_amd import Model
    m = built(request.param)
    path = str(tmp_path_factory.mktemp("beam_ties") / f"v{m.V}.k2w")
    m.write(path)
    table = Model(path, 0)
    with switch("K2HIP_DECODER_TABLE_MB", 0, 1024):
        bare = Model(path, 0)
        assert table_rows(bare) == 0
    assert table_rows(table) == (m.V + 1) * m.V, "the one-kernel forms need the all-contexts decoder table"
    yield m, table, bare
    with switch("K2HIP_DECODER_TABLE_MB", 0, 1024):
        assert table_rows(bare) == 0, "the no_table form ran with a table"
    table.close()
    bare.close()


def table_rows(model):
    """rows of the model's all-contexts decoder table (0: none).  The check itself asks for the table: on the bare model only under
    K2HIP_DECODER_TABLE_MB=0."""
    from k2transducerasr_amd import load_library
    L = load_library()
    L.k2hip_debug_decoder_table_check.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    rows, bad = C.c_int64(-1), C.c_int64(-1)
    assert L.k2hip_debug_decoder_table_check(model.handle, 4, 7, C.byref(rows), C.byref(bad)) == 0
    assert bad.value == 0
    return rows.value


def retries(model):
    from k2transducerasr_amd import load_library
    L = load_library()
    L.k2hip_debug_search_retries.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    n = C.c_int32(-1)
    assert L.k2hip_debug_search_retries(model.handle, C.byref(n)) == 0
    return n.value


def launch_counts():
    from k2transducerasr_amd import load_library
    L = load_library()
    L.k2hip_debug_beam_launch_counts.argtypes = [C.POINTER(C.c_int64)] * 2
    p, h = C.c_int64(-1), C.c_int64(-1)
    assert L.k2hip_debug_beam_launch_counts(C.byref(p), C.byref(h)) == 0
    return p.value, h.value


def forms_for(V, beam):
    two_slabs = V == 400 and beam <= 4
    return ("loop", "parts1", "hyp_global", "launches", "no_table") + (("repeat",) if two_slabs else ())


def run_form(form, table, bare, enc, beam):
    """(plain results, plain scores, N-best lists) of one form"""
    model = bare if form == "no_table" else table
    sw = SWITCHES[form]

    def both():
        plain, psc = model.beam_search(enc, beam, want_scores=True)
        return plain, psc, model.beam_search(enc, beam, nbest=8)

    if form == "no_table":
        with switch("K2HIP_DECODER_TABLE_MB", 0, 1024):
            return both()
    with switch(sw, 1) if sw else contextlib.nullcontext():
        return both()


def same_bits(a, b):
    """two N-best lists of a batch, bit for bit"""
    assert [len(x) for x in a] == [len(x) for x in b]
    for xa, xb in zip(a, b):
        for g, w in zip(xa, xb):
            assert (g["tokens"], g["timestamps"]) == (w["tokens"], w["timestamps"])
            assert np.float32(g["score"]) == np.float32(w["score"]), (g["score"], w["score"])
            assert np.array_equal(g["token_log_probs"], w["token_log_probs"])


def against_twin(m, case, beam, alts, what, worst):
    """every stream's alternatives against the float64 twin: content and order exact, numbers within the derived bounds"""
    e_u = bc.noise_terms(m.W, m.b)[0]
    for s, got in enumerate(alts):
        ref, bound = reference(m.V, case, s, beam)
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


@pytest.mark.parametrize("beam", bc.BEAMS)
def test_every_form_returns_the_float64_order(rig, beam):
    m, table, bare = rig
    worst = [0.0, 0.0, 0.0]
    for c in m.cases:
        out = {}
        for form in forms_for(m.V, beam):
            r0 = retries(table)
            plain, psc, alts = out[form] = run_form(form, table, bare, c.enc, beam)
            what = f"V={m.V} beam={beam} {c.name} {form}"
            # the one-slab repeat ran exactly where two slabs run: once for the plain call, once for the N-best call
            assert retries(table) - r0 == (2 if form == "repeat" else 0), (what, retries(table) - r0)
            against_twin(m, c.name, beam, alts, what, worst)
            for s, a in enumerate(alts):      # entry 0 is the plain call's result, bit for bit
                assert (a[0]["tokens"], a[0]["timestamps"]) == plain[s], (what, s)
                assert np.float32(a[0]["score"]) == psc[s], (what, s)
        for form in K_BEAM_LOOP[1:]:
            if form in out:
                assert out[form][0] == out["loop"][0] and out[form][1].tobytes() == out["loop"][1].tobytes(), (m.V, beam, c.name, form)
                same_bits(out[form][2], out["loop"][2])
        if m.V != 400 or beam > 4:
            # no two-slab launch at this shape: the timeout hook finds nothing to repeat
            r0 = retries(table)
            with switch("K2HIP_TEST_GREEDY_TIMEOUT", 1):
                again, asc = table.beam_search(c.enc, beam, want_scores=True)
            assert retries(table) == r0, (m.V, beam, c.name)
            assert again == out["loop"][0] and asc.tobytes() == out["loop"][1].tobytes()
    bound = max(reference(m.V, c.name, s, beam)[1] for c in m.cases for s in range(c.enc.shape[0]))
    print(f"V={m.V} beam={beam}: worst score diff {worst[0]:.3g} ({worst[2]:.2f} of its bound; largest bound {bound:.3g}), "
          f"worst token log-prob diff {worst[1]:.3g} (bound {bc.noise_terms(m.W, m.b)[0]:.3g})")


@pytest.mark.parametrize("beam", bc.BEAMS)
def test_the_biased_instantiations_alone(rig, beam):
    """k_beam_loop<.., true> / k_beam_step<true> with a hotword graph that can never fire: its only phrase is a token the twin shows is
    never selected.  Bit-equal to the plain run of the same form, and the launch counter shows that the biased kernels ran."""
    from k2transducerasr_amd import Hotwords
    m, table, bare = rig
    tok = m.V - 2
    for c in m.cases:
        for s in range(c.enc.shape[0]):
            assert tok not in reference(m.V, c.name, s, beam)[0]["selected"]
    hw = Hotwords([[tok]], 1.5, m.V)
    try:
        for c in m.cases:
            for form in forms_for(m.V, beam):
                model = bare if form == "no_table" else table
                plain, psc, alts = run_form(form, table, bare, c.enc, beam)
                p0, h0 = launch_counts()
                model.set_hotwords(hw)
                try:
                    bplain, bsc, balts = run_form(form, table, bare, c.enc, beam)
                finally:
                    model.set_hotwords(None)
                p1, h1 = launch_counts()
                assert (p1 - p0, h1 - h0) == (0, 2), (m.V, beam, c.name, form, p1 - p0, h1 - h0)
                assert bplain == plain and bsc.tobytes() == psc.tobytes(), (m.V, beam, c.name, form)
                same_bits(balts, alts)
    finally:
        hw.close()


def splits(T):
    return {"ones": [1] * T, "uneven": [3, 1, 5, T - 9], "whole": [T]}


@pytest.mark.parametrize("beam", bc.BEAMS)
def test_the_resumed_search_ends_where_the_offline_call_does(rig, beam):
    """BeamStream.search_chunk over the same frames in chunks of one frame, in an uneven split and as one chunk: after the last chunk
    tokens, timestamps, score and alternatives are the offline call's, order included -- exactly tied candidates of different saved
    hypotheses go through the relation-table merge."""
    from k2transducerasr_amd import BeamStream
    m, table, _ = rig
    table.set_decoding_method("modified_beam_search", beam)
    table.set_nbest(8)
    try:
        for c in m.cases:
            B, T, _ = c.enc.shape
            for form in ("loop", "launches"):
                sw = SWITCHES[form]
                for name, chunks in splits(T).items():
                    what = f"V={m.V} beam={beam} {c.name} {form} {name}"
                    with switch(sw, 1) if sw else contextlib.nullcontext():
                        off = table.beam_search(c.enc, beam, nbest=8)
                        ss = [BeamStream(table, beam) for _ in range(B)]
                        n = 0
                        for k in chunks:
                            BeamStream.search_chunk(ss, c.enc[:, n: n + k])
                            n += k
                    assert n == T
                    for s, st in enumerate(ss):
                        ref, bound = reference(m.V, c.name, s, beam)
                        alts = st.alternatives()
                        assert [(a["tokens"], a["timestamps"]) for a in alts] == [(a["tokens"], a["timestamps"]) for a in ref["alts"][:8]], (what, s)
                        same_bits([alts], [off[s]])
                        assert st.tokens == off[s][0]["tokens"] and st.timestamps == off[s][0]["timestamps"], (what, s)
                        assert np.float32(st.score) == np.float32(off[s][0]["score"]), (what, s, st.score, off[s][0]["score"])
                        st.close()
    finally:
        table.set_nbest(1)
        table.set_decoding_method("greedy_search")
