"""Hotword and n-gram LM biasing of the streaming CTC prefix beam search on the GPU: csrc/ctc_prefix.hip k_ctc_prefix<true, true> through
the debug op "ctc_prefix_resume_bias", a Python mirror of the host class (tests/ctc_prefix_stream_bias_twin.BiasHostCarry) carrying the
slots and their (ctx, hs, ls) between calls.

The property: after any sequence of chunk calls a biased stream holds what the offline biased kernel ("ctc_prefix_beam_bias", nbest = beam)
holds after one run over all frames the stream has been given -- the entries in final order with tokens, absolute timestamps, token
log-probs and the float32 final, BIT FOR BIT: one per-frame source, and ctx is a function of the token sequence alone.  The carried words
the offline op does not return (pb, pnb, tot, ctx, hs, ls by slot) are compared bit for bit between different chunkings of one row (a
single chunk among them on the short rows), hs / ls exactly and ctx within REL against the float64 walk of the slot's tokens.
Against the float64 twin at chunk ends: lists and order exact where the twin's consecutive finals clear the group's G
(tests/ctc_prefix_bias_cases.py; tests/test_ctc_prefix_stream_bias.py counts the ends below it), final within REL = 1e-5 relative to
max(1, |value|).  Outputs are pre-filled with -7.
Above the kernel: four CtcPrefixStreams with different tables in one k2hip_ctc_prefix_beam_search_chunk, and three OnlineRecognizer
streams with ctc_prefix_biasing=True, after every call / tick bit for bit the offline biased search (k2hip_set_ctc_prefix_biasing with the
stream's own tables) over the frames so far; the setters' and the LM rule's refusals leave every stream as it was."""
import ctypes as C

import numpy as np
import pytest

import ctc_prefix_bias_cases as bc
import ctc_prefix_cases as base
import ctc_prefix_stream_bias_cases as sbc
import ctc_prefix_stream_cases as scases
from ctc_prefix_bias_twin import dense_graph, lm_tables, walk
from ctc_prefix_stream_bias_twin import BiasHostCarry, BiasStreamTwin, SideLayout
from ctc_prefix_stream_twin import HostCarry, Layout
from hotword_twin import TwinGraph

pytestmark = pytest.mark.gpu

REL = 1e-5
WORDS = ("pb", "pnb", "tot", "ctx", "hs", "ls", "tokens", "timestamps", "token_log_probs")


def rel(got, want):
    return abs(float(got) - want) / max(1.0, abs(want))


def f32(bits):
    return float(np.int32(bits).view(np.float32))


@pytest.fixture(scope="module")
def hip_ctc(tmp_path_factory):
    from k2transducerasr_amd import Model
    from k2transducerasr_amd.synth import write_synthetic_model
    p = str(tmp_path_factory.mktemp("ctcprefixstreambias") / "ctc_tiny.k2w")
    write_synthetic_model(p, "zipformer2-ctc-tiny-test")
    m = Model(p, 0)
    assert m.vocab_size == 37
    return m


def _debug_op(model, name, ints, bufs, out_from):
    """returns (rc, message); out_from: the indices of the output buffers"""
    from k2transducerasr_amd import load_library
    L = load_library()
    L.k2hip_debug_op_run.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                     C.c_int32, C.c_uint32]
    n = len(bufs)
    ptrs = (C.c_void_p * n)(*[b.ctypes.data if b is not None else None for b in bufs])
    sizes = (C.c_int64 * n)(*[b.nbytes if b is not None else 0 for b in bufs])
    ia = (C.c_int64 * len(ints))(*ints)
    rc = L.k2hip_debug_op_run(model.handle, name, ia, len(ints), ptrs, sizes, n, sum(1 << k for k in out_from))
    return rc, L.k2hip_last_error()


def tables_of(graph, lm):
    """the nine table buffers and (S, S_lm, A, start); a missing half is None"""
    hw = [None, None, None]
    S = S_lm = A = start = 0
    if graph is not None:
        hw = [np.ascontiguousarray(x) for x in dense_graph(graph)]
        S = hw[0].shape[0]
    lmb = [None] * 6
    if lm is not None:
        t = lm_tables(lm)
        lmb = [t["states"], t["arc_tok"] if len(t["arc_tok"]) else None, t["arc_lp"] if len(t["arc_lp"]) else None,
               t["arc_next"] if len(t["arc_next"]) else None, t["uni_lp"], t["uni_next"]]
        S_lm, A, start = t["states"].shape[0], len(t["arc_tok"]), t["start"]
    return hw + lmb, (S, S_lm, A, start)


def run_offline_bias(model, lp, n_frames, beam, max_tokens, tabs, dims):
    """the parent's kernel: "ctc_prefix_beam_bias" at nbest = beam"""
    lp = np.ascontiguousarray(lp, np.float32)
    R, Tp, V = lp.shape
    tok, ts = np.full((R, beam, max_tokens), -7, np.int64), np.full((R, beam, max_tokens), -7, np.int32)
    yp, n = np.full((R, beam, max_tokens), -7, np.float32), np.full((R, beam), -7, np.int32)
    nh, sc, flag = np.full(R, -7, np.int32), np.full((R, beam), -7, np.float32), np.full(1, -7, np.int32)
    bufs = [lp, np.ascontiguousarray(n_frames, np.int32), tok, ts, yp, n, nh, sc, flag] + list(tabs)
    rc, msg = _debug_op(model, b"ctc_prefix_beam_bias", (R, Tp, V, beam, beam, max_tokens, *dims), bufs, range(2, 9))
    assert rc == 0 and flag[0] == 0, (rc, msg)
    return dict(tokens=tok, timestamps=ts, token_log_probs=yp, n_tokens=n, n_hyps=nh, scores=sc)


def run_resume_plain(model, lp, n_frames, beam, in_blocks):
    lp = np.ascontiguousarray(lp, np.float32)
    B, Tc, V = lp.shape
    out, status = np.full((B, Layout(beam, Tc).out_ints), -7, np.int32), np.full(1, -7, np.int32)
    rc, msg = _debug_op(model, b"ctc_prefix_resume", (B, Tc, V, beam), [lp, np.ascontiguousarray(n_frames, np.int32), np.ascontiguousarray(in_blocks, np.int32), out, status], (3, 4))
    assert rc == 0 and status[0] == 0, (rc, msg)
    return out


def run_resume_bias(model, lp, n_frames, beam, in_blocks, side_in, tabs, dims, row_graph, expect_ok=True):
    """the new instantiation alone; returns (rc, out [B][out_ints], side out [B][5K], status)"""
    lp = np.ascontiguousarray(lp, np.float32)
    B, Tc, V = lp.shape
    L, SL = Layout(beam, Tc), SideLayout(beam)
    inb, sin = np.ascontiguousarray(in_blocks, np.int32), np.ascontiguousarray(side_in, np.int32)
    assert inb.shape == (B, L.in_ints) and sin.shape == (B, SL.in_ints)
    out, sout, status = np.full((B, L.out_ints), -7, np.int32), np.full((B, SL.out_ints), -7, np.int32), np.full(1, -7, np.int32)
    bufs = [lp, np.ascontiguousarray(n_frames, np.int32), inb, out, status, sin, sout] + list(tabs) + [np.ascontiguousarray(row_graph, np.int32)]
    rc, msg = _debug_op(model, b"ctc_prefix_resume_bias", (B, Tc, V, beam, *dims), bufs, (3, 4, 6))
    if expect_ok:
        assert rc == 0 and status[0] == 0, (rc, msg, status)
    return rc, out, sout, status


def same_as_offline(carry, off, r):
    """a carried stream's entries in final order against row r of the offline biased op: everything bit for bit"""
    ent = carry.entries()
    assert off["n_hyps"][r] == len(ent), (r, off["n_hyps"][r], len(ent))
    for i, s in enumerate(ent):
        n = len(s["tokens"])
        assert off["n_tokens"][r, i] == n, (r, i, off["n_tokens"][r, i], n)
        assert off["tokens"][r, i, :n].tolist() == list(s["tokens"]), (r, i, off["tokens"][r, i, :n].tolist(), s["tokens"])
        assert off["timestamps"][r, i, :n].tolist() == list(s["timestamps"]), (r, i)
        assert off["token_log_probs"][r, i, :n].view(np.int32).tolist() == list(s["token_log_probs"]), (r, i)
        assert int(off["scores"][r, i].view(np.int32)) == s["final"], (r, i, off["scores"][r, i], f32(s["final"]))


def stream_rows(model, rows, beam, Tc, graph, lm, after_chunk=None, offline=True):
    """rows: [(lp [T][V], chunk lengths, reads the graph, runs the LM)], one V, one table set.  Every row is a stream carried by a
    BiasHostCarry through the new kernel; all streams that still have frames share a call (rows leave the batch as they end), per-row
    n_frames.  After EVERY step each stream that moved equals the offline biased op over its frames so far, called once per table
    combination present.  after_chunk(row index, carry): a hook for further checks."""
    tabs, dims = tables_of(graph, lm)
    S, S_lm, _, start = dims
    V = rows[0][0].shape[1]
    Tmax = max(r[0].shape[0] for r in rows)
    whole = np.full((len(rows), Tmax, V), 0.25, np.float32)
    for r, (lp, ch, _, _) in enumerate(rows):
        assert sum(ch) == lp.shape[0] and max(ch) <= Tc and min(ch) >= 1
        whole[r, : lp.shape[0]] = lp
    carries = [BiasHostCarry(beam, S if g else 0, S_lm if m else 0, start, m) for _, _, g, m in rows]
    L, SL = Layout(beam, Tc), SideLayout(beam)
    step = 0
    while True:
        active = [r for r, row in enumerate(rows) if step < len(row[1])]
        if not active:
            break
        lp = np.full((len(active), Tc, V), 0.25, np.float32)
        nf = np.zeros(len(active), np.int32)
        for b, r in enumerate(active):
            n = rows[r][1][step]
            t0 = carries[r].frames
            lp[b, :n] = rows[r][0][t0: t0 + n]
            nf[b] = n
        _, out, sout, _ = run_resume_bias(model, lp, nf, beam, np.stack([carries[r].fill_in(Tc) for r in active]),
                                          np.stack([carries[r].fill_side_in() for r in active]), tabs, dims, [int(rows[r][2]) for r in active])
        for b, r in enumerate(active):
            carries[r].apply(out[b], sout[b], Tc, int(nf[b]))
            n = len(carries[r].slots)
            assert np.all(out[b, L.out_org + n: L.out_org + beam] == -7) and np.all(out[b, L.out_ys + n * Tc: L.out_ys + beam * Tc] == -7), (r, step)
            for o in (SL.out_ctx, SL.out_hs, SL.out_ls, SL.out_fin, SL.out_ord):
                assert np.all(sout[b, o + n: o + beam] == -7), (r, step, o)
        if offline:
            for g, m in sorted({(rows[r][2], rows[r][3]) for r in active}):
                grp = [r for r in active if (rows[r][2], rows[r][3]) == (g, m)]
                t2, d2 = tables_of(graph if g else None, lm if m else None)
                off = run_offline_bias(model, whole[grp], np.array([carries[r].frames for r in grp], np.int32), beam, Tmax, t2, d2)
                for b, r in enumerate(grp):
                    same_as_offline(carries[r], off, b)
        for r in active:
            if after_chunk:
                after_chunk(r, carries[r])
        step += 1
    for r, row in enumerate(rows):
        assert carries[r].frames == row[0].shape[0]
    return carries


def same_words(a, b):
    """two carries of one row: every carried word of every slot, the float32 ones by their bits"""
    assert len(a.slots) == len(b.slots) and a.fin == b.fin and a.ord == b.ord
    for x, y in zip(a.slots, b.slots):
        for k in WORDS:
            assert x[k] == y[k], (k, x[k], y[k])


def against_walk(carry, graph, lm):
    """hs / ls exactly and ctx within REL: functions of the slot's token sequence alone"""
    for s in carry.slots:
        if f32(s["tot"]) == -np.inf:
            continue
        ctx, hs, ls = walk(s["tokens"], graph, lm)
        assert (s["hs"], s["ls"]) == (hs if graph is not None else 0, ls if lm is not None else 0), (s["tokens"], s["hs"], hs, s["ls"], ls)
        assert rel(f32(s["ctx"]), float(ctx)) <= REL, (s["tokens"], f32(s["ctx"]), ctx)


class Twin64:
    """the float64 chunked twin beside a carry, compared at chunk ends; counts the ends left out of the order assertion"""

    def __init__(self, rows, beam, graph, lm, G):
        self.rows, self.G, self.worst, self.ends, self.left_out = rows, G, 0.0, 0, 0
        self.tw = [BiasStreamTwin(beam, graph if g else None, lm if m else None) for _, _, g, m in rows]

    def __call__(self, r, carry):
        lp, _, _, _ = self.rows[r]
        tw = self.tw[r]
        tw.chunk(lp[tw.frames: carry.frames])
        assert tw.frames == carry.frames
        want, got = tw.entries(), carry.entries()
        self.ends += 1
        if min(tw.final_gaps() + [np.inf]) < self.G:        # the bit equality with the offline op stays; only this order assertion is left out
            self.left_out += 1
            return
        assert len(got) == len(want), (r, carry.frames)
        for g, w in zip(got, want):
            assert list(g["tokens"]) == w["tokens"] and list(g["timestamps"]) == w["timestamps"] and g["slot"] == w["slot"], (r, carry.frames, g["tokens"], w["tokens"])
            assert [f32(b) for b in g["token_log_probs"]] == [lp[t, v] for t, v in zip(w["timestamps"], w["tokens"])]
            if w["score"] == -np.inf:
                assert f32(g["final"]) == -np.inf
            else:
                self.worst = max(self.worst, rel(f32(g["final"]), w["score"]))
                assert rel(f32(g["final"]), w["score"]) <= REL, (r, carry.frames, f32(g["final"]), w["score"])


# ---- 1. the kernel alone against the offline biased kernel ---------------------------------------------------------------------------
def test_flip_row_in_chunks_of_one(hip_ctc):
    """V = 4, T = 3, beam 2: per step the literal results; the slots stay in selection order with the pending bonus in ctx; beside it the
    same row with null tables in the same call (the plain result, [b]) and the row in one chunk"""
    lp, graph = bc.FLIP_ROWS, bc.flip_graph()
    seen = {0: [], 1: [], 2: []}
    rows = [(lp, [1, 1, 1], True, False), (lp, [1, 1, 1], False, False), (lp, [3], True, False), (lp, [1, 2], True, False), (lp, [2, 1], True, False)]
    carries = stream_rows(hip_ctc, rows, bc.FLIP_BEAM, 3, graph, None,
                          lambda r, c: seen[r].append((list(c.entries()[0]["tokens"]), f32(c.entries()[0]["final"]), [dict(s) for s in c.slots])) if r < 3 else None)
    assert [(t, f) for t, f, _ in seen[0]] == sbc.FLIP_STEPS
    first = seen[0][0][2]
    assert [dict(tokens=list(s["tokens"]), hs=s["hs"], ctx=f32(s["ctx"])) for s in first] == sbc.FLIP_SLOTS_AFTER_FRAME_0
    assert seen[1][-1][0] == bc.FLIP_UNBIASED[0] and all(s["hs"] == 0 and s["ctx"] == 0 for s in carries[1].slots)
    assert seen[2] and (seen[2][0][0], seen[2][0][1]) == (bc.FLIP_BIASED[0], bc.FLIP_BIASED[2])
    for r in (0, 3, 4):
        same_words(carries[r], carries[2])


@pytest.mark.parametrize("kind", bc.KINDS)
def test_respelled_row_at_every_split(hip_ctc, kind):
    """V = 3, T = 10, beam 4, RESPELLED_PHRASES and the small LM: the nine two-chunk splits, chunks of 1 / 2 / 3 and one chunk, one batch"""
    row, beam = base.respelled_row(), base.RESPELLED_BEAM
    graph, lm = bc.pick(kind, bc.small_graph(bc.RESPELLED_PHRASES), bc.small_lm())
    chunkings = [ch for ch in scases.respelled_chunkings() if max(ch) != 4 or len(ch) == 2] + [[base.RESPELLED_T]]
    assert len(chunkings) == 13
    rows = [(row, ch, graph is not None, lm is not None) for ch in chunkings]
    tw = Twin64(rows, beam, graph, lm, bc.G_SMALL)
    carries = stream_rows(hip_ctc, rows, beam, base.RESPELLED_T, graph, lm, tw)
    for c in carries:
        same_words(c, carries[-1])
        against_walk(c, graph, lm)
        toks = [s["tokens"] for s in c.slots]
        assert len(set(toks)) == len(toks) == beam
    assert tw.left_out == 0
    print(f"re-spelled {kind}: worst relative difference of final against the float64 twin {tw.worst:.3g} (bound {REL:g})")


@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("beam", base.RAGGED_BEAMS)
def test_ragged_rows_leave_the_batch_as_they_end(hip_ctc, beam, kind):
    """V = 37, frames 1, 2, 7, 70, 70, 70 (a row with -inf cells, a row that is -inf everywhere) in chunks of 16 and of 7, per-row n_frames"""
    lp, nf = base.ragged_rows()
    graph, lm = bc.pick(kind, *bc.ragged_tables())
    ends = []
    for c in (sbc.CHUNK, sbc.SHORT_CHUNK):
        rows = [(lp[r, : nf[r]], scases.uniform(int(nf[r]), c), graph is not None, lm is not None) for r in range(len(nf))]
        tw = Twin64(rows, beam, graph, lm, bc.G_RAGGED)
        ends.append(stream_rows(hip_ctc, rows, beam, c, graph, lm, tw))
        assert tw.left_out <= 1, (c, tw.left_out, tw.ends)
        print(f"ragged {kind} beam {beam} chunks of {c}: worst relative difference of final {tw.worst:.3g} (bound {REL:g}); "
              f"{tw.left_out} of {tw.ends} chunk ends below G")
    for a, b in zip(*ends):
        same_words(a, b)
        against_walk(a, graph, lm)
    c = ends[0][base.RAGGED_ALL_INF_ROW]
    assert len(c.slots) == 1 and c.slots[0]["tokens"] == () and f32(c.fin[0]) == -np.inf


@pytest.mark.parametrize("kind", bc.KINDS)
def test_wide_vocabulary(hip_ctc, kind):
    """V = 600, T = 70, beam 4: several columns per thread; the LM's hub state has more than 64 arcs, so the walk's narrowing runs"""
    lp = base.wide_row()
    graph, lm = bc.pick(kind, *bc.wide_tables())
    if lm is not None:
        st = lm_tables(lm)["states"]
        assert (st[:, 1] - st[:, 0]).max() > 64
    rows = [(lp, scases.uniform(base.WIDE_T, c), graph is not None, lm is not None) for c in (sbc.CHUNK, sbc.SHORT_CHUNK)]
    tw = Twin64(rows, 4, graph, lm, bc.G_WIDE)
    carries = stream_rows(hip_ctc, rows, 4, sbc.CHUNK, graph, lm, tw)
    same_words(carries[0], carries[1])
    against_walk(carries[0], graph, lm)
    assert tw.left_out <= 1
    print(f"wide {kind}: worst relative difference of final {tw.worst:.3g} (bound {REL:g}); {tw.left_out} of {tw.ends} chunk ends below G")


@pytest.mark.parametrize("kind", bc.KINDS)
def test_long_histories(hip_ctc, kind):
    """V = 37, T = 300, beam 4, chunks of 16: 19 chunks, a pending match at every boundary of the row with both tables"""
    lp = base.long_row()
    graph, lm = bc.pick(kind, *bc.long_tables())
    rows = [(lp, scases.uniform(base.LONG_T, sbc.CHUNK), graph is not None, lm is not None)]
    tw = Twin64(rows, base.LONG_BEAM, graph, lm, bc.G_LONG)
    pending = []
    pend = None if graph is None else dense_graph(graph)[2]

    def after(r, c):
        tw(r, c)
        if pend is not None and c.frames < base.LONG_T:
            pending.append(any(pend[s["hs"]] != 0 for s in c.slots))

    carries = stream_rows(hip_ctc, rows, base.LONG_BEAM, sbc.CHUNK, graph, lm, after)
    against_walk(carries[0], graph, lm)
    assert len(carries[0].entries()[0]["tokens"]) > 100 and tw.left_out <= 1
    if kind == "both":
        assert len(pending) == 18 and all(pending)
    print(f"long {kind}: worst relative difference of final {tw.worst:.3g} (bound {REL:g}); {tw.left_out} of {tw.ends} chunk ends below G")


# ---- 2. null tables: the plain resumed kernel, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("beam", base.RAGGED_BEAMS)
def test_null_and_empty_tables_are_the_plain_resumed_kernel(hip_ctc, beam):
    """null tables for every row, an empty graph, a graph at score 0 and a zero-weight LM: every word of the plain out block equals
    "ctc_prefix_resume", chunk after chunk; ctx stays 0 and fin equals tot"""
    lp, nf = base.ragged_rows()
    Tc = sbc.CHUNK
    empty_lm = bc.TwinLm([((-1,), -99.0, 0.0), ((-3,), -7.5, 0.0)], 37).scaled(0.0)
    configs = [(None, None), (TwinGraph([], bc.SCORE, 37), None), (TwinGraph([[5, 7], [9]], 0.0, 37), None), (TwinGraph([], bc.SCORE, 37), empty_lm)]
    plain = [HostCarry(beam) for _ in nf]
    biased = [[BiasHostCarry(beam, 0 if g is None else g.num_states, 0 if m is None else lm_tables(m)["states"].shape[0],
                             0 if m is None else m.start, m is not None) for _ in nf] for g, m in configs]
    L, SL = Layout(beam, Tc), SideLayout(beam)
    for step in range(5):
        active = [r for r in range(len(nf)) if plain[r].frames < nf[r]]
        n = np.array([min(Tc, nf[r] - plain[r].frames) for r in active], np.int32)
        x = np.full((len(active), Tc, 37), 0.25, np.float32)
        for b, r in enumerate(active):
            x[b, : n[b]] = lp[r, plain[r].frames: plain[r].frames + n[b]]
        want = run_resume_plain(hip_ctc, x, n, beam, np.stack([plain[r].fill_in(Tc) for r in active]))
        for (g, m), cs in zip(configs, biased):
            tabs, dims = tables_of(g, m)
            _, out, sout, _ = run_resume_bias(hip_ctc, x, n, beam, np.stack([cs[r].fill_in(Tc) for r in active]), np.stack([cs[r].fill_side_in() for r in active]),
                                              tabs, dims, [int(g is not None)] * len(active))
            assert out.tobytes() == want.tobytes(), (step, g is not None, m is not None)
            for b, r in enumerate(active):
                cs[r].apply(out[b], sout[b], Tc, int(n[b]))
                k = len(cs[r].slots)
                assert np.all(sout[b, SL.out_ctx: SL.out_ctx + k] == 0) and sout[b, SL.out_ord: SL.out_ord + k].tolist() == list(range(k))
                assert np.array_equal(sout[b, SL.out_fin: SL.out_fin + k], out[b, L.out_tot: L.out_tot + k])
        for b, r in enumerate(active):
            plain[r].apply_out(want[b], Tc, int(n[b]))
    assert all(plain[r].frames == nf[r] for r in range(len(nf)))


def test_an_unbiased_row_among_biased_neighbours(hip_ctc):
    """one call: graph and LM, graph only, LM only, neither.  The last equals its row of the plain op bit for bit at every step, each of
    the others the offline biased op with its own tables (stream_rows), and the biased ones do differ from the plain result"""
    lp, nf = base.ragged_rows()
    graph, lm = bc.ragged_tables()
    row, Tc, beam = lp[3, : nf[3]], sbc.CHUNK, 4
    chunks = scases.uniform(int(nf[3]), Tc)
    rows = [(row, chunks, True, True), (row, chunks, True, False), (row, chunks, False, True), (row, chunks, False, False)]
    plain = HostCarry(beam)
    outs = []

    def after(r, c):
        if r == 3:
            n = chunks[len(outs)]
            x = np.full((1, Tc, 37), 0.25, np.float32)
            x[0, :n] = row[plain.frames: plain.frames + n]
            out = run_resume_plain(hip_ctc, x, [n], beam, plain.fill_in(Tc)[None])
            plain.apply_out(out[0], Tc, n)
            outs.append(out)
            assert [(s["tokens"], s["timestamps"], s["token_log_probs"], s["pb"], s["pnb"], s["tot"]) for s in c.slots] == \
                   [(s["tokens"], s["timestamps"], s["token_log_probs"], s["pb"], s["pnb"], s["tot"]) for s in plain.slots]
            assert c.fin == [s["tot"] for s in plain.slots] and c.ord == list(range(len(c.slots)))

    carries = stream_rows(hip_ctc, rows, beam, Tc, graph, lm, after)
    assert len(outs) == len(chunks)
    for r in (0, 1, 2):
        assert [s["tokens"] for s in carries[r].slots] != [s["tokens"] for s in carries[3].slots] or carries[r].fin != carries[3].fin, r


# ---- 3. the host checks ------------------------------------------------------------------------------------------------------------------
def test_bad_side_blocks_and_tables_are_refused_before_any_launch(hip_ctc):
    """a side in block with hs or ls out of range, a flag without an LM, a row_graph without tables and each kind of bad table:
    K2HIP_ERR_INVALID from the host-side check, outputs untouched"""
    lp, nf = base.ragged_rows()
    graph, lm = bc.ragged_tables()
    tabs, dims = tables_of(graph, lm)
    S, S_lm, A, start = dims
    beam, Tc = 4, sbc.CHUNK
    SL = SideLayout(beam)
    x, n = lp[:, :Tc], np.minimum(nf, Tc).astype(np.int32)
    B = len(nf)
    inb = np.stack([HostCarry(beam).fill_in(Tc) for _ in range(B)])
    side = np.stack([BiasHostCarry(beam, S, S_lm, start, True).fill_side_in() for _ in range(B)])

    def refused(side=side, tabs=tabs, dims=dims, row_graph=None):
        rc, out, sout, status = run_resume_bias(hip_ctc, x, n, beam, inb, side, tabs, dims, [1] * B if row_graph is None else row_graph, expect_ok=False)
        assert rc == -1, rc
        assert np.all(out == -7) and np.all(sout == -7) and status[0] == -7

    for off, v in ((SL.in_hs + 1, S), (SL.in_hs, -1), (SL.in_ls + 2, S_lm), (SL.in_ls, -1), (0, 3)):
        bad = side.copy()
        bad[2, off] = v
        refused(side=bad)
    bad = side.copy()
    bad[1, SL.in_hs] = 1                                  # a row without a graph carries state 0 only
    refused(side=bad, row_graph=[1, 0] + [1] * (B - 2))
    refused(tabs=[None] * 3 + tabs[3:], dims=(0, S_lm, A, start))          # row_graph = 1 without hotword tables
    refused(tabs=tabs[:3] + [None] * 6, dims=(S, 0, 0, 0))                 # the LM flag without LM tables
    refused(row_graph=[2] + [1] * (B - 1))

    def with_table(i, idx, v):
        t = [None if b is None else b.copy() for b in tabs]
        t[i][idx] = v
        return t

    refused(tabs=with_table(0, (1, 5), S))                 # next out of range
    refused(tabs=with_table(3, (S_lm - 1, 1), A + 1))      # an arc range past A
    refused(tabs=with_table(3, (1, 2), S_lm))              # a back-off state out of range
    refused(tabs=with_table(6, 0, -1))                     # arc_next
    refused(tabs=with_table(8, 7, S_lm))                   # uni_next
    refused(dims=(S, S_lm, A, S_lm))                       # the start state
    refused(tabs=tabs[:2] + [None] + tabs[3:])             # an incomplete hotword group
    rc, _, _, status = run_resume_bias(hip_ctc, x, n, beam, inb, side, tabs, dims, [1] * B)
    assert rc == 0 and status[0] == 0


# ---- 4. the operator level -----------------------------------------------------------------------------------------------------------------
def same_alternatives(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert g["tokens"] == w["tokens"] and g["timestamps"] == w["timestamps"], (g, w)
        assert np.array_equal(np.asarray(g["token_log_probs"], np.float32).view(np.int32), np.asarray(w["token_log_probs"], np.float32).view(np.int32))
        assert np.float32(g["score"]).view(np.int32) == np.float32(w["score"]).view(np.int32), (g["score"], w["score"])


def snap(s):
    return (s.tokens, s.timestamps, s.num_frames, int(np.float32(s.score).view(np.int32)), [(x["tokens"], x["timestamps"]) for x in s.alternatives()])


def off_alternative_phrase(alts):
    """a window (two tokens, else one, else three) of a runner-up that the best alternative does not contain: biasing towards it can
    change the result"""
    best = alts[0]["tokens"]
    for n in (2, 1, 3):
        have = {tuple(best[i: i + n]) for i in range(len(best) - n + 1)}
        for a in alts[1:]:
            for i in range(len(a["tokens"]) - n + 1):
                w = tuple(a["tokens"][i: i + n])
                if w not in have and 2 not in w:
                    return list(w)
    return None


def legal(phrases):
    """the phrases in order, without duplicates and without a phrase that is a prefix of (or prefixed by) an earlier one"""
    out = []
    for p in phrases:
        if not any(p[: len(q)] == q[: len(p)] for q in out):
            out.append(list(p))
    return out


def test_operator_entry_four_streams_in_one_call(hip_ctc, utts):
    """the fixture batch's own log-probs (T' = 35) in chunks of 16: two streams with different graphs, one graph-free with the switch on,
    one with the switch off (its attached graph ignored), the model's LM set.  After every call each equals Model.ctc_prefix_beam_search
    with set_ctc_prefix_biasing(True) and that stream's tables over its frames so far, bit for bit at nbest = beam; then the argument
    rules, which leave every stream as it was"""
    from k2transducerasr_amd import Hotwords, K2HipError, NgramLm
    feats = [hip_ctc.fbank(u) for u in utts[:4]]
    lp = hip_ctc.encoder_proj(hip_ctc.pad_sequence(feats).reshape(4, -1, 80))
    V, beam, T = lp.shape[2], bc.FIXTURE_BEAM, lp.shape[1]
    phrases, entries = bc.fixture_entries(lp)
    plain = hip_ctc.ctc_prefix_beam_search(lp, beam=beam, nbest=beam)
    other = [p for p in (off_alternative_phrase(plain[b]) for b in range(4)) if p]
    assert len(phrases) >= 3 and other
    lists = [legal(phrases), legal(other + phrases[:1]), None, legal(phrases)]
    assert lists[0] != lists[1]
    hws = [Hotwords(p, bc.SCORE, V) if p else None for p in lists]
    ng = NgramLm(entries, V)
    streams = [hip_ctc.create_ctc_prefix_stream(beam, beam) for _ in range(4)]

    def offline(b, frames, on):
        hip_ctc.set_ctc_prefix_biasing(on)
        hip_ctc.set_hotwords(hws[b] if on else None)
        try:
            return hip_ctc.ctc_prefix_beam_search(np.ascontiguousarray(lp[b: b + 1, :frames]), beam=beam, nbest=beam)[0]
        finally:
            hip_ctc.set_hotwords(None)
            hip_ctc.set_ctc_prefix_biasing(False)

    try:
        hip_ctc.set_ngram_lm(ng, bc.LM_SCALE)
        for s, hw in zip(streams, hws):
            if hw is not None:
                s.set_hotwords(hw)
        for s in streams[:3]:
            s.set_biasing(True)
        moved = 0
        for t0 in range(0, T, scases.CHUNK):
            n = min(scases.CHUNK, T - t0)
            x = np.full((4, scases.CHUNK, V), 0.25, np.float32)
            x[:, :n] = lp[:, t0: t0 + n]
            hip_ctc.ctc_prefix_beam_search_chunk(streams, x, None if n == scases.CHUNK else np.full(4, n, np.int32))
            for b, s in enumerate(streams):
                want = offline(b, t0 + n, b < 3)
                same_alternatives(s.alternatives(), want)
                assert s.tokens == want[0]["tokens"] and s.timestamps == want[0]["timestamps"] and s.num_frames == t0 + n
                assert np.array_equal(np.asarray(s.token_log_probs(), np.float32).view(np.int32), np.asarray(want[0]["token_log_probs"], np.float32).view(np.int32))
                assert np.float32(s.score).view(np.int32) == np.float32(want[0]["score"]).view(np.int32)
                if b == 3:
                    same_alternatives(s.alternatives(), hip_ctc.ctc_prefix_beam_search(np.ascontiguousarray(lp[3:4, : t0 + n]), beam=beam, nbest=beam)[0])
                else:
                    moved += [a["tokens"] for a in s.alternatives()] != [a["tokens"] for a in hip_ctc.ctc_prefix_beam_search(
                        np.ascontiguousarray(lp[b: b + 1, : t0 + n]), beam=beam, nbest=beam)[0]] or s.score != plain[b][0]["score"]
        assert moved > 0
        # the argument rules
        before = [snap(s) for s in streams]
        for call in (lambda: streams[0].set_hotwords(None), lambda: streams[0].set_biasing(False), lambda: streams[3].set_biasing(True)):
            with pytest.raises(K2HipError) as e:
                call()
            assert e.value.code == -1 and "reset the stream first" in str(e.value), (e.value.code, str(e.value))
        hip_ctc.set_ngram_lm(None)                       # the LM changed mid-stream: a call naming a biased stream fails, no stream changes
        x = np.ascontiguousarray(lp[:, :scases.CHUNK])
        with pytest.raises(K2HipError) as e:
            hip_ctc.ctc_prefix_beam_search_chunk(streams, x)
        assert e.value.code == -1 and "reset the stream first" in str(e.value)
        assert [snap(s) for s in streams] == before
        hip_ctc.ctc_prefix_beam_search_chunk(streams[3:], x[3:])          # a stream with the switch off is not subject to the rule
        for s in streams:
            s.reset()                                    # keeps switch and graph; the LM now set (none) is the one the streams start with
        hip_ctc.ctc_prefix_beam_search_chunk(streams, x)
        hip_ctc.set_ctc_prefix_biasing(True)
        try:
            for b in range(3):
                hip_ctc.set_hotwords(hws[b])
                same_alternatives(streams[b].alternatives(), hip_ctc.ctc_prefix_beam_search(np.ascontiguousarray(x[b: b + 1]), beam=beam, nbest=beam)[0])
        finally:
            hip_ctc.set_hotwords(None)
            hip_ctc.set_ctc_prefix_biasing(False)
        with pytest.raises(K2HipError) as e:             # a graph of another vocabulary
            streams[0].reset()
            streams[0].set_hotwords(Hotwords([[3, 4]], bc.SCORE, V - 1))
        assert e.value.code == -1 and "vocab_size" in str(e.value)
    finally:
        hip_ctc.set_ngram_lm(None)
        hip_ctc.set_hotwords(None)
        hip_ctc.set_ctc_prefix_biasing(False)
        for s in streams:
            s.close()


# ---- 5. the recognizer level ---------------------------------------------------------------------------------------------------------------
def _run_recognizer(path, feats, phrase_lists, entries, biasing):
    """three streams (one joins a tick later) through OnlineRecognizer with ctc_prefix_beam = 4, nbest = 4 and the model's LM set; route B
    feeds the same features through the online encoder entry in the same batch composition.  After every tick each stream is compared
    with the offline search over route B's log-probs so far (biased with the stream's own list, or plain).  Returns the final results."""
    from k2transducerasr_amd import Hotwords, NgramLm, OnlineProj, OnlineRecognizer
    rec, proj = OnlineRecognizer(path), OnlineProj(path)
    streams, states = [], []
    try:
        V = rec.model.vocab_size
        if entries is not None:
            rec.model.set_ngram_lm(NgramLm(entries, V), bc.LM_SCALE)
        Tch, shift = rec.chunk_length, rec.shift_length
        streams = [rec.create_online_stream(hotwords=p, hotwords_score=bc.SCORE, ctc_prefix_beam=4, nbest=4, ctc_prefix_biasing=biasing) for p in phrase_lists]
        hws = [Hotwords(p, bc.SCORE, V) if p else None for p in phrase_lists]
        states = [proj.get_encoder_init_states() for _ in range(3)]
        pos, lps, fed, ticks = [0, 0, 0], [[], [], []], [False, False, False], 0
        while True:
            for i in range(3):
                if not fed[i] and (i < 2 or ticks >= 1):
                    streams[i].add_features(feats[i])
                    fed[i] = True
            ready = [i for i in range(3) if fed[i] and feats[i].shape[0] - pos[i] >= Tch]
            if not ready:
                break
            lens_before = [len(s.tokens) for s in streams]
            dec, nnew = rec.get_results(streams)
            assert [i for i in range(3) if dec[i]] == ready, (ticks, dec, ready)
            out = proj.encoder_proj(np.stack([feats[i][pos[i]: pos[i] + Tch] for i in ready]), [states[i] for i in ready])
            for b, i in enumerate(ready):
                lps[i].append(out[b])
                pos[i] += shift
                sofar = np.concatenate(lps[i])[None]
                rec.model.set_ctc_prefix_biasing(biasing)
                rec.model.set_hotwords(hws[i] if biasing else None)
                try:
                    want = rec.model.ctc_prefix_beam_search(sofar, beam=4, nbest=4)[0]
                finally:
                    rec.model.set_hotwords(None)
                    rec.model.set_ctc_prefix_biasing(False)
                s = streams[i]
                assert s.tokens == [0, 0] + want[0]["tokens"] and s.timestamps == want[0]["timestamps"], (ticks, i)
                assert nnew[i] == len(s.tokens) - lens_before[i]
                assert np.array_equal(s.token_log_probs().view(np.int32), np.asarray(want[0]["token_log_probs"], np.float32).view(np.int32)), (ticks, i)
                same_alternatives(s.alternatives(), want)
                assert np.float32(s.score).view(np.int32) == np.float32(want[0]["score"]).view(np.int32)
            ticks += 1
        assert ticks >= 3
        return [(list(s.tokens), list(s.timestamps), s.score) for s in streams], [np.concatenate(x) for x in lps]
    finally:
        for st in states:
            proj.free_states(st)
        for s in streams:
            s.close()
        rec.model.close()
        proj.model.close()


def test_recognizer_level_against_the_offline_biased_search(tmp_path):
    """zipformer2-ctc-streaming-tiny-test: two different phrase lists and one stream with none, the model LM set, ctc_prefix_biasing=True:
    after every tick tokens, absolute timestamps, token log-probs, alternatives and score equal the offline biased search over the online
    encoder's log-probs so far.  The same audio with ctc_prefix_biasing=False gives the unbiased results bit for bit (hotwords and LM
    ignored), and at least one stream's final tokens differ between the two runs."""
    from k2transducerasr_amd import K2HipError, Model, OnlineRecognizer
    from k2transducerasr_amd.synth import synth_utterance, write_synthetic_model
    p = str(tmp_path / "ctc_streaming.k2w")
    write_synthetic_model(p, "zipformer2-ctc-streaming-tiny-test")
    m = Model(p, 0)
    try:
        feats = [np.ascontiguousarray(m.fbank(synth_utterance(u, 2.0)), np.float32) for u in range(3)]
    finally:
        m.close()
    # a first run with nothing that biases: the unbiased results and the log-probs to cut the phrases and the LM from
    off, lps = _run_recognizer(p, feats, [None, None, None], None, False)
    n = min(x.shape[0] for x in lps)
    lp = np.stack([x[:n] for x in lps])
    _, entries = bc.fixture_entries(lp)
    m = Model(p, 0)
    try:
        alts = m.ctc_prefix_beam_search(lp, beam=4, nbest=4)
    finally:
        m.close()
    print("unbiased alternatives:", [[a["tokens"] for a in row] for row in alts])
    cut = [off_alternative_phrase(alts[b]) or alts[b][0]["tokens"][:2] for b in range(2)]
    lists = [[cut[0]], legal([cut[1], cut[0]]), None]
    print("phrase lists:", lists)
    assert cut[0] and cut[1] and lists[0] != lists[1]
    plain, _ = _run_recognizer(p, feats, lists, entries, False)        # graphs attached, LM set, switch off
    assert [(t, ts, np.float32(sc).tobytes()) for t, ts, sc in plain] == [(t, ts, np.float32(sc).tobytes()) for t, ts, sc in off]
    on, _ = _run_recognizer(p, feats, lists, entries, True)
    assert any(a[0] != b[0] for a, b in zip(on, plain)), (on, plain)
    rec = OnlineRecognizer(p)
    s = rec.create_online_stream(ctc_prefix_beam=4, ctc_prefix_biasing=True)
    try:
        s.add_features(feats[0])
        rec.get_results([s])
        with pytest.raises(K2HipError) as e:
            s.set_ctc_prefix_biasing(False)
        assert e.value.code == -1 and "reset the stream first" in str(e.value)
        s.reset()
        s.set_ctc_prefix_biasing(False)
    finally:
        s.close()
        rec.model.close()


def test_a_transducer_stream_refuses_the_switch(tmp_path):
    from k2transducerasr_amd import K2HipError, OnlineRecognizer
    from k2transducerasr_amd.synth import write_synthetic_model
    p = str(tmp_path / "streaming.k2w")
    write_synthetic_model(p, "zipformer2-streaming-tiny-test")
    rec = OnlineRecognizer(p)
    s = rec.create_online_stream()
    try:
        with pytest.raises(K2HipError) as e:
            s.set_ctc_prefix_biasing(True)
        assert e.value.code == -6, (e.value.code, str(e.value))
    finally:
        s.close()
        rec.model.close()
