"""CPU tests of hotword and n-gram LM biasing in the streaming CTC prefix beam search: the numpy restatement of the biased carry
(tests/ctc_prefix_stream_bias_twin.py) against the whole-row biased twin (tests/ctc_prefix_bias_twin.py) after EVERY chunk, in float32
and float64; the events that cross the committed inputs' chunk boundaries, recounted; the flip row's per-step results as literals; and
three deliberately weaker carries that the inputs must tell from the correct one."""
import os

import numpy as np
import pytest

import ctc_prefix_bias_cases as bc
import ctc_prefix_stream_bias_cases as sbc
from ctc_prefix_bias_twin import biased_prefix_beam_search
from ctc_prefix_stream_bias_twin import BiasHostCarry, BiasStreamTwin, SideLayout, chunked_biased_search, same_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_prefix = {}


def prefix(name, lp, t, beam, graph, lm, dtype):
    """the whole-row biased twin over the first t frames, computed once"""
    k = (name, t, beam, np.dtype(dtype).name)
    if k not in _prefix:
        _prefix[k] = biased_prefix_beam_search(lp[:t], beam, graph, lm, dtype)
    return _prefix[k]


_runs = {}


def run_all(dtype):
    """every strict case at every beam in chunks of 16 and of 7 (ragged last chunk), compared after every chunk; returns the counts"""
    key = np.dtype(dtype).name
    if key in _runs:
        return _runs[key]
    stats = dict(ends=0, pending={}, reordered={}, boundaries={}, left_out={}, intermediate={})
    for name, lp, beams, graph, lm, G in bc.strict_cases():
        T = lp.shape[0]
        for beam in beams:
            for ci, chunks in enumerate(sbc.chunkings(T)):
                grp = (sbc.group_of(name), name.split()[-1])

                def after(tw):
                    want = prefix(name, lp, tw.frames, beam, graph, lm, dtype)
                    assert same_entries(tw.entries(), want["hyps"]), (name, beam, chunks[0], tw.frames)
                    assert tw.picks == want["picks"], (name, beam, tw.frames)
                    stats["ends"] += 1
                    if tw.frames < T:
                        stats["intermediate"][ci] = stats["intermediate"].get(ci, 0) + 1
                        stats["left_out"][ci] = stats["left_out"].get(ci, 0) + (min(tw.final_gaps() + [np.inf]) < G)
                        if ci == 0:
                            stats["boundaries"][grp] = stats["boundaries"].get(grp, 0) + 1
                            stats["pending"][grp] = stats["pending"].get(grp, 0) + (tw.pending_slots() > 0)
                            stats["reordered"][grp] = stats["reordered"].get(grp, 0) + tw.reordered()

                chunked_biased_search(lp, beam, chunks, graph, lm, dtype, after=after)
    _runs[key] = stats
    return stats


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_after_every_chunk_the_whole_rows_search(dtype):
    """slots, entries, final, (tot, ctx) in the dtype's own bits, hs, ls and every frame's picks, on every strict case"""
    stats = run_all(dtype)
    assert stats["ends"] > 400


def test_the_inputs_cross_boundaries_in_the_ways_that_matter():
    """float64 twin, 16-frame chunk ends: a live slot with a pending match, and a final order that differs from the slot order, occur in
    every group that has a graph and more than one chunk; recounted here so that a later change of seeds cannot empty them"""
    stats = run_all(np.float64)
    for grp in (("long", "both"), ("long", "hw"), ("ragged", "both"), ("ragged", "hw"), ("wide", "both"), ("wide", "hw")):
        print(grp, "boundaries", stats["boundaries"][grp], "pending", stats["pending"][grp], "reordered", stats["reordered"][grp])
        assert stats["boundaries"][grp] > 0 and stats["pending"][grp] > 0 and stats["reordered"][grp] > 0, grp
    assert stats["pending"][("long", "both")] == stats["boundaries"][("long", "both")] == 18
    for grp in (("long", "lm"), ("ragged", "lm"), ("wide", "lm")):        # the LM alone reorders too (no pending bonus without a graph)
        assert stats["pending"][grp] == 0 and stats["reordered"][grp] > 0, grp


def test_few_chunk_ends_are_left_out_of_the_float64_order_assertion():
    """the GPU test asserts the order against float64 only where the float64 twin's consecutive finals at that chunk end clear the group's
    G; the share of intermediate chunk ends below G stays under 2 % per chunking"""
    stats = run_all(np.float64)
    for ci in (0, 1):
        n, out = stats["intermediate"][ci], stats["left_out"][ci]
        print(f"chunks of {(sbc.CHUNK, sbc.SHORT_CHUNK)[ci]}: {out} of {n} intermediate chunk ends below G")
        assert n > 100 and out <= sbc.LEFT_OUT_LIMIT * n, (ci, out, n)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_respelled_row_at_its_nine_splits(dtype):
    splits = sbc.respelled_splits()
    assert len(splits) == 9
    for name, lp, beam, graph, lm, _ in sbc.respelled_cases():
        for ch in splits:
            chunked_biased_search(lp, beam, ch, graph, lm, dtype, after=lambda tw: _same(tw, name, lp, beam, graph, lm, dtype, ch))


def _same(tw, name, lp, beam, graph, lm, dtype, ch):
    want = prefix(name, lp, tw.frames, beam, graph, lm, dtype)
    assert same_entries(tw.entries(), want["hyps"]) and tw.picks == want["picks"], (name, ch, tw.frames)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_flip_row_step_by_step(dtype):
    """chunks of one frame and both two-chunk splits; the per-step results as literals"""
    lp, graph = bc.FLIP_ROWS, bc.flip_graph()
    for ch in sbc.FLIP_CHUNKINGS:
        seen = []
        chunked_biased_search(lp, bc.FLIP_BEAM, ch, graph, None, dtype,
                              after=lambda tw: (_same(tw, "flip hw", lp, bc.FLIP_BEAM, graph, None, dtype, ch), seen.append((tw.frames, tw.result()))))
        for frames, (tokens, score) in seen:
            assert (tokens, score) == sbc.FLIP_STEPS[frames - 1], (ch, frames, tokens, score)
    tw = BiasStreamTwin(bc.FLIP_BEAM, graph, None, dtype).chunk(lp[:1])
    got = [dict(tokens=list(s["tokens"]), hs=s["hs"], ctx=float(s["ctx"])) for s in tw.slots]
    assert got == sbc.FLIP_SLOTS_AFTER_FRAME_0                      # carried in selection order, ctx with the pending bonus
    assert tw.pending_slots() == 1 and tw.reordered()               # ... while the reported order differs
    assert tw.result() == sbc.FLIP_STEPS[0]
    plain = chunked_biased_search(lp, bc.FLIP_BEAM, 1, None, None, dtype)
    assert plain.result()[0] == bc.FLIP_UNBIASED[0]


def test_the_inputs_tell_the_correct_carry_from_weaker_ones():
    lp, graph = bc.FLIP_ROWS, bc.flip_graph()
    want = biased_prefix_beam_search(lp, bc.FLIP_BEAM, graph, None)
    assert want["hyps"][0]["score"] == bc.FLIP_BIASED[2]
    for carry in ("reset_states", "ctx_final"):
        tw = chunked_biased_search(lp, bc.FLIP_BEAM, 1, graph, None, carry=carry)
        assert not same_entries(tw.entries(), want["hyps"]), carry
        assert tw.result() == ([sbc.A, sbc.B], sbc.FLIP_WEAK_FINAL), (carry, tw.result())
    # carried in final order: caught by the slot-order comparison of the carried state after the first chunk
    tw = BiasStreamTwin(bc.FLIP_BEAM, graph, None, carry="final_order").chunk(lp[:1])
    first = biased_prefix_beam_search(lp[:1], bc.FLIP_BEAM, graph, None)
    by_slot = sorted(first["hyps"], key=lambda h: h["slot"])
    assert by_slot[0]["tokens"] == [sbc.A] and list(tw.slots[0]["tokens"]) == [sbc.B]
    assert not same_entries(tw.entries(), first["hyps"])
    # and on the committed long row the weaker carries differ as well
    name, lp, beams, graph, lm, _ = [c for c in bc.strict_cases() if c[0] == "long both"][0]
    want = prefix(name, lp, lp.shape[0], beams[0], graph, lm, np.float64)
    for carry in ("reset_states", "ctx_final", "final_order"):
        assert not same_entries(chunked_biased_search(lp, beams[0], sbc.CHUNK, graph, lm, carry=carry).entries(), want["hyps"]), carry


def test_host_mirror_side_blocks():
    """BiasHostCarry: the start state, the side in block's layout, a side out block applied, and what it refuses"""
    c = BiasHostCarry(2, S=3, S_lm=4, start=2, lm_on=True)
    L = SideLayout(2)
    blk = c.fill_side_in()
    assert blk.tolist() == [1, 0, 0, 0, 0, 2, 0] and (L.in_ints, L.out_ints) == (7, 10)
    from ctc_prefix_stream_twin import Layout, _bits
    Lo = Layout(2, 1)
    out = np.zeros(Lo.out_ints, np.int32)
    out[0] = 2
    out[Lo.out_napp: Lo.out_napp + 2] = 1
    out[Lo.out_ys], out[Lo.out_ys + 1] = 1, 3
    h = lambda v: (0x243F6A8885A308D3 * 0x9E3779B97F4A7C15 + v + 1) & ((1 << 64) - 1)
    for k, v in enumerate((1, 3)):
        out[Lo.out_hash + 2 * k: Lo.out_hash + 2 * k + 2] = np.array([h(v) & 0xFFFFFFFF, h(v) >> 32], np.uint32).view(np.int32)
        out[Lo.out_phash + 2 * k: Lo.out_phash + 2 * k + 2] = np.array([0x243F6A8885A308D3 & 0xFFFFFFFF, 0x243F6A8885A308D3 >> 32], np.uint32).view(np.int32)
    side = np.array([_bits(1.5), _bits(0.0), 1, 0, 3, 1, _bits(-1.5), _bits(-1.25), 1, 0], np.int32)
    c.apply(out, side, 1, 1)
    assert [e["tokens"] for e in c.entries()] == [(3,), (1,)] and [s["tokens"] for s in c.slots] == [(1,), (3,)]
    assert c.fill_side_in().tolist() == [1, _bits(1.5), 0, 1, 0, 3, 1]
    for bad in ((L.out_hs, 3), (L.out_ls + 1, 4), (L.out_ord, 0)):       # hs outside the graph, ls outside the LM, ord no permutation
        b = side.copy()
        b[bad[0]] = bad[1]
        with pytest.raises(AssertionError):
            BiasHostCarry(2, S=3, S_lm=4, start=2, lm_on=True).apply(out, b, 1, 1)


def test_surface_exists():
    with open(os.path.join(ROOT, "include", "k2hip_debug.h")) as f:
        assert '"ctc_prefix_resume_bias"' in f.read()
    with open(os.path.join(ROOT, "k2transducerasr_amd", "csrc", "ctc_prefix_layout.h")) as f:
        assert "CtcPrefixResumeBiasLayout" in f.read()
