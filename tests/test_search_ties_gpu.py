"""The transducer greedy search (csrc/greedy.hip) on exact ties, near-ties and the f16 screen's limits, one model per
(J, V) in {64, 128, 256, 512} x {1200, 1101} -- the four screen_round<NS> instantiations, a vocabulary that is a multiple of the 16-column
screen tile and one with a padded tail.  Inputs, float64 reference, noise bound and frame kinds: tests/search_cases.py (its own
promises are checked on the host by tests/test_search_screen_ref.py).  No excuse mechanism: a frame is held to float64 in every form,
or -- the sub-noise twins -- between the forms.

FORMS of the search.  K_GREEDY lists the entries that run k_greedy and so share its column arithmetic (the k slices' fma chains in k
order on v_mfma_f32_4x4x1, the slices summed in one tree, + bias; screen_round's re-check forms the same values from the [V][J]
layout): greedy_batch by default, with K2HIP_GREEDY_PARTS 1 / 2 / 4 and with K2HIP_GREEDY_ONE_PART, the same from a model loaded with
K2HIP_SCREEN_MIN_V=0 (no f16 screen: the f32 passes alone), and greedy_single.  K2HIP_SEARCH_ROUNDS=1 (greedy_rounds) takes its logits
from the GEMM kernels -- other summation orders -- and is held to float64 and to the twins' pair only.

Which way a round went is read from the model's counters (K2HIP_SCREEN_COUNT, k2hip_debug_op_run "greedy_screen_counts"): a screen
that always gave up, or a fallback that never ran, would otherwise pass every token comparison here.

Also CTC's first-index argmax (k_argmax_rows<true>) on V = 1200 rows, against its rule written out as a scan."""
import ctypes as C

import numpy as np
import pytest

import search_cases as sc

pytestmark = pytest.mark.gpu
K_GREEDY = ("batch", "parts1", "parts2", "parts4", "one_part", "off_batch", "off_parts2", "single", "off_single")


FLAG_SWITCHES = ("K2HIP_GREEDY_ONE_PART",)     # csrc/tunables.cpp: the variable's presence means 1


class switch:
    """a switch for the duration of a with-block.  The library has no getter, so the value to go back to is the one it took at
    start-up: the process's K2HIP_* variable where it is set (as tunables.cpp reads it), else the library's default `restore`"""

    def __init__(self, name, value, restore=0):
        import os
        env = os.environ.get(name)
        if env is not None:
            try:
                restore = 1 if name in FLAG_SWITCHES else int(env)
            except ValueError:
                restore = 0      # atoi
        self.name, self.value, self.restore = name, value, restore

    def __enter__(self):
        from k2transducerasr_amd import set_switch
        set_switch(self.name, self.value)

    def __exit__(self, *a):
        from k2transducerasr_amd import set_switch
        set_switch(self.name, self.restore)


def screen_counts(model):
    """(rounds the f16 screen decided, rounds that ran the f32 passes) since the model was created"""
    from k2transducerasr_amd import load_library
    L = load_library()
    L.k2hip_debug_op_run.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                     C.c_int32, C.c_uint32]
    out = np.full(2, -1, np.int64)
    rc = L.k2hip_debug_op_run(model.handle, b"greedy_screen_counts", (C.c_int64 * 1)(0), 0, (C.c_void_p * 1)(out.ctypes.data), (C.c_int64 * 1)(16), 1, 1)
    assert rc == 0, L.k2hip_last_error()
    return out


@pytest.fixture(scope="module", params=[(J, V) for J in sc.JS for V in sc.VS], ids=lambda p: f"J{p[0]}-V{p[1]}")
def rig(request, tmp_path_factory):
    """the (J, V) model twice: loaded with the f16 screen (default) and without it (K2HIP_SCREEN_MIN_V=0 is read at load time)"""
    from k2transducerasr_amd import Model
    J, V = request.param
    m = sc.build(J, V)
    path = str(tmp_path_factory.mktemp("ties") / f"j{J}_v{V}.k2w")
    m.write(path)
    with switch("K2HIP_DECODER_TABLE_MB", 0, 1024):      # (decoder_proj is zero: no use for the 0.4 GB all-contexts table)
        on = Model(path, 0)
        with switch("K2HIP_SCREEN_MIN_V", 0, 1024):
            off = Model(path, 0)
    yield m, on, off
    on.close()
    off.close()


def run_forms(on, off, enc):
    """enc [B, T, J] through every form -> {form: [T] tokens per frame (-1: none) for each stream},
    {form: (decided, fallen back) screen rounds the form added}"""
    T = enc.shape[1]
    out, cnt = {}, {}

    def note(name, model, fn):
        c0 = screen_counts(model)
        res = fn()
        cnt[name] = tuple(int(x) for x in screen_counts(model) - c0)
        out[name] = [sc.per_frame(r, T) for r in res]

    with switch("K2HIP_SCREEN_COUNT", 1):
        note("batch", on, lambda: on.greedy_batch(enc))
        for parts in (1, 2, 4):
            with switch("K2HIP_GREEDY_PARTS", parts):
                note(f"parts{parts}", on, lambda: on.greedy_batch(enc))
        with switch("K2HIP_GREEDY_ONE_PART", 1):
            note("one_part", on, lambda: on.greedy_batch(enc))
        note("off_batch", off, lambda: off.greedy_batch(enc))
        with switch("K2HIP_GREEDY_PARTS", 2):
            note("off_parts2", off, lambda: off.greedy_batch(enc))
        with switch("K2HIP_SEARCH_ROUNDS", 1, -1):
            note("rounds", on, lambda: on.greedy_batch(enc))
        note("single", on, lambda: [on.greedy_single(e) for e in enc])
        note("off_single", off, lambda: [off.greedy_single(e) for e in enc])
    assert set(K_GREEDY) | {"rounds"} == set(out)
    return out, cnt


def check_tokens(m, c, out):
    arg, _ = sc.reference(m.W, m.b, c.enc)
    want = np.where((arg == sc.BLANK) | (arg == sc.UNK), -1, arg)
    B, T = arg.shape
    f64 = c.kind == sc.F64
    for form, res in out.items():
        for bi in range(B):
            got = res[bi]
            bad = np.flatnonzero(f64[bi] & (got != want[bi]))
            assert bad.size == 0, (c.name, form, bi, [(int(t), int(got[t]), int(want[bi, t]), c.group[bi][t]) for t in bad[:6]])
            for t in np.flatnonzero(~f64[bi]):
                assert got[t] in c.group[bi][t], (c.name, form, bi, int(t), int(got[t]), c.group[bi][t])
    for form in K_GREEDY[1:]:
        for bi in range(B):
            diff = np.flatnonzero(out[form][bi] != out[K_GREEDY[0]][bi])
            assert diff.size == 0, (c.name, f"{form} and {K_GREEDY[0]} part on a sub-noise twin", bi,
                                    [(int(t), int(out[form][bi][t]), int(out[K_GREEDY[0]][bi][t])) for t in diff[:6]])
    return int(f64.sum()), int((~f64).sum())


@pytest.mark.parametrize("name", ["duplicate_pairs", "adversarial_and_sub_noise", "mixed"])
def test_every_form_gives_the_float64_token_and_the_k_greedy_forms_agree(rig, name):
    """Exact duplicates: the later index in every form.  f16-adversarial twins: the float64 winner although the screen's own sums put
    the other twin ahead (so the winner is only found through its eps).  Sub-noise twins: one of the pair, and the same one in every
    k_greedy form -- screen on and off, 1 / 2 / 4 parts, one part, single.  The screen decided every round of every slab in the
    forms loaded with it, and none in the forms loaded without it."""
    m, on, off = rig
    c = next(x for x in m.cases if x.name == name)
    out, cnt = run_forms(on, off, c.enc)
    n64, nforms = check_tokens(m, c, out)
    assert n64 + nforms == c.kind.size and n64 > 0
    # (no slab of any split can overflow its candidate list on these frames: search_cases.check_case counts them per slab)
    for form in ("batch", "parts1", "parts2", "parts4", "one_part", "single"):
        assert cnt[form][0] > 0 and cnt[form][1] == 0, (form, cnt)
    for form in ("off_batch", "off_parts2", "off_single", "rounds"):
        assert cnt[form] == (0, 0), (form, cnt)


@pytest.mark.parametrize("name", ["dup8", "dup9", "dup100"])
def test_candidate_list_limits(rig, name):
    """8 frames of one stream on which 8 / 9 / 100 duplicate columns tie; every frame emits, so the rounds cover 8, 7, .. 1 frames.
    8 x 8 = kScreenCand pairs fill the list exactly and the screen decides all 8 rounds; 9 x 8 = 72 send the first round to the f32
    passes and the 7 shorter ones stay with the screen; 100 send every round there.  The last index wins on either path, in every form."""
    m, on, off = rig
    c = next(x for x in m.cases if x.name == name)
    out, cnt = run_forms(on, off, c.enc)
    check_tokens(m, c, out)
    assert (out["batch"][0] == max(c.group[0][0])).all()
    for form in ("parts1", "one_part"):                # one part per stream: the whole vocabulary's candidates in one list
        assert cnt[form] == c.counts, (name, form, cnt[form], c.counts)


# ---- CTC: k_argmax_rows<true> ----------------------------------------------------------------------------------------------------
def first_argmax(row):
    """Array.IndexOf(row, row.Max()) with Enumerable.Max's order (NaN below every number): the first index of the largest number, 0
    for a row of nothing but NaNs -- as a plain scan"""
    best, v = 0, row[0]
    for k in range(1, len(row)):
        x = row[k]
        if x > v or (v != v and x == x):
            best, v = k, x
    return best


def test_ctc_first_index_argmax_on_wide_rows(tmp_path):
    from k2transducerasr_amd import Model
    from k2transducerasr_amd.synth import write_synthetic_model
    V = 1200
    p = str(tmp_path / "ctc_wide.k2w")
    write_synthetic_model(p, "zipformer2-ctc-tiny-test", meta_overrides={"vocab_size": str(V)})
    NAN = float("nan")
    rows = [
        {5: 1.0, 6: 1.0},                      # neighbouring lanes
        {70: 1.0, 5: 1.0},                     # lanes 6 and 5, different 64-strides: the tie is met later in the lane order
        {5 + 64 * 9: 1.0, 5: 1.0, 5 + 64 * 3: 1.0},   # one lane, three strides
        {1199: 2.0, 64: 2.0, 63: 2.0},         # the row's last element, lane 0 / lane 63
        {0: 1.0, 700: 1.0},                    # blank ties with a token: blank (nothing emitted)
        {700: 1.0, 900: 1.0},
        {3: NAN, 10: 1.0, 500: 1.0},           # a NaN in front of the maxima
        {10: 1.0, 500: 1.0, 1100: NAN},        # behind them
        {10: 1.0, 300: NAN, 500: 1.0},         # between them
        {0: NAN, 1: NAN, 1199: NAN, 77: -9.0}, # NaNs at both ends; every number counts, however small: 77 loses to the -5 floor's first
        {k: NAN for k in range(V)},            # nothing but NaNs: index 0
        {k: NAN for k in range(V) if k != 800},   # one number among NaNs
        {64: 3.0, 128: 3.0, 1: NAN, 65: NAN},
    ]
    T = 2 * len(rows)
    x = np.full((2, T, V), -5.0, np.float32)
    x[:, :, 0] = 0.0                           # blank between the rows, so that no two of them collapse
    for i, r in enumerate(rows):
        for b in range(2):
            t = 2 * i + 1 if b == 0 else T - 1 - 2 * i      # (the second stream: the rows in reverse order)
            x[b, t, 0] = -5.0
            for k, v in r.items():
                x[b, t, k] = v
    want = []
    for b in range(2):
        toks, ts, prev = [], [], -1
        for t in range(T):
            y = first_argmax(x[b, t])
            if y != 0 and y != prev:
                toks.append(y)
                ts.append(t)
            prev = y
        want.append((toks, ts))
    assert want[0][0][:4] == [5, 5, 5, 63] and 800 in want[0][0] and len(want[0][0]) >= 10
    hip = Model(p, 0)
    try:
        assert hip.vocab_size == V
        got, _ = hip.ctc_greedy(x)
    finally:
        hip.close()
    assert got == want, (got, want)
