"""CPU tests of the sample-rate converter: the library's plan (csrc/resample_plan.cpp, through k2hip_debug_resample_plan) against the
float64 twin (tests/resample_twin.py) -- every count exactly, the weights within one float32 ulp --, the float32 host reference
(csrc/resample_ref.h, through k2hip_debug_resample_ref) against the twin within the dot product's own error bound, its chunking rule,
the twin against the analytic signal in the passband, and the plans that are refused.  The stream rules of the accept_waveform
entries need a model: they run on the CPU in tests/native/san_resample_driver.cpp and on the device in tests/test_resample_gpu.py."""
import numpy as np
import pytest

from resample_twin import PAIRS, RATES_TO_16K, TABLE, RefStream, Twin, bound, lib_num_out, lib_plan, lib_plan_rc, ref_resample, same_bits


@pytest.fixture(scope="module")
def twins():
    return {pair: Twin(*pair) for pair in PAIRS}


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_plan_against_the_twin(twins, pair):
    tw, lp = twins[pair], lib_plan(*pair)
    assert (lp["iu"], lp["ou"], lp["max_taps"]) == (tw.iu, tw.ou, tw.max_taps)
    assert lp["first"].tolist() == tw.first and lp["ntaps"].tolist() == tw.ntaps
    assert tw.num_out_table(3000) == [lib_num_out(*pair, n) for n in range(3001)]
    assert tw.num_out(0) == 0 and tw.num_out(1) == lib_num_out(*pair, 1)
    for p in range(tw.ou):
        w64 = np.array(tw.w[p])
        w32 = lp["w"][p]
        assert w32.dtype == np.float32 and np.all(w32[tw.ntaps[p]:] == 0)
        ulp = np.spacing(np.abs(w64).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(w32[: tw.ntaps[p]].astype(np.float64) - w64) <= ulp), p


def test_the_orientation_table(twins):
    for fi, (iu, ou, taps, f_lo, f_hi) in TABLE.items():
        tw = twins[(fi, 16000)]
        assert (tw.iu, tw.ou, set(tw.ntaps), min(tw.first), max(tw.first)) == (iu, ou, taps, f_lo, f_hi), fi


def _signal(fi, n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, n).astype(np.float32)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_reference_against_the_twin(twins, pair):
    """the reference on the library's own float32 weights: per output |y32 - y64| <= (ntaps + 2) 2^-24 sum |w_j x_j|"""
    tw, lp = twins[pair], lib_plan(*pair)
    x = _signal(pair[0], 1500, 7)
    y32 = ref_resample(x, *pair)
    y64, mag, nt = tw.apply(x, lp["w"])
    assert len(y32) == len(y64) == lib_num_out(*pair, len(x)) > 100
    err = np.abs(y32.astype(np.float64) - y64)
    b = bound(mag, nt)
    print(f"{pair}: max |y32 - y64| = {err.max():.3e}, smallest bound / error margin = {np.min(b - err):.3e}, max bound = {b.max():.3e}")
    assert np.all(err <= b)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_chunking(twins, pair):
    """one push against pushes of 1, 7, iu - 1, iu, iu + 1 and random sizes: identical bits, identical num_out after every push"""
    tw = twins[pair]
    x = _signal(pair[0], 1200, 11)
    whole = ref_resample(x, *pair)
    tab = tw.num_out_table(len(x))
    rng = np.random.default_rng(5)
    plans = [[1] * 300, [7] * 172, [max(tw.iu - 1, 1)] * 8, [tw.iu] * 8, [tw.iu + 1] * 8, rng.integers(1, 97, 64).tolist()]
    for sizes in plans:
        st, got, pos, empty_pushes = RefStream(*pair), [], 0, 0
        for n in sizes:
            n = min(n, len(x) - pos)
            if n == 0:
                break
            y = st.push(x[pos:pos + n])
            pos += n
            empty_pushes += len(y) == 0
            got.append(y)
            assert st.n_in.value == pos and st.n_out.value == tab[pos] == lib_num_out(*pair, pos)
        got = np.concatenate(got)
        assert same_bits(got, whole[: len(got)]) and len(got) == lib_num_out(*pair, pos), sizes[:3]
        if sizes[0] == 1 and tw.iu >= tw.ou:
            assert empty_pushes > 0   # (a push that completes no output)
    # a signal shorter than the window gives nothing, and what it carries is the whole signal
    short = RefStream(*pair)
    n_short = max(tw.ntaps) // 2 - 1
    assert len(short.push(x[:n_short])) == 0 and short.n_out.value == 0 and short.n_tail.value == n_short


@pytest.mark.parametrize("fi", RATES_TO_16K + (16000,))
def test_twin_passband(twins, fi):
    """tones of 200 and 1000 Hz, amplitude 1, 50 ms, the interior (5 ms trimmed at each end): max |y - sin| <= 2e-3"""
    fo = 16000 if fi != 16000 else 8000
    tw = twins[(fi, fo)]
    for f in (200.0, 1000.0):
        n = int(0.05 * fi)
        x = np.sin(2 * np.pi * f * np.arange(n) / fi)
        y, _, _ = tw.apply(x)
        t = np.arange(len(y)) / fo
        keep = (t >= 0.005) & (t <= 0.045)
        err = np.max(np.abs(y[keep] - np.sin(2 * np.pi * f * t[keep])))
        print(f"{fi} -> {fo}, {f:.0f} Hz: max |y - sin| = {err:.2e}")
        assert keep.sum() > 300 and err <= 2e-3


def test_refused_plans():
    rc, msg = lib_plan_rc(16001, 16000)
    assert rc == -6 and "16001" in msg and "16000" in msg   # K2HIP_ERR_UNSUPPORTED: a table beyond 65536 floats
    rc, msg = lib_plan_rc(16000, 500)
    assert rc == -6 and "16000" in msg and "500" in msg     # more than 256 taps per phase
    for bad in (0, -8000):
        assert lib_plan_rc(bad, 16000)[0] == -1 and lib_plan_rc(16000, bad)[0] == -1   # K2HIP_ERR_INVALID
    assert lib_plan_rc(48000, 16000)[0] == 0
    assert lib_num_out(16001, 16000, 100) == -1
