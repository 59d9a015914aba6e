"""Host checks of what the greedy search's f16 screen (csrc/greedy.hip screen_round) takes on trust from the loader (csrc/model.cpp):
the f16 copy of joiner.output_linear in MFMA B-fragment order (`...weight#h16`) and the per-column bound `...weight#eps` on
|l~ - l| that decides which columns the screen may drop.  Both are read from the REAL loader through
`san_api_driver tensor <model> <name>` (tests/native/san_api_driver.cpp, AddressSanitizer + UBSan build), never re-derived here.
Also the self-checks of tests/search_cases.py, whose cases tests/test_search_ties_gpu.py runs on the device.

test_bound_holds_on_adversarial_rows -- largest achieved |l~ - l| / eps[v] (exact sums, before the accumulation allowance):
    J = 64: 0.716, J = 128: 0.709, J = 256: 0.697, J = 512: 0.674 (V = 1101 and 1200 alike; 0.725 .. 0.733 with the allowance)
so the bound has a factor of 1.36 .. 1.38 in hand on these rows, and a bound scaled by 0.25 (or anything under 0.67) fails here."""
import os
import subprocess

import numpy as np
import pytest

import search_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API_DRIVER = os.path.join(ROOT, "tests", "native", "k2hip_san_api_driver")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
H16, EPS = "joiner.output_linear.weight#h16", "joiner.output_linear.weight#eps"
ACHIEVED_MIN = 0.65    # the construction's reach (docstring): a weaker one would let a too small bound through


@pytest.fixture(scope="module")
def tensor():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "k2transducerasr_amd", "csrc"), "-s", "../../tests/native/k2hip_san_api_driver"])

    def read(path, name, dtype):
        r = subprocess.run([API_DRIVER, "tensor", path, name], capture_output=True, env=ENV, timeout=120)
        err = r.stderr.decode(errors="replace")
        assert "AddressSanitizer" not in err and "runtime error" not in err and "LeakSanitizer" not in err, err[-3000:]
        assert r.returncode == 0, (r.returncode, err[-2000:])
        return np.frombuffer(r.stdout, dtype=dtype)
    return read


def decode_h16(raw, V, J):
    """model.cpp's layout: element j of lane l of (tile t, step s) is W[16 t + (l & 15)][32 s + 8 (l >> 4) + j] -> ([nt * 16, J] bits)"""
    nt, ns = (((V + 3) // 4 * 4) + 15) // 16, J // 32
    assert raw.size == nt * ns * 64 * 8, (raw.size, nt, ns)
    fr = raw.reshape(nt, ns, 64, 8)
    out = np.zeros((nt * 16, J), np.uint16)
    for l in range(64):
        for j in range(8):
            out[(l & 15)::16, (32 * np.arange(ns) + 8 * (l >> 4) + j)] = fr[:, :, l, j]
    return out


def special_weights(rng, V, J):
    W = (rng.standard_normal((V, J)) * 0.3).astype(np.float32)
    sp = np.array([3e-6, -3e-6, 6.1e-5, 2.0 ** -24, -2.0 ** -24, 1e-9, -1e-9, 2.0 ** -25, 3 * 2.0 ** -25, -3 * 2.0 ** -25, 2.0 ** -26,   # subnormal / underflow
                   1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 0.5 + 2.0 ** -12, 0.5 + 3 * 2.0 ** -12, 2.0 ** -14 + 2.0 ** -25,   # halfway
                   2.0 ** -14 - 2.0 ** -26, 1 + 2.0 ** -11 + 2.0 ** -23, 1 + 2.0 ** -11 - 2.0 ** -23, 0.0, -0.0, 65503.0, 60000.0], np.float32)
    for i, c in enumerate((0, 15, 16, 17, V // 2, V - 17, V - 1)):
        W[c, (np.arange(sp.size) * 5 + 3 * i) % J] = sp[: min(sp.size, J)] if sp.size > J else sp
    return W


@pytest.mark.parametrize("V", sc.VS)
@pytest.mark.parametrize("J", sc.JS)
def test_fragment_layout_is_the_documented_one_bit_for_bit(tensor, tmp_path, J, V):
    rng = np.random.default_rng(J + V)
    W = special_weights(rng, V, J)
    p = str(tmp_path / "m.k2w")
    sc.write_case_model(p, W, np.zeros(V, np.float32))
    got = decode_h16(tensor(p, H16, np.uint16), V, J)
    want = W.astype(np.float16).view(np.uint16)           # numpy: IEEE round-to-nearest-even, subnormals kept
    bad = np.argwhere(got[:V] != want)
    assert bad.size == 0, (bad[:5], [(W[r, c], hex(got[r, c]), hex(want[r, c])) for r, c in bad[:5]])
    assert not got[V:].any(), "pad columns must be zero"
    eps = tensor(p, EPS, np.float32)
    assert eps.size == got.shape[0] and np.isfinite(eps[:V]).all() and not eps[V:].any()


@pytest.mark.parametrize("V", sc.VS)
@pytest.mark.parametrize("J", sc.JS)
def test_bound_holds_on_adversarial_rows(tensor, tmp_path, J, V):
    """For column v and its adversarial row a(v): l~ = exact sum of the f16-rounded a and w (f16 products are exact in float64) + bias,
    l = exact sum of the f32 values + bias; |l~ - l| + the allowance model.cpp's comment grants the two f32 accumulations
    ((J + 8) 2^-24 c (1 + 2^-10) each) and the two bias adds (one ulp of the result each) must stay within eps[v].  Adversarial:
    w_k = h_k -+ 0.49 ulp16(h_k) sign(h_k) around an f16 value h_k at the bottom of its binade, a_k with the sign of w~_k - w_k and
    |a_k| at the f16 midpoint 1 - 2^-12 (exactly: the tie goes to the even neighbour 1.0) or one f32 step under it (down to 1 - 2^-11),
    whichever gives (a~_k - a_k) w~_k that sign too: every one of the 2 J rounding errors pulls the same way.  Every row is checked against EVERY column."""
    rng = np.random.default_rng(7 * J + V)
    n_adv = 48
    W = (rng.standard_normal((V, J)) * 0.3).astype(np.float32)
    b = (rng.standard_normal(V) * 0.5).astype(np.float32)
    cols = rng.choice(V, n_adv, replace=False)
    cols[:3] = (0, 16 * 3 + 15, V - 1)
    cols = np.unique(cols)
    A = []
    for i, v in enumerate(cols):
        h = sc.f16_row(rng, J)
        sgn = 1.0 if i % 2 else -1.0                       # w above / below its f16 value
        W[v] = (h + sgn * 0.49 * sc.ulp16(h) * np.sign(h)).astype(np.float32)
        assert (sc.f16(W[v]) == sc.f16(h)).all()
        # (a~ - a) w~ must pull the way a (w~ - w) does: below its f16 value w wants |a~| > |a| (the tie goes to the even 1.0), above
        # it |a~| < |a| (one f32 step under the midpoint: down to 1 - 2^-11)
        mag = 1.0 - 2.0 ** -12 - (2.0 ** -24 if sgn > 0 else 0.0)
        a = (-sgn * np.sign(h) * mag).astype(np.float32)
        assert (np.abs(sc.f16(a)) == (1.0 - 2.0 ** -11 if sgn > 0 else 1.0)).all()
        A.append(a)
    A += [rng.uniform(-1, 1, J).astype(np.float32) for _ in range(8)]
    A = np.stack(A)
    p = str(tmp_path / "m.k2w")
    sc.write_case_model(p, W, b)
    eps = tensor(p, EPS, np.float32)[:V].astype(np.float64)
    emu = sc.eps_emulated(W, b).astype(np.float64)
    W64, c = W.astype(np.float64), np.abs(W.astype(np.float64)).sum(1)
    l = A.astype(np.float64) @ W64.T + b
    lt = sc.f16(A).astype(np.float64) @ sc.f16(W).astype(np.float64).T + b
    err = np.abs(lt - l)
    allow = 2 * (J + 8) * sc.U * c * (1 + 2.0 ** -10) + 2 * sc.U * (np.abs(l) + np.abs(lt))
    ratio = err / eps
    print(f"J={J} V={V}: largest |l~ - l| / eps = {ratio.max():.4f}, with the allowance {((err + allow) / eps).max():.4f}")
    assert np.all(err + allow <= eps), (np.argwhere(err + allow > eps)[:5], ((err + allow) / eps).max())
    own = ratio[np.arange(cols.size), cols]
    assert own.min() >= ACHIEVED_MIN, own.min()
    # (last: a loader whose bound is wrong fails on the bound above, not on this)
    assert np.all(np.abs(eps - emu) <= 2.0 ** -22 * emu), "search_cases.eps_emulated has left model.cpp's formula"


def test_non_finite_and_overflowing_weights_get_an_infinite_bound(tensor, tmp_path):
    V, J = 1101, 64
    rng = np.random.default_rng(3)
    W = (rng.standard_normal((V, J)) * 0.3).astype(np.float32)
    W[3, 0], W[4, 1], W[5, 2], W[6, 3], W[7, 4], W[8, 5], W[9, 6] = 1e6, -7e4, np.inf, -np.inf, np.nan, 65504.0, 65503.0
    p = str(tmp_path / "m.k2w")
    sc.write_case_model(p, W, np.zeros(V, np.float32))
    eps = tensor(p, EPS, np.float32)[:V]
    assert np.isinf(eps[3:9]).all() and (eps[3:9] > 0).all()
    assert np.isfinite(np.delete(eps, np.arange(3, 9))).all()           # 65503 rounds to the largest f16 and keeps a finite bound


@pytest.mark.parametrize("V", sc.VS)
@pytest.mark.parametrize("J", sc.JS)
def test_generated_cases_keep_their_promises(J, V):
    """tests/search_cases.py's own checks in float64: every F64 frame has 10 x the noise bound of margin (or is an exact tie between
    identical columns), the emulated screen order of every adversarial twin is reversed, everything else is far below."""
    from family_kernels import LIBM_TANH
    assert sc.LIBM_TANH == LIBM_TANH
    m = sc.build(J, V)
    kinds = set()
    for c in m.cases:
        arg, _ = sc.check_case(m, c)
        kinds |= set(np.unique(c.kind).tolist())
        assert c.enc.shape[0] <= 4 and c.enc.shape[1] <= 19
    assert kinds == {sc.F64, sc.FORMS}
    assert min(sc.screen_reversal_ratio(m)) >= sc.REVERSAL_FLOOR[J], sc.screen_reversal_ratio(m)
    cols = {c for p in m.dup_pairs for c in p}
    for parts in (2, 4):
        for bnd in sc.slab_boundaries(V, parts):
            assert bnd - 1 in cols and bnd in cols
    assert V - 1 in cols and sc.BLANK in cols and sc.UNK in cols
