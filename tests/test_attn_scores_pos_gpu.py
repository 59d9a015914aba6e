"""The positional term of k_attn_scores_softmax<NG> (csrc/attn.hip, the LDS-strip form) is a skewed MFMA product: the workgroup's
32 positional queries times a window of pos rows, each accumulator element (row i, window row n) scattered to the one score
(i, j = n - (T-1-i)) it belongs to.  What can go wrong is the skew: an index off by one, a window tile or a key tile that is cut
by T, by the 32-row workgroup or by the 32-column tile.  The shapes here sit on those edges, against the float64 reference and the
softmax tolerance of tests/test_kernels_gpu.py; the last test lights one single window row, so every weight off the one
anti-diagonal it belongs to shows."""
import numpy as np
import pytest

from test_kernels_gpu import check_scores, op, run_scores, scores_case, scores_ref  # noqa: F401  (op: the fixture)

pytestmark = pytest.mark.gpu

TS = [1, 2, 31, 32, 33, 63, 64, 65, 97, 129]
FORMS = [(32, "z2"), (16, "z1")]


@pytest.mark.parametrize("qh,layout", FORMS)
def test_strip_form_on_the_edges_of_the_skew(op, qh, layout):  # noqa: F811
    rng = np.random.default_rng(4100 + qh)
    for T in TS:
        for H, B in ((1, 1), (4, 2)):
            qkp, pp, ld, Tp, kargs, koff0, poff0 = scores_case(rng, B, T, H, qh, layout)
            ref = scores_ref(qkp, pp, B, T, H, qh, koff0, poff0)
            check_scores(run_scores(op, qkp, pp, ld, B, T, Tp, H, qh, kargs), ref, T, Tp, f"strip qh={qh} T={T} H={H} B={B}")


@pytest.mark.parametrize("qh,layout", FORMS)
def test_one_window_row_lights_one_anti_diagonal(op, qh, layout):  # noqa: F811
    """pp is zero except for window row n0, the positional queries are all ones and q = k = 0: score (i, j) is 8 where
    T-1-i+j = n0 and 0 elsewhere.  A row the anti-diagonal j - i = n0 - (T-1) crosses has its one largest weight there and T-1
    equal smaller ones; a row it misses has T equal weights."""
    rng = np.random.default_rng(4200 + qh)
    H, B = 4, 2
    for T in TS:
        for n0 in sorted({0, T - 1, 2 * T - 2}):
            qkp, pp, ld, Tp, kargs, koff0, poff0 = scores_case(rng, B, T, H, qh, layout)
            qkp[:, :2 * H * qh] = 0.0
            qkp[:, poff0:poff0 + 4 * H] = 1.0
            pp[:] = 0.0
            pp[n0, :] = 2.0
            aw = run_scores(op, qkp, pp, ld, B, T, Tp, H, qh, kargs)
            what = f"one window row qh={qh} T={T} n0={n0}"
            check_scores(aw, scores_ref(qkp, pp, B, T, H, qh, koff0, poff0), T, Tp, what)
            d = n0 - (T - 1)
            for i in range(T):
                rows = aw[:, :, i, :T].reshape(H * B, T)
                j = i + d
                if 0 <= j < T:
                    rest = np.delete(rows, j, axis=1)
                    assert (rows[:, j] > 0.5).all(), (what, i)
                    assert T == 1 or ((rest.max(1) == rest.min(1)).all() and (rest.max(1) < rows[:, j]).all()), (what, i, "a weight off the anti-diagonal")
                else:
                    assert (rows.max(1) == rows.min(1)).all(), (what, i, "a peak in a row the anti-diagonal misses")
