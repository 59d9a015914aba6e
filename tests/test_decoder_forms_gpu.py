"""decoder() (csrc/greedy.hip k_decoder -> decoder_block -> decoder_conv_narrow) through k2hip_decoder against a float64 evaluation of
the model's own tensors, read back with k2w.py: out = decoder_proj(relu(conv(emb[y0], emb[y1]))) + bias, a negative id embedding as
zeros.  Two of decoder_conv_narrow's three forms are reachable from a model file: cpg <= 4 (zipformer2-tiny-test: 4 channels per
group) and the per-token table (conformer-tiny-test: groups = 1; Engine::decjoin builds the table for every such model, so the
staged general form behind it is reached by no model and is not run here).  The contexts include y0 = -1 (the start context), both
ids -1, equal ids, the blank and the last id of the vocabulary.
Tolerance per element, u = 2^-24: the conv's 2 cpg-term sum (the table form: two cpg-term sums and their add) at 4 u sqrt(n) of
its magnitude sum; relu passes an error on at most unchanged; then the DD-term projection at 4 u sqrt(DD + 1) of its magnitude sum
plus the hidden values' errors through |W|, added in quadrature (independent roundings)."""
import numpy as np
import pytest

from test_kernels_gpu import check, f64, prop, sum_tol

pytestmark = pytest.mark.gpu


def decoder64(t, y):
    emb, conv = f64(t["decoder.embedding.weight"]), f64(t["decoder.conv.weight"])
    Wd, bd = f64(t["joiner.decoder_proj.weight"]), f64(t["joiner.decoder_proj.bias"])
    DD, cpg, ctx = conv.shape
    assert ctx == 2 and y.shape[1] == 2
    e = np.stack([np.where(y[:, k:k + 1] >= 0, emb[np.maximum(y[:, k], 0)], 0.0) for k in range(2)], axis=2)     # [N, DD, tap]
    g0 = (np.arange(DD) // cpg) * cpg
    idx = g0[:, None] + np.arange(cpg)[None, :]                                                                  # [co, ci]
    x = e[:, idx, :]                                                                                             # [N, co, ci, tap]
    s = (x * conv[None]).sum((2, 3))
    mag = (np.abs(x) * np.abs(conv[None])).sum((2, 3))
    h = np.maximum(s, 0.0)
    htol = sum_tol(mag, 2 * cpg + 1)
    out = h @ Wd.T + bd
    omag = (h + htol) @ np.abs(Wd).T + np.abs(bd)
    return out, sum_tol(omag, DD + 1) + prop(htol, Wd), cpg


def contexts(V):
    rng = np.random.default_rng(8)
    fixed = [[-1, 0], [-1, -1], [0, 0], [-1, V - 1], [V - 1, V - 1], [V - 1, 0], [0, V - 1], [3, 3], [-1, 5]]
    return np.array(fixed + rng.integers(0, V, (40, 2)).tolist(), np.int64)


@pytest.mark.parametrize("which", ["cpg <= 4", "per-token table"])
def test_decoder_form(which, request):
    from k2transducerasr_amd.k2w import read_k2w
    if which == "cpg <= 4":
        model, path = request.getfixturevalue("hip_tiny"), request.getfixturevalue("tiny_model_path")
    else:
        model, path = request.getfixturevalue("hip_conformer"), request.getfixturevalue("conformer_tiny_path")
    _, t = read_k2w(path)
    y = contexts(model.vocab_size)
    want, tol, cpg = decoder64(t, y)
    assert (cpg <= 4) == (which == "cpg <= 4") and (cpg <= 4 or cpg == t["decoder.conv.weight"].shape[0])
    assert (want[0] != want[2]).any() and np.abs(want).max() > 0.1          # y0 = -1 is not y0 = blank; the outputs are not trivial
    got = model.decoder_proj(y)
    check(got, want, tol, f"decoder {which}")
    print(f"decoder {which}: largest error / tolerance {float((np.abs(f64(got) - want) / tol).max()):.3f}")
    # DecoderProj(null): N rows of the start context [-1, blank]
    got0 = model.decoder_proj(None, 3)
    check(got0, np.repeat(want[:1], 3, axis=0), np.repeat(tol[:1], 3, axis=0), f"decoder {which}, null contexts")
