"""The offline Conformer's half-precision switch on the device (k2hip_set_conformer_precision): level 2's two launches alone
(csrc/conformer_f16.hip: "conformer_scores_softmax_f16", "conformer_av_f16") against float64 over f16-rounded operands, and the switch
on conformer-tiny-test."""
import numpy as np
import pytest

from family_kernels import conf_queries, conf_scores, fbits
from test_kernels_gpu import SENTINEL, check, f64, nan, op, random_weights, score_eps, softmax64, softmax_tol, sum_tol, switch, uni  # noqa: F401

pytestmark = pytest.mark.gpu

r16 = lambda a: a.astype(np.float16).astype(np.float32)   # noqa: E731
MARK = 0x5a5a                                              # sentinel halves behind the last row of aw16
B, H = 2, 2


@pytest.mark.parametrize("T", [1, 15, 17, 33, 100, 257])   # one row; both sides of a strip and of a key tile; several runs per wave; a ragged last tile
@pytest.mark.parametrize("dk", [16, 32, 48, 64])           # the 16x16x16 group alone, one 16x16x32 group, both, two groups of 32
def test_scores_kernel_against_float64(op, dk, T):
    """Both query forms.  The reference rounds the operands to f16 as the kernel does and works in float64; f16 x f16 products are exact in
    float32, so the kernel's scores carry the rounding of a 2 dk-term float32 sum only: the float32 softmax bound of the Conformer scores
    test over the rounded operands, plus the final rounding of the weight, half an f16 ulp at the expected weight's upper end.  Fused
    form: scaling = 0.25 and q, u, v multiples of 2^-8 in [-2, 2], so q * scaling + u is exact in float32 however it is contracted.
    Every row stride is wider than its row, the padding is NaN."""
    rng = np.random.default_rng(100 * dk + T)
    D, Tp16 = H * dk, (T + 7) // 8 * 8
    grid = lambda *s: (rng.integers(-512, 513, s) / 256.0).astype(np.float32)   # noqa: E731
    for form in ("pre", "bias"):
        kmat, pp = nan(B * T, D + 8), uni(rng, 2 * T - 1, D, scale=0.5)
        kmat[:, :D] = uni(rng, B * T, D, scale=0.5)
        if form == "bias":
            ldq, scaling, qu, qv, bu, bv = 3 * D + 4, 0.25, nan(B * T, 3 * D + 4), None, grid(D), grid(D)
            qu[:, :D] = grid(B * T, D)
        else:
            ldq, scaling, bu, bv = 0, 1.0, None, None
            qu, qv = uni(rng, B * T, D, scale=1.5 * dk ** -0.5), uni(rng, B * T, D, scale=1.5 * dk ** -0.5)
        QU, QV = conf_queries(np.float32, qu, qv, bu, bv, B, T, D, ldq, scaling)
        s, mag = conf_scores(f64(r16(QU)), f64(r16(QV)), f64(r16(kmat[:, :D])), f64(r16(pp)), B, H, T)
        pw, centred = softmax64(s.reshape(B * H, T, T))
        tol32 = softmax_tol(pw, centred, score_eps(mag, 2 * dk).reshape(B * H, T, T))
        tol = tol32 + 0.5 * f64(np.spacing((pw + tol32).astype(np.float16)))
        aw16 = np.full(B * H * T * Tp16 + 8, MARK, np.uint16)
        op("conformer_scores_softmax_f16", [D + 8, B, H, T, D, ldq, fbits(scaling)], [qu, qv, kmat, pp, aw16.view(np.uint32), bu, bv], {4})
        assert (aw16[-8:] == MARK).all(), "written past the last row"
        w16 = aw16[:-8].reshape(B * H, T, Tp16)
        assert not w16[..., T:].any(), "pad columns are not +0"
        err = np.abs(f64(w16[..., :T].view(np.float16)) - pw)
        print(f"conformer scores f16 dk={dk} T={T} {form}: max err {err.max():.3g}, max err / tol {(err / tol).max():.3g}")
        assert np.isfinite(err).all() and (err <= tol).all(), form


@pytest.mark.parametrize("dk", [16, 64])
def test_apply_kernel_against_float64(op, dk):
    """the given f16 weights and f16-rounded values; a T-term float32 sum within 4 u sqrt(T) of its magnitude (av_out_ref's bound for its
    first sum).  T around the 64-key step, the 8-key operand and the 64-row workgroup; rows of the value buffer behind the last key and
    its row padding are NaN; the context has room for a third head and padding, which keep their sentinel."""
    rng = np.random.default_rng(dk)
    D, ldv, ldc = H * dk, H * dk + 8, 3 * dk + 4
    for T in (1, 31, 33, 64, 65, 130):
        Tp16 = (T + 7) // 8 * 8
        aw = r16(random_weights(rng, B, H, T, T, Tp16))
        v = nan(B * T + 70, ldv)
        v[:B * T, :D] = uni(rng, B * T, D)
        out = np.full((B * T, ldc), SENTINEL, np.float32)
        op("conformer_av_f16", [B, H, T, dk, ldv, ldc], [aw.astype(np.float16).view(np.uint32), v, out], {2})
        a, vv = f64(aw)[..., :T], f64(r16(v[:B * T, :D])).reshape(B, T, H, dk)
        want = np.einsum("bhtk,bkhc->bthc", a, vv).reshape(B * T, D)
        mag = np.einsum("bhtk,bkhc->bthc", a, np.abs(vv)).reshape(B * T, D)
        check(out[:, :D], want, sum_tol(mag, T), f"conformer_av_f16 dk={dk} T={T}")
        assert (out[:, D:] == SENTINEL).all(), (T, "columns of another head were written")


# max |level - off| / max |off| of the encoder output on conformer-tiny-test over the fixture utterances: four times the worst value
# measured on an MI355X (DESIGN.md "Half-precision operands in the offline Conformer encoder")
DEVIATION_BOUND = 4 * 1.194e-4   # measured: level 1 1.194e-4, level 2 1.188e-4


def test_switch_on_the_tiny_conformer(conformer_tiny_path, utts):
    from k2transducerasr_amd import Model
    from k2transducerasr_amd.k2w import read_k2w
    layers = int(read_k2w(conformer_tiny_path)[0]["num_encoder_layers"])
    model = Model(conformer_tiny_path, 0)
    x = model.pad_sequence([model.fbank(u) for u in utts]).reshape(len(utts), -1, 80)
    bits = lambda a: a.view(np.uint32)   # noqa: E731
    out, stats = {}, {}
    for level in (0, 1, 2):
        model.set_conformer_precision(level)
        out[level], stats[level] = model.encoder_proj(x), model.encoder_f16_stats()
    assert stats[0] == dict(launches=0, panels=0, panel_bytes=0)
    assert stats[1]["launches"] == 8 * layers and stats[1]["panels"] == 8 * layers
    assert stats[2] == dict(stats[1], launches=10 * layers)           # scores + apply of every layer; no new panels
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert not np.array_equal(bits(out[a]), bits(out[b])), (a, b)
    with switch("K2HIP_F16_CONFORMER_ATTN", 3):
        model.set_conformer_precision(0)
        model.set_conformer_precision(2)
        assert np.array_equal(bits(model.encoder_proj(x)), bits(out[1])), "level 2 with the float32 core is not level 1"
        assert model.encoder_f16_stats() == stats[1]
        model.set_conformer_precision(0)                               # (a call with the current level does nothing, counters included)
    for level in (2, 1, 0):                                            # (a change of level starts the counters again)
        model.set_conformer_precision(level)
        assert np.array_equal(bits(model.encoder_proj(x)), bits(out[level])), level
        assert model.encoder_f16_stats() == stats[level], level
    dev = {lv: np.abs(out[lv].astype(np.float64) - out[0]).max() / np.abs(out[0]).max() for lv in (1, 2)}
    print(f"conformer-tiny-test: max |level - off| / max |off| = level 1: {dev[1]:.3e}, level 2: {dev[2]:.3e} (bound {DEVIATION_BOUND:.3e})")
    model.close()
    assert dev[1] <= DEVIATION_BOUND and dev[2] <= DEVIATION_BOUND


def test_refusals(tmp_path, conformer_tiny_path, utts):
    """level 3 is invalid; the other families and the streaming Conformer have no such switch; a weight beyond f16 refuses the switch,
    naming its tensor, and the model goes on decoding in float32"""
    from k2transducerasr_amd import K2HipError, Model
    from k2transducerasr_amd.k2w import read_k2w, write_k2w
    from k2transducerasr_amd.synth import write_synthetic_model

    def code(model, level):
        with pytest.raises(K2HipError) as e:
            model.set_conformer_precision(level)
        return e.value.code, str(e.value)

    for preset in ("zipformer2-tiny-test", "conformer-streaming-tiny-test"):
        write_synthetic_model(str(tmp_path / "other.k2w"), preset)
        model = Model(str(tmp_path / "other.k2w"), 0)
        assert code(model, 1)[0] == -6, preset
        model.close()
    name = "encoder.encoder.layers.1.self_attn.out_proj.weight"
    meta, tensors = read_k2w(conformer_tiny_path)
    tensors = {k: np.array(v) for k, v in tensors.items()}
    tensors[name][3, 5] = 7e4
    write_k2w(str(tmp_path / "big.k2w"), meta, tensors.items())
    model = Model(str(tmp_path / "big.k2w"), 0)
    assert code(model, 3)[0] == -1
    want = model.offline_greedy_from_samples(utts)
    rc, msg = code(model, 1)
    assert rc == -1 and name in msg
    assert model.encoder_f16_stats()["panels"] == 0
    assert model.offline_greedy_from_samples(utts) == want
    model.close()
