"""The references of tests/test_family_kernels_gpu.py, checked without a GPU.

  * every float64 reference of tests/family_kernels.py against something written independently: the rel-shift scores (offline and
    streaming) against the attention of tests/torch_twin_conformer.py, the Zipformer v1 references against the matching pieces of
    tests/torch_twin_zipformer1.py (its attn_downsample, combine and conv methods called as they are; the pooling, attention and
    norm + bypass expressions, which that file has inline in layer(), restated here in its torch vocabulary: cumsum, as_strided),
    the LSTM cell against torch.nn.LSTMCell, basicnorm and the two conv0 forms against tests/torch_twin_lstm.py's basic_norm /
    double_swish and torch conv2d.  All in float64; the bound of each comparison is 1e-12 relative to O(1) values (float64 roundoff
    of sums of at most a few hundred terms).
  * every case of the GPU test with standin() -- the same formulas in float32 numpy -- in the kernel's place: the float64 reference and
    the stand-in must agree within the derived per-element tolerance, and check() holds every tolerance under its 2e-5 ceiling.  A
    bound so tight that correct float32 arithmetic misses it, or a loose one, fails here before any kernel is involved.  The same
    run shows that the cases launch every op the hook has for these families."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import family_kernels as fk
from torch_twin_conformer import ConformerStreamTwin, ConformerTwin
from torch_twin_lstm import basic_norm, double_swish
from torch_twin_zipformer1 import Zipformer1Twin

TOL = 1e-12


def r64(rng, *shape, scale=1.0):
    return rng.uniform(-1, 1, shape) * scale


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.abs(got - want).max() <= TOL * max(1.0, np.abs(want).max()), (what, np.abs(got - want).max())


@pytest.mark.parametrize("k", range(len(fk.CASES)), ids=[name.replace(" ", "_") for name, _ in fk.CASES])
def test_float32_standin_passes_every_case(k):
    fk.CASES[k][1](fk.Env(fk.standin, fk.null_switch))


def test_the_cases_launch_every_op():
    fk.CALLED.clear()
    for _, case in fk.CASES:
        case(fk.Env(lambda name, ia, bufs, outs, expect=0: fk.standin(name, ia, bufs, outs, expect), fk.null_switch))
    assert fk.CALLED == set(fk.SIM), sorted(set(fk.SIM) - fk.CALLED)


def attn_weights_times_v(pw, v, B, H, T, S):
    """what the twins return with identity out_proj: out[t, b, h dk + d] = sum_j pw[b H + h, t, j] v[j, b, h dk + d]"""
    dk = v.shape[2] // H
    return np.einsum("bhtj,jbhd->tbhd", pw.reshape(B, H, T, S), v.reshape(S, B, H, dk)).reshape(T, B, H * dk)


@pytest.mark.parametrize("T,H,dk", [(1, 2, 16), (7, 3, 16), (20, 2, 32)])
def test_rel_shift_scores_are_the_conformer_twins_attention(T, H, dk):
    rng = np.random.default_rng(T)
    B, D = 2, H * dk
    p = "a."
    t = {p + "in_proj.weight": r64(rng, 3 * D, D, scale=D ** -0.5), p + "in_proj.bias": r64(rng, 3 * D),
         p + "linear_pos.weight": r64(rng, D, D, scale=D ** -0.5), p + "pos_bias_u": r64(rng, H, dk), p + "pos_bias_v": r64(rng, H, dk),
         p + "out_proj.weight": np.eye(D), p + "out_proj.bias": np.zeros(D)}
    twin = ConformerTwin(dict(encoder_dims=D, num_encoder_layers=1, num_heads=H, cnn_module_kernels=31), t)
    x, pos = r64(rng, T, B, D), r64(rng, 1, 2 * T - 1, D)
    got = twin.self_attn(p, torch.from_numpy(x), torch.from_numpy(pos)).numpy()
    # the kernel's operands: in_proj rows stream-major (q | k | v), the projected table, the biases as [D] rows
    qkv = (x @ t[p + "in_proj.weight"].T + t[p + "in_proj.bias"]).transpose(1, 0, 2).reshape(B * T, 3 * D)
    pp = pos[0] @ t[p + "linear_pos.weight"].T
    ia = [3 * D, B, H, T, fk.r4(T), D, 3 * D, fk.fbits(dk ** -0.5)]
    bufs = [qkv, None, qkv[:, D:], pp, None, t[p + "pos_bias_u"].reshape(D), t[p + "pos_bias_v"].reshape(D)]
    scaling = float(fk.unbits(ia[7]))
    QU, QV = fk.conf_queries(np.float64, np.ascontiguousarray(qkv), None, bufs[5], bufs[6], B, T, D, 3 * D, scaling)
    QU += qkv[:, :D] * (dk ** -0.5 - scaling)          # (the twin scales by the float64 dk^-1/2, the launcher takes a float)
    QV += qkv[:, :D] * (dk ** -0.5 - scaling)
    s, _ = fk.conf_scores(QU, QV, qkv[:, D:2 * D], pp, B, H, T)
    pw = fk._softmax(s).reshape(B * H, T, T)
    v = qkv[:, 2 * D:].reshape(B, T, D).transpose(1, 0, 2)
    close(attn_weights_times_v(pw, v, B, H, T, T), got, "offline")
    # the GEMM form's reference on the same scores: ac / bd as scores_reference() hands them to conformer_softmax_shift
    ac = np.einsum("bihd,bjhd->bhij", QU.reshape(B, T, H, dk), qkv[:, D:2 * D].reshape(B, T, H, dk)).reshape(B * H, T, T)
    bd = np.einsum("bihd,nhd->bhin", QV.reshape(B, T, H, dk), pp.reshape(2 * T - 1, H, dk)).reshape(B * H, T, 2 * T - 1)
    bufs2 = [ac.copy(), bd]
    fk.sim_conformer_softmax_shift(np.float64, [B * H, T, T, 2 * T - 1], bufs2)
    close(attn_weights_times_v(bufs2[0], v, B, H, T, T), got, "offline, GEMM form")


@pytest.mark.parametrize("Tc,left,H,dk", [(4, 0, 2, 16), (5, 7, 2, 16), (16, 64, 2, 32)])
def test_stream_softmax_shift_is_the_stream_twins_attention(Tc, left, H, dk):
    rng = np.random.default_rng(Tc)
    D, S = H * dk, left + Tc
    plen = np.array([0, 1, max(left - 1, 0), left, left + 5], np.int64)
    B = len(plen)
    p = "a."
    t = {p + "in_proj.weight": r64(rng, 3 * D, D, scale=D ** -0.5), p + "in_proj.bias": r64(rng, 3 * D),
         p + "linear_pos.weight": r64(rng, D, D, scale=D ** -0.5), p + "pos_bias_u": r64(rng, H, dk), p + "pos_bias_v": r64(rng, H, dk),
         p + "out_proj.weight": np.eye(D), p + "out_proj.bias": np.zeros(D)}
    twin = ConformerStreamTwin(dict(encoder_dims=D, num_encoder_layers=1, num_heads=H, cnn_module_kernels=31, left_context=left), t)
    key, pos = r64(rng, S, B, D), r64(rng, 1, left + 2 * Tc - 1, D)
    src = key[left:]
    j = np.arange(S)
    mask = (j[None, :] < left) & (plen[:, None] <= left - 1 - j[None, :])       # kernels.h: slot j masked while plen <= left - 1 - j
    got = twin.attn_chunk(p, torch.from_numpy(src), torch.from_numpy(key), torch.from_numpy(pos), torch.from_numpy(mask)).numpy()
    W, bias = t[p + "in_proj.weight"], t[p + "in_proj.bias"]
    q = (src @ W[:D].T + bias[:D]) * dk ** -0.5
    k = key @ W[D:2 * D].T + bias[D:2 * D]
    v = key @ W[2 * D:].T + bias[2 * D:]
    pm = (pos[0] @ t[p + "linear_pos.weight"].T).reshape(-1, H, dk)
    qu = (q.reshape(Tc, B, H, dk) + t[p + "pos_bias_u"]).transpose(1, 2, 0, 3)     # [B, H, Tc, dk]
    qv = (q.reshape(Tc, B, H, dk) + t[p + "pos_bias_v"]).transpose(1, 2, 0, 3)
    ac = np.einsum("bhid,jbhd->bhij", qu, k.reshape(S, B, H, dk)).reshape(B * H, Tc, S)
    bd = np.einsum("bhid,nhd->bhin", qv, pm).reshape(B * H, Tc, left + 2 * Tc - 1)
    bufs = [ac.copy(), bd, plen]
    fk.sim_conformer_softmax_shift_stream(np.float64, [B, H, Tc, left, S, left + 2 * Tc - 1], bufs)
    close(attn_weights_times_v(bufs[0], v, B, H, Tc, S), got, "stream")


def z1_twin(t):
    return Zipformer1Twin(dict(encoder_dims="8", attention_dims="8", num_encoder_layers="1", num_heads="2", cnn_module_kernels="5",
                               downsampling_factors="1", pos_dim="4"), t)


def test_z1_references_are_the_zipformer1_twins_pieces():
    rng = np.random.default_rng(5)
    # AttentionDownsample (the twin's method): ds 2 / 4 / 16, T no multiple
    for ds, T, Din in ((2, 7, 12), (4, 9, 8), (16, 35, 20), (1, 3, 4)):
        B = 2
        x, query = r64(rng, B, T, Din), r64(rng, Din)
        got = z1_twin({"d.query": query}).attn_downsample("d.", torch.from_numpy(x.transpose(1, 0, 2).copy()), ds).numpy()
        Td = (T + ds - 1) // ds
        bufs = [x, query, np.zeros((B, Td, Din + 4))]
        fk.sim_z1_attn_downsample(np.float64, [B, T, Din, Din + 4, ds], bufs)
        close(bufs[2][..., :Din], got.transpose(1, 0, 2), f"attn_downsample ds={ds}")
        g = [x, np.zeros((B, Td, ds * Din))]
        fk.sim_z1_group_rows(np.float64, [B, T, Din, ds], g)     # the twin's `flat`: the group's frames side by side, last one repeated
        xt = torch.from_numpy(x.transpose(1, 0, 2).copy())
        xt = torch.cat([xt, xt[-1:].expand(Td * ds - T, B, Din)], dim=0).reshape(Td, ds, B, Din).permute(0, 2, 1, 3).reshape(Td, B, ds * Din)
        close(g[1], xt.numpy().transpose(1, 0, 2), f"group_rows ds={ds}")
    # SimpleCombiner (the twin's static method), plain and with SimpleUpsample's xd.expand + bias in front
    for d1, d2 in ((6, 10), (10, 10), (14, 10)):
        for ds in (0, 2, 4):
            B, T = 2, 7
            Td = (T + ds - 1) // ds if ds else 0
            s1, w1 = r64(rng, B * T, d1), np.array([0.3])
            if ds:
                xd, ub = r64(rng, B, Td, d2), r64(rng, ds, d2)
                up = (torch.from_numpy(xd).unsqueeze(2).expand(B, Td, ds, d2) + torch.from_numpy(ub)).reshape(B, Td * ds, d2)[:, :T]
                s2t, s2, ubb = up, xd, ub
            else:
                s2 = r64(rng, B * T, d2)
                s2t, ubb = torch.from_numpy(s2).reshape(B, T, d2), None
            got = Zipformer1Twin.combine(torch.from_numpy(s1).reshape(B, T, d1), s2t, torch.tensor(0.3, dtype=torch.float64)).numpy()
            bufs = [s1, s2, w1, ubb, np.zeros((B * T, d2))]
            fk.sim_z1_combine(np.float64, [d1, d2, ds or 1, B, T, Td], bufs)
            close(bufs[4].reshape(B, T, d2), got, f"combine d1={d1} d2={d2} ds={ds}")
    # ConvolutionModule.streaming_forward (the twin's method; identity pointwise convolutions around the part the kernel computes)
    for K, Tc in ((5, 1), (5, 9), (9, 4), (31, 40)):
        B, D = 2, 6
        q = "l.conv_module1."
        t = {q + "pointwise_conv1.weight": np.eye(2 * D)[:, :, None], q + "pointwise_conv1.bias": np.zeros(2 * D),
             q + "depthwise_conv.weight": r64(rng, D, 1, K), q + "depthwise_conv.bias": r64(rng, D),
             q + "pointwise_conv2.weight": np.eye(D)[:, :, None], q + "pointwise_conv2.bias": np.zeros(D)}
        x2, cache = r64(rng, B, Tc, 2 * D, scale=2.0), r64(rng, B, D, K - 1)
        y, newc = z1_twin(t).conv("l.", 1, torch.from_numpy(x2.transpose(1, 0, 2).copy()), torch.from_numpy(cache))
        ss, off = D * (K - 1) + 5, 3
        pool = np.zeros(B * ss)
        slots = np.array([1, 0], np.int32)
        for b in range(B):
            pool[slots[b] * ss + off:slots[b] * ss + off + D * (K - 1)] = cache[b].reshape(-1)
        bufs = [x2, pool, slots, t[q + "depthwise_conv.weight"].reshape(D, K), t[q + "depthwise_conv.bias"], np.zeros((B * Tc, D))]
        fk.sim_z1_glu_conv(np.float64, [ss, off, B, Tc, D, K], bufs)
        close(bufs[5].reshape(B, Tc, D), y.numpy().transpose(1, 0, 2), f"glu_conv K={K} Tc={Tc}")
        for b in range(B):
            close(pool[slots[b] * ss + off:slots[b] * ss + off + D * (K - 1)].reshape(D, K - 1), newc[b].numpy(), f"glu_conv cache K={K} Tc={Tc}")
    # pooling: torch_twin_zipformer1.py layer(), "# pooling" (cumsum form), two chunks
    B, Tc, D = 2, 5, 6
    ss, avg_off, len_off = D + 4, 3, 1
    pool, slots = np.zeros(B * ss), np.array([1, 0], np.int32)
    clen, cavg = torch.zeros(B, dtype=torch.float64), torch.zeros(B, D, dtype=torch.float64)
    for _ in range(2):
        x = r64(rng, B, Tc, D)
        src = torch.from_numpy(x.transpose(1, 0, 2).copy())
        xx = src.cumsum(dim=0) + (cavg * clen.unsqueeze(1)).unsqueeze(0)
        cum = torch.arange(1, Tc + 1).unsqueeze(1) + clen.unsqueeze(0)
        xx = xx * (1.0 / cum).unsqueeze(2)
        clen, cavg = clen + Tc, xx[-1]
        bufs = [x, pool, slots, np.zeros((B, Tc, D))]
        fk.sim_z1_pool(np.float64, [ss, avg_off, len_off, B, Tc, D], bufs)
        close(bufs[3], xx.numpy().transpose(1, 0, 2), "pool")
        for b in range(B):
            close(pool[slots[b] * ss + avg_off:slots[b] * ss + avg_off + D], cavg[b].numpy(), "pool cached_avg")
            assert pool[slots[b] * ss + len_off] == float(clen[b])
    # attention scores: layer()'s as_strided rel-shift of the positional product
    for hd, H, Tc, L in ((4, 2, 3, 0), (8, 2, 5, 6)):
        B, A, P = 2, hd * H, 4
        ld, KL = 2 * A + A // 2 + P * H, L + Tc
        xp, kcat, pos = r64(rng, B * Tc, ld), r64(rng, B * KL, A), r64(rng, 2 * Tc - 1 + L, P * H)
        x3 = torch.from_numpy(xp.reshape(B, Tc, ld).transpose(1, 0, 2).copy())
        q = x3[..., :A].reshape(Tc, B, H, hd).permute(1, 2, 0, 3)
        pq = x3[..., 2 * A + A // 2:].reshape(Tc, B, H, P).permute(1, 2, 0, 3)
        kk = torch.from_numpy(kcat.reshape(B, KL, A).transpose(1, 0, 2).copy()).reshape(KL, B, H, hd).permute(1, 2, 3, 0)
        pw = torch.matmul(pq, torch.from_numpy(pos).reshape(1, 2 * Tc - 1 + L, H, P).permute(0, 2, 3, 1)).contiguous()
        pw = pw.as_strided((B, H, Tc, KL), (pw.stride(0), pw.stride(1), pw.stride(2) - pw.stride(3), pw.stride(3)),
                           storage_offset=pw.stride(3) * (Tc - 1))
        aw = (torch.matmul(q, kk) + pw).softmax(dim=-1).numpy()            # [B, H, Tc, KL]
        bufs = [xp, kcat, pos, np.zeros((H, B, Tc, KL + 4))]
        fk.sim_z1_attn(np.float64, [ld, B, Tc, L, KL + 4, H, A], bufs)
        close(bufs[3][..., :KL], aw.transpose(1, 0, 2, 3), f"z1_attn hd={hd}")
    # norm_final + bypass: the last two lines of layer()
    M, D = 5, 12
    x, o, le, bs = r64(rng, M, D, scale=3.0), r64(rng, M, D), np.array([-1.2]), np.array([0.6])
    xt, ot = torch.from_numpy(x), torch.from_numpy(o)
    nrm = xt * (xt.pow(2).mean(dim=-1, keepdim=True) + torch.tensor(le).exp()) ** -0.5
    bufs = [x, o, le, bs, np.zeros((M, D))]
    fk.sim_z1_norm_bypass(np.float64, [M, D], bufs)
    close(bufs[4], (ot + (nrm - ot) * 0.6).numpy(), "norm_bypass")
    close(fk.basicnorm64(x, le[0])[0], nrm.numpy(), "basicnorm64")
    # z1_mean / z1_add_bcast: PoolingModule.forward's mean over the frames, added to every frame
    x, v = r64(rng, 2, 9, 6), r64(rng, 2, 6)
    bufs = [x, np.zeros((2, 6))]
    fk.sim_z1_mean(np.float64, [2, 9, 6], bufs)
    close(bufs[1], torch.from_numpy(x).mean(dim=1).numpy(), "mean")
    bufs = [x.copy(), v]
    fk.sim_z1_add_bcast(np.float64, [2, 9, 6], bufs)
    close(bufs[0], (torch.from_numpy(x) + torch.from_numpy(v).unsqueeze(1)).numpy(), "add_bcast")


def test_lstm_references_are_torch():
    rng = np.random.default_rng(6)
    B, Hh, Din = 3, 10, 7
    cell = torch.nn.LSTMCell(Din, Hh).double()
    x, h, c = r64(rng, B, Din, scale=4.0), r64(rng, B, Hh, scale=4.0), r64(rng, B, Hh, scale=2.0)
    with torch.no_grad():
        for prm in cell.parameters():
            prm.mul_(6.0)                      # pre-activations well into saturation
        h1, c1 = cell(torch.from_numpy(x), (torch.from_numpy(h), torch.from_numpy(c)))
        gx = (torch.from_numpy(x) @ cell.weight_ih.T + cell.bias_ih).numpy()
        gh = (torch.from_numpy(h) @ cell.weight_hh.T + cell.bias_hh).numpy()
    assert np.abs(gx + gh).max() > 15
    bufs = [gx.copy(), gh.copy(), c.copy(), np.zeros((B, Hh))]
    fk.sim_lstm_cell(np.float64, [4 * Hh, 4 * Hh, B, Hh], bufs)
    close(bufs[2], c1.numpy(), "lstm_cell c")
    close(bufs[3], h1.numpy(), "lstm_cell h")
    bufs = [gx + gh, c.copy(), np.zeros((B, Hh))]
    fk.sim_lstm_cell_rows(np.float64, [B, Hh], bufs)
    close(bufs[1], c1.numpy(), "lstm_cell_rows c")
    close(bufs[2], h1.numpy(), "lstm_cell_rows h")
    # the frame kernels: x1 = Y[lo + z][frame s - lo - z] + sum of partials; Y[lo + z + 1][frame] = basic_norm(x1 + b2 + partials)
    n, T, D, lo, s, S, Lyr = 2, 4, 8, 1, 3, 3, 4
    SY, pstride, lstride = B * T * D + 8, n * B * D + 4, D + 4
    Y, hp, fp = r64(rng, (Lyr + 1) * SY), r64(rng, S * pstride), r64(rng, S * pstride)
    b2, eps = r64(rng, Lyr * lstride), r64(rng, Lyr * lstride)
    bufs = [Y, hp, np.zeros((n * B, D)), np.zeros((n * B, D))]
    fk.sim_lstm_add_frame(np.float64, [SY, pstride, S, n, B, T, D, lo, s], bufs)
    Yt = torch.from_numpy(np.stack([Y[l * SY:l * SY + B * T * D].reshape(B, T, D) for l in range(Lyr + 1)]))
    part = lambda p: torch.from_numpy(np.stack([p[q * pstride:q * pstride + n * B * D] for q in range(S)])).sum(0).reshape(n, B, D)
    x1 = torch.stack([Yt[lo + z, :, s - lo - z] + part(hp)[z] for z in range(n)])
    close(bufs[2].reshape(n, B, D), part(hp).numpy(), "add_frame h")
    close(bufs[3].reshape(n, B, D), x1.numpy(), "add_frame x1")
    Y2 = Y.copy()
    fk.sim_lstm_norm_frame(np.float64, [pstride, S, lstride, SY, n, B, T, D, lo, s], [x1.numpy().reshape(n * B, D), fp, b2, eps, Y2])
    for z in range(n):
        l = lo + z
        want = basic_norm(x1[z] + torch.from_numpy(b2[l * lstride:l * lstride + D]) + part(fp)[z], torch.tensor(eps[l * lstride]))
        Yt[l + 1, :, s - lo - z] = want
    close(np.stack([Y2[l * SY:l * SY + B * T * D].reshape(B, T, D) for l in range(Lyr + 1)]), Yt.numpy(), "norm_frame Y")


def test_basicnorm_and_conv0_references_are_the_twins():
    rng = np.random.default_rng(7)
    x, le = r64(rng, 5, 12, scale=3.0), np.array([-0.7])
    bufs = [x, le, np.zeros((5, 12))]
    fk.sim_basicnorm(np.float64, [5, 12], bufs)
    close(bufs[2], basic_norm(torch.from_numpy(x), torch.from_numpy(le)).numpy(), "basicnorm")
    for tpad, name in ((1, "conv0_pad1_dswish"), (0, "conv0_nopad_dswish")):
        for T, Fq in ((3, 7), (4, 5), (11, 9)):
            B = 2
            xin, w, b = r64(rng, B, T, Fq), r64(rng, 8, 1, 3, 3), r64(rng, 8)
            y = double_swish(F.conv2d(torch.from_numpy(xin).unsqueeze(1), torch.from_numpy(w), torch.from_numpy(b), padding=(tpad, 1)))
            bufs = [xin, w.reshape(72), b, np.zeros((B, T - 2 + 2 * tpad, Fq, 8))]
            fk.SIM[name](np.float64, [B, T, Fq], bufs)
            close(bufs[3], y.permute(0, 2, 3, 1).numpy(), f"{name} T={T}")
    # dwconv_valid_dswish: the stream twin's conv_chunk core, a valid depthwise conv1d over [cache ; chunk] frames
    B, Tc, D, K = 2, 6, 5, 15
    cat, w, b = r64(rng, B, K - 1 + Tc, D), r64(rng, K, D), r64(rng, D)
    y = double_swish(F.conv1d(torch.from_numpy(cat).permute(0, 2, 1), torch.from_numpy(w.T.copy()).unsqueeze(1), torch.from_numpy(b), groups=D))
    bufs = [cat, w, b, np.zeros((B, Tc, D))]
    fk.sim_dwconv_valid_dswish(np.float64, [B, Tc, D, K], bufs)
    close(bufs[3], y.permute(0, 2, 1).numpy(), "dwconv_valid_dswish")
