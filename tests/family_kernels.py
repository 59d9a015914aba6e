"""Cases and float64 references for the kernels of the Conformer, Zipformer v1 and LSTM families (csrc/conformer.hip,
zipformer1.hip, lstm.hip and the elementwise.hip kernels only they use), one launch at a time through k2hip_debug_op_run.

Importable without a GPU: tests/test_family_kernels_gpu.py runs every case() below with the `op` fixture of test_kernels_gpu.py,
tests/test_family_kernels_ref.py runs the same cases with standin() -- a float32 numpy evaluation of the same formulas -- in the
kernel's place, and holds the references to the torch twins.

Every operation is written ONCE, as SIM[name](dt, iargs, bufs): it takes the launcher's int arguments and buffers exactly as the
hook takes them and rewrites the buffers in place in arithmetic of type dt.  want() runs it on float64 copies (the reference),
standin() on the float32 buffers themselves.

Tolerances, per element, in units of u = 2^-24, from the helpers of test_kernels_gpu.py (sum_tol, score_eps, softmax_tol, act_tol):
  * one fp32 operation on exact operands: u of its result's magnitude (bounded by the operands' magnitudes);
  * BasicNorm y = x (mean(x^2) + e^eps)^-1/2: |y| (2 u sqrt(D) + 12 u) -- the D-term square sum at 4 u sqrt(D) relative, halved by the
    square root; then libm expf (3 ulp = 6 u, on the eps share only), the add, divide, square root, reciprocal and final product;
    an error dv of its input adds sc dv + |y| sc rms(dv) (the second term: d(ms) <= 2 sqrt(ms) rms(dv), Cauchy-Schwarz);
  * the LSTM cell uses libm expf / tanhf, not the fast intrinsics.  OpenCL's bounds for them (the ROCm device library's contract):
    exp 3 ulp, tanh 5 ulp, divide 2.5 ulp, 1 ulp = 2 u.  sigmoid = 1 / (1 + e^-z): 6 u (exp, weighted by e / (1 + e) <= 1) + u (add)
    + 5 u (divide) = 12 u relative, + dz / 4 for an error dz of its argument; tanh: 10 u relative + dz.  These replace act_tol's
    (|z| + 4) u, which models the hardware exp whose error grows with the argument."""
import contextlib

import numpy as np

from test_kernels_gpu import (ERR_UNSUPPORTED, SENTINEL, U, Ring, act_tol, check, dswish64, f64, nan, score_eps, sigmoid64, softmax64,
                              softmax_tol, sum_tol, switch, uni)

LIBM_SIG = 12.0 * U
LIBM_TANH = 10.0 * U
NORM_U = 12.0 * U


def fbits(x):
    """a float argument of a launcher as the hook takes it: the IEEE-754 bits in the int slot"""
    return int(np.array([x], np.float32).view(np.uint32)[0])


def unbits(i):
    return np.array([int(i)], np.uint32).view(np.float32)[0]


def r4(n):
    return (n + 3) // 4 * 4


class Env:
    """what a case runs on: op(name, iargs, bufs, outs, expect=0) and the branch-switch context manager"""

    def __init__(self, op, sw):
        self.op, self.switch = op, sw


# ---- the operations ----------------------------------------------------------------------------------------------------------------------

def _softmax(s, mask=None):
    s = s.copy()
    if mask is not None:
        s[mask] = -np.inf
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def _dswish(z):
    one = z.dtype.type(1.0)
    return z / (one + np.exp(one - z))


def _sigmoid(z):
    one = z.dtype.type(1.0)
    return one / (one + np.exp(-z))


def _basicnorm(x, log_eps):
    ms = (x * x).mean(-1, keepdims=True)
    return x * (ms + np.exp(log_eps)) ** x.dtype.type(-0.5)


def conf_queries(dt, qu, qv, bu, bv, B, T, D, ldq, scaling):
    """the two query operands [B*T, D]: as given, or q * scaling + pos_bias_u / pos_bias_v from the in_proj rows (conformer.hip:189)"""
    if bu is None:
        return qu.reshape(B * T, D), qv.reshape(B * T, D)
    q = qu.reshape(B * T, ldq)[:, :D] * dt(scaling)
    return q + bu, q + bv


def conf_scores(QU, QV, k, pp, B, H, T):
    """conformer.hip:155-157: s[b,h,i,j] = (q_i + u).k_j + (q_i + v).p[T-1-i+j]; also the sum of the products' magnitudes"""
    dk = QU.shape[1] // H
    qu, qv, kk = QU.reshape(B, T, H, dk), QV.reshape(B, T, H, dk), k.reshape(B, T, H, dk)
    p = pp.reshape(2 * T - 1, H, dk)
    idx = (T - 1) - np.arange(T)[:, None] + np.arange(T)[None, :]
    rows = np.arange(T)[:, None]
    s = np.einsum("bihd,bjhd->bhij", qu, kk) + np.einsum("bihd,nhd->bhin", qv, p)[:, :, rows, idx]
    mag = np.einsum("bihd,bjhd->bhij", np.abs(qu), np.abs(kk)) + np.einsum("bihd,nhd->bhin", np.abs(qv), np.abs(p))[:, :, rows, idx]
    return s, mag


def sim_conformer_qprep(dt, ia, b):
    M, D, sbits, ldq = ia
    qu, qv = conf_queries(dt, b[0], None, b[1], b[2], M, 1, D, ldq or 3 * D, unbits(sbits))
    b[3].reshape(M, D)[...] = qu
    b[4].reshape(M, D)[...] = qv


def sim_conformer_scores_softmax(dt, ia, b):
    ldk, B, H, T, Tp, D, ldq, sbits = ia
    QU, QV = conf_queries(dt, b[0], b[1], b[5], b[6], B, T, D, ldq, unbits(sbits))
    s, _ = conf_scores(QU, QV, b[2].reshape(B * T, ldk)[:, :D], b[3], B, H, T)
    aw = b[4].reshape(B * H, T, Tp)
    aw[:, :, :T] = _softmax(s).reshape(B * H, T, T)
    aw[:, :, T:] = 0


def shifted(bd, Tq, KL):
    """rel_shift in gather form: out[z,i,j] = bd[z,i,Tq-1-i+j], j < KL"""
    idx = (Tq - 1) - np.arange(Tq)[:, None] + np.arange(KL)[None, :]
    return bd[:, np.arange(Tq)[:, None], idx]


def sim_conformer_softmax_shift(dt, ia, b):
    Z, T, Tp, NPp = ia
    ac, bd = b[0].reshape(Z, T, Tp), b[1].reshape(Z, T, NPp)
    w = _softmax(ac[:, :, :T] + shifted(bd, T, T))
    ac[:, :, :T] = w
    ac[:, :, T:] = 0


def stream_mask(plen, B, H, Tc, left):
    """kernels.h conformer_softmax_shift_stream: left slot j is masked while plen[b] <= left - 1 - j; [B*H, Tc, KL]"""
    j = np.arange(left + Tc)
    m = (j[None, :] < left) & (np.asarray(plen)[:, None] <= left - 1 - j[None, :])
    return np.broadcast_to(m[:, None, None, :], (B, H, Tc, left + Tc)).reshape(B * H, Tc, left + Tc)


def sim_conformer_softmax_shift_stream(dt, ia, b):
    B, H, Tc, left, KLp, NPp = ia
    KL = left + Tc
    ac, bd = b[0].reshape(B * H, Tc, KLp), b[1].reshape(B * H, Tc, NPp)
    w = _softmax(ac[:, :, :KL] + shifted(bd, Tc, KL), stream_mask(b[2], B, H, Tc, left))
    ac[:, :, :KL] = w
    ac[:, :, KL:] = 0


def sim_slice_rows(dt, ia, b):
    B, Tin, row0, Tout, D = ia
    b[1].reshape(B, Tout, D)[...] = b[0].reshape(B, Tin, D)[:, row0:row0 + Tout]


def valid_conv(cat, w_kd, bias, Tc, K):
    """z[b,t,:] = bias + sum_k w[k] cat[b,t+k,:] and the magnitude sum"""
    z = np.broadcast_to(bias, cat[:, :Tc].shape).copy()
    zm = np.abs(z)
    for k in range(K):
        z += w_kd[k] * cat[:, k:k + Tc]
        zm += np.abs(w_kd[k]) * np.abs(cat[:, k:k + Tc])
    return z, zm


def sim_dwconv_valid_dswish(dt, ia, b):
    B, Tc, D, K = ia
    z, _ = valid_conv(b[0].reshape(B, K - 1 + Tc, D), b[1].reshape(K, D), b[2], Tc, K)
    b[3].reshape(B, Tc, D)[...] = _dswish(z)


def sim_z1_pool(dt, ia, b):
    """zipformer1.hip:16-17 (PoolingModule.streaming_forward)"""
    ss, avg_off, len_off, B, Tc, D = ia
    x, pool, slots, out = b[0].reshape(B, Tc, D), b[1], b[2], b[3].reshape(B, Tc, D)
    for s in range(B):
        st = pool[slots[s] * ss:(slots[s] + 1) * ss]
        ln = st[len_off]
        cum = np.cumsum(x[s], axis=0) + st[avg_off:avg_off + D] * ln
        out[s] = cum * (dt(1.0) / (np.arange(1, Tc + 1, dtype=dt) + ln))[:, None]
        st[avg_off:avg_off + D] = out[s, -1]
        st[len_off] = ln + dt(Tc)


def z1_scores(qkvp, ld, kcat, pp, B, Tc, L, H, A):
    """zipformer1.hip:38-40: s[h,b,i,j] = q_i.k_j + p_i.pos[Tc-1-i+j] over KL = L + Tc keys, and the magnitude sum"""
    hd, KL = A // H, L + Tc
    x = qkvp.reshape(B, Tc, ld)
    q = x[:, :, :A].reshape(B, Tc, H, hd)
    p = x[:, :, 2 * A + A // 2:2 * A + A // 2 + 4 * H].reshape(B, Tc, H, 4)
    k = kcat.reshape(B, KL, H, hd)
    e = pp.reshape(2 * Tc - 1 + L, H, 4)
    idx = (Tc - 1) - np.arange(Tc)[:, None] + np.arange(KL)[None, :]
    rows = np.arange(Tc)[:, None]
    s = np.einsum("bihd,bjhd->hbij", q, k) + np.einsum("bihc,nhc->hbin", p, e)[:, :, rows, idx]
    mag = np.einsum("bihd,bjhd->hbij", np.abs(q), np.abs(k)) + np.einsum("bihc,nhc->hbin", np.abs(p), np.abs(e))[:, :, rows, idx]
    return s, mag


def sim_z1_attn(dt, ia, b):
    ld, B, Tc, L, KLp, H, A = ia
    s, _ = z1_scores(b[0], ld, b[1], b[2], B, Tc, L, H, A)
    aw = b[3].reshape(H, B, Tc, KLp)
    aw[..., :L + Tc] = _softmax(s)
    aw[..., L + Tc:] = 0


def z1_conv_parts(x2, cache, w, bias, B, Tc, D, K):
    """zipformer1.hip:83-85: cat = [cache (K-1) ; GLU(x2)] per stream [B, K-1+Tc, D], z = bias + depthwise conv, its magnitude sum"""
    a = x2.reshape(B, Tc, 2 * D)
    g = a[..., :D] * _sigmoid(a[..., D:])
    cat = np.concatenate([cache.transpose(0, 2, 1), g], axis=1)
    z, zm = valid_conv(cat, w.reshape(D, K).T, bias, Tc, K)
    return cat, z, zm


def sim_z1_glu_conv(dt, ia, b):
    ss, off, B, Tc, D, K = ia
    pool, slots = b[1], b[2]
    sl = [pool[s * ss + off:s * ss + off + D * (K - 1)].reshape(D, K - 1) for s in slots]
    cat, z, _ = z1_conv_parts(b[0], np.stack(sl), b[3], b[4], B, Tc, D, K)
    for s in range(B):
        sl[s][...] = cat[s, Tc:].T
    b[5].reshape(B, Tc, D)[...] = _dswish(z)


def sim_z1_norm_bypass(dt, ia, b):
    M, D = ia
    x, o = b[0].reshape(M, D), b[1].reshape(M, D)
    b[4].reshape(M, D)[...] = o + (_basicnorm(x, b[2][0]) - o) * b[3][0]


def attn_ds_parts(x, query, B, T, Din, ds):
    """zipformer1.hip:138-139: the ds frames of every group (last frame repeated), their scores <frame, query> and magnitudes"""
    Td = (T + ds - 1) // ds
    idx = np.minimum(np.arange(Td)[:, None] * ds + np.arange(ds)[None, :], T - 1)
    fr = x.reshape(B, T, Din)[:, idx]                       # [B, Td, ds, Din]
    return fr, fr @ query, np.abs(fr) @ np.abs(query)


def sim_z1_attn_downsample(dt, ia, b):
    B, T, Din, ldy, ds = ia
    fr, s, _ = attn_ds_parts(b[0], b[1], B, T, Din, ds)
    b[2].reshape(B, fr.shape[1], ldy)[:, :, :Din] = (fr * _softmax(s)[..., None]).sum(2)


def sim_z1_mean(dt, ia, b):
    B, T, D = ia
    b[1].reshape(B, D)[...] = (b[0].reshape(B, T, D) * (dt(1.0) / dt(T))).sum(1)


def sim_z1_add_bcast(dt, ia, b):
    B, T, D = ia
    b[0].reshape(B, T, D)[...] += b[1].reshape(B, 1, D)


def sim_z1_group_rows(dt, ia, b):
    B, T, Din, ds = ia
    Td = (T + ds - 1) // ds
    idx = np.minimum(np.arange(Td)[:, None] * ds + np.arange(ds)[None, :], T - 1)
    b[1].reshape(B, Td, ds, Din)[...] = b[0].reshape(B, T, Din)[:, idx]


def combine_src2(s2, ub, ds, B, T, Td, d2):
    """src2 of SimpleCombiner: as given, or SimpleUpsample(xd [B,Td,d2], ub [ds,d2])[:T] = xd[b, t / ds] + ub[t % ds]"""
    if ub is None:
        return s2.reshape(B, T, d2)
    t = np.arange(T)
    return s2.reshape(B, Td, d2)[:, t // ds] + ub.reshape(ds, d2)[t % ds]


def sim_z1_combine(dt, ia, b):
    d1, d2, ds, B, T, Td = ia
    w = b[2][0]
    a = np.zeros((B, T, d2), dt)
    n = min(d1, d2)
    a[..., :n] = b[0].reshape(B, T, d1)[..., :n] * w
    b[4].reshape(B, T, d2)[...] = a + combine_src2(b[1], b[3], ds, B, T, Td, d2) * (dt(1.0) - w)


def lstm_gates(pre, c, Hh):
    """torch.nn.LSTM's gate order i, f, g, o (lstm.hip:11): the new cell and hidden-before-projection, and the four gates"""
    i, f, g, o = _sigmoid(pre[:, :Hh]), _sigmoid(pre[:, Hh:2 * Hh]), np.tanh(pre[:, 2 * Hh:3 * Hh]), _sigmoid(pre[:, 3 * Hh:4 * Hh])
    cn = f * c + i * g
    return cn, o * np.tanh(cn), (i, f, g, o)


def sim_lstm_cell(dt, ia, b):
    ldgx, ldgh, B, Hh = ia
    pre = b[0].reshape(B, ldgx)[:, :4 * Hh] + b[1].reshape(B, ldgh)[:, :4 * Hh]
    cn, hf, _ = lstm_gates(pre, b[2].reshape(B, Hh), Hh)
    b[2].reshape(B, Hh)[...] = cn
    b[3].reshape(B, Hh)[...] = hf


def sim_lstm_cell_rows(dt, ia, b):
    rows, Hh = ia
    cn, hf, _ = lstm_gates(b[0].reshape(rows, 4 * Hh), b[1].reshape(rows, Hh), Hh)
    b[1].reshape(rows, Hh)[...] = cn
    b[2].reshape(rows, Hh)[...] = hf


def partial_sum(p, pstride, S, n):
    acc = p[:n].copy()
    for q in range(1, S):
        acc += p[q * pstride:q * pstride + n]
    return acc


def sim_lstm_add_frame(dt, ia, b):
    """kernels.h lstm_add_frame: row r = z B + b; layer lo + z works on frame t = s - lo - z"""
    SY, pstride, S, n, B, T, D, lo, s = ia
    hv = partial_sum(b[1], pstride, S, n * B * D).reshape(n, B, D)
    b[2].reshape(n, B, D)[...] = hv
    for z in range(n):
        t = s - lo - z
        b[3].reshape(n, B, D)[z] = b[0][(lo + z) * SY:(lo + z) * SY + B * T * D].reshape(B, T, D)[:, t] + hv[z]


def sim_lstm_norm_frame(dt, ia, b):
    pstride, S, lstride, SY, n, B, T, D, lo, s = ia
    a = partial_sum(b[1], pstride, S, n * B * D).reshape(n, B, D)
    for z in range(n):
        t, l = s - lo - z, lo + z
        v = (a[z] + b[2][l * lstride:l * lstride + D]) + b[0].reshape(n, B, D)[z]
        b[4][(l + 1) * SY:(l + 1) * SY + B * T * D].reshape(B, T, D)[:, t] = _basicnorm(v, b[3][l * lstride])


def sim_add_inplace(dt, ia, b):
    b[0][:ia[0]] += b[1][:ia[0]]


def sim_gather_rows(dt, ia, b):
    ss, off, B, width = ia
    for s in range(B):
        b[2].reshape(B, width)[s] = b[0][b[1][s] * ss + off:b[1][s] * ss + off + width]


def sim_scatter_rows(dt, ia, b):
    ss, off, ldin, B, width = ia
    for s in range(B):
        b[0][b[1][s] * ss + off:b[1][s] * ss + off + width] = b[2].reshape(B, ldin)[s, :width]


def sim_basicnorm(dt, ia, b):
    M, D = ia
    b[2].reshape(M, D)[...] = _basicnorm(b[0].reshape(M, D), b[1][0])


def conv0_parts(x, w, bias, B, T, F, tpad):
    """elementwise.hip:46-47: 1 -> 8 channels, 3 x 3, padding (tpad, 1); z [B, T - 2 + 2 tpad, F, 8] and the magnitude sum"""
    T1 = T - 2 + 2 * tpad
    xp = np.zeros((B, T + 2 * tpad, F + 2), x.dtype)
    xp[:, tpad:tpad + T, 1:1 + F] = x.reshape(B, T, F)
    W = w.reshape(8, 3, 3)
    z = np.broadcast_to(bias.reshape(8), (B, T1, F, 8)).copy()
    zm = np.abs(z)
    for kt in range(3):
        for kf in range(3):
            sl = xp[:, kt:kt + T1, kf:kf + F, None]
            z += sl * W[:, kt, kf]
            zm += np.abs(sl) * np.abs(W[:, kt, kf])
    return z, zm


def sim_conv0(tpad):
    def sim(dt, ia, b):
        B, T, F = ia
        z, _ = conv0_parts(b[0], b[1], b[2], B, T, F, tpad)
        b[3].reshape(z.shape)[...] = _dswish(z)
    return sim


SIM = {
    "conformer_qprep": sim_conformer_qprep, "conformer_scores_softmax": sim_conformer_scores_softmax,
    "conformer_softmax_shift": sim_conformer_softmax_shift, "conformer_softmax_shift_stream": sim_conformer_softmax_shift_stream,
    "slice_rows": sim_slice_rows, "dwconv_valid_dswish": sim_dwconv_valid_dswish,
    "z1_pool": sim_z1_pool, "z1_attn": sim_z1_attn, "z1_glu_conv": sim_z1_glu_conv, "z1_norm_bypass": sim_z1_norm_bypass,
    "z1_attn_downsample": sim_z1_attn_downsample, "z1_combine": sim_z1_combine, "z1_mean": sim_z1_mean,
    "z1_add_bcast": sim_z1_add_bcast, "z1_group_rows": sim_z1_group_rows,
    "lstm_cell": sim_lstm_cell, "lstm_cell_rows": sim_lstm_cell_rows, "lstm_add_frame": sim_lstm_add_frame,
    "lstm_norm_frame": sim_lstm_norm_frame, "add_inplace": sim_add_inplace, "gather_rows": sim_gather_rows,
    "scatter_rows": sim_scatter_rows, "basicnorm": sim_basicnorm, "conv0_pad1_dswish": sim_conv0(1), "conv0_nopad_dswish": sim_conv0(0),
}
CALLED = set()   # the ops the cases have launched so far (the tests assert it covers SIM)


def want(name, ia, bufs):
    """the reference: the operation in float64 on copies of the buffers; returns the buffers after it"""
    b = [None if a is None else (a.astype(np.float64) if a.dtype == np.float32 else a.copy()) for a in bufs]
    SIM[name](np.float64, [int(v) for v in ia], b)
    return b


def standin(name, ia, bufs, outs, expect=0):
    """in the kernel's place: the same formulas in float32 numpy, on the buffers themselves.  A refusal launches nothing."""
    CALLED.add(name)
    if expect != 0:
        return expect
    assert all(b is None or b.dtype != np.float64 for b in bufs), name
    with np.errstate(over="ignore"):
        SIM[name](np.float32, [int(v) for v in ia], bufs)
    for b in bufs:
        assert b is None or b.dtype in (np.float32, np.int32, np.int64), (name, "an operation left float32")
    return 0


def null_switch(name, value):
    return contextlib.nullcontext()


def launch(env, name, ia, bufs, outs, expect=0):
    CALLED.add(name)
    return env.op(name, ia, bufs, outs, expect=expect)


def same_bits(got, orig, keep, what):
    """the elements of `keep` (a boolean mask; None: all) are bit for bit what was uploaded"""
    g, o = got.reshape(-1).view(np.uint32), orig.reshape(-1).view(np.uint32)
    bad = (g != o) if keep is None else ((g != o) & keep.reshape(-1))
    assert not bad.any(), (what, "changed at", np.argwhere(bad)[:4].ravel().tolist())


def refused(env, name, ia, bufs, outs, what):
    """a shape the launcher refuses: UNSUPPORTED, every output buffer as it was"""
    before = [None if b is None else b.copy() for b in bufs]
    launch(env, name, ia, bufs, outs, expect=ERR_UNSUPPORTED)
    for k in outs:
        assert np.array_equal(bufs[k].view(np.uint32), before[k].view(np.uint32)), (what, "a refused launch wrote buffer", k)


# ---- Conformer -------------------------------------------------------------------------------------------------------------------------

SCORE_TS = [1, 2, 15, 16, 17, 31, 32, 33, 48, 100, 177, 250, 753]   # 100 / 177: a wave with one tile fewer / an odd run of three tiles


def scores_operands(rng, B, H, T, dk, form, scale=1.0):
    """operands of conformer_scores_softmax with every row stride wider than the row; O(dk^-1/2) queries as the model's scaling
    makes them, so that the 2 dk-term scores stay O(1)"""
    D, Tp = H * dk, r4(T)
    ldk = D + 8
    kmat, pp = uni(rng, B * T, ldk, scale=0.5 * scale), uni(rng, 2 * T - 1, D, scale=0.5 * scale)
    if form == "bias":
        ldq, scaling = 3 * D + 4, float(dk) ** -0.5
        bufs = [uni(rng, B * T, ldq, scale=scale), None, kmat, pp, nan(B * H, T, Tp), uni(rng, D, scale=0.5 * dk ** -0.5),
                uni(rng, D, scale=0.5 * dk ** -0.5)]
    else:
        ldq, scaling = 0, 1.0
        bufs = [uni(rng, B * T, D, scale=1.5 * dk ** -0.5 * scale), uni(rng, B * T, D, scale=1.5 * dk ** -0.5 * scale), kmat, pp,
                nan(B * H, T, Tp), None, None]
    return [ldk, B, H, T, Tp, D, ldq, fbits(scaling)], bufs


def scores_reference(ia, bufs):
    """softmax weights [B*H, T, T], centred scores, the scores' error bound (2 dk-term sums; the bias form's queries carry two
    roundings each), and the raw scores with their two parts ac [B*H, T, T] / bd [B*H, T, 2T-1] for the GEMM form"""
    ldk, B, H, T, Tp, D, ldq, sbits = ia
    b = [None if a is None else f64(a) for a in bufs]
    QU, QV = conf_queries(np.float64, b[0], b[1], b[5], b[6], B, T, D, ldq, unbits(sbits))
    k = b[2].reshape(B * T, ldk)[:, :D]
    s, mag = conf_scores(QU, QV, k, b[3], B, H, T)
    eps = score_eps(mag, 2 * (D // H))
    if b[5] is not None:
        qs = np.abs(b[0].reshape(B * T, ldq)[:, :D] * float(unbits(sbits)))
        _, qmag = conf_scores(2 * U * (qs + np.abs(b[5])), 2 * U * (qs + np.abs(b[6])), k, b[3], B, H, T)
        eps = eps + qmag
    dk = D // H
    ac = np.einsum("bihd,bjhd->bhij", QU.reshape(B, T, H, dk), k.reshape(B, T, H, dk)).reshape(B * H, T, T)
    bd = np.einsum("bihd,nhd->bhin", QV.reshape(B, T, H, dk), b[3].reshape(2 * T - 1, H, dk)).reshape(B * H, T, 2 * T - 1)
    pw, centred = softmax64(s.reshape(B * H, T, T))
    return pw, centred, eps.reshape(B * H, T, T), s, ac, bd


def check_weights(aw, ref, T, what, large=False):
    pw, centred, eps = ref[:3]
    check(aw[..., :T], pw, softmax_tol(pw, centred, eps), what, large)
    assert (aw[..., T:] == 0.0).all(), (what, "pad columns [T, Tp) are not exactly 0.0")


def scores_all_forms(env, ia, bufs, what, large=False):
    """one shape through the fused kernel, (bias form) conformer_qprep + the pre-formed form, and conformer_softmax_shift on the
    float64-exact ac / bd rounded to fp32: all three against the same reference and tolerance"""
    ldk, B, H, T, Tp, D, ldq, sbits = ia
    ref = scores_reference(ia, bufs)
    launch(env, "conformer_scores_softmax", ia, bufs, {4})
    check_weights(bufs[4], ref, T, "fused " + what, large)
    if bufs[5] is not None:
        qp_ia, qp = [B * T, D, sbits, ldq], [bufs[0], bufs[5], bufs[6], nan(B * T, D), nan(B * T, D)]
        w = want("conformer_qprep", qp_ia, qp)
        launch(env, "conformer_qprep", qp_ia, qp, {3, 4})
        qs = np.abs(f64(bufs[0])[:, :D] * float(unbits(sbits)))
        check(qp[3], w[3], 2 * U * (qs + np.abs(f64(bufs[5]))), "qprep qu " + what)
        check(qp[4], w[4], 2 * U * (qs + np.abs(f64(bufs[6]))), "qprep qv " + what)
        pre = [qp[3], qp[4], bufs[2], bufs[3], nan(B * H, T, Tp), None, None]
        launch(env, "conformer_scores_softmax", [ldk, B, H, T, Tp, D, 0, fbits(1.0)], pre, {4})
        check_weights(pre[4], ref, T, "qprep + pre-formed " + what, large)
    NPp = r4(2 * T - 1) + 4
    ac, bd = np.zeros((B * H, T, Tp), np.float32), np.zeros((B * H, T, NPp), np.float32)
    ac[..., T:] = np.nan                                   # (the pad columns are outputs of the kernel)
    ac[..., :T], bd[..., :2 * T - 1] = ref[4], ref[5]
    bd[..., 2 * T - 1:] = np.nan                           # columns no row may read
    launch(env, "conformer_softmax_shift", [B * H, T, Tp, NPp], [ac, bd], {0})
    check_weights(ac, ref, T, "GEMM form " + what, large)
    return ref


def case_conformer_scores_every_shape(env, dk):
    """k_conformer_scores_softmax16s<NG> (NG = dk / 16): both query forms at every T of SCORE_TS (one row, strips around 16 rows and
    the 4-column pad, one to three key tiles, a wave with an odd run, runs that differ between waves, the full-size 753), B and H
    above 1"""
    rng = np.random.default_rng(2000 + dk)
    n = 0
    for T in SCORE_TS:
        B, H = (2, 2) if T > 300 else (2, 3)
        for form in ("pre", "bias"):
            ia, bufs = scores_operands(rng, B, H, T, dk, form)
            scores_all_forms(env, ia, bufs, f"dk={dk} T={T} B={B} H={H} {form}")
            n += 1
    return n


def case_conformer_scores_tie_and_large(env):
    """an exact tie (keys 0 and 2 carry the same, largest score of row 1) and scores far beyond +-88, in every head size"""
    rng = np.random.default_rng(2100)
    for dk in (16, 32, 64):
        B, H, T = 2, 2, 33
        ia, bufs = scores_operands(rng, B, H, T, dk, "pre")
        D = H * dk
        bufs[0][1, :dk] = 0.0
        bufs[0][1, 0] = 5.0
        bufs[1][1, :dk] = 0.0
        bufs[2][0, 0] = bufs[2][2, 0] = 2.0
        ref = scores_all_forms(env, ia, bufs, f"tie dk={dk}")
        aw = bufs[4]
        assert aw[0, 1, 0] == aw[0, 1, 2] and aw[0, 1, 0] == aw[0, 1, :T].max(), ("tie", dk, aw[0, 1, :3])
        T = 65
        ia, bufs = scores_operands(rng, B, H, T, dk, "pre", scale=8.0 * dk ** 0.25)
        ref = scores_reference(ia, bufs)
        assert ref[3].max() > 100 and ref[3].min() < -100, (dk, ref[3].max(), ref[3].min())
        scores_all_forms(env, ia, bufs, f"large dk={dk}", large=True)


def case_conformer_scores_refusals(env):
    """every class of shape the launcher refuses: UNSUPPORTED, nothing launched (aw keeps its NaNs)"""
    rng = np.random.default_rng(2200)
    B, H, T = 1, 2, 20

    def go(ia, bufs, what):
        refused(env, "conformer_scores_softmax", ia, bufs, {4}, what)

    ia, bufs = scores_operands(rng, B, H, T, 24, "pre")
    go(ia, bufs, "dk = 24")
    ia, bufs = scores_operands(rng, B, H, T, 32, "pre")
    ia[0] += 2
    bufs[2] = uni(rng, B * T, ia[0])
    go(ia, bufs, "ldk % 4 != 0")
    ia, bufs = scores_operands(rng, B, H, 18, 32, "pre")
    ia[4] = 18
    bufs[4] = nan(B * H, 18, 18)
    go(ia, bufs, "Tp % 4 != 0")
    ia, bufs = scores_operands(rng, B, H, T, 32, "bias")
    bufs[6] = None
    go(ia, bufs, "bias_u without bias_v")
    ia, bufs = scores_operands(rng, 1, 1, 1245, 16, "pre")   # 32 (Tp + 4) floats must stay within 156 KB: Tp <= 1244
    go(ia, bufs, "Tp = 1248 > 1244")
    ia, bufs = scores_operands(rng, B, H, T, 32, "pre")
    with env.switch("K2HIP_CONFORMER_GEMM_SCORES", 1):
        go(ia, bufs, "K2HIP_CONFORMER_GEMM_SCORES")
    ia, bufs = scores_operands(rng, 1, 1, 1244, 16, "pre")   # the largest T the kernel takes runs
    scores_all_forms(env, ia, bufs, "T=1244")


def shift_case(env, Z, T, long_form, rng):
    Tp, NPp = r4(T), r4(2 * T - 1) + 8
    ac, bd = uni(rng, Z, T, Tp, scale=3.0), uni(rng, Z, T, NPp, scale=3.0)
    ac[..., T:] = np.nan
    bd[..., 2 * T - 1:] = np.nan
    a, b = f64(ac)[..., :T], f64(bd)
    s = a + shifted(b, T, T)
    pw, centred = softmax64(s)
    eps = score_eps(np.abs(a) + np.abs(shifted(b, T, T)), 1)
    with env.switch("K2HIP_ATTN_LONG", 1) if long_form else contextlib.nullcontext():
        launch(env, "conformer_softmax_shift", [Z, T, Tp, NPp], [ac, bd], {0})
    check_weights(ac, (pw, centred, eps), T, f"softmax_shift Z={Z} T={T} long={long_form}")


def case_conformer_softmax_shift(env):
    """k_conformer_softmax_shift (the register-resident row) and, with K2HIP_ATTN_LONG, k_conformer_softmax_shift_long; T = 2049 takes
    the long form by itself; bd rows wider than 2T - 1 with NaN behind"""
    rng = np.random.default_rng(2300)
    for T in (1, 3, 64, 65, 250):
        for long_form in (False, True):
            shift_case(env, 5, T, long_form, rng)
    shift_case(env, 1, 2049, False, rng)


def case_conformer_softmax_shift_stream(env):
    """k_conformer_softmax_shift_stream: left 0 / 7 / 64, KL below, across and above 64, every stream of a launch at its own plen
    (0, 1, left - 1, left, left + 5): masked left slots are exactly 0"""
    rng = np.random.default_rng(2400)
    for left, Tc in ((0, 16), (7, 9), (7, 60), (64, 16), (64, 3)):
        plen = np.array([0, 1, max(left - 1, 0), left, left + 5], np.int64)
        B, H, KL = len(plen), 2, left + Tc
        KLp, NPp = r4(KL), r4(left + 2 * Tc - 1) + 4
        ac, bd = uni(rng, B * H, Tc, KLp, scale=3.0), uni(rng, B * H, Tc, NPp, scale=3.0)
        ac[..., KL:] = np.nan
        bd[..., left + 2 * Tc - 1:] = np.nan
        a, sh = f64(ac)[..., :KL], shifted(f64(bd), Tc, KL)
        mask = stream_mask(plen, B, H, Tc, left)
        pw, centred = softmax64(a + sh, mask)
        launch(env, "conformer_softmax_shift_stream", [B, H, Tc, left, KLp, NPp], [ac, bd, plen], {0})
        what = f"softmax_shift_stream left={left} Tc={Tc}"
        check_weights(ac, (pw, centred, score_eps(np.abs(a) + np.abs(sh), 1)), KL, what)
        assert (ac[..., :KL][mask] == 0.0).all(), (what, "a masked column is not exactly 0.0")
        assert left == 0 or mask.any()


def case_slice_rows_and_valid_conv(env):
    """slice_rows with row0 > 0 (bit-exact) and k_dwconv_valid_dswish: K 15 / 31, chunks shorter and longer than K"""
    rng = np.random.default_rng(2500)
    for B, Tin, row0, Tout, D in ((2, 20, 3, 9, 64), (3, 7, 6, 1, 4), (1, 40, 0, 40, 100)):
        x, y = uni(rng, B, Tin, D), nan(B, Tout, D)
        launch(env, "slice_rows", [B, Tin, row0, Tout, D], [x, y], {1})
        same_bits(y, np.ascontiguousarray(x[:, row0:row0 + Tout]), None, f"slice_rows row0={row0}")
    for K in (15, 31):
        for Tc in (1, K - 3, K, 45):
            for D in (4, 100):
                B = 2
                ia = [B, Tc, D, K]
                bufs = [uni(rng, B, K - 1 + Tc, D), uni(rng, K, D, scale=0.5), uni(rng, D), nan(B, Tc, D)]
                z, zm = valid_conv(f64(bufs[0]), f64(bufs[1]), f64(bufs[2]), Tc, K)
                launch(env, "dwconv_valid_dswish", ia, bufs, {3})
                check(bufs[3], dswish64(z), act_tol(z, sum_tol(zm, K + 1)), f"dwconv_valid_dswish K={K} Tc={Tc} D={D}")


# ---- Zipformer v1 ------------------------------------------------------------------------------------------------------------------------

def case_z1_pool(env):
    """k_z1_pool: three consecutive chunks of the same streams through the same pool (permuted slots, two slots no stream owns);
    outputs, cached_avg and cached_len against the float64 running mean over every frame since the start; D no multiple of 256"""
    rng = np.random.default_rng(3000)
    for D, Tc in ((384, 16), (100, 7), (256, 1)):
        B, nslots, avg_off, len_off = 3, 5, 12, 7
        ss = avg_off + D + 9
        slots = rng.permutation(nslots)[:B].astype(np.int32)
        pool = np.full(nslots * ss, SENTINEL, np.float32)
        len0 = [0.0, 37.0, 5.0]
        mean = np.zeros((B, D))                       # float64 state: the mean so far, its frame count, the kernel's bound on it
        mtol = np.zeros((B, D))
        for s in range(B):
            avg = uni(rng, D)
            pool[slots[s] * ss + avg_off:slots[s] * ss + avg_off + D] = avg
            pool[slots[s] * ss + len_off] = len0[s]
            mean[s] = f64(avg) if len0[s] else 0.0
        count = np.array(len0)
        owned = np.zeros(pool.shape, bool)
        for s in slots:
            owned[s * ss + avg_off:s * ss + avg_off + D] = True
            owned[s * ss + len_off] = True
        for chunk in range(3):
            x, out = uni(rng, B, Tc, D), nan(B, Tc, D)
            before = pool.copy()
            launch(env, "z1_pool", [ss, avg_off, len_off, B, Tc, D], [x, pool, slots, out], {1, 3})
            what = f"z1_pool D={D} Tc={Tc} chunk {chunk}"
            for s in range(B):
                base = mean[s] * count[s]
                cum = np.cumsum(f64(x[s]), axis=0) + base
                cmag = np.cumsum(np.abs(f64(x[s])), axis=0) + np.abs(base)
                inv = 1.0 / (np.arange(1, Tc + 1) + count[s])[:, None]
                w = cum * inv
                # the (t + 1)-term running sum plus the base product and its add, the reciprocal and the final product; the error of the
                # cached mean enters weighted by count / (t + 1 + count) <= 1
                tol = np.stack([sum_tol(cmag[t], t + 3) for t in range(Tc)]) * inv + 4 * U * np.abs(w) + mtol[s] * count[s] * inv
                check(out[s], w, tol, f"{what} stream {s}")
                st = pool[slots[s] * ss:(slots[s] + 1) * ss]
                check(st[avg_off:avg_off + D], w[-1], tol[-1], f"{what} cached_avg {s}")
                assert np.array_equal(st[avg_off:avg_off + D], out[s, -1]), (what, "cached_avg is not the last output row")
                assert st[len_off] == count[s] + Tc, (what, "cached_len", st[len_off])
                mean[s], mtol[s], count[s] = w[-1], tol[-1], count[s] + Tc
            same_bits(pool, before, ~owned, what + " (pool outside the streams' state)")


def case_z1_attn(env):
    """k_z1_attn: head sizes 4 / 8 / 16 / 32, left context 0 / 16 / 64, chunk rows around the four waves, KLp above KL, rows wider
    than the layout; the 128 x 192 scores of the last shape need 96 KB of LDS and are refused"""
    rng = np.random.default_rng(3100)
    for hd, H in ((4, 8), (8, 4), (16, 2), (32, 4)):
        for L, Tc in ((0, 16), (16, 5), (64, 16), (64, 64)):
            B, A = 2, hd * H
            KL = L + Tc
            KLp, ld = r4(KL) + 4, 2 * A + A // 2 + 4 * H + 8
            ia = [ld, B, Tc, L, KLp, H, A]
            bufs = [uni(rng, B * Tc, ld), uni(rng, B * KL, A), uni(rng, 2 * Tc - 1 + L, 4 * H), nan(H, B, Tc, KLp)]
            s, mag = z1_scores(f64(bufs[0]), ld, f64(bufs[1]), f64(bufs[2]), B, Tc, L, H, A)
            pw, centred = softmax64(s)
            launch(env, "z1_attn", ia, bufs, {3})
            check_weights(bufs[3], (pw, centred, score_eps(mag, hd + 4)), KL, f"z1_attn hd={hd} L={L} Tc={Tc}")
    B, H, A, Tc, L = 1, 2, 32, 128, 64
    ld = 2 * A + A // 2 + 4 * H
    refused(env, "z1_attn", [ld, B, Tc, L, L + Tc, H, A],
            [uni(rng, B * Tc, ld), uni(rng, B * (L + Tc), A), uni(rng, 2 * Tc - 1 + L, 4 * H), nan(H, B, Tc, L + Tc)], {3}, "z1_attn 96 KB")


def case_z1_glu_conv(env, K):
    """k_z1_glu_conv<KT>: K 5 / 7 / 15 / 31 (taps in registers) and 9 (the run-time form), Tc 1 / 4 / 16 / 40 (below and above K - 1),
    D 64 / 96 / 384 (a partial last 64-channel workgroup); two chunks in sequence through the same pool -- the second reads the
    cache the first wrote -- output and cache after each; cache entries that only move stay bit-exact"""
    rng = np.random.default_rng(3200 + K)
    for Tc in (1, 4, 16, 40):
        for D in (64, 96, 384):
            B = 3
            rg = Ring(rng, B, 1, 1, D * (K - 1), [0] * B)
            w, bias = uni(rng, D, K, scale=0.4), uni(rng, D)
            cache = np.stack([f64(rg.ring(rg.pool, s)).reshape(D, K - 1) for s in range(B)])
            ctol = np.zeros((B, K - 1, D))
            for chunk in range(2):
                x2, y = uni(rng, B * Tc, 2 * D, scale=2.0), nan(B * Tc, D)
                before = rg.pool.copy()
                launch(env, "z1_glu_conv", [*rg.ints(), B, Tc, D, K], [x2, rg.pool, rg.slots, w, bias, y], {1, 5})
                a = f64(x2).reshape(B, Tc, 2 * D)
                cat, z, zm = z1_conv_parts(f64(x2), cache, f64(w), f64(bias), B, Tc, D, K)
                cattol = np.concatenate([ctol, np.abs(cat[:, K - 1:]) * (np.abs(a[..., D:]) + 8) * U], axis=1)
                ztol = sum_tol(zm, K + 1) + cattol.max() * np.sqrt((f64(w) ** 2).sum(1))
                what = f"z1_glu_conv K={K} Tc={Tc} D={D} chunk {chunk}"
                check(y.reshape(B, Tc, D), dswish64(z), act_tol(z, ztol), what)
                cache, ctol = cat[:, Tc:].transpose(0, 2, 1), cattol[:, Tc:]
                got = np.stack([rg.ring(rg.pool, s).reshape(D, K - 1) for s in range(B)])
                check(got, cache, ctol.transpose(0, 2, 1), what + " (cache)")
                owned = np.zeros(rg.pool.shape, bool)
                for s in rg.slots:
                    owned[s * rg.stride + rg.off:s * rg.stride + rg.off + D * (K - 1)] = True
                same_bits(rg.pool, before, ~owned, what + " (pool outside the caches)")


def norm_tol(y, sc, D, vtol=None):
    """BasicNorm's bound (module docstring); vtol: the bound of its input's own error"""
    tol = np.abs(y) * (2 * U * np.sqrt(D) + NORM_U)
    if vtol is not None:
        tol = tol + sc * vtol + np.abs(y) * sc * np.sqrt((vtol ** 2).mean(-1, keepdims=True))
    return tol


def basicnorm64(x, log_eps):
    x = f64(x)
    sc = ((x * x).mean(-1, keepdims=True) + np.exp(float(log_eps))) ** -0.5
    return x * sc, sc


def case_z1_glue(env):
    """z1_norm_bypass (M % 4 != 0), z1_attn_downsample (ds 1 / 2 / 4 / 16, T no multiple of ds, ldy > Din with the columns behind
    Din left alone), z1_combine (d1 below, at and above d2, with and without the upsample form), z1_mean, z1_add_bcast (D % 4 != 0
    refused), z1_group_rows"""
    rng = np.random.default_rng(3300)
    for M, D in ((37, 384), (1, 4), (6, 100)):
        x, o, le, bs = uni(rng, M, D, scale=3.0), uni(rng, M, D), np.array([-1.2], np.float32), np.array([0.6], np.float32)
        y = nan(M, D)
        launch(env, "z1_norm_bypass", [M, D], [x, o, le, bs, y], {4})
        nrm, sc = basicnorm64(x, le[0])
        o64, s = f64(o), float(bs[0])
        check(y, o64 + (nrm - o64) * s, 4 * U * (np.abs(o64) + (np.abs(nrm) + np.abs(o64)) * abs(s)) + norm_tol(nrm, sc, D) * abs(s),
              f"z1_norm_bypass M={M} D={D}")
    for ds, T in ((1, 5), (2, 7), (4, 9), (16, 35), (16, 3)):
        for Din, ldy in ((64, 80), (100, 100), (196, 256)):
            B, Td = 2, (T + ds - 1) // ds
            x, query, y = uni(rng, B, T, Din), uni(rng, Din, scale=0.5 * Din ** -0.5), uni(rng, B, Td, ldy)
            y0 = y.copy()
            launch(env, "z1_attn_downsample", [B, T, Din, ldy, ds], [x, query, y], {2})
            fr, sco, mag = attn_ds_parts(f64(x), f64(query), B, T, Din, ds)
            pw, centred = softmax64(sco)
            wtol = softmax_tol(pw, centred, score_eps(mag, Din))
            val = (fr * pw[..., None]).sum(2)
            tol = sum_tol((np.abs(fr) * pw[..., None]).sum(2), ds + 1) + (np.abs(fr) * wtol[..., None]).sum(2)
            what = f"z1_attn_downsample ds={ds} T={T} Din={Din} ldy={ldy}"
            check(y[..., :Din], val, tol, what)
            keep = np.zeros(y.shape, bool)
            keep[..., Din:] = True
            same_bits(y, y0, keep, what + " (columns behind Din)")
    for d1, d2 in ((64, 96), (96, 96), (128, 96)):
        for ds in (0, 2, 4):
            B, T = 2, 7
            Td = (T + ds - 1) // ds if ds else 0
            s1, w1, y = uni(rng, B * T, d1), np.array([0.3], np.float32), nan(B * T, d2)
            s2, ub = (uni(rng, B * Td, d2), uni(rng, ds, d2)) if ds else (uni(rng, B * T, d2), None)
            ia, bufs = [d1, d2, ds or 1, B, T, Td], [s1, s2, w1, ub, y]
            ref = want("z1_combine", ia, bufs)[4]
            launch(env, "z1_combine", ia, bufs, {4})
            w = float(w1[0])
            a = np.zeros((B, T, d2))
            a[..., :min(d1, d2)] = np.abs(f64(s1)).reshape(B, T, d1)[..., :min(d1, d2)] * w
            v2 = combine_src2(np.abs(f64(s2)), None if ub is None else np.abs(f64(ub)), ds, B, T, Td, d2)
            check(y, ref, 4 * U * (a + 2 * v2 * (1 - w)).reshape(B * T, d2), f"z1_combine d1={d1} d2={d2} ds={ds}")
    for B, T, D in ((2, 1, 64), (3, 50, 100), (1, 300, 384)):
        x, m = uni(rng, B, T, D), nan(B, D)
        launch(env, "z1_mean", [B, T, D], [x, m], {1})
        check(m, f64(x).mean(1), sum_tol(np.abs(f64(x)).mean(1), T + 2), f"z1_mean T={T} D={D}")
        v = uni(rng, B, D)
        x0 = x.copy()
        launch(env, "z1_add_bcast", [B, T, D], [x, v], {0})
        check(x, f64(x0) + f64(v)[:, None], U * (np.abs(f64(x0)) + np.abs(f64(v))[:, None]), f"z1_add_bcast T={T} D={D}")
    refused(env, "z1_add_bcast", [2, 3, 6], [uni(rng, 2, 3, 6), uni(rng, 2, 6)], {0}, "z1_add_bcast D=6")
    for ds, T, Din in ((2, 7, 64), (4, 9, 100), (1, 3, 4), (4, 2, 8)):
        B, Td = 2, (T + ds - 1) // ds
        x, g = uni(rng, B, T, Din), nan(B, Td, ds * Din)
        ref = want("z1_group_rows", [B, T, Din, ds], [x, g])[1]
        launch(env, "z1_group_rows", [B, T, Din, ds], [x, g], {1})
        same_bits(g, ref.astype(np.float32), None, f"z1_group_rows ds={ds} T={T}")


# ---- LSTM --------------------------------------------------------------------------------------------------------------------------------

def cell_tol(pre, dpre, c, Hh):
    """bounds of the new cell and the hidden output (module docstring: libm sigmoid 12 u + dz / 4, tanh 10 u + dz)"""
    cn, hf, (i, f, g, o) = lstm_gates(pre, c, Hh)
    d = [dpre[:, k * Hh:(k + 1) * Hh] for k in range(4)]
    it, ft, ot = (LIBM_SIG * v + 0.25 * dz for v, dz in ((i, d[0]), (f, d[1]), (o, d[3])))
    gt = LIBM_TANH * np.abs(g) + d[2]
    ctol = np.abs(c) * ft + np.abs(g) * it + i * gt + 3 * U * (np.abs(f * c) + np.abs(i * g))
    th = np.tanh(cn)
    htol = np.abs(th) * ot + o * (LIBM_TANH * np.abs(th) + ctol) + U * np.abs(hf)
    return cn, hf, ctol, htol


def case_lstm_cells(env):
    """k_lstm_cell (gx + gh with their own row strides) and k_lstm_cell_rows, gate pre-activations out to +-30 (saturated
    sigmoids and tanh on both sides), B Hh no multiple of the 256-thread workgroup"""
    rng = np.random.default_rng(4000)
    for B, Hh in ((3, 100), (1, 4), (5, 512)):
        ldgx, ldgh = 4 * Hh + 12, 4 * Hh + 4
        gx, gh = uni(rng, B, ldgx, scale=20.0), uni(rng, B, ldgh, scale=10.0)
        gx[:, :8] = [30.0, -30.0, 20.0, -20.0, 0.0, 1.0, -1.0, 10.0]
        gh[:, :8] = 0.0
        c, hf = uni(rng, B, Hh, scale=2.0), nan(B, Hh)
        pre = f64(gx)[:, :4 * Hh] + f64(gh)[:, :4 * Hh]
        dpre = U * (np.abs(f64(gx)[:, :4 * Hh]) + np.abs(f64(gh)[:, :4 * Hh]))
        cn, h, ctol, htol = cell_tol(pre, dpre, f64(c), Hh)
        launch(env, "lstm_cell", [ldgx, ldgh, B, Hh], [gx, gh, c, hf], {2, 3})
        check(c, cn, ctol, f"lstm_cell c B={B} Hh={Hh}")
        check(hf, h, htol, f"lstm_cell hf B={B} Hh={Hh}")
        gates, c, hf = uni(rng, B, 4 * Hh, scale=30.0), uni(rng, B, Hh, scale=2.0), nan(B, Hh)
        cn, h, ctol, htol = cell_tol(f64(gates), np.zeros((B, 4 * Hh)), f64(c), Hh)
        launch(env, "lstm_cell_rows", [B, Hh], [gates, c, hf], {1, 2})
        check(c, cn, ctol, f"lstm_cell_rows c B={B} Hh={Hh}")
        check(hf, h, htol, f"lstm_cell_rows hf B={B} Hh={Hh}")


def case_lstm_frames(env):
    """k_lstm_add_frame / k_lstm_norm_frame: S 1 / 2 / 4 split-K partials `pstride` (more than a partial) apart, a wavefront of n = 3
    layers starting at lo = 1 (every z reads another frame of another layer), n B = 9 rows (no multiple of the four rows of a
    workgroup), D 4 / 256 / 1024; every row of Y the launch does not own bit for bit; D = 1028 and S = 5 refused"""
    rng = np.random.default_rng(4100)
    n, B, T, lo, s, Lyr = 3, 3, 6, 1, 5, 5
    for D in (4, 256, 1024):
        for S in (1, 2, 4):
            R = n * B * D
            SY, pstride, lstride = B * T * D + 8, R + 16, D + 4
            Y, hp = uni(rng, (Lyr + 1) * SY), uni(rng, S * pstride)
            h, x1 = nan(n * B, D), nan(n * B, D)
            ia, bufs = [SY, pstride, S, n, B, T, D, lo, s], [Y, hp, h, x1]
            ref = want("lstm_add_frame", ia, bufs)
            launch(env, "lstm_add_frame", ia, bufs, {2, 3})
            hmag = partial_sum(np.abs(f64(hp)), pstride, S, R).reshape(n * B, D)
            htol = sum_tol(hmag, S) if S > 1 else np.zeros_like(hmag)
            check(h, ref[2], htol, f"lstm_add_frame h D={D} S={S}")
            check(x1, ref[3], htol + U * (np.abs(ref[3] - ref[2]) + np.abs(ref[2])), f"lstm_add_frame x1 D={D} S={S}")
            x1, fp = uni(rng, n * B, D), uni(rng, S * pstride)
            b2, eps = uni(rng, Lyr * lstride), uni(rng, Lyr * lstride)
            Y0 = Y.copy()
            ia, bufs = [pstride, S, lstride, SY, n, B, T, D, lo, s], [x1, fp, b2, eps, Y]
            launch(env, "lstm_norm_frame", ia, bufs, {4})
            owned = np.zeros(Y.shape, bool)
            for z in range(n):
                t, l = s - lo - z, lo + z
                v = (partial_sum(f64(fp), pstride, S, R).reshape(n, B, D)[z] + f64(b2)[l * lstride:l * lstride + D]) + f64(x1).reshape(n, B, D)[z]
                vmag = (partial_sum(np.abs(f64(fp)), pstride, S, R).reshape(n, B, D)[z] + np.abs(f64(b2)[l * lstride:l * lstride + D])
                        + np.abs(f64(x1)).reshape(n, B, D)[z])
                y, sc = basicnorm64(v, eps[l * lstride])
                plane = Y[(l + 1) * SY:(l + 1) * SY + B * T * D].reshape(B, T, D)
                check(plane[:, t], y, norm_tol(y, sc, D, sum_tol(vmag, S + 2)), f"lstm_norm_frame D={D} S={S} z={z}")
                om = owned[(l + 1) * SY:(l + 1) * SY + B * T * D].reshape(B, T, D)
                om[:, t] = True
            same_bits(Y, Y0, ~owned, f"lstm_norm_frame D={D} S={S} (rows of Y the launch does not own)")
    for D, S in ((1028, 2), (256, 5)):
        R = n * B * D
        SY, pstride, lstride = B * T * D, R, D
        refused(env, "lstm_norm_frame", [pstride, S, lstride, SY, n, B, T, D, lo, s],
                [uni(rng, n * B, D), uni(rng, S * pstride), uni(rng, Lyr * lstride), uni(rng, Lyr * lstride), uni(rng, (Lyr + 1) * SY)], {4},
                f"lstm_norm_frame D={D} S={S}")


def case_lstm_moves(env):
    """gather_rows, scatter_rows (ldin wider than the row) and add_inplace: bit-exact, the pool outside the rows untouched"""
    rng = np.random.default_rng(4200)
    for B, width in ((3, 100), (1, 4), (4, 513)):
        rg = Ring(rng, B, 1, 1, width, [0] * B)
        out = nan(B, width)
        pool0 = rg.pool.copy()
        launch(env, "gather_rows", [*rg.ints(), B, width], [rg.pool, rg.slots, out], {0, 2})
        same_bits(out, np.stack([rg.ring(pool0, s)[0] for s in range(B)]), None, f"gather_rows width={width}")
        same_bits(rg.pool, pool0, None, f"gather_rows width={width} (pool)")
        ldin = width + 8
        src = uni(rng, B, ldin)
        launch(env, "scatter_rows", [*rg.ints(), ldin, B, width], [rg.pool, rg.slots, src], {0})
        exp = pool0.copy()
        for s in range(B):
            rg.ring(exp, s)[0] = src[s, :width]
        same_bits(rg.pool, exp, None, f"scatter_rows width={width}")
    for n in (4, 1000, 4100):
        a, b = uni(rng, n, scale=3.0), uni(rng, n, scale=3.0)
        exp = a + b                                    # one correctly rounded fp32 addition
        launch(env, "add_inplace", [n], [a, b], {0})
        same_bits(a, exp, None, f"add_inplace n={n}")


def case_basicnorm_and_conv0(env):
    """k_basicnorm (D 4 / 384 / 1024, M % 4 != 0; D = 1028 refused) and k_conv0<TPAD, true>: T 3 / 4 / 100, odd F; the padded form's
    border rows and columns are part of the comparison like every other element"""
    rng = np.random.default_rng(4300)
    for D in (4, 384, 1024):
        M = 37
        x, le, y = uni(rng, M, D, scale=3.0), np.array([-0.7], np.float32), nan(M, D)
        launch(env, "basicnorm", [M, D], [x, le, y], {2})
        nrm, sc = basicnorm64(x, le[0])
        check(y, nrm, norm_tol(nrm, sc, D), f"basicnorm D={D}")
    refused(env, "basicnorm", [3, 1028], [uni(rng, 3, 1028), np.array([0.1], np.float32), nan(3, 1028)], {2}, "basicnorm D=1028")
    for name, tpad in (("conv0_pad1_dswish", 1), ("conv0_nopad_dswish", 0)):
        for T in (3, 4, 100):
            for F in (7, 81):
                B, T1 = 2, T - 2 + 2 * tpad
                x, w, bias, y = uni(rng, B, T, F, scale=2.0), uni(rng, 72, scale=0.5), uni(rng, 8), nan(B, T1, F, 8)
                launch(env, name, [B, T, F], [x, w, bias, y], {3})
                z, zm = conv0_parts(f64(x), f64(w), f64(bias), B, T, F, tpad)
                assert z.shape == y.shape
                check(y, dswish64(z), act_tol(z, sum_tol(zm, 10)), f"{name} T={T} F={F}")


# every case as (name, callable(env)); the GPU test and the CPU stand-in test both run all of them
CASES = ([(f"conformer_scores dk={dk}", (lambda env, dk=dk: case_conformer_scores_every_shape(env, dk))) for dk in (16, 32, 64)]
         + [("conformer_scores tie and large", case_conformer_scores_tie_and_large),
            ("conformer_scores refusals", case_conformer_scores_refusals),
            ("conformer_softmax_shift", case_conformer_softmax_shift),
            ("conformer_softmax_shift_stream", case_conformer_softmax_shift_stream),
            ("slice_rows and dwconv_valid_dswish", case_slice_rows_and_valid_conv),
            ("z1_pool", case_z1_pool), ("z1_attn", case_z1_attn)]
         + [(f"z1_glu_conv K={K}", (lambda env, K=K: case_z1_glu_conv(env, K))) for K in (5, 7, 9, 15, 31)]
         + [("z1 glue", case_z1_glue), ("lstm cells", case_lstm_cells), ("lstm frames", case_lstm_frames),
            ("lstm moves", case_lstm_moves), ("basicnorm and conv0", case_basicnorm_and_conv0)])
