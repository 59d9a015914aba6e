"""The attention kernels (csrc/attn.hip, the streaming ring operators of csrc/online.hip) and the Zipformer2 layer glue
(csrc/elementwise.hip) one launch at a time, against float64 references written here in numpy.

Each launch goes through k2hip_debug_op_run (include/k2hip_debug.h) on operands made HERE: every buffer sits between two 16 KB
guards of NaN bytes, so a read past an operand's end whose value reaches the result shows as NaN, and a write past an output's end
fails the call; pure outputs are pre-filled with NaN, so an element the kernel never writes fails the comparison.  Branch switches
(K2HIP_ATTN_LONG, K2HIP_DW1D_TT, K2HIP_DW7_TILED) force every form of a kernel.  The end-to-end parity tests hold the engine to the
float32 oracle at 2e-4; a kernel that is slightly wrong on one branch can hide inside that, here it cannot.

Tolerances are derived per element from the operands, in units of u = 2^-24 (the fp32 unit roundoff):
  * a sum of n products whose magnitudes add up to `mag` (computed in float64 with |operands|): 4 u sqrt(n) mag -- fp32
    accumulation in some order; every kernel here keeps exact fp32 products (f32 MFMA or FMA);
  * a softmax weight p_j of a row whose scores s_k are such sums (36 terms; 2 u sqrt(n) mag_k, the scores' own errors eps_k):
    p_j (eps_j + sum_k p_k eps_k + (|s_j - max| + 4) u) + 1e-7 -- the scores' errors, then the hardware exp of (s - max) and the
    reciprocal of the sum;
  * SwooshR / DoubleSwish / sigmoid through the hardware exp / log: (|z| + 4) u relative to their argument z, + 2e-6 absolute.
With O(1) operands every bound stays below 2e-5 absolute (check() asserts that for every comparison, relative to the largest
expected magnitude where that exceeds 1; only the deliberately huge scores of one softmax case are exempt)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ERR_UNSUPPORTED = -6


@pytest.fixture(scope="module")
def op(hip_tiny):
    from k2transducerasr_amd import load_library
    L = load_library()
    L.k2hip_debug_op_run.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_void_p),
                                     C.POINTER(C.c_int64), C.c_int32, C.c_uint32]

    def run(name, iargs, bufs, outs, expect=0):
        """one launch of launcher `name`; bufs: numpy arrays (or None) in the launcher's pointer order, downloaded in place where
        their index is in `outs`"""
        for b in bufs:
            assert b is None or (b.flags.c_contiguous and b.flags.writeable and b.dtype.itemsize in (4, 8)), name
        n = len(bufs)
        ptrs = (C.c_void_p * n)(*[b.ctypes.data if b is not None else None for b in bufs])
        sizes = (C.c_int64 * n)(*[b.nbytes if b is not None else 0 for b in bufs])
        ia = (C.c_int64 * max(1, len(iargs)))(*[int(v) for v in iargs])
        mask = sum(1 << k for k in outs)
        rc = L.k2hip_debug_op_run(hip_tiny.handle, name.encode(), ia, len(iargs), ptrs, sizes, n, mask)
        assert rc == expect, (name, list(iargs), rc, L.k2hip_last_error())
        return rc
    return run


class switch:
    """a branch switch for the duration of a with-block (restored even when the block fails)"""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        from k2transducerasr_amd import set_switch
        set_switch(self.name, self.value)

    def __exit__(self, *a):
        from k2transducerasr_amd import set_switch
        set_switch(self.name, 0)


def nan(*shape):
    return np.full(shape, np.nan, np.float32)


def uni(rng, *shape, scale=1.0):
    return (rng.uniform(-1, 1, shape) * scale).astype(np.float32)


def f64(a):
    return np.asarray(a, np.float64)


def check(got, want, tol, what, large_operands=False):
    got = f64(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert large_operands or np.max(tol) <= 2e-5 * max(1.0, np.abs(want).max()), (what, "tolerance looser than 2e-5", np.max(tol))
    bad = ~np.isfinite(got)
    assert not bad.any(), (what, "non-finite (unwritten, or a guard byte read) at", np.argwhere(bad)[:4].tolist())
    err = np.abs(got - want)
    over = err > tol
    if over.any():
        i = np.unravel_index(np.argmax(err - tol), err.shape)
        raise AssertionError(f"{what}: {int(over.sum())} of {err.size} elements off, worst at {i}: got {got[i]!r} want {want[i]!r} "
                             f"err {err[i]:.3g} tol {np.broadcast_to(tol, err.shape)[i]:.3g}")


def sum_tol(mag, n):
    return 4.0 * U * np.sqrt(max(n, 1)) * mag


def prop(err, W):
    """errors err [.., n] of the n operands of a weighted sum with weights W [m, n], added in quadrature: they are roundings of
    independent sums"""
    return np.sqrt((f64(err) ** 2) @ (f64(W) ** 2).T)


def softmax64(s, mask=None):
    s = s.copy()
    if mask is not None:
        s[mask] = -1000.0
    m = s.max(axis=-1, keepdims=True)
    e = np.exp(s - m)
    return e / e.sum(axis=-1, keepdims=True), s - m


def score_eps(mag, n):
    return 2.0 * U * np.sqrt(n) * mag


def softmax_tol(p, centred, eps):
    return p * (eps + (p * eps).sum(-1, keepdims=True) + (np.abs(centred) + 4.0) * U) + 1e-7


def swoosh_r64(z):
    return np.logaddexp(0.0, z - 1.0) - 0.08 * z - 0.313261687


def dswish64(z):
    return z / (1.0 + np.exp(1.0 - z))


def sigmoid64(z):
    return 1.0 / (1.0 + np.exp(-z))


def act_tol(z, ztol):
    """SwooshR' and DoubleSwish' are below 1.1 in magnitude: the argument's tolerance passes through, plus the hardware exp / log"""
    return 1.1 * ztol + (np.abs(z) + 4.0) * U * np.maximum(1.0, np.abs(z)) + 2e-6


# ---- offline attention scores (attn.hip k_attn_scores_softmax / _long) ------------------------------------------------------------------

def scores_ref(qkp, pp, B, T, H, qh, koff0, poff0):
    """attn.hip:1-12 and kernels.h attn_scores_softmax; oracle: k2_oracle.c:661-702 (attn_weights).
    scores[h,b,i,j] = q_i . k_j + p_i . pp[T-1-i+j]; returns the softmax, its centred scores, and the per-row error bound of the scores"""
    x = f64(qkp).reshape(B, T, -1)
    q = np.stack([x[:, :, h * qh:(h + 1) * qh] for h in range(H)])                       # [H,B,T,qh]
    k = np.stack([x[:, :, koff0 + h * qh:koff0 + (h + 1) * qh] for h in range(H)])
    p = np.stack([x[:, :, poff0 + 4 * h:poff0 + 4 * h + 4] for h in range(H)])            # [H,B,T,4]
    ppr = f64(pp).reshape(2 * T - 1, H, 4)
    idx = (T - 1) - np.arange(T)[:, None] + np.arange(T)[None, :]                        # [i,j]
    e = ppr[idx].transpose(2, 0, 1, 3)                                                   # [H,i,j,4]
    s = np.einsum("hbid,hbjd->hbij", q, k) + np.einsum("hbic,hijc->hbij", p, e)
    mag = np.einsum("hbid,hbjd->hbij", np.abs(q), np.abs(k)) + np.einsum("hbic,hijc->hbij", np.abs(p), np.abs(e))
    pw, centred = softmax64(s)
    return pw, centred, score_eps(mag, qh + 4), s


def scores_case(rng, B, T, H, qh, layout, scale=1.0, tie=False):
    Tp = (T + 3) // 4 * 4
    A = H * qh
    if layout == "z2":                      # Zipformer2: q [A] | k [A] | p [H*4]
        width, koff0, poff0 = 2 * A + 4 * H, A, 2 * A
        kargs = (-1, -1)
    else:                                   # Zipformer v1: q [A] | k [A] | v [A/2] | p [H*4]
        width, koff0, poff0 = 2 * A + A // 2 + 4 * H, A, 2 * A + A // 2
        kargs = (koff0, poff0)
    ld = width + 12                         # wider than the row
    qkp = uni(rng, B * T, ld)
    qkp[:, :2 * A] *= scale
    pp = uni(rng, 2 * T - 1, 4 * H)
    if tie and T >= 3:
        # row 1 of (head 0, stream 0): no positional query, q = 10 e_0, keys 0 and 2 share the largest e_0 component -> an exact tie
        qkp[1, :qh] = 0.0
        qkp[1, 0] = 10.0
        qkp[1, poff0:poff0 + 4] = 0.0
        qkp[0, koff0] = 2.0
        qkp[2, koff0] = 2.0
    return qkp, pp, ld, Tp, kargs, koff0, poff0


def run_scores(op, qkp, pp, ld, B, T, Tp, H, qh, kargs):
    aw = nan(H, B, T, Tp)
    op("attn_scores_softmax", [ld, B, T, Tp, H, qh, *kargs], [qkp, pp, aw], {2})
    return aw


def check_scores(aw, ref, T, Tp, what, large_operands=False):
    pw, centred, eps, _ = ref
    check(aw[..., :T], pw, softmax_tol(pw, centred, eps), what, large_operands)
    assert (aw[..., T:Tp] == 0.0).all(), (what, "pad columns [T, Tp) are not exactly 0.0")


TS = [1, 2, 3, 4, 5, 31, 32, 33, 65, 250]


@pytest.mark.parametrize("qh,layout", [(32, "z2"), (24, "z1"), (16, "z1")])
def test_attn_scores_softmax_strip_and_long_forms(op, qh, layout):
    """k_attn_scores_softmax<NG> (the LDS strip) and, with K2HIP_ATTN_LONG, k_attn_scores_softmax_long<NG> on every T of TS
    (one row, rows around the 32-row workgroup and the 4-column pad, a long one), H 1 / 4 / 8, B 1 / 3, rows wider than the
    head layout; qh 24 / 16 with the Zipformer v1 row (explicit koff0 / poff0).  Every weight within the softmax tolerance of
    the module docstring (scores: 36-term sums), pad columns exactly 0.0."""
    rng = np.random.default_rng(1000 + qh)
    for T in TS:
        for H, B in ((1, 1), (4, 3), (8, 3)):
            qkp, pp, ld, Tp, kargs, koff0, poff0 = scores_case(rng, B, T, H, qh, layout, tie=True)
            ref = scores_ref(qkp, pp, B, T, H, qh, koff0, poff0)
            check_scores(run_scores(op, qkp, pp, ld, B, T, Tp, H, qh, kargs), ref, T, Tp, f"strip qh={qh} T={T} H={H} B={B}")
            with switch("K2HIP_ATTN_LONG", 1):
                aw = run_scores(op, qkp, pp, ld, B, T, Tp, H, qh, kargs)
            check_scores(aw, ref, T, Tp, f"long qh={qh} T={T} H={H} B={B}")
            if T >= 3:   # the tie row: keys 0 and 2 carry the same, largest weight
                assert aw[0, 0, 1, 0] == aw[0, 0, 1, 2] and aw[0, 0, 1, 0] == aw[0, 0, 1, :T].max()


def test_attn_scores_softmax_large_scores_and_long_rows(op):
    """Scores spanning far more than +-88 (a softmax without the max subtraction overflows fp32 there; the tolerance scales with
    the scores' magnitude, see the module docstring) in both forms; T = 1101 (LDS strip with Tp > 1024: the in-place row loop, three
    pad columns) and T = 1201 (the strip no longer fits in 160 KB: the two-pass form is taken without the switch)."""
    rng = np.random.default_rng(77)
    for qh, layout, H, B, T in ((32, "z2", 2, 2, 65), (24, "z1", 4, 1, 33), (16, "z1", 8, 1, 250)):
        qkp, pp, ld, Tp, kargs, koff0, poff0 = scores_case(rng, B, T, H, qh, layout, scale=7.0)
        ref = scores_ref(qkp, pp, B, T, H, qh, koff0, poff0)
        assert ref[3].max() > 100 and ref[3].min() < -100
        check_scores(run_scores(op, qkp, pp, ld, B, T, Tp, H, qh, kargs), ref, T, Tp, f"large strip qh={qh}", True)
        with switch("K2HIP_ATTN_LONG", 1):
            aw = run_scores(op, qkp, pp, ld, B, T, Tp, H, qh, kargs)
        check_scores(aw, ref, T, Tp, f"large long qh={qh}", True)
    for T in (1101, 1201):
        qkp, pp, ld, Tp, kargs, koff0, poff0 = scores_case(rng, 1, T, 1, 32, "z2")
        ref = scores_ref(qkp, pp, 1, T, 1, 32, koff0, poff0)
        check_scores(run_scores(op, qkp, pp, ld, 1, T, Tp, 1, 32, kargs), ref, T, Tp, f"T={T}")


# ---- attention apply + out_proj (attn.hip k_attn_av_out) ---------------------------------------------------------------------------------

def random_weights(rng, H, B, T, KL, Tp):
    """softmax-like rows over KL keys, pad columns zero"""
    aw = np.zeros((H, B, T, Tp), np.float32)
    r = rng.uniform(0, 1, (H, B, T, KL)) ** 3
    aw[..., :KL] = (r / r.sum(-1, keepdims=True)).astype(np.float32)
    return aw


def av_out_ref(aw, vals, wout, bias, xres, H, vh, KL):
    """attn.hip:304-312, kernels.h attn_av_out; oracle: k2_oracle.c:755-766 (self_attn) / k2_oracle_online.c:398-410.
    vals [B, KL, HV] in aw's column order; x = xres + concat_h(aw_h . v_h) . wout^T + bias.  Tolerance: the KL-term context sums
    (weights add up to 1) then the HV-term projection, each 4 u sqrt(n) of its magnitude sum"""
    B, T = aw.shape[1], aw.shape[2]
    a = f64(aw)[..., :KL]
    v = f64(vals).reshape(B, KL, H, vh)
    ctx = np.einsum("hbtk,bkhc->bthc", a, v).reshape(B * T, H * vh)
    cmag = np.einsum("hbtk,bkhc->bthc", np.abs(a), np.abs(v)).reshape(B * T, H * vh)
    W = f64(wout)
    want = f64(xres) + ctx @ W.T + f64(bias)
    mag = (cmag * (1 + sum_tol(1.0, KL))) @ np.abs(W).T + np.abs(f64(bias)) + np.abs(f64(xres))
    tol = sum_tol(mag, H * vh + 2) + prop(sum_tol(cmag, KL), W)
    return want, tol


def test_attn_av_out_offline(op):
    """k_attn_av_out<false>: vh 8 / 12 / 16 with H vh up to 128, D 192 / 256 / 384, T 1 / 15 / 16 / 17 / 250 (16-row strips and
    their ragged ends; the column split over blockIdx.z at few strips), B 1 / 3; x holds random values before the call, so the
    residual add is checked too.  A shape the kernel does not take (vh 24, H vh 144) comes back UNSUPPORTED with x untouched."""
    rng = np.random.default_rng(5)
    ran = 0
    for T in (1, 15, 16, 17, 250):
        for (H, vh), D, B in (((4, 8), 192, 1), ((8, 12), 256, 3), ((8, 16), 384, 3), ((3, 12), 192, 3), ((8, 16), 192, 1)):
            HV, KL, Tp = H * vh, T, (T + 3) // 4 * 4
            aw = random_weights(rng, H, B, T, KL, Tp)
            v = uni(rng, B * KL, HV)
            wout = uni(rng, D, HV, scale=HV ** -0.5)
            bias = uni(rng, D)
            x = uni(rng, B * T, D)
            want, tol = av_out_ref(aw, v, wout, bias, x, H, vh, KL)
            op("attn_av_out", [B, T, KL, Tp, H, vh, D], [aw, v, wout, bias, x], {4})
            check(x, want, tol, f"attn_av_out T={T} H={H} vh={vh} D={D} B={B}")
            ran += 1
    for H, vh in ((4, 24), (9, 16)):
        T, D, B = 17, 192, 2
        aw = random_weights(rng, H, B, T, T, 20)
        x = uni(rng, B * T, D)
        x0 = x.copy()
        op("attn_av_out", [B, T, T, 20, H, vh, D], [aw, uni(rng, B * T, H * vh), uni(rng, D, H * vh), uni(rng, D), x], {4},
           expect=ERR_UNSUPPORTED)
        assert np.array_equal(x, x0)
    assert ran == 25


# ---- the streaming ring operators -------------------------------------------------------------------------------------------------------

SENTINEL = np.float32(-7.625)


class Ring:
    """A state pool of `nslots` slots (sentinel fill), streams in permuted slots, one ring of KL rows x width floats at a non-zero
    offset inside a slot (random old contents), and each stream's chunk count (kernels.h RingRef: chunk n writes row r to ring row
    (n T + r) % KL)."""

    def __init__(self, rng, B, T, KL, width, chunks, nslots=5, off=36, extra=20):
        self.B, self.T, self.KL, self.width, self.off = B, T, KL, width, off
        self.stride = off + KL * width + extra
        self.pool = np.full(nslots * self.stride, SENTINEL, np.float32)
        self.slots = rng.permutation(nslots)[:B].astype(np.int32)
        self.chunks = np.asarray(chunks, np.int32)
        assert len(self.chunks) == B
        for s in self.slots:
            self.pool[s * self.stride + off: s * self.stride + off + KL * width] = uni(rng, KL * width)
        self.pool0 = self.pool.copy()      # (self.pool is the buffer the launch writes back into)
        self.heads = (self.chunks.astype(np.int64) * T) % KL

    def ring(self, pool, b):
        s = self.slots[b]
        return pool[s * self.stride + self.off: s * self.stride + self.off + self.KL * self.width].reshape(self.KL, self.width)

    def rows(self, b):
        return (self.heads[b] + np.arange(self.T)) % self.KL

    def after(self, newrows):
        """the pool as it must be after the chunk's rows (newrows [B, T, width]) went into the rings, and each stream's ring"""
        pool = f64(self.pool0).copy()
        for b in range(self.B):
            self.ring(pool, b)[self.rows(b)] = newrows[b]
        return pool, [self.ring(pool, b) for b in range(self.B)]

    def wraps(self):
        return bool(((self.heads + self.T) > self.KL).any())

    def bufs(self):
        return [self.pool, self.slots, self.chunks]

    def ints(self):
        return [self.stride, self.off]

    def check_pool(self, got, want, tol_rows, what):
        """rows the chunk wrote: within tol_rows (0: bit-exact copies); every other float of the pool: unchanged"""
        got = f64(got)
        written = np.zeros(got.shape, bool)
        for b in range(self.B):
            base = self.slots[b] * self.stride + self.off
            for r in self.rows(b):
                written[base + r * self.width: base + (r + 1) * self.width] = True
        assert np.array_equal(got[~written], want[~written]), (what, "pool changed outside the chunk's ring rows",
                                                                np.argwhere(got[~written] != want[~written])[:4].tolist())
        check(got[written], want[written], tol_rows, what + " (ring rows)")


def wrapping_chunk(T, KL):
    """the first chunk count whose T rows run past the ring's end"""
    return next(c for c in range(1, 4 * KL) if (c * T) % KL + T > KL)


def stream_scores_case(op, rng, form, B, Tc, L, H, ds, left50, chunks, plen):
    KL, KLp = L + Tc, (L + Tc + 3) // 4 * 4
    ld = 72 * H + 8
    qkp = uni(rng, B * Tc, ld)
    pp = uni(rng, 2 * Tc - 1 + L, 4 * H)
    plen = np.asarray(plen, np.int64)
    rg = Ring(rng, B, Tc, KL, 32 * H, chunks)
    newk = qkp.reshape(B, Tc, ld)[:, :, 32 * H:64 * H]
    want_pool, rings = rg.after(f64(newk))
    aw = nan(H, B, Tc, KLp)
    if form == "ring":
        op("attn_stream_ring", [ld, *rg.ints(), B, Tc, L, KLp, H, ds, left50], [qkp, *rg.bufs(), pp, plen, aw], {1, 6})
        keys = [r for r in rings]
        # column p = ring row p; its key index j = (p - head - Tc) mod KL (online.hip k_attn_stream_ring)
        jcol = [(np.arange(KL) - rg.heads[b] - Tc) % KL for b in range(B)]
    else:
        kcat = np.stack([np.concatenate([r[(rg.heads[b] + Tc + np.arange(KL)) % KL]]) for b, r in enumerate(rings)]).astype(np.float32)
        op("attn_stream", [ld, B, Tc, L, KLp, H, ds, left50], [qkp, kcat.reshape(B * KL, 32 * H), pp, plen, aw], {4})
        keys = list(f64(kcat))
        jcol = [np.arange(KL) for _ in range(B)]
    x = f64(qkp).reshape(B, Tc, ld)
    for b in range(B):
        j = jcol[b]
        # k2_oracle_online.c:502-505: left slot j (50 Hz slot j ds) is masked while processed_len <= left50 - 1 - j ds
        masked = (j < L) & (plen[b] <= left50 - 1 - j * ds)
        for h in range(H):
            q, k = x[b, :, 32 * h:32 * h + 32], keys[b][:, 32 * h:32 * h + 32]
            p = x[b, :, 64 * H + 4 * h:64 * H + 4 * h + 4]
            e = f64(pp)[(Tc - 1) - np.arange(Tc)[:, None] + j[None, :], 4 * h:4 * h + 4]      # [i, p, 4]
            s = q @ k.T + np.einsum("ic,ipc->ip", p, e)
            mag = np.abs(q) @ np.abs(k).T + np.einsum("ic,ipc->ip", np.abs(p), np.abs(e))
            pw, centred = softmax64(s, np.broadcast_to(masked, s.shape))
            eps = score_eps(mag, 36)
            what = f"{form} Tc={Tc} L={L} H={H} ds={ds} stream {b} head {h}"
            check(aw[h, b, :, :KL], pw, softmax_tol(pw, centred, eps), what)
            assert (aw[h, b, :, KL:] == 0.0).all(), (what, "pad columns")
    if form == "ring":
        rg.check_pool(rg.pool, want_pool, 0.0, f"attn_stream_ring Tc={Tc} L={L} pool")
    return rg


def test_attn_stream_ring_and_attn_stream(op):
    """k_attn_stream_ring (keys in the stream's ring, aw columns in ring order) and k_attn_stream (keys concatenated) at the
    chunk / left context of a ds 1 / 2 / 4 stack (Tc 16 / 8 / 4), left contexts that are no multiple of the chunk (the write
    position wraps inside a chunk for some streams), a chunk that does not divide 256 (the flat-index loop); young streams
    (processed_len 0, 16) get their unfilled left slots masked.  The pool after the call: the chunk's key rows in the right
    ring rows, bit-exact, and every other float unchanged."""
    rng = np.random.default_rng(9)
    left50 = 64
    for Tc, L, ds in ((16, 40, 1), (8, 20, 2), (4, 10, 4), (12, 40, 1), (5, 23, 2)):
        chunks = [0, wrapping_chunk(Tc, L + Tc), 1, 7]
        plen = [0, 16, 48, 4000]
        rg = stream_scores_case(op, rng, "ring", 4, Tc, L, 4, ds, left50, chunks, plen)
        assert rg.wraps(), (Tc, L)
        stream_scores_case(op, rng, "cat", 4, Tc, L, 4, ds, left50, chunks, plen)


def test_attn_stream_ring_beyond_64kb_of_lds(op):
    """The score block [Tc][L + Tc] lives in dynamic LDS: a chunk of 32 frames with a left context of 512 needs 69.6 KB, of 1248
    exactly the CU's 160 KB -- both must run and match; one frame more of left context is refused (UNSUPPORTED) before any launch."""
    rng = np.random.default_rng(11)
    for L in (512, 1248):
        for form in ("ring", "cat"):
            stream_scores_case(op, rng, form, 2, 32, L, 2, 1, L, [5, 41], [10 ** 6, 64])
    Tc, L, H, B = 32, 1249, 2, 1
    KLp = (Tc + L + 3) // 4 * 4
    rg = Ring(rng, B, Tc, Tc + L, 32 * H, [0])
    aw = nan(H, B, Tc, KLp)
    op("attn_stream_ring", [72 * H, *rg.ints(), B, Tc, L, KLp, H, 1, L],
       [uni(rng, B * Tc, 72 * H), *rg.bufs(), uni(rng, 2 * Tc - 1 + L, 4 * H), np.zeros(B, np.int64), aw], {6}, expect=ERR_UNSUPPORTED)


@pytest.mark.parametrize("proj", [False, True])
def test_attn_av_out_ring(op, proj):
    """k_attn_av_out<true> (the chunk's value rows newrows go into the ring first) and k_attn_av_out<true, true> (newrows =
    xin . win^T + bin computed in the kernel; output to a second buffer, residual from xin): T 1 / 5 / 16 rows per stream, rings that
    wrap, permuted slots.  Output against the numpy model of the ring order (aw column p = ring row p), the pool against the
    expected ring rows (exact copies; the projection within its D-term sum tolerance) and the sentinel everywhere else."""
    rng = np.random.default_rng(21 + proj)
    for T, L, (H, vh), D in ((1, 23, (4, 12), 192), (5, 37, (8, 16), 224), (16, 45, (3, 8), 256), (16, 100, (8, 12), 384)):
        B, KL = 3, L + T
        Tp = (KL + 3) // 4 * 4
        HV = H * vh
        rg = Ring(rng, B, T, KL, HV, [2, wrapping_chunk(T, KL) if T > 1 else 5, 0])
        aw = random_weights(rng, H, B, T, KL, Tp)
        wout = uni(rng, D, HV, scale=HV ** -0.5)
        bias = uni(rng, D)
        x = uni(rng, B * T, D)
        what = f"T={T} L={L} H={H} vh={vh} D={D} proj={proj}"
        if proj:
            win = uni(rng, HV, D, scale=D ** -0.5)
            bin_ = uni(rng, HV)
            newrows = f64(x) @ f64(win).T + f64(bin_)
            ntol = sum_tol(np.abs(f64(x)) @ np.abs(f64(win)).T + np.abs(f64(bin_)), D + 1)
            xout = nan(B * T, D)
            op("attn_proj_av_out_ring", [*rg.ints(), B, T, KL, Tp, H, vh, D], [aw, *rg.bufs(), x, win, bin_, wout, bias, xout], {1, 9})
        else:
            nr = uni(rng, B * T, HV)
            newrows, ntol = f64(nr), 0.0
            x0 = x.copy()
            op("attn_av_out_ring", [*rg.ints(), B, T, KL, Tp, H, vh, D], [aw, *rg.bufs(), nr, wout, bias, x], {1, 7})
            xout, x = x, x0
        want_pool, rings = rg.after(newrows.reshape(B, T, HV))
        want, tol = av_out_ref(aw, np.stack(rings).astype(np.float64), wout, bias, x, H, vh, KL)
        if proj:   # the ring rows' own rounding passes through the weights
            tol = tol + prop(np.full((1, HV), ntol.max()), wout)
        check(xout, want, tol, "attn_av_out_ring " + what)
        rg.check_pool(rg.pool, want_pool, ntol.max() if proj else 0.0, "pool " + what)
        assert rg.wraps() or T == 1, what


def test_nonlin_av_out_ring(op):
    """k_nonlin_av_out<NS, NT[, MULTI]>: KL in each of (0, 64], (64, 128], (128, 192], (192, 256] and above 256 (the MULTI trips),
    Hc 100 (8 column tiles: 512 threads) and 196 (13 tiles, the last one partial: 1024 threads while NS <= 3), with out_proj inside
    (wout set: x += ctx . wout^T + bias) and without (wout NULL: x = ctx).  The chunk's rows x * tanh(s) go into the ring first
    (NonlinAttention.streaming_forward, k2_oracle_online.c:455-470)."""
    rng = np.random.default_rng(31)
    ran = 0
    for T, L in ((3, 40), (16, 100), (7, 170), (16, 230), (9, 300), (16, 520)):
        for Hc in (100, 196):
            for with_out in (True, False):
                B, KL, D = 3, L + T, 80
                Tp = (KL + 3) // 4 * 4
                ldh = 3 * Hc + 8
                rg = Ring(rng, B, T, KL, Hc, [4, 0, wrapping_chunk(T, KL)])
                aw = random_weights(rng, 2, B, T, KL, Tp)          # head 0 is read
                hid = uni(rng, B * T, ldh, scale=1.5)
                h3 = f64(hid).reshape(B, T, ldh)
                s, xv, y = h3[..., :Hc], h3[..., Hc:2 * Hc], h3[..., 2 * Hc:3 * Hc]
                newrows = xv * np.tanh(s)
                # tanhf: a few ulps of the product
                ntol = 4 * U * np.abs(newrows) + 2e-7
                want_pool, rings = rg.after(newrows)
                R = np.stack(rings)                                # [B, KL, Hc] in ring order
                a0 = f64(aw[0])[..., :KL]
                ctx = np.einsum("btk,bkc->btc", a0, R) * y
                cmag = (np.einsum("btk,bkc->btc", np.abs(a0), np.abs(R)) * np.abs(y))
                ctol = sum_tol(cmag, KL) + np.abs(y) * ntol.max()
                what = f"nonlin T={T} L={L} Hc={Hc} wout={with_out}"
                if with_out:
                    wout = uni(rng, D, Hc, scale=Hc ** -0.5)
                    bias = uni(rng, D)
                    x = uni(rng, B * T, D)
                    want = f64(x) + ctx.reshape(B * T, Hc) @ f64(wout).T + f64(bias)
                    tol = (sum_tol(cmag.reshape(B * T, Hc) @ np.abs(f64(wout)).T + np.abs(f64(bias)) + np.abs(f64(x)), Hc + 2)
                           + prop(ctol.reshape(B * T, Hc), wout))
                    op("nonlin_av_out_ring", [*rg.ints(), ldh, B, T, KL, Tp, Hc, D], [aw, *rg.bufs(), hid, wout, bias, x], {1, 7})
                else:
                    x = nan(B * T, Hc)
                    want, tol = ctx.reshape(B * T, Hc), ctol.reshape(B * T, Hc)
                    op("nonlin_av_out_ring", [*rg.ints(), ldh, B, T, KL, Tp, Hc, D], [aw, *rg.bufs(), hid, None, None, x], {1, 7})
                check(x, want, tol, what)
                assert rg.wraps(), what
                rg.check_pool(rg.pool, want_pool, ntol.max(), "pool " + what)
                ran += 1
    assert ran == 24


def glu_causal_conv_ref(x2, cache0, wc, bc, ww, bw, sc, B, Tc, D, K, x2tol=0.0):
    """online.hip:253-312 (k_glu_causal_conv, k_glu_causal_conv_reg); oracle: k2_oracle_online.c:349-396 (online_conv_module).
    x2 [B Tc, 2 D] = (value | gate) halves (x2tol: the bound of their own error, 0 when they are operands), cache0 [B, D, K / 2]:
    y = SwooshR(chunk-causal depthwise conv(GLU(x2))) as float64 with its tolerance, and the advanced caches [B, D, K / 2]"""
    pad, Kc = K // 2, (K + 1) // 2
    a = f64(x2).reshape(B, Tc, 2 * D)
    atol = np.broadcast_to(f64(x2tol), (B * Tc, 2 * D)).reshape(B, Tc, 2 * D)
    gate = a[..., D:]
    g = a[..., :D] * sigmoid64(gate)                                      # [B, Tc, D]
    gtol = np.abs(g) * (np.abs(gate) + 8) * U + atol[..., :D] + 0.25 * np.abs(a[..., :D]) * atol[..., D:]
    cat = np.concatenate([f64(cache0).transpose(0, 2, 1), g], axis=1)     # [B, pad + Tc, D]
    cmag = np.abs(cat)
    xc = np.broadcast_to(f64(bc), (B, Tc, D)).copy()
    xcm = np.abs(xc)
    for k in range(Kc):
        xc += f64(wc)[:, k] * cat[:, k:k + Tc]
        xcm += np.abs(f64(wc)[:, k]) * cmag[:, k:k + Tc]
    xw = np.broadcast_to(f64(bw), (B, Tc, D)).copy()
    xwm = np.abs(xw)
    for k in range(K):
        for t in range(Tc):
            tt = t + k - pad
            if 0 <= tt < Tc:
                xw[:, t] += f64(ww)[:, k] * g[:, tt]
                xwm[:, t] += np.abs(f64(ww)[:, k]) * np.abs(g[:, tt])
    le, re = np.zeros((Tc, D)), np.zeros((Tc, D))
    for t in range(Tc):               # ChunkCausalDepthwiseConv1d._get_chunk_scale
        if Tc < K:
            le[t], re[t] = f64(sc)[0, :, t], f64(sc)[1, :, K - Tc + t]
        else:
            le[t] = f64(sc)[0, :, t] if t < K else 0.0
            re[t] = f64(sc)[1, :, t - (Tc - K)] if t >= Tc - K else 0.0
    scale = 1.0 + le + re
    z = xw * scale + xc
    ztol = (sum_tol(xwm * np.abs(scale) + xcm, K + Kc + 2)
            + gtol.max() * np.sqrt((f64(ww) ** 2).sum(1) * scale ** 2 + (f64(wc) ** 2).sum(1)))
    # the cache advances to the last pad frames of [cache ; chunk]
    newcache = cat[:, Tc:Tc + pad].transpose(0, 2, 1)
    return swoosh_r64(z).reshape(B * Tc, D), act_tol(z, ztol).reshape(B * Tc, D), newcache


def glu_causal_conv_case(op, rng, K, Tc, D=100, B=3):
    pad, Kc = K // 2, (K + 1) // 2
    rg = Ring(rng, B, 1, 1, D * pad, [0] * B)    # one "row": the stream's [D][pad] cache, replaced whole
    x2 = uni(rng, B * Tc, 2 * D, scale=2.0)
    wc, bc, ww, bw = uni(rng, D, Kc, scale=0.4), uni(rng, D), uni(rng, D, K, scale=0.3), uni(rng, D)
    sc = uni(rng, 2, D, K, scale=0.5)
    y = nan(B * Tc, D)
    cache0 = np.stack([f64(rg.ring(rg.pool, b)).reshape(D, pad) for b in range(B)])  # [B, D, pad]
    op("glu_causal_conv", [*rg.ints(), B, Tc, D, K], [x2, rg.pool, rg.slots, wc, bc, ww, bw, sc, y], {1, 8})
    want, tol, newcache = glu_causal_conv_ref(x2, cache0, wc, bc, ww, bw, sc, B, Tc, D, K)
    what = f"glu_causal_conv K={K} Tc={Tc} D={D}"
    check(y, want, tol, what)
    newcache = newcache.reshape(B, 1, D * pad)
    want_pool, _ = rg.after(newcache)
    rg.check_pool(rg.pool, want_pool, np.abs(newcache).max() * 16 * U + 1e-7, "cache " + what)


def test_glu_causal_conv_register_and_lds_forms(op):
    """Every (K, Tc) pair of online.hip's register form (K 31 / 15, Tc 16 / 8 / 4 / 2), the LDS form through K = 7 (Tc below and
    above K), K = 31 / 15 with chunks outside the zoo (3, 5), and the generic K = 0 instantiation (K 9, 5); 100 channels (a partial
    last 64-lane workgroup)."""
    rng = np.random.default_rng(41)
    for K in (31, 15):
        for Tc in (16, 8, 4, 2):
            glu_causal_conv_case(op, rng, K, Tc)
    for K, Tc in ((7, 4), (7, 8), (7, 16), (31, 3), (15, 5), (9, 6), (9, 12), (5, 3)):
        glu_causal_conv_case(op, rng, K, Tc)


# ---- Zipformer2 layer glue (elementwise.hip) ---------------------------------------------------------------------------------------------

def biasnorm_ref(x, nb, ls):
    """elementwise.hip:271-312, oracle k2_oracle.c:489-503: y = x (mean((x - b)^2))^-0.5 exp(log_scale)"""
    x = f64(x)
    D = x.shape[1]
    ms = ((x - f64(nb)) ** 2).mean(1, keepdims=True)
    sc = ms ** -0.5 * np.exp(f64(ls)[0])
    # the D-term square sum: 4 u sqrt(D) relative (halved by the square root), the scaling and exp a few ulps more
    return x * sc, np.abs(x * sc) * (2 * U * np.sqrt(D) + 8 * U)


def ds_weights(bias):
    b = f64(bias)
    e = np.exp(b - b.max())
    return e / e.sum()


def downsample_ref(x, bias, ds, B, T, D):
    """SimpleDownsample: softmax(bias)-weighted sum of ds frames, the last frame repeated (k2_oracle.c:825-848); x [B, T, >= D]
    already zero-extended / truncated to D"""
    w = ds_weights(bias)
    Td = (T + ds - 1) // ds
    xr = f64(x).reshape(B, T, -1)[:, :, :D]
    idx = np.minimum(np.arange(Td)[:, None] * ds + np.arange(ds)[None, :], T - 1)   # [Td, ds]
    y = np.einsum("btkd,k->btd", xr[:, idx], w)
    mag = np.einsum("btkd,k->btd", np.abs(xr[:, idx]), w)
    return y.reshape(B * Td, D), sum_tol(mag, ds + 2).reshape(B * Td, D)


def fit(x, D):
    """convert_channels: zero-extend / truncate rows to D (k2_oracle.c:849-857)"""
    x = f64(x)
    out = np.zeros(x.shape[:-1] + (D,))
    n = min(D, x.shape[-1])
    out[..., :n] = x[..., :n]
    return out


def test_biasnorm_bypass_and_their_fused_form(op):
    """biasnorm, bypass, biasnorm_bypass and biasnorm_bypass_downsample (ds2 2 / 4, T no multiple of ds2: the last frame repeated;
    D2 narrower and wider than D) for D 4 / 196 / 260 / 512 / 1024; every row of the norm is one wave, up to 4 float4 per lane."""
    rng = np.random.default_rng(51)
    for D in (4, 196, 260, 512, 1024):
        M = 37
        x, orig, nb, scale = uni(rng, M, D, scale=3.0), uni(rng, M, D), uni(rng, D), uni(rng, D)
        ls = np.array([0.3], np.float32)
        nrm, ntol = biasnorm_ref(x, nb, ls)
        y = nan(M, D)
        op("biasnorm", [M, D], [x, nb, ls, y], {3})
        check(y, nrm, ntol, f"biasnorm D={D}")
        y = nan(M, D)
        op("bypass", [M, D], [orig, x, scale, y], {3})
        o, s = f64(orig), f64(scale)
        check(y, o + (f64(x) - o) * s, 4 * U * (np.abs(o) + np.abs(f64(x)) * (1 + np.abs(s))), f"bypass D={D}")
        want = o + (nrm - o) * s
        wtol = 4 * U * (np.abs(o) + (np.abs(nrm) + np.abs(o)) * np.abs(s)) + ntol * np.abs(s)
        y = nan(M, D)
        op("biasnorm_bypass", [M, D], [x, orig, nb, ls, scale, y], {5})
        check(y, want, wtol, f"biasnorm_bypass D={D}")
        for ds2, T, B, D2 in ((2, 7, 3, D), (4, 10, 2, D + 64 if D <= 512 else D - 128), (4, 3, 1, max(4, D // 8 * 4)), (2, 1, 2, D)):
            M2 = B * T
            x2, orig2 = uni(rng, M2, D, scale=3.0), uni(rng, M2, D)
            bias2 = uni(rng, ds2)
            nrm2, ntol2 = biasnorm_ref(x2, nb, ls)
            o2 = f64(orig2)
            want2 = o2 + (nrm2 - o2) * s
            wtol2 = 4 * U * (np.abs(o2) + (np.abs(nrm2) + np.abs(o2)) * np.abs(s)) + ntol2 * np.abs(s)
            Td2 = (T + ds2 - 1) // ds2
            y, xd2 = nan(M2, D), nan(B * Td2, D2)
            op("biasnorm_bypass_downsample", [B, T, D, ds2, D2], [x2, orig2, nb, ls, scale, y, bias2, xd2], {5, 7})
            what = f"biasnorm_bypass_downsample D={D} ds2={ds2} T={T} D2={D2}"
            check(y, want2, wtol2, what)
            dwant, dtol = downsample_ref(fit(want2, D2), bias2, ds2, B, T, D2)
            check(xd2, dwant, dtol + fit(wtol2, D2).max(), what + " (xd2)")


def test_downsample(op):
    """k_downsample: ds 2 / 4 / 8, T 1 / ds - 1 / ds + 1 / 250 (the last frame repeated into a partial group), input rows narrower
    (zero-extended) and wider (truncated) than D"""
    rng = np.random.default_rng(61)
    for ds in (2, 4, 8):
        for T in (1, ds - 1, ds + 1, 250):
            for D, Din in ((64, 64), (96, 48), (48, 96), (260, 196)):
                B = 2
                x, bias = uni(rng, B * T, Din), uni(rng, ds)
                Td = (T + ds - 1) // ds
                y = nan(B * Td, D)
                op("downsample", [B, T, D, ds, Din], [x, bias, y], {2})
                want, tol = downsample_ref(fit(x, D), bias, ds, B, T, D)
                check(y, want, tol, f"downsample ds={ds} T={T} D={D} Din={Din}")


def upsample_combine_ref(orig, xd, scale, B, T, Td, D, ds):
    """elementwise.hip:614-628 (SimpleUpsample + out_combiner bypass): y[b,t] = o + (xd[b, t / ds] - o) * scale, o = orig fit to D"""
    o = fit(orig, D).reshape(B, T, D)
    u = f64(xd).reshape(B, Td, D)[:, np.arange(T) // ds]
    s = f64(scale)
    y = o + (u - o) * s
    return y.reshape(B * T, D), (4 * U * (np.abs(o) + (np.abs(u) + np.abs(o)) * np.abs(s))).reshape(B * T, D)


def test_upsample_combine_and_its_fused_downsample(op):
    """upsample_combine (orig narrower / wider than D), and upsample_combine_downsample with T no multiple of ds or ds2, D2 narrower
    and wider than D"""
    rng = np.random.default_rng(71)
    for ds, T, D, Dorig in ((2, 7, 64, 64), (4, 10, 96, 48), (8, 250, 48, 96), (2, 1, 196, 260)):
        B = 2
        Td = (T + ds - 1) // ds
        orig, xd, scale = uni(rng, B * T, Dorig), uni(rng, B * Td, D), uni(rng, D)
        want, tol = upsample_combine_ref(orig, xd, scale, B, T, Td, D, ds)
        y = nan(B * T, D)
        op("upsample_combine", [B, T, Td, D, ds, Dorig], [orig, xd, scale, y], {3})
        check(y, want, tol, f"upsample_combine ds={ds} T={T} D={D} Dorig={Dorig}")
        for ds2, D2 in ((2, D), (4, D + 32), (2, max(4, D - 16))):
            Td2 = (T + ds2 - 1) // ds2
            bias2 = uni(rng, ds2)
            y, xd2 = nan(B * T, D), nan(B * Td2, D2)
            op("upsample_combine_downsample", [B, T, Td, D, ds, Dorig, D2, ds2], [orig, xd, scale, y, bias2, xd2], {3, 5})
            what = f"upsample_combine_downsample ds={ds} T={T} D={D} Dorig={Dorig} ds2={ds2} D2={D2}"
            check(y, want, tol, what)
            dwant, dtol = downsample_ref(fit(want, D2), bias2, ds2, B, T, D2)
            check(xd2, dwant, dtol + tol.max(), what + " (xd2)")


def test_downsample_full(op):
    """k_downsample_full: the full-width row gathered from three stack outputs (segment row widths wider than their columns) and
    SimpleDownsample in one launch; then with segment 0 formed on the fly from lz_orig / lz_xd (that stack's out_combiner: orig
    zero-extended, upsampled by 2)"""
    rng = np.random.default_rng(81)
    for ds, T in ((2, 9), (4, 250), (2, 1)):
        B, D = 2, 128
        col1, ld = [64, 96, 128], [64, 112, 128]
        srcs = [uni(rng, B * T, w) for w in ld]
        bias = uni(rng, ds)
        full = np.zeros((B * T, D))
        lo = 0
        for s, c1 in zip(srcs, col1):
            full[:, lo:c1] = f64(s)[:, lo:c1]
            lo = c1
        Td = (T + ds - 1) // ds
        y = nan(B * Td, D)
        op("downsample_full", [3, *ld, *col1, 0, 1, 0, B, T, D, ds], [*srcs, None, None, None, bias, y], {7})
        want, tol = downsample_ref(full, bias, ds, B, T, D)
        check(y, want, tol, f"downsample_full ds={ds} T={T}")
        lz_ds, lz_Do = 2, 48
        lz_Td = (T + lz_ds - 1) // lz_ds
        lz_orig, lz_xd, lz_scale = uni(rng, B * T, lz_Do), uni(rng, B * lz_Td, ld[0]), uni(rng, ld[0])
        seg0, seg0_tol = upsample_combine_ref(lz_orig, lz_xd, lz_scale, B, T, lz_Td, ld[0], lz_ds)
        full[:, :col1[0]] = seg0[:, :col1[0]]
        y = nan(B * Td, D)
        op("downsample_full", [3, *ld, *col1, lz_Td, lz_ds, lz_Do, B, T, D, ds], [*srcs, lz_orig, lz_xd, lz_scale, bias, y], {7})
        want, tol = downsample_ref(full, bias, ds, B, T, D)
        check(y, want, tol + seg0_tol.max(), f"downsample_full lazy ds={ds} T={T}")


def dwconv1d_ref(x, w, b, B, T, D, K, glu, act):
    """elementwise.hip:451-553; oracle k2_oracle.c:768-800 (conv_module): act(bias + sum_k w[k] g[t + k - K/2]) with g = GLU(x)
    (value | gate halves) or x itself, zero outside [0, T)"""
    a = f64(x).reshape(B, T, -1)
    if glu:
        gate = a[..., D:]
        g = a[..., :D] * sigmoid64(gate)
        gtol = np.abs(g) * (np.abs(gate) + 8) * U
    else:
        g, gtol = a, np.zeros_like(a)
    W = f64(w)
    gp = np.zeros((B, T + K - 1, D))
    gp[:, K // 2:K // 2 + T] = g
    gm = np.abs(gp)
    z = np.broadcast_to(f64(b), (B, T, D)).copy()
    zm = np.abs(z)
    for k in range(K):
        z += W[k] * gp[:, k:k + T]
        zm += np.abs(W[k]) * gm[:, k:k + T]
    ztol = sum_tol(zm, K + 1) + gtol.max() * np.sqrt((W ** 2).sum(0))
    y = swoosh_r64(z) if act == "swoosh" else dswish64(z)
    return y.reshape(B * T, D), act_tol(z, ztol).reshape(B * T, D)


def test_depthwise_conv1d_every_outputs_per_thread(op):
    """k_glu_dwconv1d<DSWISH, GLU, TT> through glu_dwconv1d_swoosh, glu_dwconv1d_dswish and dwconv1d_swoosh: K 7 / 15 / 31,
    T 1 / K/2 / K-1 / K / 33 / 300, D 4 / 196 / 260 / 512 (one lane, a partial 256-channel workgroup, two of them), and each of
    TT = 8 / 4 / 2 forced through K2HIP_DW1D_TT"""
    rng = np.random.default_rng(91)
    ran = 0
    for K in (7, 15, 31):
        for T in sorted({1, K // 2, K - 1, K, 33, 300}):
            for D in (4, 196, 260, 512):
                B = 2 if T * D <= 300 * 260 else 1
                w, b = uni(rng, K, D, scale=0.5), uni(rng, D)
                x2 = uni(rng, B * T, 2 * D, scale=2.0)
                x1 = uni(rng, B * T, D, scale=2.0)
                cases = [("glu_dwconv1d_swoosh", x2, True, "swoosh"), ("glu_dwconv1d_dswish", x2, True, "dswish"),
                         ("dwconv1d_swoosh", x1, False, "swoosh")]
                for name, x, glu, act in cases:
                    want, tol = dwconv1d_ref(x, w, b, B, T, D, K, glu, act)
                    for tt in (8, 4, 2):
                        y = nan(B * T, D)
                        with switch("K2HIP_DW1D_TT", tt):
                            op(name, [B, T, D, K], [x, w, b, y], {3})
                        check(y, want, tol, f"{name} K={K} T={T} D={D} TT={tt}")
                        ran += 1
    assert ran == 3 * 3 * 4 * sum(len({1, K // 2, K - 1, K, 33, 300}) for K in (7, 15, 31))


def test_dwconv7x7_every_form(op):
    """ConvNeXt's depthwise 7x7 (elementwise.hip:85-269) offline (Tin = Tout, tpad 3) and streaming (Tin = Tout + 6, tpad 0):
    the sliding LDS-DMA form (C % 32 == 0, F <= 24, T >= 48), the one-shot tiled form (short T, or K2HIP_DW7_TILED), the per-pixel
    form (C = 36: no multiple of the 32-channel group); T no multiple of the 8-frame tile or of the sliding form's 32 / 64-frame
    range, F 19 / 7 / 24.  Tolerance: 49 + 1 terms."""
    rng = np.random.default_rng(101)
    for Tout, F, C, stream in ((70, 19, 64, False), (50, 7, 32, True), (13, 24, 64, False), (5, 19, 36, False), (49, 3, 36, True),
                               (300, 19, 128, True), (1, 19, 32, False)):
        B = 2
        Tin, tpad = (Tout + 6, 0) if stream else (Tout, 3)
        x, w, b = uni(rng, B * Tin * F * C), uni(rng, 49, C, scale=0.3), uni(rng, C)
        xp = np.zeros((B, Tin + 6, F + 6, C))
        xp[:, 3:3 + Tin, 3:3 + F] = f64(x).reshape(B, Tin, F, C)
        want = np.broadcast_to(f64(b), (B, Tout, F, C)).copy()
        mag = np.abs(want)
        t0 = 3 - tpad
        for kt in range(7):
            for kf in range(7):
                sl = xp[:, t0 + kt:t0 + kt + Tout, kf:kf + F]
                want += f64(w)[kt * 7 + kf] * sl
                mag += np.abs(f64(w)[kt * 7 + kf]) * np.abs(sl)
        for tiled in (0, 1):
            y = nan(B * Tout * F * C)
            with switch("K2HIP_DW7_TILED", tiled):
                op("dwconv7x7", [B, Tin, Tout, tpad, F, C], [x, w, b, y], {3})
            check(y.reshape(B, Tout, F, C), want, sum_tol(mag, 50), f"dwconv7x7 T={Tout} F={F} C={C} stream={stream} tiled={tiled}")
