"""Cases and float64 references for the kernels AROUND the encoder layers, one launch at a time through k2hip_debug_op_run: the offline
front end (gather_samples of csrc/fbank.hip; pad_logfloor, pad_logfloor_dense, conv0_swoosh of elementwise.hip), the streaming state
movers of csrc/online.hip (convnext_cat, cat_shift plain and tanh-gated, cat_keep, fifo_append, fifo_gather, logfloor_inplace,
zero_floats), the small float4 kernels (glu_sigmoid, tanh_gate, convert_channels, copy_cols, tanh_add) and the search tail of
csrc/greedy.hip (log_softmax_rows, argmax_rows, argmax_first_rows, ctc_collapse, first_emit_frame).

Importable without a GPU, like tests/family_kernels.py whose shape this file has: every operation is written ONCE, as
SIM[name](dt, iargs, bufs) on the hook's own arguments; want() runs it on float64 copies (the reference), standin() on the float32
buffers themselves.  tests/test_outer_kernels_gpu.py runs every case with the `op` fixture, tests/test_outer_kernels_ref.py runs them
with standin() in the kernel's place, holds the arithmetic references to torch, and runs every entry of MUTANTS -- a deliberately
wrong stand-in of one op -- through its own case, which must reject it.

Integer outputs and pure data movement are compared exactly: bit for bit, including every float of a state pool, FIFO or output
tail that the launch must not touch (pools are filled with a sentinel, pure outputs with NaN).  Tolerances of the arithmetic, per
element, in units of u = 2^-24:
  * conv0_swoosh: the 10-term sum at sum_tol, through act_tol (SwooshR on the hardware exp / log), as the DoubleSwish forms;
  * glu_sigmoid y = a / (1 + exp(-s)) on the hardware exp: the exponential's argument carries |s| u (the product with log2 e) and the
    instruction 2 u, the add, the divide and the product one u each, and d sigmoid / d ln e <= 1: |y| (|s| + 8) u;
  * tanh_gate y = a t, t = (1 - e) / (1 + e), e = exp(-2 |s|) on the hardware exp: e carries e (2 |s| + 2) u, which reaches t through
    2 / (1 + e)^2, i.e. (1 - t^2) (|s| + 1) u at most; 1 - e and 1 + e round at u each (both are below 2), the divide and the product
    at u: |a| (4 + 2 |s| (1 - t^2)) u + |y| u.  Near 0 this is an ABSOLUTE 4 u on t -- the form cancels there, by design;
  * the library's tanhf (cat_shift's gate, tanh_add): 5 ulp = 10 u relative (family_kernels.LIBM_TANH), + the product's u;
    tanh_add's argument e + d rounds at u |e + d| and tanh' = 1 - t^2;
  * log_softmax_rows out = (x - m) - log(sum exp(x - m)) with the library's expf / logf (3 ulp = 6 u each): c = x - m rounds at
    u |c|; a term exp(c_k) carries (|c_k| + 6) u relative, so the sum S carries sum_k p_k (|c_k| + 6) u + 4 u sqrt(V) (positive terms:
    the magnitude sum is S itself) and log S that absolute error + 6 u |log S|; the final subtraction u |out|."""
import numpy as np

from family_kernels import LIBM_TANH, Env, conv0_parts, null_switch, r4, same_bits  # noqa: F401  (Env, null_switch: for the tests)
from test_kernels_gpu import SENTINEL, U, act_tol, check, f64, nan, sum_tol, swoosh_r64, uni

LOG_FLOOR = np.float32(-23.025850929940457)    # PadHelper.cs:58, as elementwise.hip / online.hip spell it
INT_MAX = 2 ** 31 - 1
BLANK, UNK = 0, 2
IFILL = -77                                     # what integer outputs hold before a launch


# ---- the operations ----------------------------------------------------------------------------------------------------------------------

def _floor(v):
    return np.where(v == 0, v.dtype.type(LOG_FLOOR), v)


def sim_pad_logfloor(dt, ia, b):
    B, L = ia
    out = b[3].reshape(B, L)
    for s in range(B):
        n, o = int(b[2][s]), int(b[1][s])
        row = np.zeros(L, out.dtype)
        row[:min(n, L)] = b[0][o:o + min(n, L)]
        out[s] = _floor(row)


def sim_pad_logfloor_dense(dt, ia, b):
    n, B, L = ia
    out = b[1].reshape(B, L)
    for s in range(B):
        row = np.zeros(L, out.dtype)
        row[:min(n, L)] = b[0][s * n:s * n + min(n, L)]
        out[s] = _floor(row)


def sim_gather_samples(dt, ia, b):
    B, nmax = ia[:2]
    dst = b[2].reshape(B, nmax)
    for s in range(B):
        n, o = int(b[1][s]), ia[2 + s]
        dst[s, :n] = b[0][o:o + n]
        dst[s, n:] = 0


def _swoosh_r(z):
    return np.logaddexp(z.dtype.type(0.0), z - z.dtype.type(1.0)) - z.dtype.type(0.08) * z - z.dtype.type(0.313261687)


def sim_conv0_swoosh(dt, ia, b):
    B, T, F = ia
    z, _ = conv0_parts(b[0], b[1], b[2], B, T, F, 0)
    b[3].reshape(z.shape)[...] = _swoosh_r(z)


def _slot(pool, slot, ss, off, n):
    return pool[slot * ss + off:slot * ss + off + n]


def sim_convnext_cat(dt, ia, b):
    """online.hip:20-24: cat[b] = [cached_left_pad ; x], the cache ([C][3][F]) advanced to x's frames Tc-3 .. Tc-1, byp[b] = x[b, :Tc]"""
    ss, off, B, T3, Tc, F, C = ia
    a3, pool, slots = b[0].reshape(B, T3, F, C), b[1], b[2]
    cat, byp = b[3].reshape(B, T3 + 3, F, C), b[4].reshape(B, Tc, F, C)
    for s in range(B):
        cache = _slot(pool, slots[s], ss, off, C * 3 * F).reshape(C, 3, F)
        cat[s, :3] = cache.transpose(1, 2, 0)
        cat[s, 3:] = a3[s]
        cache[...] = a3[s, Tc - 3:Tc].transpose(2, 0, 1)
        byp[s] = a3[s, :Tc]


def _tanh(z):
    return np.tanh(z)


def _newrows(b2, B, Tc, ldn, width, gated):
    x = b2.reshape(B, Tc, ldn)
    return x[..., width:2 * width] * _tanh(x[..., :width]) if gated else x[..., :width]


def _cat_then_cache(ia, b, row0, gated):
    ss, off, ldn, B, L, Tc, width = ia[:7]
    rows = _newrows(b[2], B, Tc, ldn, width, gated)
    cat = b[3].reshape(B, L + Tc, width)
    for s in range(B):
        cache = _slot(b[0], b[1][s], ss, off, L * width).reshape(L, width)
        cat[s, :L] = cache
        cat[s, L:] = rows[s]
        cache[...] = cat[s, row0:row0 + L]


def sim_cat_shift(dt, ia, b):
    """online.hip:48-53: cat[b] = [cache ; new rows], cache <- cat[b][Tc:]"""
    _cat_then_cache(ia, b, ia[5], bool(ia[7]))


def sim_cat_keep(dt, ia, b):
    """kernels.h cat_keep: the same with the keep_back newest rows kept out of the cache: cache <- cat[Tc - keep_back ..)"""
    _cat_then_cache(ia, b, ia[5] - ia[7], False)


def sim_fifo_append(dt, ia, b):
    cap, feat, G, nf = ia
    fifo, src = b[0].reshape(-1, cap, feat), b[1].reshape(G, nf, feat)
    for g in range(G):
        if b[3][g] < 0:
            continue
        for i in range(nf):
            fifo[b[2][g], (b[3][g] + i) % cap] = src[g, i]


def sim_fifo_gather(dt, ia, b):
    cap, feat, B, T = ia
    fifo, x = b[0].reshape(-1, cap, feat), b[3].reshape(B, T, feat)
    for s in range(B):
        for t in range(T):
            x[s, t] = _floor(fifo[b[1][s], (b[2][s] + t) % cap])


def sim_zero_floats(dt, ia, b):
    b[0][:ia[0]] = 0


def sim_logfloor_inplace(dt, ia, b):
    b[0][:ia[0]] = _floor(b[0][:ia[0]])


def _sigmoid(z):
    return z.dtype.type(1.0) / (z.dtype.type(1.0) + np.exp(-z))


def sim_glu_sigmoid(dt, ia, b):
    M, D = ia
    x = b[0].reshape(M, 2 * D)
    b[1].reshape(M, D)[...] = x[:, :D] * _sigmoid(x[:, D:])


def sim_tanh_gate(dt, ia, b):
    M, Hc = ia
    x = b[0].reshape(M, 3 * Hc)
    b[1].reshape(M, Hc)[...] = x[:, Hc:2 * Hc] * _tanh(x[:, :Hc])


def sim_convert_channels(dt, ia, b):
    M, Din, Dout = ia
    y = b[1].reshape(M, Dout)
    y[...] = 0
    y[:, :min(Din, Dout)] = b[0].reshape(M, Din)[:, :min(Din, Dout)]


def sim_copy_cols(dt, ia, b):
    ldx, xc, ldy, yc, M, n = ia
    b[1].reshape(M, ldy)[:, yc:yc + n] = b[0].reshape(M, ldx)[:, xc:xc + n]


def sim_tanh_add(dt, ia, b):
    ds, N, J = ia
    dec = np.stack([b[1][r * ds:r * ds + J] for r in range(N)])
    b[2].reshape(N, J)[...] = _tanh(b[0].reshape(N, J) + dec)


def sim_log_softmax_rows(dt, ia, b):
    M, V = ia
    x = b[0].reshape(M, V)
    c = x - x.max(-1, keepdims=True)
    with np.errstate(divide="ignore"):
        x[...] = c - np.log(np.exp(c).sum(-1, keepdims=True))


def scan_later_wins(row):
    """OfflineRecognizer.cs:150-154 / :236-240, as quoted above k_argmax_rows, transcribed literally:
           token_num = logits[j, token_num] > logits[j, k] ? token_num : k;      (k = 1 .. V-1, token_num = 0 at the start)"""
    token_num = 0
    for k in range(1, len(row)):
        token_num = token_num if row[token_num] > row[k] else k
    return token_num


def index_of_max(row):
    """Array.IndexOf(row, row.Max()) (OfflineRecognizer.cs:335,396): Enumerable.Max orders NaN below every number, so it returns NaN
    only for a row of nothing but NaNs, and IndexOf (Equals: NaN equals NaN) then finds element 0; else the first index of the maximum"""
    mx, seen = None, False
    for v in row:
        if v != v:
            continue
        if not seen or v > mx:
            mx, seen = v, True
    if not seen:
        return 0
    for k, v in enumerate(row):
        if v == mx:
            return k
    raise AssertionError


def _argmax(pick):
    def sim(dt, ia, b):
        ld, N, V = ia
        x = b[0].reshape(N, ld)
        for r in range(N):
            b[1][r] = pick([float(v) for v in x[r, :V]])
    return sim


def sim_ctc_collapse(dt, ia, b):
    """OfflineRecognizer.cs:383-408 as k_ctc_collapse states it; an entry past max_tokens is counted, flagged and not written"""
    B, Tp, mt = ia
    tok, fo, tokens, ts, n_tokens, trail, any_, flag = b
    tok = tok.reshape(B, Tp)
    for s in range(B):
        prev, n, tr, an = -1, 0, 0, 0
        for t in range(Tp):
            y = int(tok[s, t])
            if y == BLANK:
                tr += 1
            else:
                tr, an = 0, 1
            if y != BLANK and y != prev:
                if n < mt:
                    tokens[s * mt + n] = y
                    ts[s * mt + n] = t + (0 if fo is None else int(fo[s]))
                else:
                    flag[0] = 1
                n += 1
            prev = y
        n_tokens[s], trail[s], any_[s] = min(n, mt), tr, an


def sim_first_emit_frame(dt, ia, b):
    B, Tp, skip1 = ia
    tok = b[0].reshape(B, Tp)
    emit = (tok != BLANK) & (tok != UNK) & ~((tok == 1) & bool(skip1))
    fr = np.where(emit.any(0))[0]
    b[1][0] = int(fr[0]) if len(fr) else INT_MAX


SIM = {
    "pad_logfloor": sim_pad_logfloor, "pad_logfloor_dense": sim_pad_logfloor_dense, "gather_samples": sim_gather_samples,
    "conv0_swoosh": sim_conv0_swoosh, "convnext_cat": sim_convnext_cat, "cat_shift": sim_cat_shift, "cat_keep": sim_cat_keep,
    "fifo_append": sim_fifo_append, "fifo_gather": sim_fifo_gather, "zero_floats": sim_zero_floats,
    "logfloor_inplace": sim_logfloor_inplace, "glu_sigmoid": sim_glu_sigmoid, "tanh_gate": sim_tanh_gate,
    "convert_channels": sim_convert_channels, "copy_cols": sim_copy_cols, "tanh_add": sim_tanh_add,
    "log_softmax_rows": sim_log_softmax_rows, "argmax_rows": _argmax(scan_later_wins), "argmax_first_rows": _argmax(index_of_max),
    "ctc_collapse": sim_ctc_collapse, "first_emit_frame": sim_first_emit_frame,
}
CALLED = set()   # the ops the cases have launched so far (the tests assert it covers SIM)
RATIO = [0.0]    # the largest error / tolerance of the float comparisons so far


def want(name, ia, bufs):
    """the reference: the operation in float64 on copies of the buffers; returns the buffers after it"""
    b = [None if a is None else (a.astype(np.float64) if a.dtype == np.float32 else a.copy()) for a in bufs]
    with np.errstate(invalid="ignore"):
        SIM[name](np.float64, [int(v) for v in ia], b)
    return b


def make_standin(sims):
    def run(name, ia, bufs, outs, expect=0):
        """in the kernel's place: the same formulas in float32 numpy, on the buffers themselves"""
        CALLED.add(name)
        assert expect == 0 and all(b is None or b.dtype != np.float64 for b in bufs), name
        with np.errstate(over="ignore", invalid="ignore"):
            sims[name](np.float32, [int(v) for v in ia], bufs)
        for b in bufs:
            assert b is None or b.dtype in (np.float32, np.int32, np.int64), (name, "an operation left float32")
        return 0
    return run


standin = make_standin(SIM)


def launch(env, name, ia, bufs, outs):
    CALLED.add(name)
    return env.op(name, ia, bufs, outs)


def moved(got, ref, what, keep=None):
    """pure data movement: `got` (float32) is bit for bit the float64 reference's result (which only copied float32 values)"""
    with np.errstate(invalid="ignore"):
        same_bits(got, ref.astype(np.float32), keep, what)


def ints(got, ref, what):
    assert got.dtype == ref.dtype and np.array_equal(got, ref), (what, got.reshape(-1)[:16].tolist(), ref.reshape(-1)[:16].tolist())


def close(got, ref, tol, what):
    check(got, ref, tol, what)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(f64(got) - ref) / np.broadcast_to(tol, ref.shape)
    RATIO[0] = max(RATIO[0], float(np.nanmax(np.where(np.broadcast_to(tol, ref.shape) > 0, r, 0.0))))


def zeros_into(rng, a, k=6):
    """genuine 0.0 and -0.0 at k random places each of a float32 array"""
    flat = a.reshape(-1)
    idx = rng.choice(flat.size, size=min(2 * k, flat.size), replace=False)
    flat[idx[::2]] = 0.0
    flat[idx[1::2]] = -0.0
    return a


class Pool:
    """a state pool of `nslots` slots of `stride` floats (sentinel fill), the streams' state of n floats at `off` inside their slots"""

    def __init__(self, rng, slots, nslots, n, off=36, extra=20):
        self.off, self.n, self.stride = off, n, off + n + extra
        self.slots = np.asarray(slots, np.int32)
        self.pool = np.full(nslots * self.stride, SENTINEL, np.float32)
        for s in self.slots:
            _slot(self.pool, s, self.stride, off, n)[...] = uni(rng, n)

    def ints(self):
        return [self.stride, self.off]


# ---- the offline front end -----------------------------------------------------------------------------------------------------------------

def case_pad_logfloor(env):
    """k_pad_logfloor / k_pad_logfloor_dense: B = 3 with lengths L, L - 80, 0 at offsets that are no multiples of 4, genuine 0.0 and
    -0.0 in the data (both become the floor, like the padding); L = 131072 + 160 makes the 512 x 256 grid-stride loop repeat"""
    rng = np.random.default_rng(5000)
    for L in (800, 131072 + 160):
        lens = np.array([L, L - 80, 0], np.int64)
        offs = np.array([3, 3 + L + 2, 3 + L + 2 + (L - 80) + 1], np.int64)
        packed = zeros_into(rng, uni(rng, int(offs[2]) + 5, scale=9.0), 40)
        packed[offs[0]], packed[offs[1] + L - 81] = 0.0, -0.0
        ia, bufs = [3, L], [packed, offs, lens, nan(3, L)]
        ref = want("pad_logfloor", ia, bufs)
        assert (ref[3] == LOG_FLOOR).sum() > 80 + L
        launch(env, "pad_logfloor", ia, bufs, {3})
        moved(bufs[3], ref[3], f"pad_logfloor L={L}")
        for n in ((L, L - 80, 0) if L < 1000 else (L - 80,)):
            feats = zeros_into(rng, uni(rng, max(3 * n, 4), scale=9.0), 40)
            ia, bufs = [n, 3, L], [feats, nan(3, L)]
            ref = want("pad_logfloor_dense", ia, bufs)
            launch(env, "pad_logfloor_dense", ia, bufs, {1})
            moved(bufs[1], ref[1], f"pad_logfloor_dense L={L} n={n}")


def case_gather_samples(env):
    """k_gather_samples: B = 3, counts nmax / nmax - 5 / 0 in both orders over a 16-byte-aligned source, one a float behind a boundary
    and an unread one; nmax 8, 70001 (dst + b nmax misaligned for b >= 1, the 64 x 256 x 4 grid-stride loop repeats) and 70004 (every
    dst aligned: the float4 path up to a count that is no multiple of 4).  Every source is followed by non-zero floats, so a copy
    across its count shows; dst exact including its zero tail"""
    rng = np.random.default_rng(5100)
    for nmax in (8, 70001, 70004):
        for counts in ((nmax - 5, nmax, 0), (nmax, nmax - 5, 0)):
            span = r4(nmax) + 8
            offs = [0, span + 1, 2 * span]
            samples = uni(rng, 3 * span) + np.float32(2.0)          # (no zero anywhere: what is behind a count is visibly not padding)
            n = np.array(counts, np.int64)
            ia, bufs = [3, nmax, *offs], [samples, n, nan(3, nmax)]
            ref = want("gather_samples", ia, bufs)
            launch(env, "gather_samples", ia, bufs, {2})
            moved(bufs[2], ref[2], f"gather_samples nmax={nmax} counts={counts}")


def case_conv0_swoosh(env):
    """k_conv0<0, false> (Zipformer2's conv.0: no time padding, SwooshR), the instantiation the family tests do not launch"""
    rng = np.random.default_rng(5200)
    for B, T, F in ((1, 3, 1), (2, 5, 7), (2, 9, 80)):
        x, w, bias, y = uni(rng, B, T, F, scale=2.0), uni(rng, 72, scale=0.5), uni(rng, 8), nan(B, T - 2, F, 8)
        launch(env, "conv0_swoosh", [B, T, F], [x, w, bias, y], {3})
        z, zm = conv0_parts(f64(x), f64(w), f64(bias), B, T, F, 0)
        close(y, swoosh_r64(z), act_tol(z, sum_tol(zm, 10)), f"conv0_swoosh B={B} T={T} F={F}")


# ---- the streaming state movers ------------------------------------------------------------------------------------------------------------

def case_convnext_cat(env):
    """k_convnext_cat: C = 8, F = 5, streams in slots 5, 0, 2 of 6; chunks of exactly 3 frames, shorter than the input, and 16 of 22;
    cat, byp, the advanced cache in its [C][3][F] layout and the rest of the pool bit for bit"""
    rng = np.random.default_rng(5300)
    C, F, B = 8, 5, 3
    for T3, Tc in ((3, 3), (7, 3), (9, 9), (22, 16)):
        pl = Pool(rng, [5, 0, 2], 6, C * 3 * F)
        ia = [*pl.ints(), B, T3, Tc, F, C]
        bufs = [uni(rng, B, T3, F, C), pl.pool, pl.slots, nan(B, T3 + 3, F, C), nan(B, Tc, F, C)]
        ref = want("convnext_cat", ia, bufs)
        launch(env, "convnext_cat", ia, bufs, {1, 3, 4})
        what = f"convnext_cat T3={T3} Tc={Tc}"
        moved(bufs[3], ref[3], what + " cat")
        moved(bufs[4], ref[4], what + " byp")
        moved(bufs[1], ref[1], what + " pool")


CAT_SHAPES = [(0, 4), (3, 4), (4, 4), (8, 4), (10, 4), (33, 4), (70, 4), (5, 1), (64, 16)]


def case_cat_shift(env, gated):
    """k_cat_shift<GATE>: width 8, rows of width + 4 (gated: 2 width + 4) floats with NaN behind the columns the kernel reads, B = 3 in
    permuted slots; L = 0, L < Tc, L = Tc, multiples and non-multiples of Tc, L > 8 Tc (the chain's second group of 8 loads), Tc = 1.
    Two launches in a row on the same pool: the second cat shows the cache the first one left.  What only moves is compared bit for
    bit (the whole pool and cat of the plain form; the gated form's old cache rows), the gated rows at the library tanh's bound"""
    rng = np.random.default_rng(5400 + gated)
    width, B = 8, 3
    ldn = (2 * width if gated else width) + 4
    for L, Tc in CAT_SHAPES:
        pl = Pool(rng, rng.permutation(5)[:B], 5, L * width)
        for rnd in range(2):
            new = uni(rng, B, Tc, ldn, scale=3.0)
            new[..., ldn - 4:] = np.nan
            ia, bufs = [*pl.ints(), ldn, B, L, Tc, width, gated], [pl.pool, pl.slots, new, nan(B, L + Tc, width)]
            ref = want("cat_shift", ia, bufs)
            launch(env, "cat_shift", ia, bufs, {0, 3})
            what = f"cat_shift gated={gated} L={L} Tc={Tc} launch {rnd}"
            if not gated:
                moved(bufs[3], ref[3], what + " cat")
                moved(bufs[0], ref[0], what + " pool")
                continue
            # rows computed by this launch: cat rows L.., cache rows r with r + Tc >= L
            ccat = np.zeros((B, L + Tc, width), bool)
            ccat[:, L:] = True
            cpool = np.zeros(pl.pool.shape, bool)
            for s in pl.slots:
                _slot(cpool, s, pl.stride, pl.off, L * width).reshape(L, width)[max(L - Tc, 0):] = True
            moved(bufs[3], ref[3], what + " cat (cache rows)", ~ccat)
            moved(bufs[0], ref[0], what + " pool (moved rows, other slots)", ~cpool)
            tol = lambda v: (LIBM_TANH + U) * np.abs(v)
            close(bufs[3][ccat], ref[3].reshape(B, L + Tc, width)[ccat], tol(ref[3].reshape(B, L + Tc, width)[ccat]), what + " cat (new rows)")
            if cpool.any():
                close(bufs[0][cpool], ref[0][cpool], tol(ref[0][cpool]), what + " pool (new rows)")
                # the cache's copy of a new row is the very float cat holds
                for k, s in enumerate(pl.slots):
                    c = _slot(bufs[0], s, pl.stride, pl.off, L * width).reshape(L, width)
                    same_bits(c, np.ascontiguousarray(bufs[3][k, Tc:Tc + L]), None, what + " cache vs cat")


def case_cat_keep(env):
    """k_cat_keep<0 / 1>: keep_back 0 (cat_shift's result), in between, Tc (the cache keeps its place in cat), and L < Tc"""
    rng = np.random.default_rng(5500)
    width, B = 8, 3
    ldn = width + 4
    for L, Tc, kb in ((6, 4, 0), (6, 4, 2), (6, 4, 4), (2, 4, 1)):
        pl = Pool(rng, rng.permutation(5)[:B], 5, L * width)
        new = uni(rng, B, Tc, ldn)
        new[..., width:] = np.nan
        ia, bufs = [*pl.ints(), ldn, B, L, Tc, width, kb], [pl.pool, pl.slots, new, nan(B, L + Tc, width)]
        ref = want("cat_keep", ia, bufs)
        launch(env, "cat_keep", ia, bufs, {0, 3})
        moved(bufs[3], ref[3], f"cat_keep L={L} Tc={Tc} keep_back={kb} cat")
        moved(bufs[0], ref[0], f"cat_keep L={L} Tc={Tc} keep_back={kb} pool")


def case_fifo(env):
    """k_fifo_append / k_fifo_gather: feat 80, cap 12, 3 streams in slots of 5; pos -1 (skipped: its ring bit-equal), 0, 9 (wraps with
    5 frames); head 0 / 10 / 3 with T = 6 (10 wraps); the rows hold 0.0 and -0.0, floored on gather; the FIFO itself stays as it is"""
    rng = np.random.default_rng(5600)
    feat, cap, nslots = 80, 12, 5
    fifo = zeros_into(rng, uni(rng, nslots, cap, feat), 60)
    slots = np.array([3, 0, 4], np.int32)
    for pos in ([-1, 0, 9], [9, -1, 0]):
        src = zeros_into(rng, uni(rng, 3, 5, feat), 30)
        ia, bufs = [cap, feat, 3, 5], [fifo, src, slots, np.array(pos, np.int32)]
        ref = want("fifo_append", ia, bufs)
        launch(env, "fifo_append", ia, bufs, {0})
        moved(fifo, ref[0], f"fifo_append pos={pos}")
    for head in ([0, 10, 3], [10, 0, 10]):
        fifo0 = fifo.copy()
        ia, bufs = [cap, feat, 3, 6], [fifo, slots, np.array(head, np.int32), nan(3, 6, feat)]
        ref = want("fifo_gather", ia, bufs)
        assert (ref[3] == LOG_FLOOR).sum() >= 4
        launch(env, "fifo_gather", ia, bufs, {0, 3})
        moved(bufs[3], ref[3], f"fifo_gather head={head}")
        same_bits(fifo, fifo0, None, f"fifo_gather head={head} (the FIFO)")


def case_floor_and_zero(env):
    """k_logfloor / k_zero: n 1 / 255 / 257 / 1000 inside a longer buffer whose tail must stay as it is"""
    rng = np.random.default_rng(5700)
    for n in (1, 255, 257, 1000):
        for name in ("logfloor_inplace", "zero_floats"):
            x = zeros_into(rng, uni(rng, n + 9), max(1, n // 20))
            x[0], x[n - 1] = 0.0, -0.0
            x[n:] = 0.0 if name == "logfloor_inplace" else SENTINEL       # behind n: zeros that must NOT be floored / floats that stay
            ref = want(name, [n], [x])
            launch(env, name, [n], [x], {0})
            moved(x, ref[0], f"{name} n={n}")


# ---- small float4 kernels --------------------------------------------------------------------------------------------------------------------

def case_gates(env):
    """k_glu (M 1 / 5, D 4 / 20) and k_tanh_gate (rows of 3 Hc, gate arguments out to +-12, among them 0 and values around it)"""
    rng = np.random.default_rng(5800)
    for M in (1, 5):
        for D in (4, 20):
            x, y = uni(rng, M, 2 * D, scale=6.0), nan(M, D)
            launch(env, "glu_sigmoid", [M, D], [x, y], {1})
            a, s = f64(x)[:, :D], f64(x)[:, D:]
            ref = a / (1.0 + np.exp(-s))
            close(y, ref, np.abs(ref) * (np.abs(s) + 8.0) * U, f"glu_sigmoid M={M} D={D}")
            Hc = D
            x, y = uni(rng, M, 3 * Hc, scale=12.0), nan(M, Hc)
            x[:, :4] = [12.0, -12.0, 0.0, 1e-3]
            x[:, 2 * Hc:] = np.nan                                      # the y third of NonlinAttention's row: not this kernel's
            launch(env, "tanh_gate", [M, Hc], [x, y], {1})
            s, a = f64(x)[:, :Hc], f64(x)[:, Hc:2 * Hc]
            t = np.tanh(s)
            close(y, a * t, np.abs(a) * (4.0 + 2.0 * np.abs(s) * (1.0 - t * t)) * U + np.abs(a * t) * U, f"tanh_gate M={M} Hc={Hc}")


def case_channels_and_cols(env):
    """k_convert_channels (equal, zero-extended, truncated) and k_copy_cols (both column offsets non-zero, both row strides wider than
    the rows; y outside the copied columns keeps its bits)"""
    rng = np.random.default_rng(5900)
    for Din, Dout in ((8, 8), (8, 12), (12, 8)):
        M = 5
        x, y = uni(rng, M, Din), nan(M, Dout)
        ref = want("convert_channels", [M, Din, Dout], [x, y])
        launch(env, "convert_channels", [M, Din, Dout], [x, y], {1})
        moved(y, ref[1], f"convert_channels {Din} -> {Dout}")
    for M, n, ldx, xc, ldy, yc in ((5, 8, 20, 4, 16, 8), (1, 4, 12, 8, 8, 4), (70, 16, 24, 8, 28, 4)):
        x, y = uni(rng, M, ldx), uni(rng, M, ldy)
        ia = [ldx, xc, ldy, yc, M, n]
        ref = want("copy_cols", ia, [x, y])
        launch(env, "copy_cols", ia, [x, y], {1})
        moved(y, ref[1], f"copy_cols M={M} n={n}")


def case_tanh_add(env):
    """k_tanh_add: J = 8, N = 5; dec_stride 0 (one decoder row for every frame) and J; sums out to +-9 (saturated tanh)"""
    rng = np.random.default_rng(6000)
    N, J = 5, 8
    for ds in (0, J):
        enc, dec, y = uni(rng, N, J, scale=6.0), uni(rng, (N - 1) * ds + J, scale=3.0), nan(N, J)
        launch(env, "tanh_add", [ds, N, J], [enc, dec, y], {2})
        z = f64(enc) + np.stack([f64(dec)[r * ds:r * ds + J] for r in range(N)])
        t = np.tanh(z)
        close(y, t, U * np.abs(z) * (1.0 - t * t) + LIBM_TANH * np.abs(t), f"tanh_add dec_stride={ds}")


# ---- the search tail -------------------------------------------------------------------------------------------------------------------------

def case_log_softmax(env, V):
    """k_log_softmax_rows: random rows, a row of equal values, a row spanning +-80, a row with -inf entries (V > 1), M = 6 or 7 rows
    (no multiple of the four waves); -inf stays -inf, the rest within the bound of the module docstring"""
    rng = np.random.default_rng(6100 + V)
    rows = [uni(rng, V, scale=3.0) for _ in range(3)] + [np.full(V, 1.25, np.float32)]
    rows.append(rng.permutation(np.linspace(-80.0, 80.0, V)).astype(np.float32) if V > 1 else np.array([80.0], np.float32))
    rows.append(uni(rng, V, scale=30.0))
    if V > 1:
        r = uni(rng, V, scale=3.0)
        r[rng.choice(V, size=max(1, V // 3), replace=False)] = -np.inf
        rows.append(r)
    x = np.stack(rows)
    M = len(rows)
    x0 = f64(x)
    launch(env, "log_softmax_rows", [M, V], [x], {0})
    c = x0 - x0.max(-1, keepdims=True)
    S = np.exp(c).sum(-1, keepdims=True)
    p = np.exp(c) / S
    with np.errstate(invalid="ignore"):
        dS = np.where(p > 0, p * (np.abs(c) + 6.0), 0.0).sum(-1, keepdims=True) * U + 4.0 * U * np.sqrt(V)
    ref = c - np.log(S)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isneginf(x), ~fin) and not np.isnan(x).any(), f"log_softmax_rows V={V}: -inf entries"
    tol = U * np.abs(c[fin]) + np.broadcast_to(dS + 6.0 * U * np.abs(np.log(S)), c.shape)[fin] + U * np.abs(ref[fin])
    close(x[fin], ref[fin], tol, f"log_softmax_rows V={V}")


def argmax_rows_for(rng, V):
    """the rows of the two argmax cases: random, ties (in neighbouring lanes; 64 apart, i.e. in one lane; in two lanes 65 apart), NaN at
    the front, in the middle, at the end, two NaNs, all NaN, a NaN with only -inf behind it, -inf rows"""
    rows = [uni(rng, V, scale=5.0) for _ in range(3)]

    def tied(*at):
        r = uni(rng, V, scale=5.0)
        r[list(at)] = 7.5
        return r

    def with_nan(*at):
        r = uni(rng, V, scale=5.0)
        r[list(at)] = np.nan
        return r

    if V >= 5:
        rows += [tied(1, 2), tied(0, V - 1), tied(1, 3, 4)]
    if V >= 65:
        rows += [tied(0, 64), tied(V - 65, V - 1), tied(0, 1, 64), tied(0, 63, 64)]
    if V >= 200:
        rows += [tied(5, 69, 133, 197), tied(10, 139), tied(3, 4, 67), tied(2, 67)]
    rows += [with_nan(0), with_nan(V // 2), with_nan(V - 1), with_nan(0, V - 1), np.full(V, np.nan, np.float32)]
    if V >= 5:
        rows += [with_nan(1, V - 2), with_nan(V - 2)]
        r = np.full(V, -np.inf, np.float32)
        r[1] = np.nan
        rows.append(r)
        r = with_nan(2)                      # the maximum in front of the NaN: later-wins ignores it, IndexOf finds it
        r[0] = 9.0
        rows.append(r)
    if V >= 65:
        r = with_nan(63)                     # a tie behind the NaN, in the re-scan
        r[[0, 64]] = 8.0
        rows.append(r)
    rows.append(np.full(V, -np.inf, np.float32))
    r = np.full(V, -np.inf, np.float32)
    r[V // 2] = -3.0
    rows.append(r)
    return np.stack(rows)


def case_argmax(env, name):
    """k_argmax_rows<false / true>: V 1 / 5 / 64 / 65 / 200 with ld = V + 3 (the three floats behind a row are 3e38: a read past V wins
    the row); expected tokens from the literal scans (scan_later_wins / index_of_max)"""
    rng = np.random.default_rng(6200)
    for V in (1, 5, 64, 65, 200):
        rows = argmax_rows_for(rng, V)
        N, ld = len(rows), V + 3
        x = np.full((N, ld), 3e38, np.float32)
        x[:, :V] = rows
        tok = np.full(N, IFILL, np.int32)
        ref = want(name, [ld, N, V], [x, tok])
        launch(env, name, [ld, N, V], [x, tok], {1})
        bad = np.where(tok != ref[1])[0]
        assert not len(bad), (name, V, "rows", bad.tolist(), "got", tok[bad].tolist(), "want", ref[1][bad].tolist(), rows[bad[0]].tolist())


def case_ctc_collapse(env):
    """k_ctc_collapse: Tp 1 / 9; repeats, a repeat split by a blank, all blank (any 0, trail Tp), trailing blanks; frame_off null and
    non-null; max_tokens = 2 against 4 tokens: n_tokens 2, flag 1, nothing written past entry 2 (entries no stream wrote keep their fill)"""
    rows9 = [[5, 5, 5, 0, 0, 7, 7, 0, 0], [5, 5, 0, 5, 5, 0, 0, 0, 0], [0] * 9, [3, 4, 5, 6, 6, 6, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0, 9],
             [1, 2, 2, 1, 0, 1, 1, 0, 2]]
    for Tp, rows in ((9, rows9), (1, [[0], [5]])):
        B = len(rows)
        tok = np.array(rows, np.int32)
        for mt in sorted({Tp, 2}):
            for fo in (None, np.arange(B, dtype=np.int32) * 11 + 3):
                bufs = [tok, fo, np.full(B * mt, IFILL, np.int64), np.full(B * mt, IFILL, np.int32), np.full(B, IFILL, np.int32),
                        np.full(B, IFILL, np.int32), np.full(B, IFILL, np.int32), np.zeros(1, np.int32)]
                ref = want("ctc_collapse", [B, Tp, mt], bufs)
                if Tp == 9 and mt == 2:
                    assert ref[7][0] == 1 and ref[4][3] == 2 and ref[4][5] == 2
                launch(env, "ctc_collapse", [B, Tp, mt], bufs, {2, 3, 4, 5, 6, 7})
                for k, what in ((2, "tokens"), (3, "timestamps"), (4, "n_tokens"), (5, "trail"), (6, "any"), (7, "flag")):
                    ints(bufs[k], ref[k], f"ctc_collapse Tp={Tp} max_tokens={mt} frame_off={fo is not None} {what}")


def case_first_emit(env):
    """k_first_emit: B Tp = 300 and 1250 (more than the 1024 threads); no emission -> INT_MAX; ids 0 and 2 never count, id 1 only with
    skip1 = 0; the minimum over the streams"""
    for B, Tp in ((5, 60), (5, 250)):
        quiet = np.zeros((B, Tp), np.int32)
        quiet[:, ::3] = UNK
        ones = quiet.copy()
        ones[2, Tp - 7] = 1
        late = ones.copy()
        late[4, Tp - 3], late[1, Tp - 2], late[0, Tp - 1] = 9, 4, 5
        first = late.copy()
        first[3, 0] = 6
        for tok, exp0, exp1 in ((quiet, INT_MAX, INT_MAX), (ones, Tp - 7, INT_MAX), (late, Tp - 7, Tp - 3), (first, 0, 0)):
            for skip1, exp in ((0, exp0), (1, exp1)):
                t0 = np.full(1, IFILL, np.int32)
                ref = want("first_emit_frame", [B, Tp, skip1], [tok, t0])
                assert ref[1][0] == exp
                launch(env, "first_emit_frame", [B, Tp, skip1], [tok, t0], {1})
                ints(t0, ref[1], f"first_emit_frame B={B} Tp={Tp} skip1={skip1}")


# every case as (name, callable(env)); the GPU test and the CPU stand-in test both run all of them
CASES = ([("pad_logfloor", case_pad_logfloor), ("gather_samples", case_gather_samples), ("conv0_swoosh", case_conv0_swoosh),
          ("convnext_cat", case_convnext_cat), ("cat_shift plain", lambda env: case_cat_shift(env, 0)),
          ("cat_shift gated", lambda env: case_cat_shift(env, 1)), ("cat_keep", case_cat_keep), ("fifo", case_fifo),
          ("logfloor_inplace and zero_floats", case_floor_and_zero), ("gates", case_gates),
          ("convert_channels and copy_cols", case_channels_and_cols), ("tanh_add", case_tanh_add)]
         + [(f"log_softmax_rows V={V}", (lambda env, V=V: case_log_softmax(env, V))) for V in (1, 63, 64, 65, 500)]
         + [("argmax_rows", lambda env: case_argmax(env, "argmax_rows")),
            ("argmax_first_rows", lambda env: case_argmax(env, "argmax_first_rows")),
            ("ctc_collapse", case_ctc_collapse), ("first_emit_frame", case_first_emit)])


# ---- deliberately wrong stand-ins: (case, op, what is wrong, sim).  tests/test_outer_kernels_ref.py runs each through its case, which
# must fail: the cases have teeth before any kernel is involved ----------------------------------------------------------------------------

def _mut_pad_positive_zero_only(dt, ia, b):
    B, L = ia
    out = b[3].reshape(B, L)
    for s in range(B):
        n, o = int(b[2][s]), int(b[1][s])
        row = np.zeros(L, out.dtype)
        row[:n] = b[0][o:o + n]
        out[s] = np.where((row == 0) & ~np.signbit(row), out.dtype.type(LOG_FLOOR), row)


def _mut_dense_stride_L(dt, ia, b):
    n, B, L = ia
    out = b[1].reshape(B, L)
    for s in range(B):
        row = np.zeros(L, out.dtype)
        m = min(n, L, max(b[0].size - s * L, 0))
        row[:m] = b[0][s * L:s * L + m]
        row[min(n, L):] = 0
        out[s] = _floor(row)


def _mut_gather_float4_across_count(dt, ia, b):
    B, nmax = ia[:2]
    dst = b[2].reshape(B, nmax)
    for s in range(B):
        n, o = int(b[1][s]), ia[2 + s]
        n4 = min(r4(n), nmax) if (o % 4 == 0 and (s * nmax) % 4 == 0) else n     # a whole float4 where the aligned path runs
        dst[s, :n4] = b[0][o:o + n4]
        dst[s, n4:] = 0


def _mut_conv0_swoosh_l(dt, ia, b):
    B, T, F = ia
    z, _ = conv0_parts(b[0], b[1], b[2], B, T, F, 0)
    b[3].reshape(z.shape)[...] = np.logaddexp(z.dtype.type(0.0), z - z.dtype.type(4.0)) - z.dtype.type(0.08) * z - z.dtype.type(0.035)


def _mut_convnext_cache_from_input_end(dt, ia, b):
    ss, off, B, T3, Tc, F, C = ia
    sim_convnext_cat(dt, ia, b)
    for s in range(B):
        _slot(b[1], b[2][s], ss, off, C * 3 * F).reshape(C, 3, F)[...] = b[0].reshape(B, T3, F, C)[s, T3 - 3:].transpose(2, 0, 1)


def _mut_cat_shift_by_one_less(dt, ia, b):
    _cat_then_cache(ia, b, ia[5] - 1, bool(ia[7]))


def _mut_cat_keep_ignores_keep_back(dt, ia, b):
    _cat_then_cache(ia, b, ia[5], False)


def _mut_fifo_gather_no_floor(dt, ia, b):
    cap, feat, B, T = ia
    fifo, x = b[0].reshape(-1, cap, feat), b[3].reshape(B, T, feat)
    for s in range(B):
        for t in range(T):
            x[s, t] = fifo[b[1][s], (b[2][s] + t) % cap]


def _mut_fifo_append_writes_skipped(dt, ia, b):
    pos = b[3].copy()
    pos[pos < 0] = 0
    sim_fifo_append(dt, ia, [b[0], b[1], b[2], pos])


def _mut_logfloor_whole_block(dt, ia, b):
    n = (ia[0] + 255) // 256 * 256
    b[0][:n] = _floor(b[0][:n])


def _mut_zero_whole_quad(dt, ia, b):
    b[0][:r4(ia[0])] = 0


def _mut_glu_gate_from_value(dt, ia, b):
    M, D = ia
    x = b[0].reshape(M, 2 * D)
    b[1].reshape(M, D)[...] = x[:, :D] * _sigmoid(x[:, :D])


def _mut_tanh_gate_swapped(dt, ia, b):
    M, Hc = ia
    x = b[0].reshape(M, 3 * Hc)
    b[1].reshape(M, Hc)[...] = x[:, :Hc] * _tanh(x[:, Hc:2 * Hc])


def _mut_convert_no_zero_fill(dt, ia, b):
    M, Din, Dout = ia
    b[1].reshape(M, Dout)[:, :min(Din, Dout)] = b[0].reshape(M, Din)[:, :min(Din, Dout)]
    b[1].reshape(M, Dout)[:, min(Din, Dout):] = 1e-30


def _mut_copy_cols_ignores_ycol0(dt, ia, b):
    ldx, xc, ldy, yc, M, n = ia
    b[1].reshape(M, ldy)[:, :n] = b[0].reshape(M, ldx)[:, xc:xc + n]


def _mut_tanh_add_row_zero(dt, ia, b):
    ds, N, J = ia
    b[2].reshape(N, J)[...] = _tanh(b[0].reshape(N, J) + b[1][:J])


def _mut_log_softmax_drops_tail(dt, ia, b):
    M, V = ia
    x = b[0].reshape(M, V)
    c = x - x.max(-1, keepdims=True)
    n = V if V % 64 == 0 or V < 64 else V // 64 * 64
    with np.errstate(divide="ignore"):
        x[...] = c - np.log(np.exp(c[:, :n]).sum(-1, keepdims=True))


def _mut_log_softmax_f32_ulp(dt, ia, b):
    """(V = 1 and multiples of 64, where the tail form above is right): the sum one part in 2^17 too large"""
    M, V = ia
    x = b[0].reshape(M, V)
    c = x - x.max(-1, keepdims=True)
    with np.errstate(divide="ignore"):
        x[...] = c - np.log(np.exp(c).sum(-1, keepdims=True) * x.dtype.type(1.0 + 2.0 ** -17))


def _first_wins(row):
    token_num = 0
    for k in range(1, len(row)):
        token_num = token_num if row[token_num] >= row[k] else k       # (the reference's scan with >= for >: only ties change)
    return token_num


def _nan_is_max(row):
    return int(np.argmax(np.array(row)))


def _mut_ctc_no_clamp(dt, ia, b):
    B, Tp, mt = ia
    tok = b[0].reshape(B, Tp)
    sim_ctc_collapse(dt, ia, b)
    for s in range(B):
        prev, n = -1, 0
        for y in tok[s]:
            n += int(y != BLANK and y != prev)
            prev = y
        b[4][s] = n


def _mut_first_emit_counts_one(dt, ia, b):
    sim_first_emit_frame(dt, [ia[0], ia[1], 0], b)


MUTANTS = [
    ("pad_logfloor", "pad_logfloor", "-0.0 is not floored", _mut_pad_positive_zero_only),
    ("pad_logfloor", "pad_logfloor_dense", "streams L apart in the input instead of n_each", _mut_dense_stride_L),
    ("gather_samples", "gather_samples", "a full float4 copied across the count", _mut_gather_float4_across_count),
    ("conv0_swoosh", "conv0_swoosh", "SwooshL", _mut_conv0_swoosh_l),
    ("convnext_cat", "convnext_cat", "cache advanced to the input's last frames, not the chunk's", _mut_convnext_cache_from_input_end),
    ("cat_shift plain", "cat_shift", "cache advanced by Tc - 1", _mut_cat_shift_by_one_less),
    ("cat_shift gated", "cat_shift", "cache advanced by Tc - 1", _mut_cat_shift_by_one_less),
    ("cat_keep", "cat_keep", "keep_back ignored", _mut_cat_keep_ignores_keep_back),
    ("fifo", "fifo_gather", "no floor", _mut_fifo_gather_no_floor),
    ("fifo", "fifo_append", "a skipped stream is written at 0", _mut_fifo_append_writes_skipped),
    ("logfloor_inplace and zero_floats", "logfloor_inplace", "the whole last block is floored", _mut_logfloor_whole_block),
    ("logfloor_inplace and zero_floats", "zero_floats", "the whole last float4 is zeroed", _mut_zero_whole_quad),
    ("gates", "glu_sigmoid", "the gate is the value half", _mut_glu_gate_from_value),
    ("gates", "tanh_gate", "value and gate exchanged", _mut_tanh_gate_swapped),
    ("convert_channels and copy_cols", "convert_channels", "the extension is 1e-30, not 0", _mut_convert_no_zero_fill),
    ("convert_channels and copy_cols", "copy_cols", "ycol0 ignored", _mut_copy_cols_ignores_ycol0),
    ("tanh_add", "tanh_add", "decoder row 0 for every frame whatever the stride", _mut_tanh_add_row_zero),
    ("log_softmax_rows V=1", "log_softmax_rows", "the sum 2^-17 too large", _mut_log_softmax_f32_ulp),
    ("log_softmax_rows V=63", "log_softmax_rows", "the sum 2^-17 too large", _mut_log_softmax_f32_ulp),
    ("log_softmax_rows V=64", "log_softmax_rows", "the sum 2^-17 too large", _mut_log_softmax_f32_ulp),
    ("log_softmax_rows V=65", "log_softmax_rows", "the columns behind the last full 64 left out of the sum", _mut_log_softmax_drops_tail),
    ("log_softmax_rows V=500", "log_softmax_rows", "the columns behind the last full 64 left out of the sum", _mut_log_softmax_drops_tail),
    ("argmax_rows", "argmax_rows", "the first index wins a tie", _argmax(_first_wins)),
    ("argmax_first_rows", "argmax_first_rows", "a NaN is the maximum", _argmax(_nan_is_max)),
    ("argmax_first_rows", "argmax_first_rows", "the later index wins a tie", _argmax(scan_later_wins)),
    ("ctc_collapse", "ctc_collapse", "n_tokens not clamped to max_tokens", _mut_ctc_no_clamp),
    ("first_emit_frame", "first_emit_frame", "id 1 counts whatever skip1 says", _mut_first_emit_counts_one),
]
