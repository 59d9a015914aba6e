"""Cases of tests/test_gemm_forms_gpu.py: every operand form and epilogue term of GemmArgs (csrc/kernels.h) as a launch description,
its float64 reference and its per-element tolerance.  No GPU is touched here: the GPU test file launches each description through
k2hip_debug_op_run's "gemm" op, tests/test_gemm_forms_ref.py runs the same descriptions with a float32 numpy product standing in
for the kernel (which checks the references, the bounds and check()'s 2e-5 ceiling on the CPU) and holds the conv-gather mapping to
torch's conv2d.

reference(): the documented meaning of each field in kernels.h, written with index arrays -- a row / column / k of a batch member
z = z0 + nb0 z1 is an index into the flat operand buffer -- so one function serves every form.  The same index arrays size the
buffers, and Launch.check_extents() asserts that every index the documented form touches lies inside its buffer before anything is
launched.

Tolerances (units of u = 2^-24, helpers of tests/test_kernels_gpu.py): sum_tol(|A| |W|^T + |b|, K + 1) for the accumulated product
(exact fp32 products summed in some order; the skinny and ring kernels split K over waves, which "some order" covers); act_tol()
through SwooshL / SwooshR / DoubleSwish / tanh / sigmoid (slope <= 1.1, hardware exp / log), unchanged through ReLU (slope <= 1,
exact); a residual adds one rounding of the sum; mul scales the bound by |mul| and adds one rounding of the product; the bypass
o + (v - o) s scales it by |s| and adds two roundings (the difference, then the sum) of the magnitudes involved.  Operands are
uniform in [-1, 1); W is scaled by min(1, 2 / K) and the bias by 0.5 so that the bound stays under check()'s ceiling up to
K = 1280 with an activation behind it."""
import numpy as np

from test_kernels_gpu import U, act_tol, f64, sum_tol, uni

ACT_NONE, ACT_SWOOSH_L, ACT_SWOOSH_R, ACT_TANH, ACT_SIGMOID, ACT_RELU, ACT_DOUBLE_SWISH = range(7)

# the int / stride fields of GemmArgs in their declared order (the "gemm" op's argument order, include/k2hip_debug.h)
FIELDS = ["M", "N", "K", "lda", "ldw", "ldc", "ldr", "act", "act_cols", "w_kn", "nb0", "nb1", "sA0", "sA1", "sW0", "sW1", "sC0", "sC1",
          "sR0", "sR1", "sBias0", "cv_Fout", "cv_Tout", "cv_Tin", "cv_Fin", "cv_C", "cv_st", "cv_sf", "seg_len", "seg_stride", "res_div",
          "act_after_res", "glu", "glu_cols", "ldm", "sM0", "sM1", "ld_orig"]
DEFAULTS = dict.fromkeys(FIELDS, 0)
DEFAULTS.update(nb0=1, nb1=1, cv_st=1, cv_sf=1, res_div=1)
OFFSETS = ["oA", "oW", "oR", "oC", "oM", "oO"]
FAMILY = ["reg", "dma", "pipe", "p16", "ring", "skinny3", "skinny6", "skinny6_8"]        # enum GemmFamily
MODE = ["reg.plain", "reg.conv", "reg.wkn"]                                               # enum GemmMode


def plan_name(rep):
    """(family, idx) of the hook's plan report [family, idx, BM, BN, mode], the family spelt as tests/golden/gemm_plans.txt does"""
    fam, idx, _, _, mode = (int(v) for v in rep)
    return (MODE[mode] if fam == 0 else FAMILY[fam], idx)


def act_dt(x, act):
    """csrc/kernels.h enum Act (icefall's definitions) in x's own precision"""
    if act == ACT_NONE:
        return x
    if act == ACT_SWOOSH_L:
        return np.logaddexp(0.0, x - 4.0) - 0.08 * x - 0.035
    if act == ACT_SWOOSH_R:
        return np.logaddexp(0.0, x - 1.0) - 0.08 * x - 0.313261687
    if act == ACT_TANH:
        return np.tanh(x)
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + np.exp(-x))
    if act == ACT_RELU:
        return np.maximum(x, 0.0)
    if act == ACT_DOUBLE_SWISH:
        return x / (1.0 + np.exp(1.0 - x))
    raise ValueError(act)


class Launch:
    """One gemm() call: GemmArgs' int fields (`f`), the cfg force code, flat float32 operand buffers with the float offset of each
    pointer inside its buffer, res_is_C (the residual is C's own buffer: in place), the skip flag (None: no skip_if_zero pointer)"""

    def __init__(self, what, cfg=-1, res_is_C=False, skip=None, **f):
        bad = set(f) - set(FIELDS) - set(OFFSETS)
        assert not bad, bad
        self.what, self.cfg, self.res_is_C, self.skip = what, cfg, res_is_C, skip
        self.o = {k: int(f.pop(k, 0)) for k in OFFSETS}
        self.f = dict(DEFAULTS, **f)
        assert self.f["glu"] == 0, "the gated epilogue is tests/test_gemm_gpu.py's"
        self.A = self.W = self.bias = self.res = self.C = self.mul = self.orig = self.scale = None

    # ---- the documented addressing (kernels.h GemmArgs), as flat indexes per batch member ---------------------------------------
    def batches(self):
        return [(z0, z1) for z1 in range(self.f["nb1"]) for z0 in range(self.f["nb0"])]

    def a_index(self, z0, z1):
        f = self.f
        r, k = np.arange(f["M"], dtype=np.int64)[:, None], np.arange(f["K"], dtype=np.int64)[None, :]
        base = self.o["oA"] + z0 * f["sA0"] + z1 * f["sA1"]
        if f["cv_Fout"]:
            #   row r = (b*Tout + t)*Fout + f  ->  base = ((b*Tin + t*st)*Fin + f*sf)*C;  k -> (k / seg_len) * seg_stride + k % seg_len
            fo, bt = r % f["cv_Fout"], r // f["cv_Fout"]
            t, b = bt % f["cv_Tout"], bt // f["cv_Tout"]
            rbase = ((b * f["cv_Tin"] + t * f["cv_st"]) * f["cv_Fin"] + fo * f["cv_sf"]) * f["cv_C"]
            return base + rbase + (k // f["seg_len"]) * f["seg_stride"] + k % f["seg_len"]
        return base + r * f["lda"] + k

    def w_index(self, z0, z1):
        f = self.f
        n, k = np.arange(f["N"], dtype=np.int64)[:, None], np.arange(f["K"], dtype=np.int64)[None, :]
        base = self.o["oW"] + z0 * f["sW0"] + z1 * f["sW1"]
        return base + (k * f["ldw"] + n if f["w_kn"] else n * f["ldw"] + k)

    def _rc(self, off, s0, s1, ld, z0, z1, div=1):
        f = self.f
        r, n = np.arange(f["M"], dtype=np.int64)[:, None], np.arange(f["N"], dtype=np.int64)[None, :]
        return off + z0 * s0 + z1 * s1 + (r // div) * ld + n

    def c_index(self, z0, z1):
        return self._rc(self.o["oC"], self.f["sC0"], self.f["sC1"], self.f["ldc"], z0, z1)

    def r_index(self, z0, z1):
        return self._rc(self.o["oR"], self.f["sR0"], self.f["sR1"], self.f["ldr"], z0, z1, self.f["res_div"])

    def m_index(self, z0, z1):
        return self._rc(self.o["oM"], self.f["sM0"], self.f["sM1"], self.f["ldm"], z0, z1)

    def o_index(self):
        return self._rc(self.o["oO"], 0, 0, self.f["ld_orig"], 0, 0)

    def _extent(self, index, row):
        """floats a buffer needs: the largest documented index, its row filled up to the leading dimension, and 8 floats more"""
        return int(max(index(*z).max() for z in self.batches())) + 1 + row + 8

    def fill(self, rng, bias=True, res=False, mul=False, byp=False, wscale=None):
        """operands from the seeded generator, buffers sized by the documented addressing (whole rows); C holds NaN, or the residual
        when the launch is in place"""
        f = self.f
        K = f["K"]
        self.A = uni(rng, self._extent(self.a_index, 0 if f["cv_Fout"] else f["lda"] - K))
        if f["w_kn"]:     # the contract: A rows zero-padded to a multiple of 4 (beyond that the row may hold anything)
            Kp = (K + 3) // 4 * 4
            for z in self.batches():
                idx = self.a_index(*z)[:, :1] + np.arange(K, Kp)[None, :]
                self.A[idx] = 0.0
        self.W = uni(rng, self._extent(self.w_index, f["ldw"]), scale=wscale or min(1.0, 2.0 / K))
        if bias:
            self.bias = uni(rng, (f["nb0"] - 1) * f["sBias0"] + f["N"], scale=0.5)
        csize = self._extent(self.c_index, max(0, f["ldc"] - f["N"]))
        if self.res_is_C:
            self.C = uni(rng, csize)
        else:
            self.C = np.full(csize, np.nan, np.float32)
            if res:
                self.res = uni(rng, self._extent(self.r_index, max(0, f["ldr"] - f["N"])))
        if mul:
            self.mul = uni(rng, self._extent(self.m_index, max(0, f["ldm"] - f["N"])))
        if byp:
            self.orig = uni(rng, self._extent(lambda *_: self.o_index(), max(0, f["ld_orig"] - f["N"])))
            self.scale = uni(rng, f["N"])
        self.C0 = self.C.copy()
        self.check_extents()
        return self

    def check_extents(self):
        f = self.f
        assert f["lda"] % 4 == 0 and f["ldw"] % 4 == 0 and self.o["oA"] % 4 == 0 and self.o["oW"] % 4 == 0, self.what
        for s in ("sA0", "sA1", "sW0", "sW1"):
            assert f[s] % 4 == 0, (self.what, s, "float4 loads")
        Kp = (f["K"] + 3) // 4 * 4
        seen = np.zeros(self.C.size, bool)
        for z in self.batches():
            a = self.a_index(*z)
            assert a.min() >= 0 and a.max() + (Kp - f["K"]) < self.A.size, (self.what, "A")
            w = self.w_index(*z)
            assert w.min() >= 0 and w.max() < self.W.size, (self.what, "W")
            c = self.c_index(*z)
            assert c.min() >= 0 and c.max() < self.C.size, (self.what, "C")
            assert not seen[c].any(), (self.what, "two batch members write one element of C")
            seen[c] = True
            if self.res is not None or self.res_is_C:
                r = self.r_index(*z)
                assert r.min() >= 0 and r.max() < (self.C if self.res_is_C else self.res).size, (self.what, "res")
                # in place: a thread reads the element it writes and no other
                assert not self.res_is_C or np.array_equal(r, c), (self.what, "in place needs res == C element by element")
            if self.mul is not None:
                m = self.m_index(*z)
                assert m.min() >= 0 and m.max() < self.mul.size, (self.what, "mul")
        if self.bias is not None:
            assert (f["nb0"] - 1) * f["sBias0"] + f["N"] <= self.bias.size, (self.what, "bias")
        if self.orig is not None:
            o = self.o_index()
            assert o.min() >= 0 and o.max() < self.orig.size and self.scale.size >= f["N"], (self.what, "byp_orig")

    # ---- the hook's arguments ---------------------------------------------------------------------------------------------------
    def iargs(self):
        return [self.f[k] for k in FIELDS] + [self.cfg, int(self.res_is_C)] + [self.o[k] for k in OFFSETS]

    def plan_line(self):
        """this launch as an input line of tests/golden/gemm_plans.txt (the sanitizer driver's `plans` command)"""
        f = self.f
        return (f"gemm {f['M']} {f['N']} {f['K']} {f['nb0'] * f['nb1']} {f['cv_Fout']} {f['w_kn']} {int(self.mul is not None)} "
                f"{f['res_div']} {f['act_after_res']} {f['glu']} {f['lda']} {f['ldw']} {self.cfg}")

    # ---- reference --------------------------------------------------------------------------------------------------------------
    def reference(self, dt=np.float64):
        """C's whole buffer after the launch, computed in precision dt (float64: the reference; float32: the stand-in for a kernel),
        the per-element tolerance (float64 pass) and the mask of the elements the launch writes"""
        f = self.f
        A, W = self.A.astype(dt), self.W.astype(dt)
        out = self.C0.astype(dt)
        tol = np.zeros(out.size)
        written = np.zeros(out.size, bool)
        if self.skip == 0:
            return out, tol, written
        R = self.C0 if self.res_is_C else self.res
        cols = np.arange(f["N"])
        act_on = (cols < f["act_cols"]) if f["act_cols"] > 0 else np.ones(f["N"], bool)
        for z0, z1 in self.batches():
            a, w = A[self.a_index(z0, z1)], W[self.w_index(z0, z1)]
            v = a @ w.T
            mag = np.abs(f64(a)) @ np.abs(f64(w)).T
            if self.bias is not None:
                b = self.bias[z0 * f["sBias0"] + cols].astype(dt)
                v = v + b
                mag = mag + np.abs(f64(b))
            t = sum_tol(mag, f["K"] + 1)
            rv = R[self.r_index(z0, z1)].astype(dt) if R is not None else None
            if rv is not None and f["act_after_res"]:
                v = v + rv
                t = t + U * np.abs(f64(v))
            if f["act"] != ACT_NONE:
                ta = t if f["act"] == ACT_RELU else act_tol(f64(v), t)
                t = np.where(act_on, ta, t)
                v = np.where(act_on, act_dt(v, f["act"]), v)
            if rv is not None and not f["act_after_res"]:
                v = v + rv
                t = t + U * np.abs(f64(v))
            if self.mul is not None:
                m = self.mul[self.m_index(z0, z1)].astype(dt)
                v = v * m
                t = t * np.abs(f64(m)) + U * np.abs(f64(v))
            if self.orig is not None:
                o, s = self.orig[self.o_index()].astype(dt), self.scale[cols].astype(dt)
                d = v - o
                v = o + d * s
                t = t * np.abs(f64(s)) + 2 * U * (np.abs(f64(o)) + np.abs(f64(d * s))) + U * np.abs(f64(d)) * np.abs(f64(s))
            c = self.c_index(z0, z1)
            out[c], tol[c], written[c] = v, t, True
        return out, tol, written


def judge(launch, got, check):
    """every element the launch writes against the float64 reference within its tolerance (check() of tests/test_kernels_gpu.py, its
    2e-5 ceiling included); every other float of C's buffer bit-unchanged"""
    want, tol, written = launch.reference()
    got = np.asarray(got)
    assert got.shape == launch.C0.shape, launch.what
    same = got.view(np.uint32) == launch.C0.view(np.uint32)
    assert same[~written].all(), (launch.what, "C changed outside the launch's elements at", np.argwhere(~same & ~written)[:4].tolist())
    if written.any():
        check(got[written], want[written], tol[written], launch.what)


def standin(launch):
    """what a kernel that computes in float32 would leave in C's buffer"""
    out, _, _ = launch.reference(np.float32)
    return out.astype(np.float32)


# ---- shapes and builders ---------------------------------------------------------------------------------------------------------

def plain(rng, what, M, N, K, cfg=-1, act=ACT_NONE, bias=True, res=False, inplace=False, pad=(8, 4, 12, 20), off=(4, 8, 5, 3), byp=False,
          skip=None, **extra):
    """the Linear form with leading dimensions larger than the logical width (pad: lda - K, ldw - K, ldc - N, ldr - N) and pointers
    inside their buffers (off: A, W, C, res).  In place: res is C itself."""
    f = dict(M=M, N=N, K=K, lda=K + pad[0], ldw=K + pad[1], ldc=N + pad[2], act=act, oA=off[0], oW=off[1], oC=off[2])
    if inplace:
        f.update(ldr=f["ldc"], oR=f["oC"])
    elif res:
        f.update(ldr=N + pad[3], oR=off[3])
    if byp:
        f.update(ld_orig=N + 16, oO=7)
    f.update(extra)
    return Launch(what, cfg=cfg, res_is_C=inplace, skip=skip, **f).fill(rng, bias=bias, res=res, byp=byp)


PIPE = [2001, 2005, 2008, 2013, 2002, 2004, 2009, 2012]          # tests/test_gemm_gpu.py's forced codes
OTHER = [66, 5, 9, 100, 108, 118]
P16 = [3000, 3001, 3002, 3003]
FORCED = OTHER + PIPE + P16
FORCED_PLANS = {("reg.plain", 2), ("dma", 5), ("dma", 9), ("ring", 0), ("ring", 8), ("ring", 18), ("pipe", 1), ("pipe", 5), ("pipe", 8),
                ("pipe", 13), ("pipe", 2), ("pipe", 4), ("pipe", 9), ("pipe", 12), ("p16", 0), ("p16", 1), ("p16", 2), ("p16", 3)}
# one plan of each family: forced codes on a tiled shape, automatic dispatch on the three skinny shapes
ONE_OF_EACH = [(66, (130, 100, 128)), (5, (130, 100, 128)), (2001, (130, 100, 128)), (3000, (130, 100, 128)), (100, (130, 100, 128)),
               (-1, (33, 36, 128)), (-1, (33, 50, 192)), (-1, (600, 50, 640))]
ONE_OF_EACH_PLANS = {("reg.plain", 2), ("dma", 5), ("pipe", 1), ("p16", 0), ("ring", 0), ("skinny3", 0), ("skinny6", 0), ("skinny6_8", 0)}


def case_skinny(rng):
    """1. the skinny families by automatic dispatch: a wave's K slice of 16 / 32 / 48 / 80 floats (K / 4), M around the 16-row
    workgroup, N around the 16-column tiles and the 48 / 96-column chunk; eight waves (K / 8 = 64, 80, 128); and the beam search's
    joiner launch: N > 96 ragged against 96 and 16, a shared residual row, tanh after the residual"""
    acts = [ACT_NONE, ACT_SWOOSH_L, ACT_TANH, ACT_SWOOSH_R, ACT_SIGMOID]
    i = 0
    for K in (64, 128, 192, 320):
        for M in (1, 15, 16, 17, 300):
            for N in (4, 36, 48, 50, 96):
                i += 1
                yield plain(rng, f"skinny M={M} N={N} K={K}", M, N, K, act=acts[i % 5], res=i % 2 == 0, bias=i % 3 != 0)
    for K in (512, 640, 1024):
        for M, N in ((513, 50), (600, 96)):
            i += 1
            yield plain(rng, f"skinny8 M={M} N={N} K={K}", M, N, K, act=acts[i % 5], res=i % 2 == 0)
    for beam, B in ((4, 3), (8, 5)):
        for N, K in ((500, 512), (512, 512), (500, 320), (100, 192)):
            Tp, t = 3, 1          # beam.hip: res = enc + t J, ldr = Tp J, one encoder row per stream
            yield plain(rng, f"joiner beam={beam} B={B} N={N} K={K}", B * beam, N, K, act=ACT_TANH, res=True, res_div=beam, act_after_res=1,
                        ldr=Tp * N, oR=t * N)


case_skinny.floor = 100 + 6 + 8
case_skinny.plans = {("skinny3", 0), ("skinny6", 0), ("skinny6_8", 0)}


def case_res_div(rng):
    """2. res_div and act_after_res separately and together: on the skinny path, on the register-staged path (K % 64 != 0 is not
    `plain`; M > 4096 is too many rows for the skinny kernel)"""
    for M, N, K in ((40, 96, 128), (37, 200, 192), (300, 160, 100), (70, 50, 36), (4100, 128, 64)):
        for div, after in ((4, 0), (1, 1), (5, 1), (3, 0)):
            yield plain(rng, f"res_div={div} act_after_res={after} M={M} N={N} K={K}", M, N, K, act=ACT_TANH if after else ACT_SWOOSH_R,
                        res=True, res_div=div, act_after_res=after, ldr=N + 8, oR=16)


case_res_div.floor = 20
case_res_div.plans = {("skinny6", 0), ("reg.plain", 3), ("reg.plain", 2)}


TS = [1, 2, 3, 5, 31, 32, 33, 65, 250]


def case_wkn(rng):
    """3. the [K,N] operand, batched nb0 x nb1, K = T rows of W with A's rows zero-padded to Tp: the attention apply of Zipformer2
    (z0 = stream, z1 = head: column block z1 of hid and of the output), NonlinAttention's (one head, the output gate `mul` read from
    a wider row: ldm != ldc, sM0) and the Conformer's (z0 = head: column block, z1 = stream: sW1 = T * 3 D)"""
    NS = [4, 12, 24, 32, 96, 288]
    i = 0
    for T in TS:
        Tp = (T + 3) // 4 * 4
        for form in ("zipformer2", "nonlin", "conformer"):
            N = NS[i % 6]
            i += 1
            what = f"wkn {form} T={T} N={N}"
            if form == "zipformer2":
                B, H, vh = 3, 4, N
                HV = H * vh
                g = Launch(what, M=T, N=vh, K=T, w_kn=1, nb0=B, nb1=H, lda=Tp, sA0=T * Tp, sA1=B * T * Tp, ldw=HV, sW0=T * HV, sW1=vh,
                           ldc=HV, sC0=T * HV, sC1=vh, oA=8, oW=4, oC=0)
                yield g.fill(rng, bias=False, wscale=min(1.0, 2.0 / T))
            elif form == "nonlin":
                B, Hc = 3, N
                g = Launch(what, M=T, N=Hc, K=T, w_kn=1, nb0=B, nb1=1, lda=Tp, sA0=T * Tp, ldw=2 * Hc, sW0=T * 2 * Hc, ldc=Hc, sC0=T * Hc,
                           ldm=2 * Hc, sM0=T * 2 * Hc, oM=Hc, oW=0, oA=4)
                yield g.fill(rng, bias=False, mul=True)
            else:
                B, H, dk = 2, 4, N
                D = H * dk
                g = Launch(what, M=T, N=dk, K=T, w_kn=1, nb0=H, nb1=B, lda=Tp, sA0=T * Tp, sA1=H * T * Tp, ldw=3 * D, sW0=dk, sW1=T * 3 * D,
                           oW=2 * D, ldc=D, sC0=dk, sC1=T * D)
                yield g.fill(rng, bias=False)


case_wkn.floor = 27
case_wkn.plans = {("reg.wkn", 2), ("reg.wkn", 3)}


def conv_launch(rng, what, B, Tin, Fin, C, st, sf, N, act=ACT_SWOOSH_R):
    """a 3 x 3 convolution over NHWC [B, Tin, Fin, C] without padding as an implicit GEMM: K = 9 C, a k segment = one time tap's
    3 C contiguous floats (3 frequency taps x C channels), segments Fin C apart"""
    Tout, Fout = (Tin - 3) // st + 1, (Fin - 3) // sf + 1
    g = Launch(what, M=B * Tout * Fout, N=N, K=9 * C, ldw=9 * C, ldc=N, act=act, cv_Fout=Fout, cv_Tout=Tout, cv_Tin=Tin, cv_Fin=Fin, cv_C=C,
               cv_st=st, cv_sf=sf, seg_len=3 * C, seg_stride=Fin * C)
    g.fill(rng)
    full = B * Tin * Fin * C          # the whole tensor, also where the strides leave its last rows or columns unread
    assert g.a_index(0, 0).max() < full
    if g.A.size < full:
        g.A = np.concatenate([g.A, uni(rng, full - g.A.size)])
    return g


def case_conv(rng):
    """4. the conv gather in the two layouts of encoder_embed (conv.4: 8 channels, stride 2 x 2, 24-float segments; conv.7: 32
    channels, frequency stride 2, time stride 1 and 2, 96-float segments), B > 1, M ragged against the tile"""
    yield conv_launch(rng, "conv C=8 M>=4096", 2, 97, 87, 8, 2, 2, 32)           # M = 2 * 48 * 43 = 4128: 128x32 tiles (REG 12)
    yield conv_launch(rng, "conv C=8", 3, 21, 27, 8, 2, 2, 32)                   # M = 3 * 10 * 13 = 390: REG 2
    yield conv_launch(rng, "conv C=8 one row over", 1, 11, 55, 8, 2, 2, 32)      # M = 5 * 27 = 135 = 2 * 64 + 7
    yield conv_launch(rng, "conv C=32 st=1", 2, 9, 19, 32, 1, 2, 128)            # M = 2 * 7 * 9 = 126
    yield conv_launch(rng, "conv C=32 st=2", 3, 13, 23, 32, 2, 2, 128)           # M = 3 * 6 * 11 = 198
    yield conv_launch(rng, "conv C=32 st=1 wide", 2, 70, 93, 32, 1, 2, 160)      # M = 2 * 68 * 46 = 6256: 128x64 tiles (REG 5)
    yield conv_launch(rng, "conv C=32 st=2 wide", 3, 93, 93, 32, 2, 2, 160)      # M = 3 * 46 * 46 = 6348


case_conv.floor = 7
case_conv.plans = {("reg.conv", 12), ("reg.conv", 2), ("reg.conv", 5), ("reg.conv", 3)}

TILED = [(333, 260, 128), (129, 192, 192)]      # K: a multiple of 64 (ring entry 8 splits it in two), four pipe stages


def case_bypass(rng):
    """5. the bypass epilogue o + (v - o) byp_scale[col] with the residual in place (C == res: feed_forward2.out_proj), on every
    forced family and the automatic choice"""
    for M, N, K in TILED:
        for cfg in [-1] + FORCED:
            yield plain(rng, f"bypass cfg={cfg} M={M} N={N} K={K}", M, N, K, cfg=cfg, inplace=True, byp=True, pad=(8, 4, 0, 0))
    yield plain(rng, "bypass skinny", 40, 96, 128, inplace=True, byp=True)
    yield plain(rng, "bypass reg ragged K", 130, 100, 36, inplace=True, byp=True)


case_bypass.floor = 2 * 19 + 2
case_bypass.plans = FORCED_PLANS | {("skinny6", 0), ("reg.plain", 3)}


def case_act_cols(rng):
    """6. act_cols with SwooshL: the boundary at a column that is no multiple of 16 and at one that is (the engines' F * 3 / 4),
    ldc = N, then with the in-place residual"""
    for M, N, K in TILED:
        for cfg in [-1] + FORCED:
            for cols, inplace in ((N * 3 // 4 // 16 * 16 + 5, False), (N * 3 // 4 // 16 * 16, True)):
                yield plain(rng, f"act_cols={cols} cfg={cfg} M={M} N={N} K={K} inplace={inplace}", M, N, K, cfg=cfg, act=ACT_SWOOSH_L,
                            act_cols=cols, inplace=inplace, pad=(8, 4, 0, 0))
    for N, cols in ((96, 37), (40, 32), (200, 144)):
        yield plain(rng, f"act_cols={cols} skinny N={N}", 40, N, 192, act=ACT_SWOOSH_L, act_cols=cols, pad=(8, 4, 0, 0),
                    res_div=2 if N == 200 else 1, res=N == 200)


case_act_cols.floor = 2 * 19 * 2 + 3
case_act_cols.plans = FORCED_PLANS | {("skinny3", 0), ("skinny6", 0)}


def case_batched(rng):
    """7. the batched plain form: a handful of rows against many layers' weights with a bias per layer (the LSTM wavefront: LDS-DMA
    tiles 20 and 21), its in-place second product, split-K partials written sC1 apart; the Conformer's per-(head, stream) score
    products on the LDS-DMA kernel and, with K % 32 != 0, on the register-staged one"""
    for B, nl, N, K in ((5, 7, 160, 64), (33, 3, 100, 96), (64, 150, 256, 64), (1, 80, 512, 64)):
        for inplace in (False, True):
            g = Launch(f"layers B={B} n={nl} N={N} K={K} inplace={inplace}", res_is_C=inplace, M=B, N=N, K=K, nb0=nl, lda=K + 4,
                       sA0=B * (K + 4) + 8, ldw=K, sW0=N * K, sBias0=N + 4, ldc=N, sC0=B * N, ldr=N if inplace else 0,
                       sR0=B * N if inplace else 0, oC=6, oR=6 if inplace else 0)
            yield g.fill(rng)
    for B, nl, N, Kfull, S in ((5, 6, 96, 256, 4), (16, 3, 200, 512, 2)):
        PST = nl * B * N + 12
        g = Launch(f"split-K B={B} n={nl} N={N} K={Kfull}/{S}", M=B, N=N, K=Kfull // S, nb0=nl, nb1=S, lda=Kfull, sA0=B * Kfull, sA1=Kfull // S,
                   ldw=Kfull, sW0=N * Kfull, sW1=Kfull // S, ldc=N, sC0=B * N, sC1=PST)
        yield g.fill(rng, bias=False)
    for T, H, B, dk in ((200, 4, 5, 64), (200, 4, 5, 48), (33, 4, 2, 64), (65, 2, 3, 40)):
        D, Tp = H * dk, (T + 3) // 4 * 4
        g = Launch(f"conformer scores T={T} H={H} B={B} dk={dk}", M=T, N=T, K=dk, nb0=H, nb1=B, lda=D, sA0=dk, sA1=T * D, ldw=3 * D, sW0=dk,
                   sW1=T * 3 * D, oW=D, ldc=Tp, sC0=T * Tp, sC1=H * T * Tp)
        yield g.fill(rng, bias=False)


case_batched.floor = 14
case_batched.plans = {("dma", 20), ("dma", 21), ("dma", 5), ("reg.plain", 5)}


def case_skip(rng):
    """8. skip_if_zero: flag 0 leaves C as it was, flag 1 computes, on one plan of each family (each kernel has its own early return)"""
    for cfg, (M, N, K) in ONE_OF_EACH:
        for flag in (0, 1):
            yield plain(rng, f"skip_if_zero={flag} cfg={cfg} M={M} N={N} K={K}", M, N, K, cfg=cfg, act=ACT_SWOOSH_R, skip=flag)


case_skip.floor = 16
case_skip.plans = ONE_OF_EACH_PLANS


def case_relu_dswish(rng):
    """9. ACT_RELU and ACT_DOUBLE_SWISH on one plan of each family"""
    for cfg, (M, N, K) in ONE_OF_EACH:
        for act, res in ((ACT_RELU, False), (ACT_DOUBLE_SWISH, True)):
            yield plain(rng, f"act={act} cfg={cfg} M={M} N={N} K={K}", M, N, K, cfg=cfg, act=act, res=res)


case_relu_dswish.floor = 16
case_relu_dswish.plans = ONE_OF_EACH_PLANS

CASES = [case_skinny, case_res_div, case_wkn, case_conv, case_bypass, case_act_cols, case_batched, case_skip, case_relu_dswish]


def run_case(case, seed, runner, check):
    """every launch of a case through runner(launch) -> (C's buffer after the launch, plan name); the launches made against the case's
    floor and the plans reached against the ones it was written for.  Returns (launches, plans) for the report."""
    rng = np.random.default_rng(seed)
    n, plans = 0, {}
    for launch in case(rng):
        got, plan = runner(launch)
        judge(launch, got, check)
        plans[plan] = plans.get(plan, 0) + 1
        n += 1
    assert n >= case.floor, (case.__name__, n, case.floor)
    assert case.plans <= set(plans), (case.__name__, "plans not reached:", sorted(case.plans - set(plans)), "reached:", sorted(plans))
    print(f"{case.__name__}: {n} launches, plans {dict(sorted(plans.items()))}")
    return n, plans


# ---- 10. gemm_glu_causal_conv -----------------------------------------------------------------------------------------------------

def glu_interleave(D):
    """GEMM column of (value c, gate c) under the "#glu" row order: blocks of 32 = 16 values | their 16 gates"""
    c = np.arange(D)
    val = (c // 16) * 32 + c % 16
    return val, val + 16


# (B, Tc, D, K): ring entries 16 (32x32 tiles), 17 (64x32), 12 (32x64), 8 (64x64); conv kernels 7 / 15 / 31; every Tc; B Tc ragged
# against the tile's 32 / 64 rows
CONV_SHAPES = [(3, 8, 128, 31, 16), (5, 4, 128, 15, 16), (7, 2, 128, 7, 16), (1, 32, 128, 31, 16), (3, 16, 128, 7, 16),
               (97, 8, 256, 31, 17), (25, 32, 256, 15, 17), (3, 8, 192, 31, 12), (9, 4, 64, 15, 12), (5, 16, 192, 7, 12), (11, 2, 64, 7, 12),
               (173, 8, 192, 31, 8), (131, 8, 256, 15, 8)]
# shapes without a fused form: Tc no divisor of 32, D no multiple of 64, a kernel size without a tail, one over the staging limit
# (entry 16 holds 8 * 256 cached values: 16 streams x 16 channels x 15 frames = 3840)
CONV_REFUSED = [(3, 3, 128, 31), (3, 8, 96, 31), (3, 8, 128, 9), (3, 2, 128, 31)]
