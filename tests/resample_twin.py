"""Float64 twin of the sample-rate converter: an independent restatement of its definition (include/k2hip.h "Input at other sample
rates") with `math` and Python integers -- Kaldi's LinearResample, a Hann-windowed sinc with 6 zero crossings and cutoff
0.99 * 0.5 * min(fi, fo), no flush.  Nothing here is shared with csrc/resample_plan.cpp.

Time is counted in ticks of 1 / lcm(fi, fo) seconds: input sample j sits at tick j * ou, output sample k at tick k * iu.  A tap is an
input sample strictly inside the window, |j * ou - k * iu| * 99 * min(fi, fo) < 600 * lcm, an inequality of integers; an output exists
once its last tap has been accepted.  Only the weights are floating point."""
import ctypes as C
import math

import numpy as np

NUM_ZEROS = 6
RATES_TO_16K = (8000, 11025, 22050, 32000, 44100, 48000)
PAIRS = [(fi, 16000) for fi in RATES_TO_16K] + [(16000, 8000)]
# the issue's orientation table for fo = 16000: fi -> (iu, ou, set of taps per phase, min first, max first)
TABLE = {8000: (1, 2, {12, 13}, -6, -5), 11025: (441, 640, {12, 13}, -6, 435), 22050: (441, 320, {16, 17}, -8, 432),
         32000: (2, 1, {25}, -12, -12), 44100: (441, 160, {33, 34}, -16, 422), 48000: (3, 1, {37}, -18, -18)}


class Twin:
    def __init__(self, fi, fo):
        g = math.gcd(fi, fo)
        self.fi, self.fo, self.iu, self.ou = fi, fo, fi // g, fo // g
        self.lcm = fi * self.ou
        self.lo = min(fi, fo)
        self.fc = 0.99 * 0.5 * self.lo
        self.first, self.ntaps, self.w = [], [], []
        for p in range(self.ou):
            js = self.taps(p)
            self.first.append(js[0])
            self.ntaps.append(len(js))
            self.w.append([self.weight(j * self.ou - p * self.iu) for j in js])
        self.max_taps = max(self.ntaps)

    def inside(self, ticks):
        return abs(ticks) * 99 * self.lo < 600 * self.lcm

    def taps(self, k):
        """input indices of output k's taps (absolute; negative = in front of the stream), ascending"""
        c = k * self.iu // self.ou   # an input sample near the output's instant
        j = c
        while self.inside((j - 1) * self.ou - k * self.iu):
            j -= 1
        while not self.inside(j * self.ou - k * self.iu):
            j += 1
        out = []
        while self.inside(j * self.ou - k * self.iu):
            out.append(j)
            j += 1
        return out

    def weight(self, ticks):
        d = ticks / self.lcm   # seconds, input minus output
        ww = NUM_ZEROS / (2.0 * self.fc)
        hann = 0.5 * (1.0 + math.cos(2.0 * math.pi * self.fc / NUM_ZEROS * d)) if abs(d) < ww else 0.0
        filt = math.sin(2.0 * math.pi * self.fc * d) / (math.pi * d) if d != 0.0 else 2.0 * self.fc
        return filt * hann / self.fi

    def num_out(self, n):
        """outputs whose last tap lies below n: counted one by one from the definition"""
        k = 0
        while self.taps(k)[-1] < n:
            k += 1
        return k

    def num_out_table(self, n_max):
        """num_out(n) for n = 0 .. n_max in one walk"""
        out, k, last = [], 0, self.taps(0)[-1]
        for n in range(n_max + 1):
            while last < n:
                k += 1
                last = self.taps(k)[-1]
            out.append(k)
        return out

    def apply(self, x, w32=None):
        """y (float64) over the whole signal and, per output, sum_j |w_j x_j|; w32: the library's float32 table [ou][max_taps] in
        place of the twin's own weights (the dot product alone is then what differs from the float32 reference)"""
        x = np.asarray(x, np.float64)
        n = len(x)
        y, mag, nt = [], [], []
        k = 0
        while True:
            p, u = k % self.ou, k // self.ou
            s = self.first[p] + u * self.iu
            if s + self.ntaps[p] - 1 >= n:
                break
            w = self.w[p] if w32 is None else [float(v) for v in w32[p][: self.ntaps[p]]]
            terms = [w[j] * (x[s + j] if s + j >= 0 else 0.0) for j in range(self.ntaps[p])]
            y.append(math.fsum(terms))
            mag.append(math.fsum(abs(t) for t in terms))
            nt.append(self.ntaps[p])
            k += 1
        return np.array(y), np.array(mag), np.array(nt)


def bound(mag, nt):
    """the float32 dot product's error bound from its operands: (ntaps + 2) * 2^-24 * sum |w_j x_j|"""
    return (nt + 2) * 2.0 ** -24 * mag


# ---- the library's side, no GPU (include/k2hip_debug.h) ------------------------------------------------------------------------
_ip, _fp, _lp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int64)


def _lib():
    from k2transducerasr_amd import load_library
    L = load_library()
    L.k2hip_debug_resample_plan.argtypes = [C.c_int32, C.c_int32, _ip, _ip, _ip, _ip, _ip, _fp, C.c_int32, C.c_int64]
    L.k2hip_debug_resample_num_out.restype = C.c_int64
    L.k2hip_debug_resample_num_out.argtypes = [C.c_int32, C.c_int32, C.c_int64]
    L.k2hip_debug_resample_ref.argtypes = [C.c_int32, C.c_int32, _fp, _lp, C.c_int64, _lp, _lp, _fp, C.c_int64, _fp, C.c_int64, _lp]
    return L


def lib_plan_rc(fi, fo):
    """(return code, message) of asking for the plan's sizes"""
    L = _lib()
    a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
    rc = L.k2hip_debug_resample_plan(fi, fo, C.byref(a), C.byref(b), C.byref(c), None, None, None, 0, 0)
    return rc, L.k2hip_last_error().decode()


def lib_plan(fi, fo):
    L = _lib()
    iu, ou, mt = C.c_int32(), C.c_int32(), C.c_int32()
    rc = L.k2hip_debug_resample_plan(fi, fo, C.byref(iu), C.byref(ou), C.byref(mt), None, None, None, 0, 0)
    assert rc == 0, L.k2hip_last_error()
    first, ntaps = np.zeros(ou.value, np.int32), np.zeros(ou.value, np.int32)
    w = np.full((ou.value, mt.value), np.nan, np.float32)
    rc = L.k2hip_debug_resample_plan(fi, fo, C.byref(iu), C.byref(ou), C.byref(mt), first.ctypes.data_as(_ip), ntaps.ctypes.data_as(_ip),
                                     w.ctypes.data_as(_fp), ou.value, w.size)
    assert rc == 0, L.k2hip_last_error()
    return {"iu": iu.value, "ou": ou.value, "max_taps": mt.value, "first": first, "ntaps": ntaps, "w": w}


def lib_num_out(fi, fo, n):
    return int(_lib().k2hip_debug_resample_num_out(fi, fo, n))


class RefStream:
    """csrc/resample_ref.h with its carried block held here, as a host of the library would hold it"""

    def __init__(self, fi, fo):
        self.fi, self.fo = fi, fo
        self.tail = np.zeros(8192, np.float32)
        self.n_tail, self.n_in, self.n_out = C.c_int64(0), C.c_int64(0), C.c_int64(0)

    def push(self, x):
        L = _lib()
        x = np.ascontiguousarray(x, np.float32)
        cap = len(x) * self.fo // self.fi + 64
        out = np.full(cap, np.nan, np.float32)
        got = C.c_int64(0)
        rc = L.k2hip_debug_resample_ref(self.fi, self.fo, self.tail.ctypes.data_as(_fp), C.byref(self.n_tail), self.tail.size, C.byref(self.n_in),
                                        C.byref(self.n_out), x.ctypes.data_as(_fp), len(x), out.ctypes.data_as(_fp), cap, C.byref(got))
        assert rc == 0, L.k2hip_last_error()
        return out[: got.value].copy()


def ref_resample(x, fi, fo=16000):
    """the host reference over a whole signal in one push"""
    return RefStream(fi, fo).push(x)


def same_bits(a, b):
    """bit for bit, the sign of a zero aside"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))))

