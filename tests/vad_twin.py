"""Float64 numpy twin of the voice activity detector (csrc/vad_ref.h is the normative float32 text; DESIGN.md "Voice activity detection
and long recordings" the prose), the error bound the float32 reference is held to, and the views of the library the VAD tests share:
the host reference through k2hip_debug_vad_ref_* (no GPU), the config rules, the packing rule.

The twin follows the definition with the definition's own float32 constants (1.0f / (hi - lo), 0.2f, rise) taken exactly and every
sum and product in float64."""
import ctypes as C

import numpy as np

F32 = np.float32


def default_config(num_bins=80, sample_rate=16000, low_freq=20.0, high_freq=0.0):
    from k2transducerasr_amd import VadConfig, load_library
    from k2transducerasr_amd.binding import _bind_vad
    L = load_library()
    _bind_vad(L)
    cfg = VadConfig()
    rc = L.k2hip_debug_vad_default_config(sample_rate, num_bins, low_freq, high_freq, C.byref(cfg))
    assert rc == 0, L.k2hip_last_error()
    return cfg


def check_config(cfg, num_bins=80):
    """(return code, message) of the library's config rules"""
    from k2transducerasr_amd import load_library
    from k2transducerasr_amd.binding import _bind_vad
    L = load_library()
    _bind_vad(L)
    rc = L.k2hip_debug_vad_check_config(C.byref(cfg), num_bins)
    return rc, L.k2hip_last_error().decode()


def lib_pack(lens, max_batch, max_batch_frames):
    """(return code, batch index per segment) of the long entry's packing rule"""
    from k2transducerasr_amd import load_library
    from k2transducerasr_amd.binding import _bind_vad
    L = load_library()
    _bind_vad(L)
    a = np.ascontiguousarray(lens, dtype=np.int64)
    out = np.full(max(len(a), 1), -1, np.int32)
    rc = L.k2hip_debug_vad_pack(a.ctypes.data_as(C.POINTER(C.c_int64)), len(a), max_batch, max_batch_frames, out.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, out[: len(a)].tolist()


def twin_pack(lens, max_batch, max_batch_frames):
    """the packing rule from its sentence: a batch closes at max_batch segments, or when (count + 1) * longest would exceed max_batch_frames"""
    out, batch, count, longest = [], 0, 0, 0
    for n in lens:
        if count and (count >= max_batch or (count + 1) * max(longest, n) > max_batch_frames):
            batch, count, longest = batch + 1, 0, 0
        out.append(batch)
        count, longest = count + 1, max(longest, n)
    return out


class Twin:
    """the detector over a whole feature matrix in float64: taps s, m, n, d, the magnitudes the bound needs, the segments"""

    def __init__(self, cfg):
        self.c = cfg
        self.lo, self.hi, self.W = cfg.band_lo, cfg.band_hi, cfg.floor_window
        self.inv = float(F32(1.0) / F32(self.hi - self.lo))
        self.fifth = float(F32(0.2))
        self.rise, self.margin, self.abs_floor = float(F32(cfg.rise)), float(F32(cfg.margin)), float(F32(cfg.abs_floor))

    def taps(self, x):
        x = np.asarray(x, np.float64)[:, self.lo:self.hi]
        T = x.shape[0]
        s = x.sum(axis=1) * self.inv
        s_mag = np.abs(x).sum(axis=1) * self.inv
        sp = np.concatenate([np.full(4, s[0]), s]) if T else s
        mp = np.concatenate([np.full(4, s_mag[0]), s_mag]) if T else s_mag
        m = np.array([(sp[t] + sp[t + 1] + sp[t + 2] + sp[t + 3] + sp[t + 4]) * self.fifth for t in range(T)])
        m_mag = np.array([(mp[t] + mp[t + 1] + mp[t + 2] + mp[t + 3] + mp[t + 4]) * self.fifth for t in range(T)])
        n, n_mag = np.zeros(T), np.zeros(T)
        for t in range(T):
            u0 = max(0, t - self.W + 1)
            ramp = self.rise * np.arange(t - u0, -1, -1, dtype=np.float64)
            n[t] = np.min(m[u0:t + 1] + ramp)
            n_mag[t] = np.max(m_mag[u0:t + 1] + np.abs(ramp))
        d = (m - n > self.margin) & (m > self.abs_floor)
        return dict(s=s, m=m, n=n, d=d, s_mag=s_mag, m_mag=m_mag, n_mag=n_mag)

    def bound(self, mag):
        """the float32 chain's own bound from its operands: (hi - lo + 6) * 2^-24 * sum |x|"""
        return (self.hi - self.lo + 6) * 2.0 ** -24 * mag

    def machine(self, d, m, flush=True, forced_at=None):
        """the segmentation machine and the reporting rule over decisions d and smoothed scores m -> [(start, end, forced)], is_speech;
        forced_at (a list) collects the frames at which a forced cut happened"""
        return machine(self.c, d, m, flush, forced_at)


def machine(c, d, m, flush=True, forced_at=None):
    T = len(d)
    trig, start, te, prev_end, out = 0, 0, -1, 0, []

    def emit(a, b, forced, seen):
        nonlocal prev_end
        a2 = max(a - c.speech_pad, prev_end, 0)
        b2 = b if forced else min(b + c.speech_pad, seen)
        out.append((a2, b2, forced))
        prev_end = b2

    for t in range(T):
        if d[t]:
            if not trig:
                trig, start = 1, t
            te = -1
        elif trig:
            if te < 0:
                te = t
            if t + 1 - te >= c.min_silence:
                if te - start >= c.min_speech:
                    emit(start, te, 0, t + 1)
                trig, te = 0, -1
        if trig and t + 1 - start >= c.max_speech:
            lo = t + 1 - c.max_speech // 2
            cut = lo + int(np.argmin(np.asarray(m[lo:t + 1])))   # (argmin: the first of equal minima)
            emit(start, cut, 1, t + 1)
            if forced_at is not None:
                forced_at.append(t)
            start = cut
            te = -1 if d[t] else max(te, cut)
    speech = bool(trig)
    if flush and trig:
        e = te if te >= 0 else T
        if e - start >= c.min_speech:
            emit(start, e, 0, T)
    return out, speech


# ---- the library's float32 host reference, no GPU ------------------------------------------------------------------------------------
def ref_stream(cfg, num_bins=80):
    from k2transducerasr_amd import VadStream
    return VadStream(None, cfg, num_bins=num_bins)


def ref_run(cfg, x, chunks=None, flush=True):
    """the reference over x [T, num_bins], fed whole or in the given chunk lengths -> dict(m, n, d, segs, speech): speech = is_speech
    before the flush"""
    x = np.ascontiguousarray(x, np.float32)
    st = ref_stream(cfg, x.shape[1])
    taps, pos = [], 0
    for n in ([x.shape[0]] if chunks is None else chunks):
        taps.append(st.ref_push(x[pos:pos + n]))
        pos += n
    assert pos == x.shape[0] == st.num_frames
    speech = st.is_speech
    if flush:
        st.flush()
    segs = [(g["start"], g["end"], g["forced"]) for g in st.segments()]
    st.close()
    return dict(m=np.concatenate([t[0] for t in taps]), n=np.concatenate([t[1] for t in taps]), d=np.concatenate([t[2] for t in taps]), segs=segs,
                speech=speech)


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all(a.view(np.uint32) == b.view(np.uint32)))
