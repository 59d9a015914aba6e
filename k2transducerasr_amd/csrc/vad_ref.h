// Host reference of the voice activity detector (vad.hip), float32, header only: the NORMATIVE text of the detector.  What the GPU
// kernels are compared with bit for bit, what the CPU stand-in of the engine under tests/native runs, and where the configuration
// rules, the carried state, the reporting rule (padding) and the long entry's batch packing live.  DESIGN.md "Voice activity
// detection and long recordings" has the definition in prose.
//
// Everything is counted in fbank frames.  Per frame t of a stream (numbered from its start or its last reset), x[t] its feature row:
//   s_t  the mean of x[t][lo .. hi) in the order of vad_ref_score below,
//   m_t  = ((((s_{t-4} + s_{t-3}) + s_{t-2}) + s_{t-1}) + s_t) * 0.2f, with s_u := s_0 for u < 0,
//   n_t  = min over max(0, t - W + 1) <= u <= t, u ascending, of m_u + rise * (float)(t - u): product and sum rounded separately,
//   d_t  = (m_t - n_t > margin) && (m_t > abs_floor).
// The level defaults (rise, margin, abs_floor) are in natural-log power units, the unit of the features, and are UNTUNED: nobody has
// measured them on real speech.
//
// The order of s_t is one a wave of 64 lanes can do: lane l sums x[lo + l], x[lo + 64 + l], ... ascending from +0.0f, then six
// butterfly steps p[l] = p[l] + p[l + off] for off = 32, 16, 8, 4, 2, 1 (lanes beyond the band hold +0.0f), then p[0] * (1.0f / (hi - lo)).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "errors.h"

namespace k2hip {

constexpr int kVadMaxWindow = 1024;                  // floor_window beyond this is K2HIP_ERR_UNSUPPORTED (the floor pass stages W - 1 + a tile in LDS)
constexpr int64_t kVadMaxFrames = (int64_t)1 << 30;  // frames of one stream between resets: the kernels count in int32

inline void vad_default_levels(k2hip_vad_config* c) {
    c->floor_window = 1000;
    c->rise = 0.002f;
    c->margin = 2.0f;
    c->abs_floor = -12.0f;
    c->min_silence = 50;
    c->min_speech = 25;
    c->speech_pad = 10;
    c->max_speech = 2000;
}

// the mel bins whose centre frequency lies in [300, 3500] Hz, for the filterbank model.cpp builds (centres evenly spaced in mel)
inline void vad_default_config(int sample_rate, int num_bins, float low_freq, float high_freq, k2hip_vad_config* c) {
    vad_default_levels(c);
    double hi = high_freq;
    if (hi <= 0.0) hi += 0.5 * sample_rate;
    const double mel_low = 1127.0 * log(1.0 + low_freq / 700.0), mel_high = 1127.0 * log(1.0 + hi / 700.0);
    const double delta = (mel_high - mel_low) / (num_bins + 1);
    int lo = num_bins, h = 0;
    for (int b = 0; b < num_bins; b++) {
        const double f = 700.0 * (exp((mel_low + (b + 1) * delta) / 1127.0) - 1.0);
        if (f >= 300.0 && f <= 3500.0) {
            lo = std::min(lo, b);
            h = std::max(h, b + 1);
        }
    }
    if (lo >= h) { lo = 0; h = num_bins; }   // (a filterbank with no centre in the band: every bin)
    c->band_lo = lo;
    c->band_hi = h;
}

// every refusal of include/k2hip.h "Voice activity detection", the field named
inline void vad_check_config(const k2hip_vad_config& c, int num_bins) {
    K2_REQUIRE(c.band_lo >= 0 && c.band_hi <= num_bins && c.band_lo < c.band_hi, "vad config: band_lo = %d, band_hi = %d: need 0 <= band_lo < band_hi <= %d",
               c.band_lo, c.band_hi, num_bins);
    K2_REQUIRE(c.floor_window > 0, "vad config: floor_window = %d must be positive", c.floor_window);
    K2_REQUIRE(c.min_silence > 0, "vad config: min_silence = %d must be positive", c.min_silence);
    K2_REQUIRE(c.min_speech > 0, "vad config: min_speech = %d must be positive", c.min_speech);
    K2_REQUIRE(c.speech_pad > 0, "vad config: speech_pad = %d must be positive", c.speech_pad);
    K2_REQUIRE(c.max_speech > 0, "vad config: max_speech = %d must be positive", c.max_speech);
    K2_REQUIRE(std::isfinite(c.rise), "vad config: rise is not finite");
    K2_REQUIRE(std::isfinite(c.margin), "vad config: margin is not finite");
    K2_REQUIRE(std::isfinite(c.abs_floor), "vad config: abs_floor is not finite");
    K2_REQUIRE(c.floor_window >= 8, "vad config: floor_window = %d is below 8", c.floor_window);
    if (c.floor_window > kVadMaxWindow) failf(K2HIP_ERR_UNSUPPORTED, "vad config: floor_window = %d exceeds %d", c.floor_window, kVadMaxWindow);
    K2_REQUIRE(c.min_silence >= 2 * (int64_t)c.speech_pad, "vad config: min_silence = %d is below 2 * speech_pad = %lld", c.min_silence, 2 * (long long)c.speech_pad);
    K2_REQUIRE(c.max_speech >= 2 * (int64_t)c.min_speech, "vad config: max_speech = %d is below 2 * min_speech = %lld", c.max_speech, 2 * (long long)c.min_speech);
    // (the forced cut looks at frames [t + 1 - max_speech / 2, t]: frame t and the W - 1 carried values of m in front of it)
    K2_REQUIRE(c.max_speech / 2 <= c.floor_window, "vad config: max_speech / 2 = %d exceeds floor_window = %d", c.max_speech / 2, c.floor_window);
}

// what the machine emits: frames [a, b) of the stream, before padding
struct VadRaw {
    int32_t a, b, forced;
};
// a reported segment: frames [start, end)
struct VadSeg {
    int64_t start, end;
    int32_t forced;
};

// The carried state of one stream: the last min(frames, W - 1) values of m (oldest first), the last 4 of s (s_0 repeated at the
// start), the machine's three variables, the frame count and the end of the previous reported segment.
struct VadState {
    std::vector<float> m;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    int32_t trig = 0;
    int64_t start = 0, te = -1;
    int64_t frames = 0, prev_end = 0;
};

inline float vad_ref_score(const float* row, int lo, int hi) {
    float p[64];
    for (int l = 0; l < 64; l++) {
        float acc = 0.0f;
        for (int j = lo + l; j < hi; j += 64) acc = acc + row[j];
        p[l] = acc;
    }
    for (int off = 32; off >= 1; off >>= 1)
        for (int l = 0; l < off; l++) p[l] = p[l] + p[l + off];
    return p[0] * (1.0f / (float)(hi - lo));
}

// rise * k, rounded to float32 before it is added (no fused multiply-add, whatever the compiler's contraction setting)
inline float vad_ref_ramp(float rise, int64_t k) {
    volatile float p = rise * (float)k;
    return p;
}

// The reporting rule: raw segment -> [a', b').  T: the frames the stream has seen (a flush clips the padded end to it).
inline VadSeg vad_report(const k2hip_vad_config& c, const VadRaw& r, int64_t* prev_end, int64_t T) {
    VadSeg s;
    s.start = std::max<int64_t>(std::max<int64_t>((int64_t)r.a - c.speech_pad, *prev_end), 0);
    s.end = r.forced ? (int64_t)r.b : std::min<int64_t>((int64_t)r.b + c.speech_pad, T);
    s.forced = r.forced;
    *prev_end = s.end;
    return s;
}

// n frames (rows `stride` floats apart) into the stream: the reported segments are appended to *segs, the taps (each may be null)
// get n entries.  The config must have passed vad_check_config.
inline void vad_ref_push(const k2hip_vad_config& c, VadState& st, const float* x, int64_t n, int64_t stride, std::vector<VadSeg>* segs, float* tap_m,
                         float* tap_n, uint8_t* tap_d) {
    K2_REQUIRE(n >= 0 && st.frames + n < kVadMaxFrames, "vad: %lld + %lld frames in one stream", (long long)st.frames, (long long)n);
    const int W = c.floor_window;
    // the logical array of m: [carried history ; this call's], index 0 = frame t0
    std::vector<float> mm(st.m);
    const int64_t t0 = st.frames - (int64_t)st.m.size();
    mm.reserve(st.m.size() + (size_t)n);
    auto m_at = [&](int64_t t) { return mm[(size_t)(t - t0)]; };
    for (int64_t i = 0; i < n; i++) {
        const int64_t t = st.frames;
        const float s = vad_ref_score(x + i * stride, c.band_lo, c.band_hi);
        if (t == 0) st.s[0] = st.s[1] = st.s[2] = st.s[3] = s;
        const float m = ((((st.s[0] + st.s[1]) + st.s[2]) + st.s[3]) + s) * 0.2f;
        st.s[0] = st.s[1]; st.s[1] = st.s[2]; st.s[2] = st.s[3]; st.s[3] = s;
        mm.push_back(m);
        float nf = 0.f;
        for (int64_t u = std::max<int64_t>(0, t - W + 1); u <= t; u++) {
            const float v = m_at(u) + vad_ref_ramp(c.rise, t - u);
            if (u == std::max<int64_t>(0, t - W + 1) || v < nf) nf = v;
        }
        const bool d = (m - nf > c.margin) && (m > c.abs_floor);
        if (tap_m) tap_m[i] = m;
        if (tap_n) tap_n[i] = nf;
        if (tap_d) tap_d[i] = d;
        // the machine
        auto emit = [&](int64_t a, int64_t b, int forced) {
            segs->push_back(vad_report(c, VadRaw{(int32_t)a, (int32_t)b, forced}, &st.prev_end, t + 1));
        };
        if (d) {
            if (!st.trig) { st.trig = 1; st.start = t; }
            st.te = -1;
        } else if (st.trig) {
            if (st.te < 0) st.te = t;
            if (t + 1 - st.te >= c.min_silence) {
                if (st.te - st.start >= c.min_speech) emit(st.start, st.te, 0);
                st.trig = 0;
                st.te = -1;
            }
        }
        if (st.trig && t + 1 - st.start >= c.max_speech) {
            int64_t cut = t + 1 - c.max_speech / 2;
            for (int64_t u = cut + 1; u <= t; u++)
                if (m_at(u) < m_at(cut)) cut = u;   // the smallest m, the earliest on ties
            emit(st.start, cut, 1);
            st.start = cut;
            st.te = d ? -1 : std::max(st.te, cut);
        }
        st.frames = t + 1;
    }
    const size_t keep = (size_t)std::min<int64_t>(st.frames, W - 1);
    st.m.assign(mm.end() - keep, mm.end());
}

// end of audio: the open segment, if any, is closed; then the stream is as after a reset
inline void vad_ref_flush(const k2hip_vad_config& c, VadState& st, std::vector<VadSeg>* segs) {
    if (st.trig) {
        const int64_t e = st.te >= 0 ? st.te : st.frames;
        if (e - st.start >= c.min_speech) segs->push_back(vad_report(c, VadRaw{(int32_t)st.start, (int32_t)e, 0}, &st.prev_end, st.frames));
    }
    st = VadState();
}

// ---- the long entry's batch packing: the segments in order; a batch closes at max_batch segments, or when (count + 1) * longest
// would exceed max_batch_frames (a segment longer than max_batch_frames on its own forms a batch of one).  batch_of gets one batch
// index per segment.
inline void vad_pack_batches(const int64_t* len, int n, int max_batch, int64_t max_batch_frames, std::vector<int32_t>* batch_of) {
    K2_REQUIRE(max_batch > 0 && max_batch_frames > 0, "recognize_long: max_batch = %d, max_batch_frames = %lld", max_batch, (long long)max_batch_frames);
    batch_of->assign((size_t)n, 0);
    int batch = 0, count = 0;
    int64_t longest = 0;
    for (int i = 0; i < n; i++) {
        K2_REQUIRE(len[i] > 0, "recognize_long: segment %d has %lld frames", i, (long long)len[i]);
        if (count > 0 && (count >= max_batch || (int64_t)(count + 1) * std::max(longest, len[i]) > max_batch_frames)) {
            batch++;
            count = 0;
            longest = 0;
        }
        (*batch_of)[(size_t)i] = batch;
        count++;
        longest = std::max(longest, len[i]);
    }
}

}  // namespace k2hip
