// AddressSanitizer / UBSan driver of the voice activity detector's host side: the header-only float32 reference (csrc/vad_ref.h) and
// the stream and result bookkeeping of the k2hip_vad_* / k2hip_offline_recognize_long entries (csrc/api.cpp) through the C ABI over the
// CPU stand-ins of the engine (engine_stub*.cpp; engine_stub_vad.cpp runs the reference where the engine launches the kernels, behind
// a fake fbank whose frame t holds the frame's first sample in every bin).  TEST INFRASTRUCTURE: its own program
// (`make -C k2transducerasr_amd/csrc san_vad`, tests/test_vad_sanitizers.py), never loaded into another process.
// Exercised: the reference over random configs and chunkings against one push bit for bit (taps, segments, the carried state), the
// machine against a frame-by-frame restatement; every refusal of the config with its field; the streams: features and samples in
// any chunking against one call, remainders short of a frame, a stream at 8 kHz against the reference resampler, the rate rules with
// their messages, untouched streams of a batch, create / reset / flush / pop / destroy in every order; the long entry: segments,
// packing, the result object's getters and capacity rule, the refusals.
//   san_vad_driver <offline.k2w>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/k2hip.h"
#include "../../include/k2hip_debug.h"
#include "../../k2transducerasr_amd/csrc/resample_plan.h"
#include "../../k2transducerasr_amd/csrc/resample_ref.h"
#include "../../k2transducerasr_amd/csrc/vad_ref.h"

#define CHECK(cond)                                                                                                          \
    do {                                                                                                                     \
        if (!(cond)) {                                                                                                       \
            fprintf(stderr, "CHECK failed at %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, k2hip_last_error()); \
            exit(3);                                                                                                         \
        }                                                                                                                    \
    } while (0)
#define OK(call) CHECK((call) == K2HIP_OK)

namespace {

using k2hip::VadSeg;
using k2hip::VadState;

unsigned long long rng_state = 88172645463325252ull;
unsigned rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 32);
}
float rndf() { return (float)(rnd() >> 8) * (1.0f / 8388608.0f) - 1.0f; }
bool same_bits(const float* a, const float* b, size_t n) { return n == 0 || memcmp(a, b, n * sizeof(float)) == 0; }
bool same_segs(const std::vector<VadSeg>& a, const std::vector<VadSeg>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (a[i].start != b[i].start || a[i].end != b[i].end || a[i].forced != b[i].forced) return false;
    return true;
}
bool same_state(const VadState& a, const VadState& b) {
    return a.m.size() == b.m.size() && same_bits(a.m.data(), b.m.data(), a.m.size()) && same_bits(a.s, b.s, 4) && a.trig == b.trig &&
           (!a.trig || (a.start == b.start && a.te == b.te)) && a.frames == b.frames && a.prev_end == b.prev_end;
}

k2hip_vad_config random_config(int num_bins) {
    k2hip_vad_config c;
    c.band_lo = (int)(rnd() % (unsigned)num_bins);
    c.band_hi = c.band_lo + 1 + (int)(rnd() % (unsigned)(num_bins - c.band_lo));
    c.floor_window = 8 + (int)(rnd() % 60);
    c.rise = (float)(rnd() % 100) * 0.001f;
    c.margin = 0.5f + (float)(rnd() % 30) * 0.1f;
    c.abs_floor = -14.0f + (float)(rnd() % 8);
    c.speech_pad = 1 + (int)(rnd() % 4);
    c.min_silence = 2 * c.speech_pad + (int)(rnd() % 6);
    c.min_speech = 1 + (int)(rnd() % 6);
    c.max_speech = std::max(2 * c.min_speech, 2 + (int)(rnd() % (unsigned)(2 * c.floor_window - 1)));
    k2hip::vad_check_config(c, num_bins);
    return c;
}
// rows of noise near -10 with stretches near -2
std::vector<float> random_rows(int64_t T, int num_bins) {
    std::vector<float> x((size_t)(T * num_bins));
    bool speech = false;
    int64_t left = 0;
    for (int64_t t = 0; t < T; t++) {
        if (left-- <= 0) {
            speech = !speech;
            left = 1 + rnd() % (speech ? 70 : 25);
        }
        for (int c = 0; c < num_bins; c++) x[(size_t)(t * num_bins + c)] = (speech ? -2.0f : -10.0f) + rndf();
    }
    return x;
}
// the machine restated frame by frame on given decisions and scores (no padding): what the reference's segments are checked against
std::vector<VadSeg> restated(const k2hip_vad_config& c, const std::vector<uint8_t>& d, const std::vector<float>& m) {
    std::vector<VadSeg> out;
    int64_t trig = 0, start = 0, te = -1, prev = 0;
    const int64_t T = (int64_t)d.size();
    auto emit = [&](int64_t a, int64_t b, int forced, int64_t seen) {
        VadSeg s;
        s.start = std::max<int64_t>({a - c.speech_pad, prev, 0});
        s.end = forced ? b : std::min<int64_t>(b + c.speech_pad, seen);
        s.forced = forced;
        prev = s.end;
        out.push_back(s);
    };
    for (int64_t t = 0; t < T; t++) {
        if (d[(size_t)t]) {
            if (!trig) { trig = 1; start = t; }
            te = -1;
        } else if (trig) {
            if (te < 0) te = t;
            if (t + 1 - te >= c.min_silence) {
                if (te - start >= c.min_speech) emit(start, te, 0, t + 1);
                trig = 0;
                te = -1;
            }
        }
        if (trig && t + 1 - start >= c.max_speech) {
            int64_t cut = t + 1 - c.max_speech / 2;
            for (int64_t u = cut; u <= t; u++)
                if (m[(size_t)u] < m[(size_t)cut]) cut = u;
            emit(start, cut, 1, t + 1);
            start = cut;
            te = d[(size_t)t] ? -1 : std::max(te, cut);
        }
    }
    if (trig) {
        const int64_t e = te >= 0 ? te : T;
        if (e - start >= c.min_speech) emit(start, e, 0, T);
    }
    return out;
}

void reference() {
    int forced = 0, total = 0;
    for (int round = 0; round < 60; round++) {
        const int nb = 1 + (int)(rnd() % 80);
        const k2hip_vad_config c = random_config(nb);
        const int64_t T = 1 + rnd() % 700;
        const std::vector<float> x = random_rows(T, nb);
        VadState whole;
        std::vector<VadSeg> segs;
        std::vector<float> m((size_t)T), n((size_t)T);
        std::vector<uint8_t> d((size_t)T);
        k2hip::vad_ref_push(c, whole, x.data(), T, nb, &segs, m.data(), n.data(), d.data());
        CHECK(whole.frames == T && (int64_t)whole.m.size() == std::min<int64_t>(T, c.floor_window - 1));
        VadState st;
        std::vector<VadSeg> got;
        std::vector<float> m2((size_t)T), n2((size_t)T);
        std::vector<uint8_t> d2((size_t)T);
        for (int64_t pos = 0; pos < T;) {
            const int64_t k = std::min<int64_t>(T - pos, rnd() % 5 == 0 ? 0 : 1 + rnd() % 90);
            // an exact-size copy of the chunk: a read past it is a heap overflow
            const std::vector<float> piece(x.begin() + pos * nb, x.begin() + (pos + k) * nb);
            k2hip::vad_ref_push(c, st, piece.data(), k, nb, &got, m2.data() + pos, n2.data() + pos, d2.data() + pos);
            pos += k;
        }
        CHECK(same_bits(m.data(), m2.data(), (size_t)T) && same_bits(n.data(), n2.data(), (size_t)T) && d == d2 && same_segs(segs, got) && same_state(whole, st));
        for (int64_t t = 0; t < T; t++) CHECK(std::isfinite(m[(size_t)t]) && n[(size_t)t] <= m[(size_t)t]);
        k2hip::vad_ref_flush(c, whole, &segs);
        k2hip::vad_ref_flush(c, st, &got);
        CHECK(same_segs(segs, got) && whole.frames == 0 && whole.m.empty() && !whole.trig && whole.prev_end == 0);
        CHECK(same_segs(segs, restated(c, d, m)));
        for (size_t i = 0; i < segs.size(); i++) {
            CHECK(segs[i].start >= 0 && segs[i].start < segs[i].end && segs[i].end <= T && (i == 0 || segs[i].start >= segs[i - 1].end));
            forced += segs[i].forced;
            total++;
        }
    }
    CHECK(total > 100 && forced > 10);
}

struct Segs {
    std::vector<int64_t> start, end;
    std::vector<int32_t> forced;
};
Segs segments_of(const k2hip_vad_stream_t* s) {
    Segs g;
    const int32_t n = k2hip_vad_stream_num_segments(s);
    CHECK(n >= 0);
    g.start.resize((size_t)n); g.end.resize((size_t)n); g.forced.resize((size_t)n);
    OK(k2hip_vad_stream_get_segments(s, g.start.data(), g.end.data(), g.forced.data(), n));
    if (n > 0) CHECK(k2hip_vad_stream_get_segments(s, g.start.data(), g.end.data(), g.forced.data(), n - 1) == K2HIP_ERR_CAPACITY);
    return g;
}
bool same(const Segs& a, const Segs& b) { return a.start == b.start && a.end == b.end && a.forced == b.forced; }

// samples whose fake frames are speech (-2) or noise (-10): frame t's first sample is sample 160 t
std::vector<float> steer_samples(int64_t n, int shift) {
    std::vector<float> x((size_t)n);
    bool speech = false;
    int64_t left = 0;
    for (int64_t i = 0; i < n; i++) {
        if (i % shift == 0 && left-- <= 0) {
            speech = !speech;
            left = speech ? 30 + rnd() % 200 : 20 + rnd() % 90;
        }
        x[(size_t)i] = (speech ? -2.0f : -10.0f) + 0.25f * rndf();
    }
    return x;
}

void config_refusals(k2hip_model_t* m) {
    k2hip_vad_config base;
    OK(k2hip_vad_default_config(m, &base));
    CHECK(base.band_lo == 10 && base.band_hi == 57 && base.floor_window == 1000 && base.max_speech == 2000 && base.min_silence == 50 &&
          base.min_speech == 25 && base.speech_pad == 10 && base.rise == 0.002f && base.margin == 2.0f && base.abs_floor == -12.0f);
    struct Bad {
        void (*change)(k2hip_vad_config&);
        int code;
        const char* field;
    };
    const Bad bad[] = {
        {[](k2hip_vad_config& c) { c.band_lo = c.band_hi; }, K2HIP_ERR_INVALID, "band_lo"},
        {[](k2hip_vad_config& c) { c.band_hi = 81; }, K2HIP_ERR_INVALID, "band_hi"},
        {[](k2hip_vad_config& c) { c.floor_window = 7; c.max_speech = 50; }, K2HIP_ERR_INVALID, "floor_window"},
        {[](k2hip_vad_config& c) { c.floor_window = 1025; }, K2HIP_ERR_UNSUPPORTED, "floor_window"},
        {[](k2hip_vad_config& c) { c.min_silence = 19; }, K2HIP_ERR_INVALID, "min_silence"},
        {[](k2hip_vad_config& c) { c.max_speech = 49; }, K2HIP_ERR_INVALID, "max_speech"},
        {[](k2hip_vad_config& c) { c.floor_window = 100; c.max_speech = 202; }, K2HIP_ERR_INVALID, "max_speech"},
        {[](k2hip_vad_config& c) { c.min_speech = 0; }, K2HIP_ERR_INVALID, "min_speech"},
        {[](k2hip_vad_config& c) { c.speech_pad = -1; }, K2HIP_ERR_INVALID, "speech_pad"},
        {[](k2hip_vad_config& c) { c.min_silence = 0; }, K2HIP_ERR_INVALID, "min_silence"},
        {[](k2hip_vad_config& c) { c.max_speech = 0; }, K2HIP_ERR_INVALID, "max_speech"},
        {[](k2hip_vad_config& c) { c.floor_window = 0; }, K2HIP_ERR_INVALID, "floor_window"},
        {[](k2hip_vad_config& c) { c.rise = INFINITY; }, K2HIP_ERR_INVALID, "rise"},
        {[](k2hip_vad_config& c) { c.margin = NAN; }, K2HIP_ERR_INVALID, "margin"},
        {[](k2hip_vad_config& c) { c.abs_floor = -INFINITY; }, K2HIP_ERR_INVALID, "abs_floor"},
    };
    for (const Bad& b : bad) {
        k2hip_vad_config c = base;
        b.change(c);
        k2hip_vad_stream_t* s = reinterpret_cast<k2hip_vad_stream_t*>(1);
        CHECK(k2hip_vad_stream_create(m, &c, &s) == b.code && s == nullptr && strstr(k2hip_last_error(), b.field));
        CHECK(k2hip_debug_vad_check_config(&c, 80) == b.code);
        k2hip_long_result_t* r = nullptr;
        const float x[4] = {0, 0, 0, 0};
        CHECK(k2hip_offline_recognize_long(m, 16000, x, 4, &c, 4, 1000, &r) == b.code && r == nullptr);
    }
    k2hip_vad_stream_t* s = nullptr;
    CHECK(k2hip_vad_stream_create(nullptr, &base, &s) == K2HIP_ERR_INVALID && k2hip_vad_stream_create(m, nullptr, &s) == K2HIP_ERR_INVALID &&
          k2hip_vad_stream_create(m, &base, nullptr) == K2HIP_ERR_INVALID);
    CHECK(k2hip_vad_stream_is_speech(nullptr) == -1 && k2hip_vad_stream_num_frames(nullptr) == -1 && k2hip_vad_stream_num_segments(nullptr) == -1);
    CHECK(k2hip_vad_stream_reset(nullptr) == K2HIP_ERR_INVALID && k2hip_vad_stream_flush(nullptr) == K2HIP_ERR_INVALID);
    OK(k2hip_vad_stream_destroy(nullptr));
}

// a config that segments the steered samples into many pieces, with forced cuts
k2hip_vad_config stream_config(k2hip_model_t* m) {
    k2hip_vad_config c;
    OK(k2hip_vad_default_config(m, &c));
    c.floor_window = 200; c.max_speech = 120; c.min_speech = 10; c.min_silence = 12; c.speech_pad = 4;
    return c;
}

void streams(k2hip_model_t* m) {
    const k2hip_vad_config c = stream_config(m);
    const int F = 80, shift = 160;
    const std::vector<float> x = steer_samples(16000 * 16 + 77, shift);
    const int64_t T = 1 + ((int64_t)x.size() - 400) / shift;
    // the reference over the fake frames, whole
    std::vector<float> rows((size_t)(T * F));
    for (int64_t t = 0; t < T; t++)
        for (int k = 0; k < F; k++) rows[(size_t)(t * F + k)] = x[(size_t)(t * shift)];
    k2hip_vad_stream_t* ref = nullptr;
    OK(k2hip_debug_vad_ref_stream_create(F, &c, &ref));
    std::vector<float> rm((size_t)T), rn((size_t)T);
    std::vector<uint8_t> rd((size_t)T);
    OK(k2hip_debug_vad_ref_push(ref, rows.data(), T, rm.data(), rn.data(), rd.data()));
    const int ref_speech = k2hip_vad_stream_is_speech(ref);
    CHECK(k2hip_vad_stream_num_frames(ref) == T);
    OK(k2hip_vad_stream_flush(ref));
    const Segs want = segments_of(ref);
    CHECK(want.start.size() >= 5 && std::count(want.forced.begin(), want.forced.end(), 1) >= 2 && k2hip_vad_stream_num_frames(ref) == 0);
    // a reference stream takes no accept call
    {
        const float* fp[1] = {rows.data()};
        const int64_t one[1] = {1};
        CHECK(k2hip_vad_accept_features_batch(m, &ref, fp, one, 1) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "another model"));
    }
    // features in: three streams in the same calls, each with its own chunking, some chunks empty; the taps of every call
    for (int round = 0; round < 3; round++) {
        k2hip_vad_stream_t* s[3];
        int64_t pos[3] = {0, 0, 0};
        for (auto& p : s) OK(k2hip_vad_stream_create(m, &c, &p));
        while (pos[0] < T || pos[1] < T || pos[2] < T) {
            int64_t n[3];
            std::vector<std::vector<float>> piece(3);
            const float* fp[3];
            for (int b = 0; b < 3; b++) {
                n[b] = std::min<int64_t>(T - pos[b], round == 0 ? 1 + 63 * b : rnd() % 4 == 0 ? 0 : 1 + rnd() % 130);
                piece[(size_t)b].assign(rows.begin() + pos[b] * F, rows.begin() + (pos[b] + n[b]) * F);   // exact size
                fp[b] = n[b] ? piece[(size_t)b].data() : nullptr;
            }
            OK(k2hip_vad_accept_features_batch(m, s, fp, n, 3));
            for (int b = 0; b < 3; b++) {
                std::vector<float> tm((size_t)n[b] + 1), tn((size_t)n[b] + 1);
                std::vector<uint8_t> td((size_t)n[b] + 1);
                int64_t cnt = -1;
                OK(k2hip_debug_vad_taps(m, b, tm.data(), tn.data(), td.data(), n[b], &cnt));
                CHECK(cnt == n[b] && same_bits(tm.data(), rm.data() + pos[b], (size_t)cnt) && same_bits(tn.data(), rn.data() + pos[b], (size_t)cnt) &&
                      (cnt == 0 || memcmp(td.data(), rd.data() + pos[b], (size_t)cnt) == 0));
                if (cnt > 0) CHECK(k2hip_debug_vad_taps(m, b, tm.data(), tn.data(), td.data(), cnt - 1, &cnt) == K2HIP_ERR_CAPACITY);
                pos[b] += n[b];
                CHECK(k2hip_vad_stream_num_frames(s[b]) == pos[b]);
            }
        }
        int64_t cnt = 0;
        CHECK(k2hip_debug_vad_taps(m, 3, nullptr, nullptr, nullptr, 0, &cnt) == K2HIP_ERR_INVALID);
        for (auto& p : s) {
            CHECK(k2hip_vad_stream_is_speech(p) == ref_speech);
            OK(k2hip_vad_stream_flush(p));
            CHECK(same(segments_of(p), want) && k2hip_vad_stream_is_speech(p) == 0);
            OK(k2hip_vad_stream_destroy(p));
        }
    }
    // the same stream twice in a call, a stream of another kind of list
    {
        k2hip_vad_stream_t* a = nullptr;
        OK(k2hip_vad_stream_create(m, &c, &a));
        k2hip_vad_stream_t* two[2] = {a, a};
        const float* fp[2] = {rows.data(), rows.data()};
        const int64_t n[2] = {3, 3};
        CHECK(k2hip_vad_accept_features_batch(m, two, fp, n, 2) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "twice"));
        const int64_t neg[2] = {-1, 0};
        CHECK(k2hip_vad_accept_features_batch(m, two, fp, neg, 1) == K2HIP_ERR_INVALID);
        CHECK(k2hip_vad_accept_features_batch(m, two, fp, n, 0) == K2HIP_ERR_INVALID && k2hip_vad_stream_num_frames(a) == 0);
        OK(k2hip_vad_stream_destroy(a));
    }
    // samples in, at the model's rate: any chunking leaves what one call leaves -- pieces short of a frame, pieces that end inside a
    // frame shift, a frame completed by a single sample
    for (int round = 0; round < 4; round++) {
        k2hip_vad_stream_t* s = nullptr;
        OK(k2hip_vad_stream_create(m, &c, &s));
        const int64_t sizes[] = {1, 37, 159, 160, 161, 399, 400, 401, 4000, 12345};
        for (size_t pos = 0; pos < x.size();) {
            const size_t n = round == 0 ? x.size() : std::min<size_t>(x.size() - pos, (size_t)sizes[rnd() % 10]);
            const std::vector<float> piece(x.begin() + pos, x.begin() + pos + n);
            const float* sp[1] = {piece.data()};
            const int64_t nn[1] = {(int64_t)n};
            OK(k2hip_vad_accept_samples_batch(m, &s, 16000, sp, nn, 1));
            pos += n;
            CHECK(k2hip_vad_stream_num_frames(s) == (pos < 400 ? 0 : 1 + ((int64_t)pos - 400) / shift));
        }
        CHECK(k2hip_vad_stream_is_speech(s) == ref_speech);
        // the rate rule: fixed by the first samples, both rates in the message
        const float* sp[1] = {x.data()};
        const int64_t nn[1] = {100};
        CHECK(k2hip_vad_accept_samples_batch(m, &s, 8000, sp, nn, 1) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "16000") &&
              strstr(k2hip_last_error(), "8000"));
        // features do not mix with samples short of a frame
        const float* fp[1] = {rows.data()};
        const int64_t one[1] = {1};
        CHECK(k2hip_vad_accept_features_batch(m, &s, fp, one, 1) == K2HIP_ERR_INVALID);
        OK(k2hip_vad_stream_flush(s));
        CHECK(same(segments_of(s), want));
        OK(k2hip_vad_accept_samples_batch(m, &s, 8000, sp, nn, 1));   // (a flush opens the rate again)
        OK(k2hip_vad_stream_destroy(s));
    }
    // a stream at 8 kHz: its frames are those of the reference resampler's output, whatever the chunking
    {
        const std::vector<float> x8 = steer_samples(8000 * 5 + 31, 80);
        const k2hip::ResamplePlan p = k2hip::resample_plan(8000, 16000);
        k2hip::ResampleRefState rs;
        std::vector<float> y;
        k2hip::resample_ref_push(p, rs, x8.data(), (int64_t)x8.size(), &y);
        const int64_t T8 = 1 + ((int64_t)y.size() - 400) / shift;
        std::vector<float> rows8((size_t)(T8 * F));
        for (int64_t t = 0; t < T8; t++)
            for (int k = 0; k < F; k++) rows8[(size_t)(t * F + k)] = y[(size_t)(t * shift)];
        k2hip_vad_stream_t* r8 = nullptr;
        OK(k2hip_debug_vad_ref_stream_create(F, &c, &r8));
        OK(k2hip_debug_vad_ref_push(r8, rows8.data(), T8, nullptr, nullptr, nullptr));
        OK(k2hip_vad_stream_flush(r8));
        const Segs want8 = segments_of(r8);
        CHECK(!want8.start.empty());
        OK(k2hip_vad_stream_destroy(r8));
        for (int round = 0; round < 3; round++) {
            k2hip_vad_stream_t* s = nullptr;
            OK(k2hip_vad_stream_create(m, &c, &s));
            for (size_t pos = 0; pos < x8.size();) {
                const size_t n = round == 0 ? x8.size() : std::min<size_t>(x8.size() - pos, 1 + rnd() % (round == 1 ? 7000 : 90));
                const std::vector<float> piece(x8.begin() + pos, x8.begin() + pos + n);
                const float* sp[1] = {piece.data()};
                const int64_t nn[1] = {(int64_t)n};
                OK(k2hip_vad_accept_samples_batch(m, &s, 8000, sp, nn, 1));
                pos += n;
            }
            CHECK(k2hip_vad_stream_num_frames(s) == T8);
            const float* sp[1] = {x.data()};
            const int64_t nn[1] = {100};
            CHECK(k2hip_vad_accept_samples_batch(m, &s, 16000, sp, nn, 1) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "8000"));
            OK(k2hip_vad_stream_flush(s));
            CHECK(same(segments_of(s), want8));
            OK(k2hip_vad_stream_destroy(s));
        }
        // refused rates move nothing
        k2hip_vad_stream_t* s = nullptr;
        OK(k2hip_vad_stream_create(m, &c, &s));
        const float* sp[1] = {x.data()};
        const int64_t nn[1] = {1000};
        CHECK(k2hip_vad_accept_samples_batch(m, &s, 16001, sp, nn, 1) == K2HIP_ERR_UNSUPPORTED && strstr(k2hip_last_error(), "16001"));
        CHECK(k2hip_vad_accept_samples_batch(m, &s, 0, sp, nn, 1) == K2HIP_ERR_INVALID && k2hip_vad_accept_samples_batch(m, &s, -8000, sp, nn, 1) == K2HIP_ERR_INVALID);
        OK(k2hip_vad_accept_samples_batch(m, &s, 48000, sp, nn, 1));   // (... and leave the stream without a rate)
        OK(k2hip_vad_stream_destroy(s));
    }
    OK(k2hip_vad_stream_destroy(ref));
}

// create, feed, reset, flush, pop and destroy in every order of the middle four
void life_cycle(k2hip_model_t* m) {
    const k2hip_vad_config c = stream_config(m);
    const std::vector<float> x = steer_samples(16000 * 4, 160);
    int order[4] = {0, 1, 2, 3};
    int orders = 0;
    do {
        k2hip_vad_stream_t* s = nullptr;
        OK(k2hip_vad_stream_create(m, &c, &s));
        for (int rep = 0; rep < 2; rep++)
            for (int op : order) {
                const float* sp[1] = {x.data()};
                const int64_t nn[1] = {(int64_t)x.size() - 1000 * (rep + op)};
                switch (op) {
                case 0:
                    OK(k2hip_vad_accept_samples_batch(m, &s, 16000, sp, nn, 1));
                    CHECK(k2hip_vad_stream_num_frames(s) > 0);
                    break;
                case 1:
                    OK(k2hip_vad_stream_reset(s));
                    CHECK(k2hip_vad_stream_num_frames(s) == 0 && k2hip_vad_stream_num_segments(s) == 0 && k2hip_vad_stream_is_speech(s) == 0);
                    break;
                case 2: {
                    const int32_t before = k2hip_vad_stream_num_segments(s);
                    OK(k2hip_vad_stream_flush(s));
                    CHECK(k2hip_vad_stream_num_frames(s) == 0 && k2hip_vad_stream_num_segments(s) >= before && k2hip_vad_stream_is_speech(s) == 0);
                    break;
                }
                default: {
                    const int32_t n = k2hip_vad_stream_num_segments(s);
                    CHECK(k2hip_vad_stream_pop_segments(s, n + 1) == K2HIP_ERR_INVALID && k2hip_vad_stream_pop_segments(s, -1) == K2HIP_ERR_INVALID);
                    const Segs all = segments_of(s);
                    OK(k2hip_vad_stream_pop_segments(s, n / 2));
                    const Segs rest = segments_of(s);
                    CHECK((int32_t)rest.start.size() == n - n / 2 && std::equal(rest.start.begin(), rest.start.end(), all.start.begin() + n / 2));
                    OK(k2hip_vad_stream_pop_segments(s, 0));
                }
                }
            }
        OK(k2hip_vad_stream_destroy(s));
        orders++;
    } while (std::next_permutation(order, order + 4));
    CHECK(orders == 24);
    // streams outlive nothing they point into but the model: destroy in any order among themselves
    k2hip_vad_stream_t* a = nullptr;
    k2hip_vad_stream_t* b = nullptr;
    OK(k2hip_vad_stream_create(m, &c, &a));
    OK(k2hip_vad_stream_create(m, &c, &b));
    OK(k2hip_vad_stream_destroy(a));
    OK(k2hip_vad_stream_destroy(b));
}

void long_entry(k2hip_model_t* m) {
    const k2hip_vad_config c = stream_config(m);
    const std::vector<float> x = steer_samples(16000 * 20 + 5, 160);
    const int64_t T = 1 + ((int64_t)x.size() - 400) / 160;
    // the segments the streams give for the same samples
    k2hip_vad_stream_t* s = nullptr;
    OK(k2hip_vad_stream_create(m, &c, &s));
    const float* sp[1] = {x.data()};
    const int64_t nn[1] = {(int64_t)x.size()};
    OK(k2hip_vad_accept_samples_batch(m, &s, 16000, sp, nn, 1));
    OK(k2hip_vad_stream_flush(s));
    const Segs want = segments_of(s);
    OK(k2hip_vad_stream_destroy(s));
    CHECK(want.start.size() >= 10);
    const struct { int mb; int64_t mbf; } packs[] = {{3, 100000}, {100, 250}, {1, 1}, {4, 130}, {100, 1 << 30}};
    for (const auto& pk : packs) {
        k2hip_long_result_t* r = nullptr;
        OK(k2hip_offline_recognize_long(m, 16000, x.data(), (int64_t)x.size(), &c, pk.mb, pk.mbf, &r));
        const int32_t S = k2hip_long_result_num_segments(r);
        CHECK(S == (int32_t)want.start.size());
        std::vector<int64_t> len((size_t)S);
        std::vector<int32_t> batch((size_t)S), packed((size_t)S);
        for (int32_t i = 0; i < S; i++) {
            int64_t a = -1, b = -1;
            int32_t f = -1;
            OK(k2hip_long_result_get_segment(r, i, &a, &b, &f, &batch[(size_t)i]));
            CHECK(a == want.start[(size_t)i] && b == want.end[(size_t)i] && f == want.forced[(size_t)i] && b <= T);
            OK(k2hip_long_result_get_segment(r, i, nullptr, nullptr, nullptr, nullptr));
            len[(size_t)i] = b - a;
            int32_t n = -1;
            CHECK(k2hip_long_result_get_tokens(r, i, nullptr, nullptr, 0, &n) == K2HIP_ERR_CAPACITY && n > 0);
            std::vector<int64_t> tok((size_t)n);   // exact size: a write past n is a heap overflow
            std::vector<int32_t> ts((size_t)n);
            CHECK(k2hip_long_result_get_tokens(r, i, tok.data(), ts.data(), n - 1, &n) == K2HIP_ERR_CAPACITY);
            OK(k2hip_long_result_get_tokens(r, i, tok.data(), ts.data(), n, &n));
            CHECK(tok[0] == 3 + len[(size_t)i] % 5 && ts[0] == 0);
        }
        OK(k2hip_debug_vad_pack(len.data(), S, pk.mb, pk.mbf, packed.data()));
        CHECK(packed == batch && batch[0] == 0);
        for (int32_t i = 1; i < S; i++) CHECK(batch[(size_t)i] == batch[(size_t)i - 1] || batch[(size_t)i] == batch[(size_t)i - 1] + 1);
        if (pk.mb == 1) CHECK(batch[(size_t)S - 1] == S - 1);
        if (pk.mbf == 1 << 30 && pk.mb == 100) CHECK(batch[(size_t)S - 1] == 0);
        int32_t n = 0;
        CHECK(k2hip_long_result_get_segment(r, S, nullptr, nullptr, nullptr, nullptr) == K2HIP_ERR_INVALID &&
              k2hip_long_result_get_segment(r, -1, nullptr, nullptr, nullptr, nullptr) == K2HIP_ERR_INVALID &&
              k2hip_long_result_get_tokens(r, S, nullptr, nullptr, 0, &n) == K2HIP_ERR_INVALID);
        OK(k2hip_long_result_destroy(r));
    }
    // the defaults (cfg == NULL), a recording shorter than a frame, an empty one, another rate, the refusals
    k2hip_long_result_t* r = nullptr;
    OK(k2hip_offline_recognize_long(m, 16000, x.data(), (int64_t)x.size(), nullptr, 8, 4000, &r));
    CHECK(k2hip_long_result_num_segments(r) >= 1);
    OK(k2hip_long_result_destroy(r));
    OK(k2hip_offline_recognize_long(m, 16000, x.data(), 399, &c, 8, 4000, &r));
    CHECK(k2hip_long_result_num_segments(r) == 0);
    OK(k2hip_long_result_destroy(r));
    OK(k2hip_offline_recognize_long(m, 16000, nullptr, 0, &c, 8, 4000, &r));
    CHECK(k2hip_long_result_num_segments(r) == 0);
    OK(k2hip_long_result_destroy(r));
    OK(k2hip_offline_recognize_long(m, 8000, x.data(), 8000 * 6, &c, 8, 4000, &r));
    CHECK(k2hip_long_result_num_segments(r) >= 1);
    OK(k2hip_long_result_destroy(r));
    CHECK(k2hip_offline_recognize_long(m, 16000, x.data(), (int64_t)x.size(), &c, 0, 4000, &r) == K2HIP_ERR_INVALID && r == nullptr);
    CHECK(k2hip_offline_recognize_long(m, 16000, x.data(), (int64_t)x.size(), &c, 8, 0, &r) == K2HIP_ERR_INVALID);
    CHECK(k2hip_offline_recognize_long(m, 16001, x.data(), (int64_t)x.size(), &c, 8, 4000, &r) == K2HIP_ERR_UNSUPPORTED);
    CHECK(k2hip_offline_recognize_long(m, 16000, x.data(), ((int64_t)1 << 27) + 1, &c, 8, 4000, &r) == K2HIP_ERR_UNSUPPORTED && strstr(k2hip_last_error(), "limit"));
    CHECK(k2hip_offline_recognize_long(m, 16000, x.data(), -1, &c, 8, 4000, &r) == K2HIP_ERR_INVALID);
    CHECK(k2hip_offline_recognize_long(m, 16000, x.data(), 10, &c, 8, 4000, nullptr) == K2HIP_ERR_INVALID);
    CHECK(k2hip_long_result_num_segments(nullptr) == -1);
    OK(k2hip_long_result_destroy(nullptr));
    // the packing rule's own refusals and a hand-made list: a segment longer than max_batch_frames is a batch of one
    const int64_t len[5] = {100, 200, 50, 400, 30}, big[3] = {700, 10, 10};
    int32_t b5[5], b3[3];
    OK(k2hip_debug_vad_pack(len, 5, 3, 600, b5));
    CHECK(b5[0] == 0 && b5[1] == 0 && b5[2] == 0 && b5[3] == 1 && b5[4] == 2);
    OK(k2hip_debug_vad_pack(big, 3, 8, 600, b3));
    CHECK(b3[0] == 0 && b3[1] == 1 && b3[2] == 1);
    CHECK(k2hip_debug_vad_pack(len, 5, 0, 600, b5) == K2HIP_ERR_INVALID && k2hip_debug_vad_pack(len, 5, 3, 0, b5) == K2HIP_ERR_INVALID);
    OK(k2hip_debug_vad_pack(nullptr, 0, 3, 600, nullptr));
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: san_vad_driver <offline.k2w>\n");
        return 2;
    }
    reference();
    k2hip_model_t* m = nullptr;
    OK(k2hip_model_create(argv[1], nullptr, 0, &m));
    config_refusals(m);
    streams(m);
    life_cycle(m);
    long_entry(m);
    OK(k2hip_model_destroy(m));
    printf("san_vad_driver ok\n");
    return 0;
}
