// AddressSanitizer / UBSan driver of the sample-rate converter's host side: the plan builder (csrc/resample_plan.cpp), the header-only
// float32 reference (csrc/resample_ref.h) and the stream bookkeeping of the accept_waveform entries (csrc/api.cpp) through the C ABI
// over the CPU stand-ins of the engine (engine_stub*.cpp; engine_stub_resample.cpp runs the reference where the engine launches the
// kernel).  TEST INFRASTRUCTURE: its own program (`make -C k2transducerasr_amd/csrc san_resample`, tests/test_resample_sanitizers.py),
// never loaded into another process.
// Exercised: plans of random rate pairs against the window's integer definition tap by tap and num_out against a count from the tap
// ranges, every refusal with its code; the reference over random chunkings against one push bit for bit, its carried block and the
// hook's capacity rule; then the streams: SpeechLength after every push, the frames after get_speech and after a search (the queue
// erase), the rate rules with their messages, a refused rate, reset, IsFinished's zeros, the batch entry, k2hip_resample.
//   san_resample_driver <offline.k2w> <streaming.k2w>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../include/k2hip.h"
#include "../../include/k2hip_debug.h"
#include "../../k2transducerasr_amd/csrc/resample_plan.h"
#include "../../k2transducerasr_amd/csrc/resample_ref.h"
#include "../../k2transducerasr_amd/csrc/errors.h"

#define CHECK(cond)                                                                                                          \
    do {                                                                                                                     \
        if (!(cond)) {                                                                                                       \
            fprintf(stderr, "CHECK failed at %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, k2hip_last_error()); \
            exit(3);                                                                                                         \
        }                                                                                                                    \
    } while (0)
#define OK(call) CHECK((call) == K2HIP_OK)

namespace {

using k2hip::ResamplePlan;
using k2hip::ResampleRefState;

unsigned long long rng_state = 88172645463325252ull;
unsigned rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 32);
}
float rndf() { return (float)(rnd() >> 8) * (1.0f / 8388608.0f) - 1.0f; }
std::vector<float> signal(size_t n) {
    std::vector<float> x(n);
    for (auto& v : x) v = rndf();
    return x;
}
bool same_bits(const float* a, const float* b, size_t n) { return n == 0 || memcmp(a, b, n * sizeof(float)) == 0; }

int plan_code(int fi, int fo) {
    try {
        k2hip::resample_plan(fi, fo);
        return K2HIP_OK;
    } catch (const k2hip::Error& e) {
        return e.code;
    }
}

void plans() {
    const int rates[] = {8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 96000, 7, 3, 1000, 15999};
    int built = 0;
    for (int fi : rates)
        for (int fo : rates) {
            if (fi == fo) continue;
            if (plan_code(fi, fo) != K2HIP_OK) {
                CHECK(plan_code(fi, fo) == K2HIP_ERR_UNSUPPORTED);
                continue;
            }
            const ResamplePlan p = k2hip::resample_plan(fi, fo);
            built++;
            const long long g = std::gcd(fi, fo), iu = fi / g, ou = fo / g, lcm = (long long)fi * ou, lo = fi < fo ? fi : fo;
            CHECK(p.iu == iu && p.ou == ou && (long long)p.w.size() == ou * p.max_taps && ou * p.max_taps <= k2hip::kResampleMaxTable &&
                  p.max_taps <= k2hip::kResampleMaxTaps);
            auto inside = [&](long long ticks) { return (ticks < 0 ? -ticks : ticks) * 99 * lo < 600 * lcm; };
            int mt = 0;
            for (long long ph = 0; ph < ou; ph++) {
                const long long f = p.first[(size_t)ph], n = p.ntaps[(size_t)ph];
                CHECK(n >= 1 && !inside((f - 1) * ou - ph * iu) && !inside((f + n) * ou - ph * iu));
                for (long long j = f; j < f + n; j++) CHECK(inside(j * ou - ph * iu));
                for (int j = (int)n; j < p.max_taps; j++) CHECK(p.w[(size_t)(ph * p.max_taps + j)] == 0.f);
                for (int j = 0; j < (int)n; j++) CHECK(std::isfinite(p.w[(size_t)(ph * p.max_taps + j)]));
                mt = mt > (int)n ? mt : (int)n;
            }
            CHECK(mt == p.max_taps);
            // num_out(n) = outputs whose last tap lies below n; ends never decrease
            long long k = 0;
            for (long long n = 0; n <= 700; n++) {
                while (p.end(k) <= n) {
                    CHECK(p.end(k + 1) >= p.end(k) && p.start(k + 1) >= p.start(k));
                    k++;
                }
                CHECK(p.num_out(n) == k);
                CHECK(p.keep_from(k) <= n || k == 0 || p.keep_from(k) <= p.end(k - 1));
            }
        }
    CHECK(built > 100);
    CHECK(plan_code(0, 16000) == K2HIP_ERR_INVALID && plan_code(16000, 0) == K2HIP_ERR_INVALID && plan_code(-1, 16000) == K2HIP_ERR_INVALID);
    CHECK(plan_code(16001, 16000) == K2HIP_ERR_UNSUPPORTED && plan_code(16000, 500) == K2HIP_ERR_UNSUPPORTED);
    CHECK(plan_code(1 << 25, 16000) == K2HIP_ERR_UNSUPPORTED && plan_code(16777213, 16777199) == K2HIP_ERR_UNSUPPORTED);
    int32_t iu = 0, ou = 0, mt = 0;
    CHECK(k2hip_debug_resample_plan(16001, 16000, &iu, &ou, &mt, nullptr, nullptr, nullptr, 0, 0) == K2HIP_ERR_UNSUPPORTED);
    CHECK(strstr(k2hip_last_error(), "16001") && strstr(k2hip_last_error(), "16000"));
    OK(k2hip_debug_resample_plan(44100, 16000, &iu, &ou, &mt, nullptr, nullptr, nullptr, 0, 0));
    CHECK(iu == 441 && ou == 160 && mt == 34);
    std::vector<int32_t> first(160), ntaps(160);
    std::vector<float> w(160 * 34);
    CHECK(k2hip_debug_resample_plan(44100, 16000, &iu, &ou, &mt, first.data(), ntaps.data(), w.data(), 159, 160 * 34) == K2HIP_ERR_CAPACITY);
    CHECK(k2hip_debug_resample_plan(44100, 16000, &iu, &ou, &mt, first.data(), ntaps.data(), w.data(), 160, 160 * 34 - 1) == K2HIP_ERR_CAPACITY);
    OK(k2hip_debug_resample_plan(44100, 16000, &iu, &ou, &mt, first.data(), ntaps.data(), w.data(), 160, 160 * 34));
    CHECK(k2hip_debug_resample_num_out(48000, 16000, 19) == 1 && k2hip_debug_resample_num_out(48000, 16000, 18) == 0 &&
          k2hip_debug_resample_num_out(48000, 16000, -1) == -1);
}

void reference() {
    const int pairs[][2] = {{8000, 16000}, {11025, 16000}, {44100, 16000}, {48000, 16000}, {16000, 8000}, {7, 3}, {3, 7}, {22050, 16000}};
    for (const auto& pr : pairs) {
        const ResamplePlan p = k2hip::resample_plan(pr[0], pr[1]);
        const std::vector<float> x = signal(1500 + rnd() % 1500);
        ResampleRefState whole;
        std::vector<float> y;
        k2hip::resample_ref_push(p, whole, x.data(), (int64_t)x.size(), &y);
        CHECK((int64_t)y.size() == p.num_out((int64_t)x.size()) && whole.n_out == (int64_t)y.size());
        for (int trial = 0; trial < 6; trial++) {
            ResampleRefState st;
            std::vector<float> got;
            size_t pos = 0;
            while (pos < x.size()) {
                size_t n = trial == 0 ? 1 : trial == 1 ? (size_t)p.iu : trial == 2 ? (size_t)p.iu + 1 : 1 + rnd() % (trial == 3 ? 5 : 400);
                n = n < x.size() - pos ? n : x.size() - pos;
                std::vector<float> piece(x.begin() + (long)pos, x.begin() + (long)(pos + n));   // (exact size: an over-read is seen)
                k2hip::resample_ref_push(p, st, piece.data(), (int64_t)n, &got);
                pos += n;
                CHECK(st.n_in == (int64_t)pos && st.n_out == p.num_out((int64_t)pos) && (int64_t)got.size() == st.n_out);
                CHECK((int64_t)st.tail.size() == st.n_in - (p.keep_from(st.n_out) < st.n_in ? p.keep_from(st.n_out) : st.n_in));
                CHECK((int)st.tail.size() <= p.max_taps + p.iu);
            }
            CHECK(got.size() == y.size() && same_bits(got.data(), y.data(), y.size()));
        }
    }
    // the hook: its carried block in the caller's hands, its capacity rule, a block that does not belong to its counts
    std::vector<float> x = signal(3000), tail(512), out(2000);
    int64_t n_tail = 0, n_in = 0, n_out = 0, got = 0;
    OK(k2hip_debug_resample_ref(48000, 16000, tail.data(), &n_tail, 512, &n_in, &n_out, x.data(), 1000, out.data(), 2000, &got));
    CHECK(got == k2hip_debug_resample_num_out(48000, 16000, 1000) && n_in == 1000 && n_out == got && n_tail > 0 && n_tail <= 40);
    int64_t t2 = n_tail, i2 = n_in, o2 = n_out;
    CHECK(k2hip_debug_resample_ref(48000, 16000, tail.data(), &t2, 512, &i2, &o2, x.data() + 1000, 2000, out.data(), 10, &got) == K2HIP_ERR_CAPACITY);
    CHECK(t2 == n_tail && i2 == n_in && o2 == n_out);   // (a refused push changes nothing)
    o2 = n_out + 1;
    CHECK(k2hip_debug_resample_ref(48000, 16000, tail.data(), &t2, 512, &i2, &o2, x.data() + 1000, 10, out.data(), 2000, &got) == K2HIP_ERR_INVALID);
    OK(k2hip_debug_resample_ref(48000, 16000, tail.data(), &n_tail, 512, &n_in, &n_out, x.data() + 1000, 2000, out.data(), 2000, &got));
    CHECK(n_in == 3000 && n_out == k2hip_debug_resample_num_out(48000, 16000, 3000));
}

// what a stream fed x at rate fi must hold: the stand-in's frame t is y[160 t] * 0.5 + c over the reference's output y
std::vector<float> ref_all(int fi, int fo, const std::vector<float>& x) {
    const ResamplePlan p = k2hip::resample_plan(fi, fo);
    ResampleRefState st;
    std::vector<float> y;
    k2hip::resample_ref_push(p, st, x.data(), (int64_t)x.size(), &y);
    return y;
}
void check_frames(const std::vector<float>& speech, const std::vector<float>& y, int64_t frame0, int feat) {
    CHECK(speech.size() % (size_t)feat == 0);
    for (size_t t = 0; t < speech.size() / (size_t)feat; t++)
        for (int c = 0; c < feat; c += 17) CHECK(speech[t * (size_t)feat + c] == y[(size_t)(frame0 + (int64_t)t) * 160] * 0.5f + (float)c);
}

void offline(const char* path) {
    k2hip_model_t* m = nullptr;
    OK(k2hip_model_create(path, nullptr, 0, &m));
    k2hip_model_info info;
    OK(k2hip_model_get_info(m, &info));
    const int feat = info.feature_dim;
    CHECK(info.sample_rate == 16000);
    int32_t np = -1;
    // the one-call entries
    const std::vector<float> x = signal(20000);
    CHECK(k2hip_resample_num_out(m, 16000, 777) == 777 && k2hip_resample_num_out(m, 0, 5) == -1 && k2hip_resample_num_out(m, 16001, 5) == -1);
    OK(k2hip_debug_resample_plans(m, &np));
    CHECK(np == 0);
    for (int fi : {8000, 44100, 48000}) {
        const std::vector<float> y = ref_all(fi, 16000, x);
        CHECK(k2hip_resample_num_out(m, fi, (int64_t)x.size()) == (int64_t)y.size());
        std::vector<float> out(y.size());
        int64_t n = -1;
        CHECK(k2hip_resample(m, fi, x.data(), (int64_t)x.size(), out.data(), (int64_t)y.size() - 1, &n) == K2HIP_ERR_CAPACITY && n == (int64_t)y.size());
        OK(k2hip_resample(m, fi, x.data(), (int64_t)x.size(), out.data(), (int64_t)y.size(), &n));
        CHECK(n == (int64_t)y.size() && same_bits(out.data(), y.data(), y.size()));
        OK(k2hip_resample(m, fi, x.data(), 3, out.data(), 0, &n));   // shorter than the window: nothing
        CHECK(n == 0);
    }
    OK(k2hip_debug_resample_plans(m, &np));
    CHECK(np == 3);
    {
        std::vector<float> out(100);
        int64_t n = -1;
        OK(k2hip_resample(m, 16000, x.data(), 100, out.data(), 100, &n));
        CHECK(n == 100 && same_bits(out.data(), x.data(), 100));
    }
    // streams: counts after every push, the frames, the erase behind a materialisation and behind a search
    for (int fi : {8000, 44100, 48000}) {
        const std::vector<float> y = ref_all(fi, 16000, x);
        k2hip_offline_stream_t* s = nullptr;
        OK(k2hip_offline_stream_create(m, &s));
        size_t pos = 0;
        int64_t frames_done = 0;
        int round = 0;
        while (pos < x.size()) {
            size_t n = 1 + rnd() % 3000;
            n = n < x.size() - pos ? n : x.size() - pos;
            std::vector<float> piece(x.begin() + (long)pos, x.begin() + (long)(pos + n));
            OK(k2hip_offline_stream_accept_waveform(s, fi, piece.data(), (int64_t)n));
            pos += n;
            const int64_t due = k2hip_resample_num_out(m, fi, (int64_t)pos) - frames_done * 160;
            const int64_t nf = k2hip_fbank_num_frames(m, due);
            if (round % 3 == 2 && nf > 0 && fi == 8000) {   // a search takes the queue (the stand-in reads both ends of it)
                CHECK(k2hip_offline_stream_speech_length(s) == nf * feat);
                OK(k2hip_offline_recognizer_get_results(m, &s, 1));
                CHECK(k2hip_offline_stream_speech_length(s) == 0);
                frames_done += nf;
            } else if (round % 3 == 1) {                    // the frames are materialised
                std::vector<float> sp((size_t)(nf * feat) + 1, -1.f);
                CHECK(k2hip_offline_stream_speech_length(s) == nf * feat);
                if (nf > 0) CHECK(k2hip_offline_stream_get_speech(s, sp.data(), nf * feat - 1) == K2HIP_ERR_CAPACITY);
                OK(k2hip_offline_stream_get_speech(s, sp.data(), nf * feat));
                CHECK(sp.back() == -1.f);
                sp.pop_back();
                check_frames(sp, y, frames_done, feat);
                // Speech stays with the stream; start over with a fresh one fed the same input so far, minus nothing: the counts go on
                OK(k2hip_offline_stream_destroy(s));
                OK(k2hip_offline_stream_create(m, &s));
                std::vector<float> again(x.begin(), x.begin() + (long)pos);
                OK(k2hip_offline_stream_accept_waveform(s, fi, again.data(), (int64_t)pos));
                frames_done = 0;
            } else {
                CHECK(k2hip_offline_stream_speech_length(s) == (nf > 0 ? nf : 0) * feat);
            }
            round++;
        }
        // two materialisations in a row on one stream: the second sees only what the first left queued
        std::vector<float> sp((size_t)k2hip_offline_stream_speech_length(s));
        OK(k2hip_offline_stream_get_speech(s, sp.data(), (int64_t)sp.size()));
        check_frames(sp, y, frames_done, feat);
        const std::vector<float> more = signal(5000);
        std::vector<float> xx(x);
        xx.insert(xx.end(), more.begin(), more.end());
        const std::vector<float> yy = ref_all(fi, 16000, xx);
        OK(k2hip_offline_stream_accept_waveform(s, fi, more.data(), (int64_t)more.size()));
        std::vector<float> sp2((size_t)k2hip_offline_stream_speech_length(s));
        OK(k2hip_offline_stream_get_speech(s, sp2.data(), (int64_t)sp2.size()));
        CHECK(sp2.size() > sp.size() && (int64_t)(sp2.size() / (size_t)feat) == k2hip_fbank_num_frames(m, (int64_t)yy.size() - frames_done * 160));
        check_frames(sp2, yy, frames_done, feat);
        // the rules
        CHECK(k2hip_offline_stream_accept_samples(s, x.data(), 10) == K2HIP_ERR_INVALID);
        CHECK(strstr(k2hip_last_error(), "16000") != nullptr);
        CHECK(k2hip_offline_stream_accept_waveform(s, fi == 8000 ? 48000 : 8000, x.data(), 10) == K2HIP_ERR_INVALID);
        CHECK(strstr(k2hip_last_error(), fi == 8000 ? "8000 Hz" : fi == 44100 ? "44100 Hz" : "48000 Hz") != nullptr);
        CHECK(k2hip_offline_stream_accept_waveform(s, fi, nullptr, 10) == K2HIP_ERR_INVALID);
        OK(k2hip_offline_stream_accept_waveform(s, fi, nullptr, 0));
        OK(k2hip_offline_stream_destroy(s));
    }
    {   // the model's own rate is accept_samples; a refused rate leaves the stream free; a batch that mixes rates
        k2hip_offline_stream_t *a = nullptr, *b = nullptr, *c = nullptr;
        OK(k2hip_offline_stream_create(m, &a));
        OK(k2hip_offline_stream_create(m, &b));
        OK(k2hip_offline_stream_create(m, &c));
        CHECK(k2hip_offline_stream_accept_waveform(a, 16001, x.data(), 100) == K2HIP_ERR_UNSUPPORTED);
        CHECK(k2hip_offline_stream_accept_waveform(a, 0, x.data(), 100) == K2HIP_ERR_INVALID);
        OK(k2hip_offline_stream_accept_waveform(a, 16000, x.data(), 6000));
        OK(k2hip_offline_stream_accept_samples(b, x.data(), 6000));
        CHECK(k2hip_offline_stream_speech_length(a) == k2hip_offline_stream_speech_length(b));
        std::vector<float> sa((size_t)k2hip_offline_stream_speech_length(a)), sb(sa.size());
        OK(k2hip_offline_stream_get_speech(a, sa.data(), (int64_t)sa.size()));
        OK(k2hip_offline_stream_get_speech(b, sb.data(), (int64_t)sb.size()));
        CHECK(same_bits(sa.data(), sb.data(), sa.size()));
        CHECK(k2hip_offline_stream_accept_waveform(a, 8000, x.data(), 10) == K2HIP_ERR_INVALID);
        OK(k2hip_offline_stream_accept_samples(a, x.data(), 10));
        OK(k2hip_offline_stream_accept_waveform(c, 8000, x.data(), 4000));
        OK(k2hip_offline_stream_destroy(a));
        OK(k2hip_offline_stream_destroy(b));
        OK(k2hip_offline_stream_create(m, &a));
        OK(k2hip_offline_stream_accept_samples(a, x.data(), 7000));
        k2hip_offline_stream_t* both[2] = {a, c};
        OK(k2hip_offline_recognizer_get_results(m, both, 2));
        CHECK(k2hip_offline_stream_speech_length(a) == 0 && k2hip_offline_stream_speech_length(c) == 0);
        OK(k2hip_offline_stream_accept_waveform(c, 8000, x.data() + 4000, 4000));
        const int64_t used = k2hip_fbank_num_frames(m, k2hip_resample_num_out(m, 8000, 4000)) * 160;
        CHECK(k2hip_offline_stream_speech_length(c) == k2hip_fbank_num_frames(m, k2hip_resample_num_out(m, 8000, 8000) - used) * feat);
        OK(k2hip_offline_recognizer_get_result(m, c));
        OK(k2hip_offline_stream_destroy(a));
        OK(k2hip_offline_stream_destroy(c));
    }
    OK(k2hip_debug_resample_plans(m, &np));
    CHECK(np == 3);
    OK(k2hip_model_destroy(m));
}

void online(const char* path) {
    k2hip_model_t* m = nullptr;
    OK(k2hip_model_create(path, nullptr, 0, &m));
    k2hip_model_info info;
    OK(k2hip_model_get_info(m, &info));
    const int feat = info.feature_dim;
    const std::vector<float> x = signal(30000);
    for (int fi : {8000, 11025, 48000}) {
        const std::vector<float> y = ref_all(fi, 16000, x);
        k2hip_online_stream_t* s = nullptr;
        OK(k2hip_online_stream_create(m, &s));
        size_t pos = 0;
        int round = 0;
        while (pos < x.size()) {
            size_t n = round < 30 ? 1 + rnd() % 4 : 1 + rnd() % 2500;
            n = n < x.size() - pos ? n : x.size() - pos;
            std::vector<float> piece(x.begin() + (long)pos, x.begin() + (long)(pos + n));
            OK(k2hip_online_stream_accept_waveform(s, fi, piece.data(), (int64_t)n));
            pos += n;
            const int64_t nf = k2hip_fbank_num_frames(m, k2hip_resample_num_out(m, fi, (int64_t)pos));
            CHECK(k2hip_online_stream_speech_length(s) == (nf > 0 ? nf : 0) * feat);
            if (round % 4 == 0) {
                std::vector<float> sp((size_t)k2hip_online_stream_speech_length(s));
                OK(k2hip_online_stream_get_speech(s, sp.data(), (int64_t)sp.size()));
                check_frames(sp, y, 0, feat);
                CHECK(k2hip_online_stream_speech_length(s) == (int64_t)sp.size());
            }
            round++;
        }
        CHECK(k2hip_online_stream_accept_samples(s, x.data(), 10) == K2HIP_ERR_INVALID);
        CHECK(k2hip_online_stream_accept_waveform(s, fi + 1, x.data(), 10) == K2HIP_ERR_INVALID);
        OK(k2hip_online_stream_reset(s));
        CHECK(k2hip_online_stream_speech_length(s) == 0);
        OK(k2hip_online_stream_accept_samples(s, x.data(), 4000));   // the rate went with the reset
        CHECK(k2hip_online_stream_speech_length(s) == k2hip_fbank_num_frames(m, 4000) * feat);
        CHECK(k2hip_online_stream_accept_waveform(s, fi, x.data(), 10) == K2HIP_ERR_INVALID);
        OK(k2hip_online_stream_reset(s));
        // IsFinished's 400 zero samples enter at the stream's rate: ceil(400 iu / ou) of them
        OK(k2hip_online_stream_accept_waveform(s, fi, x.data(), fi / 10));
        const int64_t before = k2hip_online_stream_speech_length(s);
        int32_t fin = -1;
        OK(k2hip_online_stream_is_finished(s, 1, &fin));
        const int64_t g = std::gcd(fi, 16000), zeros = (400 * (int64_t)(fi / g) + 16000 / g - 1) / (16000 / g);
        CHECK(fin == 0 && before > 0);
        CHECK(k2hip_online_stream_speech_length(s) == k2hip_fbank_num_frames(m, k2hip_resample_num_out(m, fi, fi / 10 + zeros)) * feat);
        OK(k2hip_online_stream_destroy(s));
    }
    {   // the batch entry, a mix of rates in one step's materialisation, a refused rate
        k2hip_online_stream_t* ss[3] = {nullptr, nullptr, nullptr};
        for (auto& s : ss) OK(k2hip_online_stream_create(m, &s));
        const float* ptr[2] = {x.data(), x.data() + 100};
        const int64_t n[2] = {30000, 29000};
        OK(k2hip_online_accept_waveform_batch(m, ss, 2, 44100, ptr, n));
        OK(k2hip_online_stream_accept_waveform(ss[2], 8000, x.data(), 9000));
        const float* ptr3[3] = {x.data(), x.data(), x.data()};
        const int64_t n3[3] = {10, 10, 10};
        CHECK(k2hip_online_accept_waveform_batch(m, ss, 3, 44100, ptr3, n3) == K2HIP_ERR_INVALID);
        int32_t dec[3], nn[3];
        const int64_t len0 = k2hip_online_stream_speech_length(ss[0]);
        CHECK(len0 == k2hip_fbank_num_frames(m, k2hip_resample_num_out(m, 44100, 30000)) * feat);   // (the refused batch call added nothing)
        OK(k2hip_online_step(m, ss, 3, dec, nn));
        CHECK(dec[0] == 1 && dec[1] == 1 && dec[2] == 1);
        CHECK(k2hip_online_stream_accept_waveform(ss[0], 16001, x.data(), 1) == K2HIP_ERR_INVALID);   // (its rate is fixed: 44100)
        k2hip_online_stream_t* f = nullptr;
        OK(k2hip_online_stream_create(m, &f));
        CHECK(k2hip_online_stream_accept_waveform(f, 16001, x.data(), 1) == K2HIP_ERR_UNSUPPORTED);
        OK(k2hip_online_stream_accept_waveform(f, 16000, x.data(), 3000));
        OK(k2hip_online_stream_accept_samples(f, x.data(), 3000));
        CHECK(k2hip_online_stream_speech_length(f) == k2hip_fbank_num_frames(m, 6000) * feat);
        OK(k2hip_online_stream_destroy(f));
        for (auto& s : ss) OK(k2hip_online_stream_destroy(s));
    }
    OK(k2hip_model_destroy(m));
}

}  // namespace

int main(int argc, char** argv) {
    plans();
    reference();
    if (argc >= 3) {
        offline(argv[1]);
        online(argv[2]);
    } else {
        fprintf(stderr, "san_resample_driver: no model files given, the ABI part is skipped\n");
    }
    printf("san_resample_driver ok\n");
    return 0;
}
