// AddressSanitizer / UBSan driver of the CTC forced alignment's host side: the header-only reference of the trellis recursions
// (csrc/ctc_lattice_ref.h) and the argument checks of k2hip_ctc_align / k2hip_offline_ctc_align_from_samples (csrc/api.cpp) over the CPU
// stand-ins of the engine (engine_stub*.cpp).  TEST INFRASTRUCTURE: its own program (`make -C k2transducerasr_amd/csrc san_ctc_align`,
// tests/test_ctc_align.py), never loaded into another process.
// Exercised: random log_probs with -inf cells against brute-force enumeration of every frame labelling that collapses to the target
// (V = 3, T <= 6, every target up to length 3, repeats included: U = 0, T = 1, targets that need exactly T frames), the three tie rules;
// then, through both entries: blank and out-of-range ids, a target one frame too long, a bad stream_of, a bad n_frames, lens >
// max_tokens (nothing written), a transducer model, NULL outputs, and a valid call after every refused one.
//   san_ctc_align_driver <ctc.k2w> <offline.k2w>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/k2hip.h"
#include "../../k2transducerasr_amd/csrc/ctc_lattice_ref.h"

#define CHECK(cond)                                                                                                          \
    do {                                                                                                                     \
        if (!(cond)) {                                                                                                       \
            fprintf(stderr, "CHECK failed at %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, k2hip_last_error()); \
            exit(3);                                                                                                         \
        }                                                                                                                    \
    } while (0)
#define OK(call) CHECK((call) == K2HIP_OK)

namespace {

using k2hip::ctc_lattice_ref;
using k2hip::CtcLatticeRefResult;

unsigned long long rng_state = 88172645463325252ull;
unsigned rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 32);
}

constexpr int V = 3;

// every labelling of the T frames over V symbols that collapses (merge repeats, drop blanks) to y, in double
void brute(const std::vector<float>& lp, const std::vector<int64_t>& y, int T, double* total, double* best) {
    double sum = 0, mx = -INFINITY;
    bool any = false;
    int n = 1;
    for (int t = 0; t < T; t++) n *= V;
    for (int code = 0; code < n; code++) {
        std::vector<int64_t> got;
        double s = 0;
        int64_t prev = -1;
        for (int t = 0, c = code; t < T; t++, c /= V) {
            const int64_t v = c % V;
            s += lp[(size_t)t * V + (size_t)v];
            if (v != 0 && v != prev) got.push_back(v);
            prev = v;
        }
        if (got != y || s == -INFINITY) continue;
        if (!any || s > mx) { sum = sum * (any ? std::exp(mx - s) : 0.0) + 1.0; mx = s; any = true; }
        else sum += std::exp(s - mx);
    }
    *total = any ? mx + std::log(sum) : -INFINITY;
    *best = mx;
}

void check_case(const std::vector<int64_t>& y, int T, int inf_per_16) {
    const int U = (int)y.size();
    std::vector<float> lp((size_t)T * V);
    for (float& x : lp) x = (int)(rnd() % 16) < inf_per_16 ? -INFINITY : -0.25f * (float)(rnd() % 24);
    const CtcLatticeRefResult r = ctc_lattice_ref(lp.data(), V, y.data(), T, U);
    double total, best;
    brute(lp, y, T, &total, &best);
    CHECK(!std::isnan(r.total) && !std::isnan(r.best));
    CHECK((double)r.best == best);   // multiples of 0.25: sums are exact in float32
    if (total == -INFINITY) CHECK(r.total == -INFINITY);
    else CHECK(std::fabs((double)r.total - total) <= 1e-5 * std::fmax(1.0, std::fabs(total)));
    CHECK((int)r.timestamps.size() == U && (int)r.end_frames.size() == U && (int)r.token_log_probs.size() == U);
    for (int u = 0; u < U; u++) CHECK(r.timestamps[(size_t)u] >= 0 && r.end_frames[(size_t)u] < T);
    if (best == -INFINITY) return;
    // the labelling the two frame lists describe collapses to y and scores `best`
    std::vector<int64_t> lab((size_t)T, 0);
    for (int u = 0; u < U; u++) {
        CHECK(r.timestamps[(size_t)u] <= r.end_frames[(size_t)u]);
        if (u + 1 < U) CHECK(r.end_frames[(size_t)u] < r.timestamps[(size_t)u + 1]);
        if (u + 1 < U && y[(size_t)u] == y[(size_t)u + 1]) CHECK(r.end_frames[(size_t)u] + 1 < r.timestamps[(size_t)u + 1]);
        for (int t = r.timestamps[(size_t)u]; t <= r.end_frames[(size_t)u]; t++) lab[(size_t)t] = y[(size_t)u];
        CHECK(r.token_log_probs[(size_t)u] == lp[(size_t)r.timestamps[(size_t)u] * V + (size_t)y[(size_t)u]]);
    }
    double path = 0;
    for (int t = 0; t < T; t++) path += lp[(size_t)t * V + (size_t)lab[(size_t)t]];
    CHECK(path == best);
}

void reference() {
    std::vector<std::vector<int64_t>> targets = {{}};
    for (int len = 1; len <= 3; len++) {
        int n = 1;
        for (int k = 0; k < len; k++) n *= 2;
        for (int code = 0; code < n; code++) {
            std::vector<int64_t> y;
            for (int k = 0; k < len; k++) y.push_back(1 + (code >> k & 1));
            targets.push_back(y);
        }
    }
    int exact_fit = 0;
    for (int T = 1; T <= 6; T++)
        for (const auto& y : targets) {
            const int need = k2hip::ctc_min_frames(y.data(), (int)y.size());
            if (need > T) continue;
            exact_fit += need == T && need > (int)y.size();
            for (int inf : {0, 0, 2, 6, 16}) check_case(y, T, inf);
        }
    CHECK(exact_fit > 0);
    // the tie rules, on multiples of 0.25 (lp rows are [blank, a, b]).
    // s-2 against s-1: T = 3, y = a b.
    {
        // frame 0: a = 0; frame 1: a = -0.5, blank = -0.5, b = -1; frame 2: b = 0.  Into state 3 (b) at frame 2: from s-2 = state 1 (a a: -0.5)
        // and from s-1 = state 2 (a -: -0.5) tie; s-2 wins, so a lasts through frame 1
        const float lp[9] = {-4.f, 0.f, -4.f, -0.5f, -0.5f, -1.f, -4.f, -4.f, 0.f};
        const int64_t y[2] = {1, 2};
        const CtcLatticeRefResult r = ctc_lattice_ref(lp, 3, y, 3, 2);
        CHECK(r.best == -0.5f && r.timestamps[0] == 0 && r.end_frames[0] == 1 && r.timestamps[1] == 2);
    }
    {
        // s-1 against s: T = 2, y = a.  Into state 1 (a) at frame 1: from s-1 = state 0 (blank at 0: -0.25) and from s = state 1 (a at 0: -0.25)
        // tie; s-1 wins, so a starts at frame 1.  (The final state S-2 = a; ending in S-1 = blank would cost -4.)
        const float lp[6] = {-0.25f, -0.25f, -4.f, -4.f, -0.5f, -4.f};
        const int64_t y[1] = {1};
        const CtcLatticeRefResult r = ctc_lattice_ref(lp, 3, y, 2, 1);
        CHECK(r.best == -0.75f && r.timestamps[0] == 1 && r.end_frames[0] == 1 && r.token_log_probs[0] == -0.5f);
    }
    {
        // the end: T = 2, y = a.  (a a) ends in S-2 with -0.5, (a -) ends in S-1 with -0.5: S-2 wins, a lasts through frame 1; (- a) is
        // blocked by a -inf cell, so total = -0.5 + log 2
        const float lp[6] = {-INFINITY, -0.25f, -4.f, -0.25f, -0.25f, -4.f};
        const int64_t y[1] = {1};
        const CtcLatticeRefResult r = ctc_lattice_ref(lp, 3, y, 2, 1);
        CHECK(r.best == -0.5f && r.timestamps[0] == 0 && r.end_frames[0] == 1);
        CHECK(std::fabs(r.total - (-0.5f + std::log(2.0f))) < 1e-6f);
    }
}

void abi(const char* ctc_path, const char* transducer_path) {
    k2hip_model_t* m = nullptr;
    OK(k2hip_model_create(ctc_path, nullptr, 0, &m));
    k2hip_model_info info;
    OK(k2hip_model_get_info(m, &info));
    const int Vm = info.vocab_size;
    const int R = 2, Tp = 5, H = 3, mt = 4;
    std::vector<float> lp((size_t)R * Tp * Vm);
    for (float& x : lp) x = -0.25f * (float)(1 + rnd() % 12);
    std::vector<int64_t> ids = {3, 3, 4, 5, 6, 7};   // targets: (3 3 4) needs 4 frames, (5) and (6 7)
    int32_t lens[3] = {3, 1, 2}, nf[2] = {5, 2}, so[3] = {0, 1, 0};
    std::vector<int32_t> ts((size_t)H * mt, -7), en((size_t)H * mt, -7);
    std::vector<float> yp((size_t)H * mt, -7.f), tot(H, -7.f), best(H, -7.f);
    auto untouched = [&] { return ts[0] == -7 && ts[mt] == -7 && en[0] == -7 && yp[0] == -7.f && tot[0] == -7.f && best[2] == -7.f; };
    auto wipe = [&] {
        std::fill(ts.begin(), ts.end(), -7); std::fill(en.begin(), en.end(), -7); std::fill(yp.begin(), yp.end(), -7.f);
        std::fill(tot.begin(), tot.end(), -7.f); std::fill(best.begin(), best.end(), -7.f);
    };
    auto call = [&](const int32_t* n_frames, const int32_t* stream_of, const int64_t* y, const int32_t* l, int max_tokens) {
        return k2hip_ctc_align(m, lp.data(), R, Tp, n_frames, H, stream_of, y, l, ts.data(), en.data(), yp.data(), tot.data(), best.data(), max_tokens);
    };
    auto valid = [&] {
        OK(call(nf, so, ids.data(), lens, mt));
        CHECK(ts[0] <= en[0] && en[0] + 1 < ts[1] && en[1] < ts[2] && en[2] < 5 && ts[3] == -7 && en[mt] < 2 && ts[2 * mt] <= en[2 * mt] &&
              en[2 * mt] < ts[2 * mt + 1] && yp[0] <= 0.f && best[0] <= tot[0] && best[1] <= tot[1] && best[2] <= tot[2]);
        // one target against the host reference
        const CtcLatticeRefResult r = ctc_lattice_ref(lp.data(), Vm, ids.data(), 5, 3);
        CHECK(r.best == best[0] && r.total == tot[0] && r.timestamps[2] == ts[2] && r.end_frames[1] == en[1]);
        wipe();
    };
    valid();
    // a target one frame too long: (3 3 4) needs 4 frames, row 0 gets 3; the message names the target
    int32_t nf3[2] = {3, 2};
    CHECK(call(nf3, so, ids.data(), lens, mt) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "target 0") != nullptr && untouched());
    valid();
    int32_t so_short[3] = {0, 1, 1};   // (6 7) on row 1 with its 2 frames fits exactly; (6 6) would not
    OK(call(nf, so_short, ids.data(), lens, mt));
    CHECK(ts[2 * mt] == 0 && en[2 * mt] == 0 && ts[2 * mt + 1] == 1);
    wipe();
    std::vector<int64_t> rep = ids;
    rep[5] = 6;
    CHECK(call(nf, so_short, rep.data(), lens, mt) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "target 2") != nullptr && untouched());
    valid();
    for (int64_t bad : {(int64_t)K2HIP_BLANK_ID, (int64_t)Vm, (int64_t)-1}) {
        std::vector<int64_t> y = ids;
        y[3] = bad;
        CHECK(call(nf, so, y.data(), lens, mt) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "target 1") != nullptr && untouched());
        valid();
    }
    {   // unk is legal on the CTC path
        std::vector<int64_t> y = ids;
        y[3] = K2HIP_UNK_ID;
        OK(call(nf, so, y.data(), lens, mt));
        wipe();
    }
    for (int32_t bad : {-1, 2}) {
        int32_t so_bad[3] = {0, bad, 0};
        CHECK(call(nf, so_bad, ids.data(), lens, mt) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "stream_of") != nullptr && untouched());
        valid();
    }
    CHECK(call(nf, nullptr, ids.data(), lens, mt) == K2HIP_ERR_INVALID && untouched());   // stream_of NULL needs H == R
    for (int32_t bad : {0, 6}) {
        int32_t nf_bad[2] = {5, bad};
        CHECK(call(nf_bad, so, ids.data(), lens, mt) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "n_frames") != nullptr && untouched());
        valid();
    }
    CHECK(call(nf, so, ids.data(), lens, 2) == K2HIP_ERR_CAPACITY && untouched());   // lens[0] = 3 > max_tokens: nothing written
    valid();
    int32_t lens_neg[3] = {3, -1, 2};
    CHECK(call(nf, so, ids.data(), lens_neg, mt) == K2HIP_ERR_INVALID && untouched());
    CHECK(call(nf, so, ids.data(), nullptr, mt) == K2HIP_ERR_INVALID);
    CHECK(call(nf, so, nullptr, lens, mt) == K2HIP_ERR_INVALID && untouched());
    CHECK(k2hip_ctc_align(nullptr, lp.data(), R, Tp, nf, H, so, ids.data(), lens, ts.data(), en.data(), yp.data(), tot.data(), best.data(), mt) == K2HIP_ERR_INVALID);
    CHECK(k2hip_ctc_align(m, nullptr, R, Tp, nf, H, so, ids.data(), lens, ts.data(), en.data(), yp.data(), tot.data(), best.data(), mt) == K2HIP_ERR_INVALID);
    CHECK(k2hip_ctc_align(m, lp.data(), R, Tp, nf, 0, so, ids.data(), lens, ts.data(), en.data(), yp.data(), tot.data(), best.data(), mt) == K2HIP_ERR_INVALID);
    // every output is optional; n_frames NULL = T'; stream_of NULL = the identity (H == R); U = 0 everywhere needs no ids and max_tokens = 0
    OK(k2hip_ctc_align(m, lp.data(), R, Tp, nullptr, H, so, ids.data(), lens, nullptr, nullptr, nullptr, nullptr, nullptr, mt));
    int32_t lens2[2] = {3, 1};
    OK(k2hip_ctc_align(m, lp.data(), R, Tp, nullptr, R, nullptr, ids.data(), lens2, ts.data(), en.data(), yp.data(), tot.data(), best.data(), mt));
    CHECK(ts[mt] >= 0 && ts[2 * mt] == -7 && best[2] == -7.f);
    wipe();
    int32_t lens0[2] = {0, 0};
    OK(k2hip_ctc_align(m, lp.data(), R, Tp, nullptr, R, nullptr, nullptr, lens0, ts.data(), en.data(), yp.data(), tot.data(), best.data(), 0));
    float blank_sum = 0;
    for (int t = 0; t < Tp; t++) blank_sum += lp[(size_t)t * Vm];
    CHECK(ts[0] == -7 && tot[0] == best[0] && tot[0] == blank_sum);
    wipe();
    {   // the plan's own rule (the launch grid's limit): 65536 empty targets are one too many, and nothing is written
        const int many = 65536;
        std::vector<int32_t> lens_many((size_t)many, 0), so_many((size_t)many, 0);
        CHECK(k2hip_ctc_align(m, lp.data(), R, Tp, nullptr, many, so_many.data(), nullptr, lens_many.data(), ts.data(), en.data(), yp.data(), tot.data(),
                              best.data(), 0) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "at most 65535") != nullptr && untouched());
        valid();
    }
    // the fused entry
    std::vector<float> wav(16000);
    for (size_t i = 0; i < wav.size(); i++) wav[i] = (float)((int)(i * 2654435761u % 2001) - 1000) / 1000.f;
    const float* ptr[2] = {wav.data(), wav.data()};
    int64_t ns[2] = {16000, 12000};
    int32_t Tpo = -7;
    auto fused = [&](const int32_t* stream_of, const int64_t* y, const int32_t* l, int max_tokens) {
        return k2hip_offline_ctc_align_from_samples(m, ptr, ns, R, H, stream_of, y, l, ts.data(), en.data(), yp.data(), tot.data(), best.data(),
                                                    max_tokens, &Tpo);
    };
    auto fused_valid = [&] {
        OK(fused(so, ids.data(), lens, mt));
        CHECK(Tpo > 4 && en[2] < Tpo && ts[0] <= en[0] && en[0] + 1 < ts[1] && best[0] <= tot[0] && ts[3] == -7);
        wipe();
    };
    fused_valid();
    OK(k2hip_offline_ctc_align_from_samples(m, ptr, ns, R, H, so, ids.data(), lens, nullptr, nullptr, nullptr, nullptr, nullptr, mt, nullptr));
    CHECK(fused(so, ids.data(), lens, 2) == K2HIP_ERR_CAPACITY && untouched());
    fused_valid();
    for (int64_t bad : {(int64_t)K2HIP_BLANK_ID, (int64_t)Vm}) {
        std::vector<int64_t> y = ids;
        y[4] = bad;
        CHECK(fused(so, y.data(), lens, mt) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "target 2") != nullptr && untouched());
        fused_valid();
    }
    int32_t so_bad[3] = {0, 2, 0};
    CHECK(fused(so_bad, ids.data(), lens, mt) == K2HIP_ERR_INVALID && untouched());
    fused_valid();
    CHECK(fused(nullptr, ids.data(), lens, mt) == K2HIP_ERR_INVALID && untouched());
    int64_t ns_bad[2] = {16000, 10};
    CHECK(k2hip_offline_ctc_align_from_samples(m, ptr, ns_bad, R, H, so, ids.data(), lens, ts.data(), en.data(), yp.data(), tot.data(), best.data(), mt,
                                               &Tpo) == K2HIP_ERR_INVALID && untouched());
    CHECK(k2hip_offline_ctc_align_from_samples(m, nullptr, ns, R, H, so, ids.data(), lens, ts.data(), en.data(), yp.data(), tot.data(), best.data(), mt,
                                               &Tpo) == K2HIP_ERR_INVALID);
    {   // one frame too long for T' of one second of audio: Tpo + 1 distinct-neighbour tokens
        OK(fused(so, ids.data(), lens, mt));
        wipe();
        const int n = Tpo + 1;
        std::vector<int64_t> many;
        for (int k = 0; k < n; k++) many.push_back(3 + k % 2);
        many.push_back(5); many.push_back(6); many.push_back(7);
        int32_t lens_many[3] = {n, 1, 2};
        std::vector<int32_t> ts_many((size_t)H * n, -7);
        CHECK(k2hip_offline_ctc_align_from_samples(m, ptr, ns, R, H, so, many.data(), lens_many, ts_many.data(), nullptr, nullptr, nullptr, nullptr, n,
                                                   &Tpo) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "target 0") != nullptr && ts_many[0] == -7);
        lens_many[0] = n - 1;   // exactly T' tokens: the single path
        many.erase(many.begin());
        OK(k2hip_offline_ctc_align_from_samples(m, ptr, ns, R, H, so, many.data(), lens_many, ts_many.data(), nullptr, nullptr, tot.data(), best.data(), n, &Tpo));
        CHECK(ts_many[0] == 0 && ts_many[(size_t)n - 2] == n - 2 && tot[0] == best[0]);
        wipe();
    }
    fused_valid();
    valid();
    OK(k2hip_model_destroy(m));
    // a transducer model has no CTC head
    k2hip_model_t* tr = nullptr;
    OK(k2hip_model_create(transducer_path, nullptr, 0, &tr));
    k2hip_model_info ti;
    OK(k2hip_model_get_info(tr, &ti));
    std::vector<float> tlp((size_t)R * Tp * (size_t)ti.vocab_size, -1.f);
    CHECK(k2hip_ctc_align(tr, tlp.data(), R, Tp, nf, H, so, ids.data(), lens, ts.data(), en.data(), yp.data(), tot.data(), best.data(), mt) ==
              K2HIP_ERR_UNSUPPORTED && untouched());
    CHECK(k2hip_offline_ctc_align_from_samples(tr, ptr, ns, R, H, so, ids.data(), lens, ts.data(), en.data(), yp.data(), tot.data(), best.data(), mt,
                                               &Tpo) == K2HIP_ERR_UNSUPPORTED && untouched());
    OK(k2hip_model_destroy(tr));
}

}  // namespace

int main(int argc, char** argv) {
    reference();
    if (argc >= 3) abi(argv[1], argv[2]);
    else fprintf(stderr, "san_ctc_align_driver: no model files given, the ABI part is skipped\n");
    printf("san_ctc_align_driver ok\n");
    return 0;
}
