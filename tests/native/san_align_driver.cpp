// AddressSanitizer / UBSan driver of the forced alignment's host side: the header-only reference of the lattice recursions
// (csrc/lattice_ref.h) and the argument checks of k2hip_transducer_align / k2hip_offline_align_from_samples (csrc/api.cpp) over the CPU
// stand-ins of the engine (engine_stub*.cpp).  TEST INFRASTRUCTURE: its own program (`make -C k2transducerasr_amd/csrc san_align`,
// tests/test_align.py), never loaded into another process.
// Exercised: random planes with -inf cells against brute-force enumeration of every path, U = 0, U = T, T = 1, planes that block every
// path, the tie rule; then U > T, blank / unk / out-of-vocabulary targets, lens > max_tokens (nothing written), NULL outputs, n_frames
// out of range, a CTC model, and a valid call after every refused one.
//   san_align_driver <offline.k2w> <ctc.k2w>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/k2hip.h"
#include "../../k2transducerasr_amd/csrc/lattice_ref.h"

#define CHECK(cond)                                                                                                          \
    do {                                                                                                                     \
        if (!(cond)) {                                                                                                       \
            fprintf(stderr, "CHECK failed at %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, k2hip_last_error()); \
            exit(3);                                                                                                         \
        }                                                                                                                    \
    } while (0)
#define OK(call) CHECK((call) == K2HIP_OK)

namespace {

using k2hip::lattice_dp_ref;
using k2hip::LatticeRefResult;

unsigned long long rng_state = 88172645463325252ull;
unsigned rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 32);
}

// every path (0,0) -> (T,U) as the set of frames that emit, in double
void brute(const std::vector<float>& stay, const std::vector<float>& emit, int T, int U, double* total, double* best) {
    const int U1 = U + 1;
    double sum = 0, mx = -INFINITY;
    bool any = false;
    for (unsigned mask = 0; mask < (1u << T); mask++) {
        if (__builtin_popcount(mask) != U) continue;
        double lp = 0;
        int u = 0;
        for (int t = 0; t < T; t++) {
            if (mask >> t & 1u) lp += emit[(size_t)t * U1 + u], u++;
            else lp += stay[(size_t)t * U1 + u];
        }
        if (lp == -INFINITY) continue;
        if (!any || lp > mx) { sum = sum * (any ? std::exp(mx - lp) : 0.0) + 1.0; mx = lp; any = true; }
        else sum += std::exp(lp - mx);
    }
    *total = any ? mx + std::log(sum) : -INFINITY;
    *best = mx;
}

void check_case(int T, int U, int inf_per_16) {
    const int U1 = U + 1;
    std::vector<float> stay((size_t)T * U1), emit((size_t)T * U1);
    for (size_t i = 0; i < stay.size(); i++) {
        stay[i] = (int)(rnd() % 16) < inf_per_16 ? -INFINITY : -0.25f * (float)(rnd() % 24);
        emit[i] = (int)(rnd() % 16) < inf_per_16 ? -INFINITY : -0.25f * (float)(rnd() % 24);
    }
    const LatticeRefResult r = lattice_dp_ref(stay.data(), emit.data(), T, U);
    double total, best;
    brute(stay, emit, T, U, &total, &best);
    CHECK(!std::isnan(r.total) && !std::isnan(r.best));
    CHECK((double)r.best == best);   // multiples of 0.25: sums are exact in float32
    if (total == -INFINITY) CHECK(r.total == -INFINITY);
    else CHECK(std::fabs((double)r.total - total) <= 1e-5 * std::fmax(1.0, std::fabs(total)));
    CHECK((int)r.timestamps.size() == U && (int)r.token_log_probs.size() == U);
    double path = 0;
    int u = 0;
    for (int t = 0; t < T; t++) {   // the path the timestamps describe scores `best`
        if (u < U && r.timestamps[(size_t)u] == t) {
            CHECK(r.token_log_probs[(size_t)u] == emit[(size_t)t * U1 + u]);
            path += emit[(size_t)t * U1 + u], u++;
        } else {
            path += stay[(size_t)t * U1 + u];
        }
    }
    CHECK(u == U);
    for (int k = 1; k < U; k++) CHECK(r.timestamps[(size_t)k] > r.timestamps[(size_t)k - 1]);
    if (best != -INFINITY) CHECK(path == best);
}

void reference() {
    for (int T = 1; T <= 9; T++)
        for (int U = 0; U <= T; U++)
            for (int inf : {0, 2, 6, 16}) check_case(T, U, inf);
    // the tie rule: T = 2, U = 1, both paths score -1.0 -> the emit predecessor wins at (2,1): the token sits on frame 1
    const float stay[4] = {-0.5f, -0.75f, -0.25f, -0.25f}, emit[4] = {-0.75f, -INFINITY, -0.5f, -INFINITY};
    const LatticeRefResult r = lattice_dp_ref(stay, emit, 2, 1);
    CHECK(r.best == -1.0f && r.timestamps[0] == 1 && r.token_log_probs[0] == -0.5f);
    CHECK(std::fabs(r.total - (-1.0f + std::log(2.0f))) < 1e-6f);
}

void abi(const char* path, const char* ctc_path) {
    k2hip_model_t* m = nullptr;
    OK(k2hip_model_create(path, nullptr, 0, &m));
    k2hip_model_info info;
    OK(k2hip_model_get_info(m, &info));
    const int B = 2, Tp = 5, mt = 4;
    std::vector<float> enc((size_t)B * Tp * info.joiner_dim, 0.25f);
    std::vector<int64_t> ids = {3, 4, 5, 6};
    int32_t lens[2] = {3, 1}, nf[2] = {5, 2};
    std::vector<int32_t> ts((size_t)B * mt, -7);
    std::vector<float> lp((size_t)B * mt, -7.f), tot(B, -7.f), best(B, -7.f);
    auto untouched = [&] { return ts[0] == -7 && ts[mt] == -7 && lp[0] == -7.f && tot[0] == -7.f && best[1] == -7.f; };
    auto call = [&](const int32_t* n_frames, const int64_t* y, const int32_t* l, int max_tokens) {
        return k2hip_transducer_align(m, enc.data(), B, Tp, n_frames, y, l, ts.data(), lp.data(), tot.data(), best.data(), max_tokens);
    };
    auto valid = [&] {
        OK(call(nf, ids.data(), lens, mt));
        CHECK(ts[0] < ts[1] && ts[1] < ts[2] && ts[2] < 5 && ts[mt] < 2 && ts[3] == -7 && lp[0] <= 0.f && best[0] <= tot[0] && best[1] <= tot[1]);
        std::fill(ts.begin(), ts.end(), -7); std::fill(lp.begin(), lp.end(), -7.f); std::fill(tot.begin(), tot.end(), -7.f);
        std::fill(best.begin(), best.end(), -7.f);
    };
    valid();
    // U > T: no path, the message names the stream
    int32_t nf_short[2] = {5, 0};
    int32_t lens_long[2] = {3, 1}, nf2[2] = {2, 2};
    CHECK(call(nf2, ids.data(), lens_long, mt) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "stream 0") != nullptr && untouched());
    valid();
    CHECK(call(nf_short, ids.data(), lens, mt) == K2HIP_ERR_INVALID && untouched());   // n_frames outside [1, T']
    int32_t nf_big[2] = {6, 2};
    CHECK(call(nf_big, ids.data(), lens, mt) == K2HIP_ERR_INVALID && untouched());
    for (int64_t bad : {(int64_t)K2HIP_BLANK_ID, (int64_t)K2HIP_UNK_ID, (int64_t)info.vocab_size, (int64_t)-1}) {
        std::vector<int64_t> y = ids;
        y[3] = bad;
        CHECK(call(nf, y.data(), lens, mt) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "stream 1") != nullptr && untouched());
        valid();
    }
    CHECK(call(nf, ids.data(), lens, 2) == K2HIP_ERR_CAPACITY && untouched());   // lens[0] = 3 > max_tokens: nothing written
    valid();
    int32_t lens_neg[2] = {-1, 1};
    CHECK(call(nf, ids.data(), lens_neg, mt) == K2HIP_ERR_INVALID && untouched());
    CHECK(call(nf, ids.data(), nullptr, mt) == K2HIP_ERR_INVALID);
    CHECK(call(nf, nullptr, lens, mt) == K2HIP_ERR_INVALID && untouched());
    CHECK(k2hip_transducer_align(nullptr, enc.data(), B, Tp, nf, ids.data(), lens, ts.data(), lp.data(), tot.data(), best.data(), mt) == K2HIP_ERR_INVALID);
    CHECK(k2hip_transducer_align(m, nullptr, B, Tp, nf, ids.data(), lens, ts.data(), lp.data(), tot.data(), best.data(), mt) == K2HIP_ERR_INVALID);
    CHECK(k2hip_transducer_align(m, enc.data(), 0, Tp, nf, ids.data(), lens, ts.data(), lp.data(), tot.data(), best.data(), mt) == K2HIP_ERR_INVALID);
    // every output is optional; n_frames NULL = T'; U = 0 everywhere needs no ids and max_tokens = 0
    OK(k2hip_transducer_align(m, enc.data(), B, Tp, nullptr, ids.data(), lens, nullptr, nullptr, nullptr, nullptr, mt));
    int32_t lens0[2] = {0, 0};
    OK(k2hip_transducer_align(m, enc.data(), B, Tp, nullptr, nullptr, lens0, ts.data(), lp.data(), tot.data(), best.data(), 0));
    CHECK(ts[0] == -7 && tot[0] == best[0] && tot[0] < 0.f);
    std::fill(tot.begin(), tot.end(), -7.f); std::fill(best.begin(), best.end(), -7.f);
    // the fused entry
    std::vector<float> wav(16000);
    for (size_t i = 0; i < wav.size(); i++) wav[i] = (float)((int)(i * 2654435761u % 2001) - 1000) / 1000.f;
    const float* ptr[2] = {wav.data(), wav.data()};
    int64_t ns[2] = {16000, 12000};
    int32_t Tpo = -7;
    OK(k2hip_offline_align_from_samples(m, ptr, ns, B, ids.data(), lens, ts.data(), lp.data(), tot.data(), best.data(), mt, &Tpo));
    CHECK(Tpo > 3 && ts[2] < Tpo && ts[0] < ts[1] && best[0] <= tot[0]);
    std::fill(ts.begin(), ts.end(), -7); std::fill(lp.begin(), lp.end(), -7.f); std::fill(tot.begin(), tot.end(), -7.f);
    std::fill(best.begin(), best.end(), -7.f);
    OK(k2hip_offline_align_from_samples(m, ptr, ns, B, ids.data(), lens, nullptr, nullptr, nullptr, nullptr, mt, nullptr));
    CHECK(k2hip_offline_align_from_samples(m, ptr, ns, B, ids.data(), lens, ts.data(), lp.data(), tot.data(), best.data(), 2, &Tpo) == K2HIP_ERR_CAPACITY &&
          untouched());
    int64_t ns_bad[2] = {16000, 10};
    CHECK(k2hip_offline_align_from_samples(m, ptr, ns_bad, B, ids.data(), lens, ts.data(), lp.data(), tot.data(), best.data(), mt, &Tpo) == K2HIP_ERR_INVALID &&
          untouched());
    CHECK(k2hip_offline_align_from_samples(m, nullptr, ns, B, ids.data(), lens, ts.data(), lp.data(), tot.data(), best.data(), mt, &Tpo) == K2HIP_ERR_INVALID);
    std::vector<int64_t> many((size_t)400, 5);
    int32_t lens_many[2] = {200, 200};
    std::vector<int32_t> ts_many(400, -7);
    CHECK(k2hip_offline_align_from_samples(m, ptr, ns, B, many.data(), lens_many, ts_many.data(), nullptr, nullptr, nullptr, 200, &Tpo) == K2HIP_ERR_INVALID &&
          ts_many[0] == -7);   // U > T' of one second of audio
    valid();
    OK(k2hip_model_destroy(m));
    // a CTC model has no lattice
    k2hip_model_t* c = nullptr;
    OK(k2hip_model_create(ctc_path, nullptr, 0, &c));
    k2hip_model_info ci;
    OK(k2hip_model_get_info(c, &ci));
    std::vector<float> cenc((size_t)B * Tp * (size_t)std::max(ci.joiner_dim, ci.vocab_size), 0.f);
    CHECK(k2hip_transducer_align(c, cenc.data(), B, Tp, nf, ids.data(), lens, ts.data(), lp.data(), tot.data(), best.data(), mt) == K2HIP_ERR_UNSUPPORTED &&
          untouched());
    CHECK(k2hip_offline_align_from_samples(c, ptr, ns, B, ids.data(), lens, ts.data(), lp.data(), tot.data(), best.data(), mt, &Tpo) == K2HIP_ERR_UNSUPPORTED &&
          untouched());
    OK(k2hip_model_destroy(c));
}

}  // namespace

int main(int argc, char** argv) {
    reference();
    if (argc >= 3) abi(argv[1], argv[2]);
    else fprintf(stderr, "san_align_driver: no model files given, the ABI part is skipped\n");
    printf("san_align_driver ok\n");
    return 0;
}
