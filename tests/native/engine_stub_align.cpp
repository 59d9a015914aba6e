// CPU stand-in for the engine's forced-alignment entry points (Engine::align_host, Engine::align_samples) -- TEST INFRASTRUCTURE for
// the sanitizer builds of csrc/api.cpp, next to engine_stub.cpp.  The argument rules are the engine's own (lattice_ref.h); the cells
// are a fixed function of (b, t, u) instead of the joiner's (there are no kernels here), and the recursions are the header-only host
// reference, so what api.cpp hands in and out runs under the sanitizers exactly as far as the device path reads and writes it.
// Never linked into libk2hip.so.
#include <algorithm>
#include <cstring>

#include "../../k2transducerasr_amd/csrc/engine.h"
#include "../../k2transducerasr_amd/csrc/lattice_ref.h"

namespace k2hip {

namespace {
void align_streams(const Config& cf, int B, int Tp, const int32_t* n_frames, const int64_t* ids, const int32_t* lens, int32_t* timestamps,
                   float* token_log_probs, float* total, float* best, int max_tokens) {
    if (cf.ctc) failf(K2HIP_ERR_UNSUPPORTED, "align: a CTC model has no transducer lattice");
    lattice_check_targets(cf.V, B, Tp, n_frames, ids, lens);
    for (int b = 0; b < B; b++)
        if (lens[b] > max_tokens) failf(K2HIP_ERR_CAPACITY, "align: stream %d has %d target tokens, max_tokens is %d", b, lens[b], max_tokens);
    size_t io = 0;
    for (int b = 0; b < B; b++) {
        const int T = n_frames ? n_frames[b] : Tp, U = lens[b], U1 = U + 1;
        std::vector<float> stay((size_t)T * U1), emit((size_t)T * U1);
        for (int t = 0; t < T; t++)
            for (int u = 0; u < U1; u++) {
                const unsigned h = (unsigned)(b * 7919 + t * 131 + u * 17) * 2654435761u;
                stay[(size_t)t * U1 + u] = -0.25f * (float)(1 + (h >> 28));
                emit[(size_t)t * U1 + u] = u < U ? -0.25f * (float)(1 + ((h >> 24) & 15) + (unsigned)(ids[io + (size_t)u] & 3)) : -INFINITY;
            }
        const LatticeRefResult r = lattice_dp_ref(stay.data(), emit.data(), T, U);
        const size_t o = (size_t)b * (size_t)max_tokens;
        if (timestamps && U) memcpy(timestamps + o, r.timestamps.data(), sizeof(int32_t) * (size_t)U);
        if (token_log_probs && U) memcpy(token_log_probs + o, r.token_log_probs.data(), sizeof(float) * (size_t)U);
        if (total) total[b] = r.total;
        if (best) best[b] = r.best;
        io += (size_t)U;
    }
}
}  // namespace

void Engine::align_host(const float* enc_out, int B, int Tp, const int32_t* n_frames, const int64_t* ids, const int32_t* lens, int32_t* timestamps,
                        float* token_log_probs, float* total, float* best, int max_tokens) {
    K2_REQUIRE(enc_out != nullptr && max_tokens >= 0, "align: bad arguments");
    K2_REQUIRE(B > 0 && Tp > 0, "align: bad shape B=%d T'=%d", B, Tp);
    volatile float sink = enc_out[0] + enc_out[(size_t)B * Tp * model_->cfg().J - 1];
    (void)sink;
    align_streams(model_->cfg(), B, Tp, n_frames, ids, lens, timestamps, token_log_probs, total, best, max_tokens);
}

void Engine::align_samples(const float* const* samples, const int64_t* n_samples, int B, const int64_t* ids, const int32_t* lens,
                           int32_t* timestamps, float* token_log_probs, float* total, float* best, int max_tokens, int32_t* Tp_out) {
    K2_REQUIRE(samples != nullptr && n_samples != nullptr && B > 0 && max_tokens >= 0, "align_from_samples: bad arguments");
    if (model_->cfg().ctc) failf(K2HIP_ERR_UNSUPPORTED, "align: a CTC model has no transducer lattice");
    int64_t nmax = 0;
    for (int b = 0; b < B; b++) {
        K2_REQUIRE(samples[b] != nullptr && fbank_num_frames(n_samples[b]) > 0, "stream %d: %lld samples give no frame", b, (long long)n_samples[b]);
        volatile float sink = samples[b][0] + samples[b][n_samples[b] - 1];
        (void)sink;
        nmax = std::max(nmax, n_samples[b]);
    }
    const int Tp = encoder_out_frames((int)fbank_num_frames(nmax) + 19);
    K2_REQUIRE(Tp > 0, "align_from_samples: %lld samples give no encoder frame", (long long)nmax);
    align_streams(model_->cfg(), B, Tp, nullptr, ids, lens, timestamps, token_log_probs, total, best, max_tokens);
    if (Tp_out) *Tp_out = Tp;
}

}  // namespace k2hip
