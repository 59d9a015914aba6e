// CPU stand-in for the engine's forced-alignment entry points (Engine::align_host, Engine::align_samples) -- TEST INFRASTRUCTURE for
// the sanitizer builds of csrc/api.cpp, next to engine_stub.cpp.  Both run the engine's own plan (Engine::align_plan, csrc/search_plan.cpp)
// and then read its blob as lattice_dp would: T, U and the id offset from the descriptors, the ids behind them.  The cells are a fixed
// function of (b, t, u) instead of the joiner's (there are no kernels here), and the recursions are the header-only host reference, so
// the argument rules, the layout and what api.cpp hands in and out run under the sanitizers as far as the device path reads and writes.
// Never linked into libk2hip.so.
#include <algorithm>
#include <cstring>

#include "../../k2transducerasr_amd/csrc/engine.h"
#include "../../k2transducerasr_amd/csrc/lattice_ref.h"

namespace k2hip {

namespace {
// the host reference on what lattice_dp reads: the plan's descriptors and the ids behind them
void align_streams(const AlignStream* st, const int* ids, int B, int32_t* timestamps, float* token_log_probs, float* total, float* best,
                   int max_tokens) {
    for (int b = 0; b < B; b++) {
        const int T = st[b].T, U = st[b].U, U1 = U + 1;
        const int* y = ids + st[b].id_off;
        std::vector<float> stay((size_t)T * U1), emit((size_t)T * U1);
        for (int t = 0; t < T; t++)
            for (int u = 0; u < U1; u++) {
                const unsigned h = (unsigned)(b * 7919 + t * 131 + u * 17) * 2654435761u;
                stay[(size_t)t * U1 + u] = -0.25f * (float)(1 + (h >> 28));
                emit[(size_t)t * U1 + u] = u < U ? -0.25f * (float)(1 + ((h >> 24) & 15) + (unsigned)(y[u] & 3)) : -INFINITY;
            }
        const LatticeRefResult r = lattice_dp_ref(stay.data(), emit.data(), T, U);
        const size_t o = (size_t)b * (size_t)max_tokens;
        if (timestamps && U) memcpy(timestamps + o, r.timestamps.data(), sizeof(int32_t) * (size_t)U);
        if (token_log_probs && U) memcpy(token_log_probs + o, r.token_log_probs.data(), sizeof(float) * (size_t)U);
        if (total) total[b] = r.total;
        if (best) best[b] = r.best;
    }
}
}  // namespace

void Engine::align_host(const float* enc_out, int B, int Tp, const int32_t* n_frames, const int64_t* ids, const int32_t* lens, int32_t* timestamps,
                        float* token_log_probs, float* total, float* best, int max_tokens) {
    K2_REQUIRE(enc_out != nullptr && max_tokens >= 0, "align: bad arguments");
    const AlignPlan p = align_plan(B, Tp, n_frames, ids, lens, max_tokens);
    volatile float sink = enc_out[0] + enc_out[(size_t)B * Tp * model_->cfg().J - 1];
    (void)sink;
    align_streams(p.streams(), reinterpret_cast<const int*>(p.blob.data() + p.o_ids), B, timestamps, token_log_probs, total, best, max_tokens);
}

void Engine::align_samples(const float* const* samples, const int64_t* n_samples, int B, const int64_t* ids, const int32_t* lens,
                           int32_t* timestamps, float* token_log_probs, float* total, float* best, int max_tokens, int32_t* Tp_out) {
    K2_REQUIRE(samples != nullptr && n_samples != nullptr && B > 0 && max_tokens >= 0, "align_from_samples: bad arguments");
    if (model_->cfg().ctc) failf(K2HIP_ERR_UNSUPPORTED, "align: a CTC model has no transducer lattice");
    const int Tp = samples_frames("align_from_samples", samples, n_samples, B);
    const AlignPlan p = align_plan(B, Tp, nullptr, ids, lens, max_tokens);
    align_streams(p.streams(), reinterpret_cast<const int*>(p.blob.data() + p.o_ids), B, timestamps, token_log_probs, total, best, max_tokens);
    if (Tp_out) *Tp_out = Tp;
}

}  // namespace k2hip
