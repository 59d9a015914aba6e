// CPU stand-in for the engine's CTC forced-alignment entry points (Engine::ctc_align_host, Engine::ctc_align_samples) -- TEST
// INFRASTRUCTURE for the sanitizer builds of csrc/api.cpp, next to engine_stub.cpp.  The argument rules are the engine's own
// (ctc_lattice_ref.h); the recursions are the header-only host reference on the caller's log_probs (ctc_align_host) or on a fixed
// function of (row, t, v) (ctc_align_samples: there is no encoder here), so what api.cpp hands in and out runs under the sanitizers
// exactly as far as the device path reads and writes it.  Never linked into libk2hip.so.
#include <algorithm>
#include <cstring>

#include "../../k2transducerasr_amd/csrc/ctc_lattice_ref.h"
#include "../../k2transducerasr_amd/csrc/engine.h"

namespace k2hip {

namespace {
void align_targets(const Config& cf, const float* log_probs, int R, int Tp, const int32_t* n_frames, int H, const int32_t* stream_of,
                   const int64_t* ids, const int32_t* lens, int32_t* timestamps, int32_t* end_frames, float* token_log_probs, float* total,
                   float* best, int max_tokens) {
    if (!cf.ctc) failf(K2HIP_ERR_UNSUPPORTED, "ctc_align: model_type '%s' has no CTC head", cf.model_type.c_str());
    ctc_check_targets(cf.V, R, Tp, n_frames, H, stream_of, ids, lens);
    for (int h = 0; h < H; h++) {
        if (lens[h] > max_tokens) failf(K2HIP_ERR_CAPACITY, "ctc_align: target %d has %d tokens, max_tokens is %d", h, lens[h], max_tokens);
        K2_REQUIRE(lens[h] <= kCtcAlignMaxU, "ctc_align: target %d has %d tokens (at most %d)", h, lens[h], kCtcAlignMaxU);
    }
    size_t io = 0;
    for (int h = 0; h < H; h++) {
        const int r = stream_of ? stream_of[h] : h, T = n_frames ? n_frames[r] : Tp, U = lens[h];
        const CtcLatticeRefResult res = ctc_lattice_ref(log_probs + (size_t)r * (size_t)Tp * (size_t)cf.V, cf.V, U ? ids + io : nullptr, T, U);
        const size_t o = (size_t)h * (size_t)max_tokens;
        if (timestamps && U) memcpy(timestamps + o, res.timestamps.data(), sizeof(int32_t) * (size_t)U);
        if (end_frames && U) memcpy(end_frames + o, res.end_frames.data(), sizeof(int32_t) * (size_t)U);
        if (token_log_probs && U) memcpy(token_log_probs + o, res.token_log_probs.data(), sizeof(float) * (size_t)U);
        if (total) total[h] = res.total;
        if (best) best[h] = res.best;
        io += (size_t)U;
    }
}
}  // namespace

void Engine::ctc_align_host(const float* log_probs, int R, int Tp, const int32_t* n_frames, int H, const int32_t* stream_of, const int64_t* ids,
                            const int32_t* lens, int32_t* timestamps, int32_t* end_frames, float* token_log_probs, float* total, float* best,
                            int max_tokens) {
    K2_REQUIRE(log_probs != nullptr && max_tokens >= 0, "ctc_align: bad arguments");
    K2_REQUIRE(R > 0 && Tp > 0 && H > 0, "ctc_align: bad shape R=%d T'=%d H=%d", R, Tp, H);
    align_targets(model_->cfg(), log_probs, R, Tp, n_frames, H, stream_of, ids, lens, timestamps, end_frames, token_log_probs, total, best,
                  max_tokens);
}

void Engine::ctc_align_samples(const float* const* samples, const int64_t* n_samples, int B, int H, const int32_t* stream_of, const int64_t* ids,
                               const int32_t* lens, int32_t* timestamps, int32_t* end_frames, float* token_log_probs, float* total, float* best,
                               int max_tokens, int32_t* Tp_out) {
    K2_REQUIRE(samples != nullptr && n_samples != nullptr && B > 0 && max_tokens >= 0, "ctc_align_from_samples: bad arguments");
    const Config& cf = model_->cfg();
    if (!cf.ctc) failf(K2HIP_ERR_UNSUPPORTED, "ctc_align: model_type '%s' has no CTC head", cf.model_type.c_str());
    int64_t nmax = 0;
    for (int b = 0; b < B; b++) {
        K2_REQUIRE(samples[b] != nullptr && fbank_num_frames(n_samples[b]) > 0, "stream %d: %lld samples give no frame", b, (long long)n_samples[b]);
        volatile float sink = samples[b][0] + samples[b][n_samples[b] - 1];
        (void)sink;
        nmax = std::max(nmax, n_samples[b]);
    }
    const int Tp = encoder_out_frames((int)fbank_num_frames(nmax) + 19);
    K2_REQUIRE(Tp > 0, "ctc_align_from_samples: %lld samples give no encoder frame", (long long)nmax);
    std::vector<float> lp((size_t)B * (size_t)Tp * (size_t)cf.V);
    for (int b = 0; b < B; b++)
        for (int t = 0; t < Tp; t++)
            for (int v = 0; v < cf.V; v++) {
                const unsigned hsh = (unsigned)(b * 7919 + t * 131 + v * 17) * 2654435761u;
                lp[((size_t)b * (size_t)Tp + (size_t)t) * (size_t)cf.V + (size_t)v] = -0.25f * (float)(1 + (hsh >> 28));
            }
    align_targets(cf, lp.data(), B, Tp, nullptr, H, stream_of, ids, lens, timestamps, end_frames, token_log_probs, total, best, max_tokens);
    if (Tp_out) *Tp_out = Tp;
}

}  // namespace k2hip
