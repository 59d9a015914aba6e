// CPU stand-in for the engine's CTC forced-alignment entry points (Engine::ctc_align_host, Engine::ctc_align_samples) -- TEST
// INFRASTRUCTURE for the sanitizer builds of csrc/api.cpp, next to engine_stub.cpp.  Both run the engine's own plan
// (Engine::ctc_align_plan, csrc/search_plan.cpp) and then read its blob as ctc_lattice would: row, T, U and the id offset from the
// descriptors, the ids behind them.  The recursions are the header-only host reference on the caller's log_probs (ctc_align_host) or on a
// fixed function of (row, t, v) (ctc_align_samples: there is no encoder here), so the argument rules, the layout and what api.cpp hands
// in and out run under the sanitizers as far as the device path reads and writes.  Never linked into libk2hip.so.
#include <algorithm>
#include <cstring>

#include "../../k2transducerasr_amd/csrc/ctc_lattice_ref.h"
#include "../../k2transducerasr_amd/csrc/engine.h"

namespace k2hip {

namespace {
// the host reference on what ctc_lattice reads: the plan's descriptors and the ids behind them
void align_targets(const CtcAlignTarget* tg, const int* ids, int H, const float* log_probs, int Tp, int V, int32_t* timestamps, int32_t* end_frames,
                   float* token_log_probs, float* total, float* best, int max_tokens) {
    for (int h = 0; h < H; h++) {
        const int T = tg[h].T, U = tg[h].U;
        const std::vector<int64_t> y(ids + tg[h].id_off, ids + tg[h].id_off + U);
        const CtcLatticeRefResult res = ctc_lattice_ref(log_probs + (size_t)tg[h].row * (size_t)Tp * (size_t)V, V, U ? y.data() : nullptr, T, U);
        const size_t o = (size_t)h * (size_t)max_tokens;
        if (timestamps && U) memcpy(timestamps + o, res.timestamps.data(), sizeof(int32_t) * (size_t)U);
        if (end_frames && U) memcpy(end_frames + o, res.end_frames.data(), sizeof(int32_t) * (size_t)U);
        if (token_log_probs && U) memcpy(token_log_probs + o, res.token_log_probs.data(), sizeof(float) * (size_t)U);
        if (total) total[h] = res.total;
        if (best) best[h] = res.best;
    }
}
}  // namespace

void Engine::ctc_align_host(const float* log_probs, int R, int Tp, const int32_t* n_frames, int H, const int32_t* stream_of, const int64_t* ids,
                            const int32_t* lens, int32_t* timestamps, int32_t* end_frames, float* token_log_probs, float* total, float* best,
                            int max_tokens) {
    K2_REQUIRE(log_probs != nullptr && max_tokens >= 0, "ctc_align: bad arguments");
    const CtcAlignPlan p = ctc_align_plan(R, Tp, n_frames, H, stream_of, ids, lens, max_tokens);
    align_targets(p.targets(), reinterpret_cast<const int*>(p.blob.data() + p.o_ids), H, log_probs, Tp, model_->cfg().V, timestamps, end_frames,
                  token_log_probs, total, best, max_tokens);
}

void Engine::ctc_align_samples(const float* const* samples, const int64_t* n_samples, int B, int H, const int32_t* stream_of, const int64_t* ids,
                               const int32_t* lens, int32_t* timestamps, int32_t* end_frames, float* token_log_probs, float* total, float* best,
                               int max_tokens, int32_t* Tp_out) {
    K2_REQUIRE(samples != nullptr && n_samples != nullptr && B > 0 && max_tokens >= 0, "ctc_align_from_samples: bad arguments");
    const Config& cf = model_->cfg();
    if (!cf.ctc) failf(K2HIP_ERR_UNSUPPORTED, "ctc_align: model_type '%s' has no CTC head", cf.model_type.c_str());
    const int Tp = samples_frames("ctc_align_from_samples", samples, n_samples, B);
    const CtcAlignPlan p = ctc_align_plan(B, Tp, nullptr, H, stream_of, ids, lens, max_tokens);
    std::vector<float> lp((size_t)B * (size_t)Tp * (size_t)cf.V);
    for (int b = 0; b < B; b++)
        for (int t = 0; t < Tp; t++)
            for (int v = 0; v < cf.V; v++) {
                const unsigned hsh = (unsigned)(b * 7919 + t * 131 + v * 17) * 2654435761u;
                lp[((size_t)b * (size_t)Tp + (size_t)t) * (size_t)cf.V + (size_t)v] = -0.25f * (float)(1 + (hsh >> 28));
            }
    align_targets(p.targets(), reinterpret_cast<const int*>(p.blob.data() + p.o_ids), H, lp.data(), Tp, cf.V, timestamps, end_frames, token_log_probs,
                  total, best, max_tokens);
    if (Tp_out) *Tp_out = Tp;
}

}  // namespace k2hip
