// CPU stand-in for the engine's CTC prefix beam search entry (Engine::ctc_prefix_host) -- TEST INFRASTRUCTURE for the sanitizer builds
// of csrc/api.cpp, next to engine_stub.cpp.  The argument rules are the engine's own (ctc_prefix_ref.h); the search is the header-only
// host reference on the caller's log_probs, so what api.cpp hands in and out runs under the sanitizers exactly as far as the device
// path reads and writes it.  Never linked into libk2hip.so.
#include <algorithm>
#include <cstring>

#include "../../k2transducerasr_amd/csrc/ctc_prefix_ref.h"
#include "../../k2transducerasr_amd/csrc/engine.h"

namespace k2hip {

void Engine::ctc_prefix_host(const float* log_probs, int R, int Tp, const int32_t* n_frames, int beam, int nbest, int64_t* tokens, int32_t* timestamps,
                             float* token_log_probs, int32_t* n_tokens, int32_t* n_hyps, float* scores, int max_tokens) {
    const Config& cf = model_->cfg();
    if (!cf.ctc) failf(K2HIP_ERR_UNSUPPORTED, "ctc_prefix_beam_search: model_type '%s' has no CTC head", cf.model_type.c_str());
    K2_REQUIRE(log_probs && tokens && timestamps && token_log_probs && n_tokens && n_hyps && scores, "ctc_prefix_beam_search: null argument");
    ctc_prefix_check_args(R, Tp, cf.V, n_frames, beam, nbest, max_tokens);
    std::vector<CtcPrefixRefResult> res;
    for (int r = 0; r < R; r++) {
        res.push_back(ctc_prefix_ref(log_probs + (size_t)r * (size_t)Tp * (size_t)cf.V, cf.V, n_frames ? n_frames[r] : Tp, cf.V, beam));
        const int nh = std::min((int)res.back().hyps.size(), nbest);
        for (int i = 0; i < nh; i++)   // one over-long entry fails the whole call, nothing is written
            if ((int)res.back().hyps[(size_t)i].tokens.size() > max_tokens)
                failf(K2HIP_ERR_CAPACITY, "a stream emitted more than max_tokens=%d symbols", max_tokens);
    }
    for (int r = 0; r < R; r++) {
        const int nh = std::min((int)res[(size_t)r].hyps.size(), nbest);
        n_hyps[r] = nh;
        for (int i = 0; i < nh; i++) {
            const CtcPrefixRefHyp& h = res[(size_t)r].hyps[(size_t)i];
            const size_t en = (size_t)r * (size_t)nbest + (size_t)i, o = en * (size_t)max_tokens, len = h.tokens.size();
            if (len) {
                memcpy(tokens + o, h.tokens.data(), sizeof(int64_t) * len);
                memcpy(timestamps + o, h.timestamps.data(), sizeof(int32_t) * len);
                memcpy(token_log_probs + o, h.token_log_probs.data(), sizeof(float) * len);
            }
            n_tokens[en] = (int32_t)len;
            scores[en] = h.tot;
        }
    }
}

}  // namespace k2hip
