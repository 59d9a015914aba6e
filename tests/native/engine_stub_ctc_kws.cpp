// CPU stand-in for the engine's CTC keyword-spotting entry points (Engine::ctc_kws_chunk_host, Engine::ctc_kws_samples) -- TEST
// INFRASTRUCTURE for the sanitizer builds of csrc/api.cpp, next to engine_stub.cpp.  Both run the engine's own plan (Engine::ctc_kws_plan,
// csrc/search_plan.cpp: everything the kernel would turn into an address is checked there) and then read its blob as ctc_trie_dp would:
// the descriptors, the six tables at each one's table offset, the carried blocks at 2 * state_off.  The chunk entry walks the caller's
// log-probs, the fused entry a fixed function of (frame, column) instead of the encoder's (there are no kernels here), and the token
// passing is the header-only host reference, so the argument rules, the layout and what api.cpp hands in and out run under the
// sanitizers as far as the device path reads and writes.  Never linked into libk2hip.so.
#include <algorithm>
#include <cstring>

#include "../../k2transducerasr_amd/csrc/ctc_kws_ref.h"
#include "../../k2transducerasr_amd/csrc/engine.h"

namespace k2hip {

namespace {
// the host reference on what ctc_trie_dp reads: the descriptors, the six tables at each one's table offset, the carried blocks at
// 2 * state_off.  lp == nullptr: the fixed plane
void spot_streams(const CtcKwsStream* st, const float* v_in, const int32_t* st_in, const int32_t* tables, int B, int n_states, int mt,
                  const std::vector<int32_t>& state_off, const float* lp, int Tp, int V, Engine::KwsResult* res) {
    Engine::KwsResult r;
    r.mt = mt;
    r.keyword.assign((size_t)B * r.mt, 0);
    r.end.assign((size_t)B * r.mt, 0);
    r.start.assign((size_t)B * r.mt, 0);
    r.sum.assign((size_t)B * r.mt, 0.f);
    r.n.assign((size_t)B, 0);
    r.a.assign(v_in, v_in + 2 * (size_t)n_states);
    r.st.assign(st_in, st_in + 2 * (size_t)n_states);
    r.state_off = state_off;
    for (int b = 0; b < B; b++) {
        const int T = st[b].T, S = st[b].S;
        const size_t so = 2 * (size_t)st[b].state_off;
        const int32_t* tab = tables + st[b].table_off;
        std::vector<float> fixed;
        const float* rows = lp ? lp + (size_t)st[b].row * Tp * V : nullptr;
        if (!rows) {
            fixed.resize((size_t)T * V);
            for (int t = 0; t < T; t++)
                for (int v = 0; v < V; v++) {
                    const unsigned h = (unsigned)(t * 131 + v * 17 + b) * 2654435761u;
                    fixed[(size_t)t * V + v] = -0.25f * (float)((h >> 28) & 7);
                }
            rows = fixed.data();
        }
        std::vector<KwsRefEvent> ev;
        ctc_kws_dp_ref(tab, tab + S, tab + 2 * (size_t)S, tab + 3 * (size_t)S, reinterpret_cast<const float*>(tab + 4 * (size_t)S), tab + 5 * (size_t)S, S,
                       rows, V, T, r.a.data() + so, r.st.data() + so, &ev);
        for (size_t i = 0; i < ev.size(); i++) {
            const size_t o = (size_t)b * r.mt + i;
            r.keyword[o] = ev[i].keyword; r.start[o] = ev[i].start; r.end[o] = ev[i].end; r.sum[o] = ev[i].sum_logp;
        }
        r.n[(size_t)b] = (int32_t)ev.size();
    }
    *res = std::move(r);
}
}  // namespace

void Engine::ctc_kws_chunk_host(const float* log_probs, int B, int Tc, const CtcKwsIO* io, KwsResult* res) {
    K2_REQUIRE(log_probs != nullptr && res != nullptr, "CTC keyword spotting: bad arguments");
    const CtcKwsPlan p = ctc_kws_plan(B, Tc, io, false);
    const char* blob = p.blob.data();
    spot_streams(reinterpret_cast<const CtcKwsStream*>(blob), reinterpret_cast<const float*>(blob + p.o_v), reinterpret_cast<const int32_t*>(blob + p.o_st),
                 reinterpret_cast<const int32_t*>(blob + p.o_tab), B, p.n_states, std::max(p.max_T, 1), p.state_off, log_probs, Tc, p.V, res);
}

void Engine::ctc_kws_samples(const float* const* samples, const int64_t* n_samples, int B, const CtcKwsIO* io, KwsResult* res, int32_t* Tp_out) {
    K2_REQUIRE(samples != nullptr && n_samples != nullptr && B > 0 && res != nullptr, "ctc_spot_keywords_from_samples: bad arguments");
    if (!model_->cfg().ctc) failf(K2HIP_ERR_UNSUPPORTED, "CTC keyword spotting: model_type '%s' has no CTC head", model_->cfg().model_type.c_str());
    const int Tp = samples_frames("ctc_spot_keywords_from_samples", samples, n_samples, B);
    const CtcKwsPlan p = ctc_kws_plan(B, Tp, io, true);
    const char* blob = p.blob.data();
    spot_streams(reinterpret_cast<const CtcKwsStream*>(blob), reinterpret_cast<const float*>(blob + p.o_v), reinterpret_cast<const int32_t*>(blob + p.o_st),
                 reinterpret_cast<const int32_t*>(blob + p.o_tab), B, p.n_states, Tp, p.state_off, nullptr, Tp, p.V, res);
    if (Tp_out) *Tp_out = Tp;
}

}  // namespace k2hip
