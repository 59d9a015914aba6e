// CPU stand-in for the engine's CTC keyword-spotting entry points (Engine::ctc_kws_chunk_host, Engine::ctc_kws_samples) -- TEST
// INFRASTRUCTURE for the sanitizer builds of csrc/api.cpp, next to engine_stub.cpp.  The argument rules are the engine's own (everything
// the kernel would turn into an address is checked); the chunk entry walks the caller's log-probs, the fused entry a fixed function of
// (frame, column) instead of the encoder's (there are no kernels here), and the token passing is the header-only host reference, so what
// api.cpp hands in and out runs under the sanitizers exactly as far as the device path reads and writes it.  Never linked into
// libk2hip.so.
#include <algorithm>
#include <climits>
#include <cstring>

#include "../../k2transducerasr_amd/csrc/ctc_kws_ref.h"
#include "../../k2transducerasr_amd/csrc/engine.h"

namespace k2hip {

namespace {
// lp == nullptr: the fixed plane
void spot_streams(const Config& cf, const float* lp, int B, int Tp, const Engine::CtcKwsIO* io, bool all_frames, Engine::KwsResult* res) {
    if (!cf.ctc) failf(K2HIP_ERR_UNSUPPORTED, "CTC keyword spotting: model_type '%s' has no CTC head", cf.model_type.c_str());
    K2_REQUIRE(B > 0 && B <= 65535 && Tp >= 1 && io != nullptr, "CTC keyword spotting: bad shape B=%d T'=%d", B, Tp);
    const int V = cf.V;
    int max_T = 0, n_states = 0;
    for (int b = 0; b < B; b++) {
        const int T = all_frames ? Tp : io[b].T;
        const Engine::CtcKwsGraph* g = io[b].graph;
        K2_REQUIRE(g && g->parent && g->tok && g->depth && g->kw && g->bar && g->rc && io[b].v && io[b].st, "CTC keyword spotting: stream %d has no graph", b);
        K2_REQUIRE(T >= 0 && T <= Tp, "CTC keyword spotting: stream %d: n_frames %d outside [0, %d]", b, T, Tp);
        const int S = g->S;
        K2_REQUIRE(S >= 1 && S <= kKwsMaxStates, "CTC keyword spotting: stream %d: %d trie states", b, S);
        for (int s = 1; s < S; s++) {
            K2_REQUIRE(g->parent[s] >= 0 && g->parent[s] < s, "CTC keyword spotting: stream %d: parent(%d) = %d", b, s, g->parent[s]);
            K2_REQUIRE(g->tok[s] >= 1 && g->tok[s] < V, "CTC keyword spotting: stream %d: tok(%d) = %d", b, s, g->tok[s]);
            const int r = g->rc[s];
            K2_REQUIRE(r == -1 || (r >= 1 && r < S && g->parent[r] == 0 && g->tok[r] == g->tok[s]), "CTC keyword spotting: stream %d: rc(%d) = %d", b, s, r);
        }
        const int32_t hold = io[b].st[S], frames = io[b].st[0];
        K2_REQUIRE(hold == -1 || (hold >= 1 && hold < S && g->parent[hold] == 0), "CTC keyword spotting: stream %d carries hold = %d", b, hold);
        K2_REQUIRE(frames >= 0 && (int64_t)frames + T <= INT32_MAX, "CTC keyword spotting: stream %d has run out of frame numbers", b);
        max_T = std::max(max_T, T);
        n_states += S;
    }
    Engine::KwsResult r;
    r.mt = all_frames ? Tp : std::max(max_T, 1);
    r.keyword.assign((size_t)B * r.mt, 0);
    r.end.assign((size_t)B * r.mt, 0);
    r.start.assign((size_t)B * r.mt, 0);
    r.sum.assign((size_t)B * r.mt, 0.f);
    r.n.assign((size_t)B, 0);
    r.a.resize(2 * (size_t)n_states);
    r.st.resize(2 * (size_t)n_states);
    int so = 0;
    for (int b = 0; b < B; b++) {
        const Engine::CtcKwsGraph& g = *io[b].graph;
        const int T = all_frames ? Tp : io[b].T, S = g.S;
        r.state_off.push_back(so);
        memcpy(r.a.data() + 2 * (size_t)so, io[b].v, sizeof(float) * 2 * (size_t)S);
        memcpy(r.st.data() + 2 * (size_t)so, io[b].st, sizeof(int32_t) * 2 * (size_t)S);
        std::vector<float> fixed;
        const float* rows = lp ? lp + (size_t)b * Tp * V : nullptr;
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
        ctc_kws_dp_ref(g.parent, g.tok, g.depth, g.kw, g.bar, g.rc, S, rows, V, T, r.a.data() + 2 * (size_t)so, r.st.data() + 2 * (size_t)so, &ev);
        for (size_t i = 0; i < ev.size(); i++) {
            const size_t o = (size_t)b * r.mt + i;
            r.keyword[o] = ev[i].keyword; r.start[o] = ev[i].start; r.end[o] = ev[i].end; r.sum[o] = ev[i].sum_logp;
        }
        r.n[(size_t)b] = (int32_t)ev.size();
        so += S;
    }
    *res = std::move(r);
}
}  // namespace

void Engine::ctc_kws_chunk_host(const float* log_probs, int B, int Tc, const CtcKwsIO* io, KwsResult* res) {
    K2_REQUIRE(log_probs != nullptr && res != nullptr, "CTC keyword spotting: bad arguments");
    spot_streams(model_->cfg(), log_probs, B, Tc, io, false, res);
}

void Engine::ctc_kws_samples(const float* const* samples, const int64_t* n_samples, int B, const CtcKwsIO* io, KwsResult* res, int32_t* Tp_out) {
    K2_REQUIRE(samples != nullptr && n_samples != nullptr && B > 0 && res != nullptr, "ctc_spot_keywords_from_samples: bad arguments");
    if (!model_->cfg().ctc) failf(K2HIP_ERR_UNSUPPORTED, "CTC keyword spotting: model_type '%s' has no CTC head", model_->cfg().model_type.c_str());
    int64_t nmax = 0;
    for (int b = 0; b < B; b++) {
        K2_REQUIRE(samples[b] != nullptr && fbank_num_frames(n_samples[b]) > 0, "stream %d: %lld samples give no frame", b, (long long)n_samples[b]);
        volatile float sink = samples[b][0] + samples[b][n_samples[b] - 1];
        (void)sink;
        nmax = std::max(nmax, n_samples[b]);
    }
    const int Tp = encoder_out_frames((int)fbank_num_frames(nmax) + 19);
    K2_REQUIRE(Tp > 0, "ctc_spot_keywords_from_samples: %lld samples give no encoder frame", (long long)nmax);
    spot_streams(model_->cfg(), nullptr, B, Tp, io, true, res);
    if (Tp_out) *Tp_out = Tp;
}

}  // namespace k2hip
