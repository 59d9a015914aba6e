// CPU stand-in for the engine's keyword-spotting entry points (Engine::kws_graph_upload, Engine::kws_chunk_host, Engine::kws_samples)
// -- TEST INFRASTRUCTURE for the sanitizer builds of csrc/api.cpp, next to engine_stub.cpp.  The argument rules are the engine's own;
// the "resident" graph is a host copy of the trie's tables in one allocation, the cells are a fixed function of (absolute frame, state)
// instead of the joiner's (there are no kernels here), and the token passing is the header-only host reference, so what api.cpp hands
// in and out runs under the sanitizers exactly as far as the device path reads and writes it.  Never linked into libk2hip.so.
#include <algorithm>
#include <cstring>

#include "../../k2transducerasr_amd/csrc/engine.h"
#include "../../k2transducerasr_amd/csrc/kws_ref.h"

namespace k2hip {

void* Engine::kws_graph_upload(const KeywordGraph& g, KwsGraphDev* out) {
    const Config& cf = model_->cfg();
    if (cf.ctc) failf(K2HIP_ERR_UNSUPPORTED, "keyword spotting: a CTC model has no transducer lattice");
    K2_REQUIRE(g.vocab_size() == cf.V, "keyword spotting: the graph was built for vocab_size %d, the model has %d", g.vocab_size(), cf.V);
    const int S = g.num_states();
    const std::vector<int64_t> ctx = g.contexts(2);
    for (int64_t y : ctx) K2_REQUIRE(y >= 0 && y < cf.V, "keyword spotting: context id %lld", (long long)y);
    int32_t* d = static_cast<int32_t*>(dev_alloc((int64_t)sizeof(int32_t) * 4 * S));
    memcpy(d, g.parent().data(), sizeof(int32_t) * (size_t)S);
    memcpy(d + S, g.depth().data(), sizeof(int32_t) * (size_t)S);
    memcpy(d + 2 * S, g.kw().data(), sizeof(int32_t) * (size_t)S);
    memcpy(d + 3 * S, g.bar().data(), sizeof(float) * (size_t)S);
    out->dec = reinterpret_cast<const float*>(d);   // (non-null; there are no decoder rows here)
    out->parent = d;
    out->depth = d + S;
    out->kw = d + 2 * S;
    out->bar = reinterpret_cast<const float*>(d + 3 * S);
    out->S = S;
    return d;
}

namespace {
void spot_streams(const Config& cf, int B, int Tp, const Engine::KwsIO* io, bool all_frames, Engine::KwsResult* res) {
    if (cf.ctc) failf(K2HIP_ERR_UNSUPPORTED, "keyword spotting: a CTC model has no transducer lattice");
    K2_REQUIRE(B > 0 && Tp >= 1 && io != nullptr, "keyword spotting: bad shape B=%d T'=%d", B, Tp);
    int max_T = 0, n_states = 0;
    for (int b = 0; b < B; b++) {
        const int T = all_frames ? Tp : io[b].T;
        K2_REQUIRE(io[b].graph && io[b].graph->dec && io[b].a && io[b].start, "keyword spotting: stream %d has no resident graph", b);
        K2_REQUIRE(T >= 0 && T <= Tp, "keyword spotting: stream %d: n_frames %d outside [0, %d]", b, T, Tp);
        max_T = std::max(max_T, T);
        n_states += io[b].graph->S;
    }
    Engine::KwsResult r;
    r.mt = std::max(max_T, 1);
    r.keyword.assign((size_t)B * r.mt, 0);
    r.end.assign((size_t)B * r.mt, 0);
    r.start.assign((size_t)B * r.mt, 0);
    r.sum.assign((size_t)B * r.mt, 0.f);
    r.n.assign((size_t)B, 0);
    r.a.resize((size_t)n_states);
    r.st.resize((size_t)n_states);
    int so = 0;
    for (int b = 0; b < B; b++) {
        const KwsGraphDev& g = *io[b].graph;
        const int T = all_frames ? Tp : io[b].T, S = g.S;
        r.state_off.push_back(so);
        memcpy(r.a.data() + so, io[b].a, sizeof(float) * (size_t)S);
        memcpy(r.st.data() + so, io[b].start, sizeof(int32_t) * (size_t)S);
        const int t0 = io[b].start[0];
        std::vector<float> stay((size_t)T * S), emit((size_t)T * S);
        for (int t = 0; t < T; t++)
            for (int s = 0; s < S; s++) {
                const unsigned h = (unsigned)((t0 + t) * 131 + s * 17) * 2654435761u;
                stay[(size_t)t * S + s] = -0.25f * (float)(1 + (h >> 28));
                emit[(size_t)t * S + s] = s ? -0.25f * (float)((h >> 24) & 7) : -INFINITY;
            }
        std::vector<KwsRefEvent> ev;
        kws_dp_ref(g.parent, g.depth, g.kw, g.bar, S, stay.data(), emit.data(), T, r.a.data() + so, r.st.data() + so, &ev);
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

void Engine::kws_chunk_host(const float* enc_out, int B, int Tc, const KwsIO* io, KwsResult* res) {
    K2_REQUIRE(enc_out != nullptr && res != nullptr, "keyword spotting: bad arguments");
    K2_REQUIRE(B > 0 && Tc >= 1, "keyword spotting: bad shape B=%d T'=%d", B, Tc);
    volatile float sink = enc_out[0] + enc_out[(size_t)B * Tc * model_->cfg().J - 1];
    (void)sink;
    spot_streams(model_->cfg(), B, Tc, io, false, res);
}

void Engine::kws_samples(const float* const* samples, const int64_t* n_samples, int B, const KwsIO* io, KwsResult* res, int32_t* Tp_out) {
    K2_REQUIRE(samples != nullptr && n_samples != nullptr && B > 0 && res != nullptr, "spot_keywords_from_samples: bad arguments");
    if (model_->cfg().ctc) failf(K2HIP_ERR_UNSUPPORTED, "keyword spotting: a CTC model has no transducer lattice");
    int64_t nmax = 0;
    for (int b = 0; b < B; b++) {
        K2_REQUIRE(samples[b] != nullptr && fbank_num_frames(n_samples[b]) > 0, "stream %d: %lld samples give no frame", b, (long long)n_samples[b]);
        volatile float sink = samples[b][0] + samples[b][n_samples[b] - 1];
        (void)sink;
        nmax = std::max(nmax, n_samples[b]);
    }
    const int Tp = encoder_out_frames((int)fbank_num_frames(nmax) + 19);
    K2_REQUIRE(Tp > 0, "spot_keywords_from_samples: %lld samples give no encoder frame", (long long)nmax);
    spot_streams(model_->cfg(), B, Tp, io, true, res);
    if (Tp_out) *Tp_out = Tp;
}

}  // namespace k2hip
