// CPU stand-in for the engine's keyword-spotting entry points (Engine::kws_graph_upload, Engine::kws_chunk_host, Engine::kws_samples)
// -- TEST INFRASTRUCTURE for the sanitizer builds of csrc/api.cpp, next to engine_stub.cpp.  The chunk and the fused entry run the engine's
// own plan (Engine::kws_plan, csrc/search_plan.cpp) and then read its blob as trie_dp would: S, T and the tables from each descriptor's
// graph copy, the carried blocks at its state_off.  The "resident" graph is a host copy of the trie's tables in one allocation, the cells
// are a fixed function of (absolute frame, state) instead of the joiner's (there are no kernels here), and the token passing is the
// header-only host reference, so the argument rules, the layout and what api.cpp hands in and out run under the sanitizers as far as the
// device path reads and writes.  Never linked into libk2hip.so.
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
// the host reference on what trie_dp reads: S, T and the tables from each descriptor's graph copy, the carried blocks at its state_off
void spot_streams(const KwsStream* st, const float* a_in, const int32_t* start_in, int B, int n_states, int mt, const std::vector<int32_t>& state_off,
                  Engine::KwsResult* res) {
    Engine::KwsResult r;
    r.mt = mt;
    r.keyword.assign((size_t)B * r.mt, 0);
    r.end.assign((size_t)B * r.mt, 0);
    r.start.assign((size_t)B * r.mt, 0);
    r.sum.assign((size_t)B * r.mt, 0.f);
    r.n.assign((size_t)B, 0);
    r.a.assign(a_in, a_in + n_states);
    r.st.assign(start_in, start_in + n_states);
    r.state_off = state_off;
    for (int b = 0; b < B; b++) {
        const KwsGraphDev& g = st[b].g;
        const int T = st[b].T, S = g.S, so = st[b].state_off;
        const int t0 = start_in[so];
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
    }
    *res = std::move(r);
}
}  // namespace

void Engine::kws_chunk_host(const float* enc_out, int B, int Tc, const KwsIO* io, KwsResult* res) {
    K2_REQUIRE(enc_out != nullptr && res != nullptr, "keyword spotting: bad arguments");
    const KwsPlan p = kws_plan(B, Tc, io, false);
    volatile float sink = enc_out[0] + enc_out[(size_t)B * Tc * model_->cfg().J - 1];
    (void)sink;
    spot_streams(reinterpret_cast<const KwsStream*>(p.blob.data()), reinterpret_cast<const float*>(p.blob.data() + p.o_a),
                 reinterpret_cast<const int32_t*>(p.blob.data() + p.o_st), B, p.n_states, std::max(p.max_T, 1), p.state_off, res);
}

void Engine::kws_samples(const float* const* samples, const int64_t* n_samples, int B, const KwsIO* io, KwsResult* res, int32_t* Tp_out) {
    K2_REQUIRE(samples != nullptr && n_samples != nullptr && B > 0 && res != nullptr, "spot_keywords_from_samples: bad arguments");
    if (model_->cfg().ctc) failf(K2HIP_ERR_UNSUPPORTED, "keyword spotting: a CTC model has no transducer lattice");
    const int Tp = samples_frames("spot_keywords_from_samples", samples, n_samples, B);
    const KwsPlan p = kws_plan(B, Tp, io, true);
    spot_streams(reinterpret_cast<const KwsStream*>(p.blob.data()), reinterpret_cast<const float*>(p.blob.data() + p.o_a),
                 reinterpret_cast<const int32_t*>(p.blob.data() + p.o_st), B, p.n_states, Tp, p.state_off, res);
    if (Tp_out) *Tp_out = Tp;
}

}  // namespace k2hip
