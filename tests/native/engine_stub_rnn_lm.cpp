// CPU stand-in of the engine's neural-LM entries (Engine::rnn_lm_upload, Engine::rnn_lm_score_host) for the sanitizer builds of the
// host layer: the float32 host reference of csrc/rnn_lm_ref.h where the engine launches the kernels, over exact-size copies of the
// caller's tokens and offsets (a read past a hypothesis is a heap overflow the sanitizer sees), behind the same host checks and the
// real row plan (rnn_lm_plan.cpp), so that api.cpp's set / clear bookkeeping and the re-ordering of the N-best lists run unmodified.
// The other stand-ins' searches keep no N-best list; k2hip_stub_rnn_lm_seed_nbest hands this one a list that the next rnn_lm_upload
// (k2hip_set_rnn_lm) installs as the engine's last list, so that a driver reaches the re-ordering of k2hip_offline_recognizer_get_results.
// Never linked into libk2hip.so.
#include <memory>
#include <vector>

#include "../../k2transducerasr_amd/csrc/engine.h"

namespace k2hip {

namespace {
std::unique_ptr<Engine::NbestHost> g_seed;
}
// tokens [B][N][max_tokens], n_tokens / scores [B][N], n_hyps [B]; timestamps are the positions, token log-probs -0.1 (k + 1)
extern "C" void k2hip_stub_rnn_lm_seed_nbest(int B, int N, int max_tokens, const int64_t* tokens, const int32_t* n_tokens, const float* scores,
                                             const int32_t* n_hyps) {
    g_seed.reset(new Engine::NbestHost());
    Engine::NbestHost& h = *g_seed;
    h.B = B; h.N = N; h.max_tokens = max_tokens;
    const size_t n = (size_t)B * N;
    h.tokens.assign(tokens, tokens + n * max_tokens);
    h.n_tokens.assign(n_tokens, n_tokens + n);
    h.scores.assign(scores, scores + n);
    h.n_hyps.assign(n_hyps, n_hyps + B);
    h.timestamps.resize(n * max_tokens);
    h.token_log_probs.resize(n * max_tokens);
    for (size_t i = 0; i < n * max_tokens; i++) {
        h.timestamps[i] = (int32_t)(i % max_tokens);
        h.token_log_probs[i] = -0.1f * (float)(i % max_tokens + 1);
    }
}

void* Engine::rnn_lm_upload(const RnnLm& m, RnnLmDev* out) {
    K2_REQUIRE(m.L >= 1 && m.L <= kRnnLmMaxLayers && m.H % 32 == 0 && m.E % 4 == 0, "rnn lm: %d layers, hidden_dim %d, embedding_dim %d", m.L, m.H, m.E);
    RnnLmDev d;
    d.V = m.V; d.Vp = (m.V + 31) / 32 * 32; d.E = m.E; d.H = m.H; d.L = m.L; d.sos = m.sos; d.eos = m.eos;
    *out = d;
    if (g_seed) {
        last_nbest_ = *g_seed;
        g_seed.reset();
    }
    return dev_alloc(64);   // (what the caller owns and frees; the stand-in scores from the host copy)
}

void Engine::rnn_lm_score_host(const int64_t* tokens, const int64_t* offsets, int Hn, bool with_eos, float* token_log_probs, float* totals) {
    K2_REQUIRE(rnn_host_, "rnn_lm_score: no LM is attached to the model (k2hip_set_rnn_lm)");
    rnn_lm_check_hyps(rnn_dev_.V, tokens, offsets, Hn, "rnn_lm_score");
    if (Hn == 0) return;
    K2_REQUIRE(totals, "rnn_lm_score: no place for the totals");
    const RnnLmPlan p = rnn_lm_plan(offsets, Hn, with_eos, rnn_dev_.H, kRnnLmGxCapFloats);
    rnn_last_blocks_ = (int)p.block.size() - 1;
    for (int i = 0; i < Hn; i++) totals[i] = 0.f;
    if (p.R == 0) return;
    rnn_calls_++;
    const std::vector<int64_t> off(offsets, offsets + Hn + 1);
    const std::vector<int64_t> tok(tokens ? tokens + off[0] : nullptr, tokens ? tokens + off[(size_t)Hn] : nullptr);
    std::vector<int64_t> rel((size_t)Hn + 1);
    for (int i = 0; i <= Hn; i++) rel[(size_t)i] = off[(size_t)i] - off[0];
    std::vector<float> lp((size_t)p.R), tot((size_t)Hn);
    rnn_lm_ref_score_all(*rnn_host_, tok.data(), rel.data(), Hn, with_eos, lp.data(), tot.data());
    if (token_log_probs) memcpy(token_log_probs, lp.data(), sizeof(float) * lp.size());
    memcpy(totals, tot.data(), sizeof(float) * tot.size());
}

void Engine::rnn_lm_step_bench(int, int, int, float*, float*) { failf(K2HIP_ERR_UNSUPPORTED, "rnn_lm_step_bench: the CPU stand-in has no kernels"); }

}  // namespace k2hip
