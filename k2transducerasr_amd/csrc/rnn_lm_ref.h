// Neural LM rescoring: the LM itself and the normative float32 host reference of its scores (include/k2hip.h "Neural LM rescoring",
// DESIGN.md "Neural LM rescoring").  Pure host code (no HIP): loaded, checked and scored without a GPU.
//
// The model is icefall's RnnLmModel: embedding [V, E] -> L LSTM layers of width H (torch gate order i, f, g, o; no projection) ->
// linear [V, H] + bias -> log_softmax.  A hypothesis y_1 .. y_n is scored on the inputs [sos, y_1 .. y_n] against the targets
// [y_1 .. y_n, eos] (n + 1 positions with_eos, the first n without), every layer starting from h = c = 0:
//   gates = (x_t . W_ih^T + (b_ih + b_hh)) + h_{t-1} . W_hh^T      (the two biases summed once, in float32, at load)
//   c = sigmoid(f) c + sigmoid(i) tanh(g);  h = sigmoid(o) tanh(c)
//   lp_t = log_softmax(h^{L-1}_t . W_out^T + b_out)[target_t];  total = the float32 sum of lp_t in position order.
// Every sum here runs in ascending index order in one float32 accumulator.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "errors.h"

namespace k2hip {

constexpr int kRnnLmMaxLayers = 8;

struct RnnLm {
    int V = 0, E = 0, H = 0, L = 0, sos = 0, eos = 0;
    bool tied = false;
    std::vector<float> emb;                  // [V][E]
    std::vector<std::vector<float>> w_ih;    // [L] of [4H][in], in = E for layer 0, else H
    std::vector<std::vector<float>> w_hh;    // [L] of [4H][H]
    std::vector<std::vector<float>> bias;    // [L] of [4H]: b_ih + b_hh
    std::vector<float> w_out;                // [V][H] (a copy of emb when the file ties them)
    std::vector<float> b_out;                // [V]
    int in_dim(int k) const { return k == 0 ? E : H; }
};

// A .k2w container with model_type=rnn_lm (rnn_lm_load.cpp).  Throws Error: K2HIP_ERR_IO for a file that cannot be read,
// K2HIP_ERR_UNSUPPORTED for H % 32 != 0 or E % 4 != 0, K2HIP_ERR_INVALID (naming the tensor) for everything else.
RnnLm* rnn_lm_load(const std::string& path);

inline float rnn_lm_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// One hypothesis: tokens[0 .. n) in [0, V) (checked by the caller).  lp (may be null) gets the positions' log-probs; returns the total.
inline float rnn_lm_ref_score(const RnnLm& m, const int64_t* tokens, int64_t n, bool with_eos, float* lp) {
    const int64_t P = n + (with_eos ? 1 : 0);
    const int H = m.H, G = 4 * m.H;
    std::vector<float> h((size_t)m.L * H, 0.f), c((size_t)m.L * H, 0.f), gates((size_t)G), hn((size_t)H), logit((size_t)m.V);
    float total = 0.f;
    for (int64_t t = 0; t < P; t++) {
        const int64_t x = t == 0 ? m.sos : tokens[t - 1], target = t < n ? tokens[t] : m.eos;
        const float* in = m.emb.data() + (size_t)x * m.E;
        for (int k = 0; k < m.L; k++) {
            const int I = m.in_dim(k);
            const float *wi = m.w_ih[(size_t)k].data(), *wh = m.w_hh[(size_t)k].data(), *b = m.bias[(size_t)k].data();
            float *hk = h.data() + (size_t)k * H, *ck = c.data() + (size_t)k * H;
            for (int g = 0; g < G; g++) {
                float ax = 0.f, ah = 0.f;
                for (int i = 0; i < I; i++) ax = fmaf(in[i], wi[(size_t)g * I + i], ax);
                for (int i = 0; i < H; i++) ah = fmaf(hk[i], wh[(size_t)g * H + i], ah);
                gates[(size_t)g] = (ax + b[g]) + ah;
            }
            for (int j = 0; j < H; j++) {
                const float ig = rnn_lm_sigmoid(gates[(size_t)j]), fg = rnn_lm_sigmoid(gates[(size_t)(H + j)]), gg = tanhf(gates[(size_t)(2 * H + j)]),
                            og = rnn_lm_sigmoid(gates[(size_t)(3 * H + j)]);
                ck[j] = fg * ck[j] + ig * gg;
                hn[(size_t)j] = og * tanhf(ck[j]);
            }
            for (int j = 0; j < H; j++) hk[j] = hn[(size_t)j];
            in = hk;
        }
        float mx = -INFINITY;
        for (int v = 0; v < m.V; v++) {
            float a = 0.f;
            const float* w = m.w_out.data() + (size_t)v * H;
            for (int i = 0; i < H; i++) a = fmaf(in[i], w[i], a);
            logit[(size_t)v] = a + m.b_out[(size_t)v];
            mx = fmaxf(mx, logit[(size_t)v]);
        }
        float s = 0.f;
        for (int v = 0; v < m.V; v++) s += expf(logit[(size_t)v] - mx);
        const float l = logit[(size_t)target] - (mx + logf(s));
        if (lp) lp[t] = l;
        total += l;
    }
    return total;
}

// Hn hypotheses back to back in `tokens`, hypothesis i at [offsets[i], offsets[i + 1]); token_log_probs (may be null) packed per
// hypothesis with its positions back to back; totals [Hn].  Checks the offsets and the ids: K2HIP_ERR_INVALID names the hypothesis.
inline void rnn_lm_check_hyps(int V, const int64_t* tokens, const int64_t* offsets, int Hn, const char* who) {
    K2_REQUIRE(Hn >= 0 && (Hn == 0 || offsets), "%s: %d hypotheses", who, Hn);
    if (Hn == 0) return;
    K2_REQUIRE(offsets[0] >= 0, "%s: hypothesis 0 starts at offset %lld", who, (long long)offsets[0]);
    for (int i = 0; i < Hn; i++) {
        K2_REQUIRE(offsets[i + 1] >= offsets[i], "%s: hypothesis %d: offsets decrease (%lld after %lld)", who, i, (long long)offsets[i + 1],
                   (long long)offsets[i]);
        K2_REQUIRE(offsets[i + 1] == offsets[i] || tokens, "%s: hypothesis %d: no tokens", who, i);
        for (int64_t k = offsets[i]; k < offsets[i + 1]; k++)
            K2_REQUIRE(tokens[k] >= 0 && tokens[k] < V, "%s: hypothesis %d: token %lld at position %lld is outside [0, %d)", who, i, (long long)tokens[k],
                       (long long)(k - offsets[i]), V);
    }
}
inline void rnn_lm_ref_score_all(const RnnLm& m, const int64_t* tokens, const int64_t* offsets, int Hn, bool with_eos, float* token_log_probs,
                                 float* totals) {
    rnn_lm_check_hyps(m.V, tokens, offsets, Hn, "rnn_lm_score_host");
    int64_t o = 0;
    for (int i = 0; i < Hn; i++) {
        const int64_t n = offsets[i + 1] - offsets[i];
        totals[i] = rnn_lm_ref_score(m, n ? tokens + offsets[i] : nullptr, n, with_eos, token_log_probs ? token_log_probs + o : nullptr);
        o += n + (with_eos ? 1 : 0);
    }
}

}  // namespace k2hip
