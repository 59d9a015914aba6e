// CPU stand-in for the engine's resumed CTC prefix beam search (Engine::ctc_prefix_chunk_host) -- TEST INFRASTRUCTURE for the sanitizer
// builds of csrc/api.cpp, next to engine_stub_ctc_prefix.cpp.  It is the float32 host reference of the resumed step: the frame step is
// ctc_prefix_ref.h's own (ctc_prefix_ref_frame), and only the fold table is decided here, from what an in block holds -- a hypothesis
// is (carried slot, the tokens appended in this chunk), and two of them are compared FORWARDS through the relation tables (the kernel
// walks its chains backwards).  The argument rules are the engine's (ctc_prefix_chunk_check_args).  Never linked into libk2hip.so.
#include <cmath>
#include <cstring>

#include "../../k2transducerasr_amd/csrc/ctc_prefix_layout.h"
#include "../../k2transducerasr_amd/csrc/ctc_prefix_ref.h"
#include "../../k2transducerasr_amd/csrc/engine.h"

namespace k2hip {

namespace {
// S_a + u == S_b + w as token sequences (u, w: in-chunk tokens; the carried sequences only through rel / relx)
bool same_sequence(const int* in, const CtcPrefixResumeLayout& L, int a, const int64_t* u, size_t nu, int b, const int64_t* w, size_t nw) {
    if (nu > nw) return same_sequence(in, L, b, w, nw, a, u, nu);
    const size_t d = nw - nu;   // S_a = S_b + w[0 .. d)
    for (size_t i = 0; i < nu; i++)
        if (u[i] != w[d + i]) return false;
    if (d == 0) return a == b;
    if (in[L.in_rel() + a * L.K + b] != (int)d) return false;
    for (size_t i = 0; i < d; i++)
        if (in[L.in_relx() + (a * L.K + b) * L.Tc + (int)i] != w[i]) return false;
    return true;
}
}  // namespace

// the resumed step on the host, any V (tests/native/san_ctc_prefix_stream_driver.cpp calls it directly)
void ctc_prefix_chunk_ref(const float* log_probs, int B, int Tc, int V, const int32_t* n_frames, int K, const int* in_all, int* out_all) {
    const CtcPrefixResumeLayout L{K, Tc};
    ctc_prefix_chunk_check_args(B, Tc, V, n_frames, K, in_all, L.in_ints(), L.in_e(), L.in_rel());
    for (int b = 0; b < B; b++) {
        const int* in = in_all + (size_t)b * (size_t)L.in_ints();
        int* out = out_all + (size_t)b * (size_t)L.out_ints();
        const int n0 = in[0], T = n_frames ? n_frames[b] : Tc;
        std::vector<CtcPrefixRefSlot> cur((size_t)n0);
        std::vector<int> clen((size_t)K, 0);
        std::vector<uint64_t> chash((size_t)K, 0), cphash((size_t)K, 0);
        for (int k = 0; k < K; k++) {
            clen[(size_t)k] = in[L.in_len() + k];
            chash[(size_t)k] = (uint64_t)(uint32_t)in[L.in_hash() + 2 * k] | (uint64_t)(uint32_t)in[L.in_hash() + 2 * k + 1] << 32;
            cphash[(size_t)k] = (uint64_t)(uint32_t)in[L.in_phash() + 2 * k] | (uint64_t)(uint32_t)in[L.in_phash() + 2 * k + 1] << 32;
        }
        for (int k = 0; k < n0; k++) {
            CtcPrefixRefSlot& s = cur[(size_t)k];
            memcpy(&s.h.pb, &in[L.in_pb() + k], sizeof(float));
            memcpy(&s.h.pnb, &in[L.in_pnb() + k], sizeof(float));
            s.h.tot = ctc_prefix_logaddexp(s.h.pb, s.h.pnb);
            s.last = in[L.in_e() + k];
            s.origin = k;
        }
        long long next_node = 0;
        for (int t = 0; t < T; t++) {
            const int n = (int)cur.size();
            std::vector<int> fold_par((size_t)n, -1);
            for (int j = 0; j < n; j++)
                for (int k = 0; k < n; k++) {
                    if (j == k) continue;
                    const std::vector<int64_t>&xj = cur[(size_t)j].h.tokens, &xk = cur[(size_t)k].h.tokens;
                    const int a = cur[(size_t)j].origin, o = cur[(size_t)k].origin;
                    if (clen[(size_t)a] + (int)xj.size() != clen[(size_t)o] + (int)xk.size() + 1) continue;
                    bool yes;
                    if (!xj.empty()) yes = same_sequence(in, L, a, xj.data(), xj.size() - 1, o, xk.data(), xk.size());
                    else {   // a carried slot with nothing appended: S_a = S_o + x_k + [e_a]
                        std::vector<int64_t> w(xk);
                        w.push_back(cur[(size_t)j].last);
                        yes = (int)w.size() <= Tc && same_sequence(in, L, a, nullptr, 0, o, w.data(), w.size());
                    }
                    if (yes) fold_par[(size_t)j] = k;
                }
            cur = ctc_prefix_ref_frame(cur, fold_par, log_probs + ((size_t)b * (size_t)Tc + (size_t)t) * (size_t)V, t, V, K, &next_node);
        }
        out[0] = (int)cur.size();
        for (size_t k = 0; k < cur.size(); k++) {
            const CtcPrefixRefSlot& s = cur[k];
            const int na = (int)s.h.tokens.size();
            uint64_t h = chash[(size_t)s.origin], ph = cphash[(size_t)s.origin];
            for (int i = 0; i < na; i++) {
                ph = h;
                h = h * kCtcPrefixHashMul + (uint64_t)(s.h.tokens[(size_t)i] + 1);
                out[L.out_ys() + (int)k * Tc + i] = (int)s.h.tokens[(size_t)i];
                out[L.out_ts() + (int)k * Tc + i] = s.h.timestamps[(size_t)i];
                memcpy(&out[L.out_yp() + (int)k * Tc + i], &s.h.token_log_probs[(size_t)i], sizeof(float));
            }
            out[L.out_org() + (int)k] = s.origin;
            out[L.out_napp() + (int)k] = na;
            memcpy(&out[L.out_pb() + (int)k], &s.h.pb, sizeof(float));
            memcpy(&out[L.out_pnb() + (int)k], &s.h.pnb, sizeof(float));
            memcpy(&out[L.out_tot() + (int)k], &s.h.tot, sizeof(float));
            out[L.out_hash() + 2 * (int)k] = (int)(uint32_t)h; out[L.out_hash() + 2 * (int)k + 1] = (int)(uint32_t)(h >> 32);
            out[L.out_phash() + 2 * (int)k] = (int)(uint32_t)ph; out[L.out_phash() + 2 * (int)k + 1] = (int)(uint32_t)(ph >> 32);
        }
    }
}

void Engine::ctc_prefix_chunk_host(const float* log_probs, int B, int Tc, const int32_t* n_frames, int K, const int* in, int* out) {
    const Config& cf = model_->cfg();
    if (!cf.ctc) failf(K2HIP_ERR_UNSUPPORTED, "ctc_prefix_beam_search_chunk: model_type '%s' has no CTC head", cf.model_type.c_str());
    K2_REQUIRE(log_probs && in && out, "ctc_prefix_beam_search_chunk: null argument");
    ctc_prefix_chunk_ref(log_probs, B, Tc, cf.V, n_frames, K, in, out);
}

// the streaming tick of a CTC model under the carried prefix search: there is no encoder here, so the chunk's log-probs are quarter
// steps derived from its first feature (ties included) -- what api.cpp stages, hands in and applies runs as on the device path
void Engine::online_step_ctc_prefix(const int* slots, const float* const* chunks, const long long*, const int*, int B, int K, const int* cp_in,
                                    int* cp_out, const int*) {
    const Config& c = model_->cfg();
    K2_REQUIRE(K >= 1 && K <= kCtcPrefixMaxBeam && c.ctc, "stub: online ctc prefix search with beam %d", K);
    const int Tp = online_frames_per_chunk(), V = c.V;
    std::vector<float> lp((size_t)B * (size_t)Tp * (size_t)V);
    for (int b = 0; b < B; b++) {
        K2_REQUIRE(slots[b] >= 0 && slots[b] < online_cap_, "stub: slot %d", slots[b]);
        const float f0 = chunks[b][0] + chunks[b][(size_t)c.chunk_T * c.feat - 1];
        const int salt = (int)(std::fabs(f0) * 16.f) % 64;
        for (int t = 0; t < Tp; t++)
            for (int v = 0; v < V; v++) lp[((size_t)b * (size_t)Tp + (size_t)t) * (size_t)V + (size_t)v] = -0.25f * (float)((v * 7 + t * 3 + salt) % 16);
    }
    ctc_prefix_chunk_ref(lp.data(), B, Tp, V, nullptr, K, cp_in, cp_out);
}

}  // namespace k2hip
