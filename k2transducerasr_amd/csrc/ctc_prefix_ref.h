// Host reference of the CTC prefix beam search of ctc_prefix.hip (k_ctc_prefix) and the argument rules of its entry points (semantics:
// include/k2hip.h, DESIGN.md "CTC prefix beam search").  No HIP in here: tests/native/engine_stub_ctc_prefix.cpp (the CPU stand-in of
// Engine::ctc_prefix_host) and tests/native/san_ctc_prefix_driver.cpp build it with a plain C++ compiler under AddressSanitizer / UBSan,
// and engine.cpp uses the same argument check.  Float32 throughout, any beam >= 1 (the device takes 1..8).
//
// A live hypothesis is a prefix y with pb (paths ending in blank), pnb (paths ending in y's last token) and tot = logaddexp(pb, pnb);
// the start is the empty prefix with pb = 0, pnb = -inf.  Frame t, live slots k = 0 .. n-1 with last token e_k:
//   stay candidate of slot k, flat index k V:        spb = tot_k + lp(t, 0), spnb = pnb_k + lp(t, e_k) (-inf for the empty prefix)
//   extension of slot k by v in 1 .. V-1:            x = (v == e_k ? pb_k : tot_k) + lp(t, v)
// THE FOLD RULE (written down here once; the twin tests/ctc_prefix_twin.py and the kernel follow it): if a live slot j spells
// y_k + [v] -- AS A TOKEN SEQUENCE, whatever history nodes the two came by -- the extension is no candidate of its own but joins j's
// stay candidate, spnb_j = logaddexp(spnb_j, x).  Live prefixes are pairwise distinct, so a slot receives at most one fold per frame.
// Every other extension is the candidate k V + v with pb = -inf, pnb = x.  A candidate's total is logaddexp(pb, pnb).
// THE TIE RULE: candidates whose total is not above -inf are dropped; the rest are ordered by total descending, exact float32 ties by
// the LOWER flat index; the first `beam` become the new slots in that order.  With no candidate left, slot 0's stay candidate alone
// survives (its scores are -inf from then on).
// A selected extension appends v with timestamp t and token log-prob lp(t, v) (the input value); a stay keeps the slot's history, also
// when it received a fold (the first-inserted rule).  After the last frame the slots are the result, entry 0 the best; score = tot.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "errors.h"

namespace k2hip {

constexpr int kCtcPrefixMaxBeam = 8;   // the device's beam limit (local lists and slots are unrolled over it)

// logaddexp(a, b) = m + log1p(exp(min - m)); a -inf operand gives the other one, two give -inf (never NaN)
inline float ctc_prefix_logaddexp(float a, float b) {
    const float m = a > b ? a : b, n = a > b ? b : a;
    if (n == -std::numeric_limits<float>::infinity()) return m;
    return m + log1pf(expf(n - m));
}

struct CtcPrefixRefHyp {
    std::vector<int64_t> tokens;
    std::vector<int32_t> timestamps;
    std::vector<float> token_log_probs;
    float pb = 0, pnb = 0, tot = 0;
    long long node = -1, parent_node = -1;   // history nodes: an extension makes a new one; only used to COUNT re-spelled folds
};
struct CtcPrefixRefResult {
    std::vector<CtcPrefixRefHyp> hyps;   // the live slots after the last frame, in rank order
    long long respelled_folds = 0;       // folds into a slot whose history parent is not the folded slot's node (the trap)
};

// lp: [T][ld] (ld >= V)
inline CtcPrefixRefResult ctc_prefix_ref(const float* lp, int64_t ld, int T, int V, int beam) {
    K2_REQUIRE(T >= 1 && V >= 1 && beam >= 1, "ctc_prefix_ref: T=%d V=%d beam=%d", T, V, beam);
    const float ninf = -std::numeric_limits<float>::infinity();
    struct Cand {
        float tot, pb, pnb;
        long long idx;
    };
    CtcPrefixRefResult res;
    std::vector<CtcPrefixRefHyp> cur(1), nxt;
    cur[0].pb = 0.f; cur[0].pnb = ninf; cur[0].tot = 0.f;
    long long next_node = 0;
    for (int t = 0; t < T; t++) {
        const float* row = lp + (size_t)t * (size_t)ld;
        const int n = (int)cur.size();
        // fold_into[k V + v] as a short list: (k, v) -> j
        std::vector<int> fold_par((size_t)n, -1);   // j -> the slot k whose extension by e_j spells j
        for (int j = 0; j < n; j++)
            for (int k = 0; k < n; k++) {
                if (j == k || cur[(size_t)j].tokens.size() != cur[(size_t)k].tokens.size() + 1) continue;
                if (std::equal(cur[(size_t)k].tokens.begin(), cur[(size_t)k].tokens.end(), cur[(size_t)j].tokens.begin())) {
                    fold_par[(size_t)j] = k;
                    if (cur[(size_t)j].parent_node != cur[(size_t)k].node) res.respelled_folds++;
                }
            }
        std::vector<Cand> cands;
        for (int k = 0; k < n; k++) {
            const CtcPrefixRefHyp& h = cur[(size_t)k];
            const int64_t e = h.tokens.empty() ? -1 : h.tokens.back();
            Cand s;
            s.idx = (long long)k * V;
            s.pb = h.tot + row[0];
            s.pnb = e >= 0 ? h.pnb + row[e] : ninf;
            if (fold_par[(size_t)k] >= 0) {
                const CtcPrefixRefHyp& p = cur[(size_t)fold_par[(size_t)k]];
                const int64_t ep = p.tokens.empty() ? -1 : p.tokens.back();
                s.pnb = ctc_prefix_logaddexp(s.pnb, (e == ep ? p.pb : p.tot) + row[e]);
            }
            s.tot = ctc_prefix_logaddexp(s.pb, s.pnb);
            cands.push_back(s);
            for (int v = 1; v < V; v++) {
                bool folded = false;
                for (int j = 0; j < n; j++) folded = folded || (fold_par[(size_t)j] == k && cur[(size_t)j].tokens.back() == v);
                if (folded) continue;
                const float x = (v == e ? h.pb : h.tot) + row[v];
                cands.push_back(Cand{x, ninf, x, (long long)k * V + v});
            }
        }
        const Cand stay0 = cands[0];
        cands.erase(std::remove_if(cands.begin(), cands.end(), [&](const Cand& c) { return !(c.tot > ninf); }), cands.end());
        std::sort(cands.begin(), cands.end(), [](const Cand& a, const Cand& b) { return a.tot > b.tot || (a.tot == b.tot && a.idx < b.idx); });
        if (cands.empty()) cands.push_back(stay0);
        if ((int)cands.size() > beam) cands.resize((size_t)beam);
        nxt.clear();
        for (const Cand& c : cands) {
            const int k = (int)(c.idx / V), v = (int)(c.idx % V);
            CtcPrefixRefHyp h = cur[(size_t)k];
            h.pb = c.pb; h.pnb = c.pnb; h.tot = c.tot;
            if (v) {
                h.tokens.push_back(v);
                h.timestamps.push_back(t);
                h.token_log_probs.push_back(row[v]);
                h.parent_node = h.node;
                h.node = next_node++;
            }
            nxt.push_back(std::move(h));
        }
        cur.swap(nxt);
    }
    res.hyps = std::move(cur);
    return res;
}

// The argument rules of k2hip_ctc_prefix_beam_search / Engine::ctc_prefix_host, checked before any device work
inline void ctc_prefix_check_args(int R, int Tp, int V, const int32_t* n_frames, int beam, int nbest, int max_tokens) {
    K2_REQUIRE(R >= 1 && R <= 65535, "ctc_prefix_beam_search: R = %d rows outside [1, 65535]", R);
    K2_REQUIRE(Tp >= 1 && V >= 1 && max_tokens >= 1, "ctc_prefix_beam_search: bad shape T'=%d V=%d max_tokens=%d", Tp, V, max_tokens);
    K2_REQUIRE(beam >= 1 && beam <= kCtcPrefixMaxBeam, "ctc_prefix_beam_search: beam %d out of range [1,%d]", beam, kCtcPrefixMaxBeam);
    K2_REQUIRE(nbest >= 1 && nbest <= beam, "ctc_prefix_beam_search: nbest %d out of range [1, beam = %d]", nbest, beam);
    if (n_frames)
        for (int r = 0; r < R; r++)
            K2_REQUIRE(n_frames[r] >= 1 && n_frames[r] <= Tp, "ctc_prefix_beam_search: row %d has n_frames = %d outside [1, T' = %d]", r, n_frames[r], Tp);
}

}  // namespace k2hip
