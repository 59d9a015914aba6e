// Host reference of the BIASED CTC prefix beam search of ctc_prefix.hip (k_ctc_prefix<false, true>) and the host-side check of the tables
// it indexes with (semantics: include/k2hip.h "Hotword and n-gram LM biasing of the CTC prefix beam search").  No HIP in here: float32
// throughout, built on ctc_prefix_ref.h's hypotheses, logaddexp and fold rule; tests/native/san_ctc_prefix_bias_driver.cpp builds it with
// a plain C++ compiler under AddressSanitizer / UBSan, and engine.cpp uses the same table check before a debug launch.
//
// Every live slot carries hs (hotword graph state, start 0), ls (LM state, start `start`) and ctx (float32, start 0) beside the acoustic
// pb / pnb / tot.  Keys: stay st_k + ctx_k; extension cb = ctx_k + bonus[hs_k][v], key x + cb.  A candidate is dropped when its ACOUSTIC
// total is -inf; order (key desc, flat index asc).  A selected extension takes hs' = next[hs_k][v], then (term, ls') = Step(ls_k, v)
// over the scaled tables (skipped for unk) and ctx' = cb + term.  final = (tot + ctx) - pending[hs]; entries by (final desc, slot asc).
#pragma once
#include <cstring>

#include "../../include/k2hip.h"
#include "ctc_prefix_ref.h"

namespace k2hip {

// The tables as the kernel reads them, on the host.  next == null: no hotwords; states == null: no LM.
struct CtcPrefixBiasTables {
    int V = 0;
    int S = 0;                           // hotword states: next / bonus [S][V], pending [S]
    const int32_t* next = nullptr;
    const float* bonus = nullptr;
    const float* pending = nullptr;
    int S_lm = 0;                        // LM states [S_lm][4] = (arc begin, arc end, back-off state, back-off weight bits)
    long long A = 0;                     // arcs: arc_tok / arc_lp / arc_next [A]; uni_lp / uni_next [V]
    const int32_t* states = nullptr;
    const int32_t* arc_tok = nullptr;
    const float* arc_lp = nullptr;
    const int32_t* arc_next = nullptr;
    const float* uni_lp = nullptr;
    const int32_t* uni_next = nullptr;
    int start = 0;
};

// Everything the kernel INDEXES with, before any launch: a bad table must not be able to fault the device
inline void ctc_prefix_bias_check_tables(const CtcPrefixBiasTables& t) {
    K2_REQUIRE(t.V >= 1, "ctc_prefix biasing: V = %d", t.V);
    if (t.next) {
        K2_REQUIRE(t.bonus && t.pending && t.S >= 1, "ctc_prefix biasing: incomplete hotword tables (S = %d)", t.S);
        for (long long i = 0; i < (long long)t.S * t.V; i++)
            K2_REQUIRE(t.next[i] >= 0 && t.next[i] < t.S, "ctc_prefix biasing: next[%lld][%lld] = %d outside [0, S = %d)", i / t.V, i % t.V, t.next[i], t.S);
    }
    if (t.states) {
        K2_REQUIRE(t.uni_lp && t.uni_next && t.S_lm >= 1 && t.A >= 0 && (t.A == 0 || (t.arc_tok && t.arc_lp && t.arc_next)),
                   "ctc_prefix biasing: incomplete LM tables (S = %d, A = %lld)", t.S_lm, t.A);
        K2_REQUIRE(t.start >= 0 && t.start < t.S_lm, "ctc_prefix biasing: LM start state %d outside [0, %d)", t.start, t.S_lm);
        for (int s = 0; s < t.S_lm; s++) {
            const int32_t* st = t.states + 4 * (size_t)s;
            K2_REQUIRE(st[0] >= 0 && st[0] <= st[1] && st[1] <= t.A, "ctc_prefix biasing: LM state %d has the arc range [%d, %d) outside [0, A = %lld]", s, st[0], st[1], t.A);
            K2_REQUIRE(st[2] >= 0 && st[2] < t.S_lm, "ctc_prefix biasing: LM state %d backs off to state %d outside [0, %d)", s, st[2], t.S_lm);
            for (int i = st[0] + 1; i < st[1]; i++)
                K2_REQUIRE(t.arc_tok[i - 1] < t.arc_tok[i], "ctc_prefix biasing: the arcs of LM state %d are not sorted by token", s);
        }
        for (long long i = 0; i < t.A; i++)
            K2_REQUIRE(t.arc_next[i] >= 0 && t.arc_next[i] < t.S_lm, "ctc_prefix biasing: arc_next[%lld] = %d outside [0, %d)", i, t.arc_next[i], t.S_lm);
        for (int v = 0; v < t.V; v++)
            K2_REQUIRE(t.uni_next[v] >= 0 && t.uni_next[v] < t.S_lm, "ctc_prefix biasing: uni_next[%d] = %d outside [0, %d)", v, t.uni_next[v], t.S_lm);
    }
}

// The resumed biased search's side in block [flags | ctx[K] | hs[K] | ls[K]] of one stream, before any launch: every carried hs inside
// that stream's graph (S states; S = 0: no graph, every hs must be 0), every carried ls inside the LM when the row runs it (flag bit 0;
// S_lm = 0: the call has no LM, the flag must be clear)
inline void ctc_prefix_bias_check_side_in(const int* side, int K, int S, int S_lm, int stream) {
    K2_REQUIRE((side[0] & ~1) == 0 && (!(side[0] & 1) || S_lm >= 1), "ctc_prefix biasing: stream %d has the flags %d (LM states: %d)", stream, side[0], S_lm);
    for (int k = 0; k < K; k++) {
        const int hs = side[1 + K + k], ls = side[1 + 2 * K + k];
        K2_REQUIRE(hs >= 0 && hs < (S >= 1 ? S : 1), "ctc_prefix biasing: stream %d slot %d carries the hotword state %d outside [0, %d)", stream, k, hs, S >= 1 ? S : 1);
        K2_REQUIRE(!(side[0] & 1) || (ls >= 0 && ls < S_lm), "ctc_prefix biasing: stream %d slot %d carries the LM state %d outside [0, %d)", stream, k, ls, S_lm);
    }
}

// Step(s, tok) over the sparse tables as beam_lm_walk (lm_walk.h) takes it: at most order - 1 levels, then state 0's dense row
inline void ctc_prefix_bias_lm_step(const CtcPrefixBiasTables& t, int s, int tok, float* term, int* next) {
    float acc = 0.f;
    for (int lvl = 0; lvl < K2HIP_NGRAM_MAX_ORDER - 1 && s != 0; lvl++) {
        const int32_t* st = t.states + 4 * (size_t)s;
        const int32_t* hit = std::lower_bound(t.arc_tok + st[0], t.arc_tok + st[1], tok);
        if (hit != t.arc_tok + st[1] && *hit == tok) {
            *term = acc + t.arc_lp[hit - t.arc_tok];
            *next = t.arc_next[hit - t.arc_tok];
            return;
        }
        float bow;
        memcpy(&bow, &st[3], sizeof bow);
        acc = acc + bow;
        s = st[2];
    }
    *term = acc + t.uni_lp[tok];
    *next = t.uni_next[tok];
}

struct CtcPrefixBiasRefHyp {
    CtcPrefixRefHyp h;        // tokens, timestamps, token log-probs, the ACOUSTIC pb / pnb / tot
    int hs = 0, ls = 0;
    float ctx = 0.f;
    float final_score = 0.f;
    int slot = 0;             // the slot it held after the last frame
};
struct CtcPrefixBiasRefResult {
    std::vector<CtcPrefixBiasRefHyp> hyps;   // in (final desc, slot asc) order
    long long respelled_folds = 0;
};

// (ctx, hs, ls) of a token sequence: the additions the search makes, in its order
inline void ctc_prefix_bias_walk(const CtcPrefixBiasTables& t, const std::vector<int64_t>& tokens, float* ctx, int* hs, int* ls) {
    *ctx = 0.f; *hs = 0; *ls = t.states ? t.start : 0;
    for (int64_t v : tokens) {
        if (t.next) {
            *ctx += t.bonus[(size_t)*hs * t.V + v];
            *hs = t.next[(size_t)*hs * t.V + v];
        }
        float term = 0.f;
        if (t.states && v != K2HIP_UNK_ID) ctc_prefix_bias_lm_step(t, *ls, (int)v, &term, ls);
        *ctx = *ctx + term;
    }
}

// lp: [T][ld] (ld >= V = tb.V); the tables have passed ctc_prefix_bias_check_tables
inline CtcPrefixBiasRefResult ctc_prefix_bias_ref(const float* lp, int64_t ld, int T, int beam, const CtcPrefixBiasTables& tb) {
    const int V = tb.V;
    K2_REQUIRE(T >= 1 && V >= 1 && beam >= 1, "ctc_prefix_bias_ref: T=%d V=%d beam=%d", T, V, beam);
    const float ninf = -std::numeric_limits<float>::infinity();
    CtcPrefixBiasRefResult res;
    std::vector<CtcPrefixBiasRefHyp> cur(1);
    cur[0].h.pb = 0.f; cur[0].h.pnb = ninf; cur[0].h.tot = 0.f;
    cur[0].ls = tb.states ? tb.start : 0;
    long long next_node = 0;
    struct Cand {
        float key, tot, pb, pnb, cb;
        long long idx;
    };
    for (int t = 0; t < T; t++) {
        const float* row = lp + (size_t)t * (size_t)ld;
        const int n = (int)cur.size();
        std::vector<int> fold_par((size_t)n, -1);   // THE FOLD RULE of ctc_prefix_ref.h: sequence identity
        for (int j = 0; j < n; j++)
            for (int k = 0; k < n; k++) {
                const CtcPrefixRefHyp &hj = cur[(size_t)j].h, &hk = cur[(size_t)k].h;
                if (j == k || hj.tokens.size() != hk.tokens.size() + 1) continue;
                if (std::equal(hk.tokens.begin(), hk.tokens.end(), hj.tokens.begin())) {
                    fold_par[(size_t)j] = k;
                    if (hj.parent_node != hk.node) res.respelled_folds++;
                }
            }
        auto last = [&](int k) { return cur[(size_t)k].h.tokens.empty() ? (int64_t)-1 : cur[(size_t)k].h.tokens.back(); };
        std::vector<Cand> cands;
        for (int k = 0; k < n; k++) {
            const CtcPrefixBiasRefHyp& s = cur[(size_t)k];
            const int64_t e = last(k);
            Cand c;
            c.idx = (long long)k * V;
            c.pb = s.h.tot + row[0];
            c.pnb = e >= 0 ? s.h.pnb + row[e] : ninf;
            if (fold_par[(size_t)k] >= 0) {
                const int p = fold_par[(size_t)k];
                c.pnb = ctc_prefix_logaddexp(c.pnb, (e == last(p) ? cur[(size_t)p].h.pb : cur[(size_t)p].h.tot) + row[e]);
            }
            c.tot = ctc_prefix_logaddexp(c.pb, c.pnb);
            c.cb = s.ctx;
            c.key = c.tot + s.ctx;
            cands.push_back(c);
            for (int v = 1; v < V; v++) {
                bool folded = false;
                for (int j = 0; j < n; j++) folded = folded || (fold_par[(size_t)j] == k && last(j) == v);
                if (folded) continue;
                const float x = (v == e ? s.h.pb : s.h.tot) + row[v];
                float cb = s.ctx;
                if (tb.next) cb += tb.bonus[(size_t)s.hs * V + v];
                cands.push_back(Cand{x + cb, x, ninf, x, cb, (long long)k * V + v});
            }
        }
        const Cand stay0 = cands[0];
        cands.erase(std::remove_if(cands.begin(), cands.end(), [&](const Cand& c) { return !(c.tot > ninf); }), cands.end());
        std::sort(cands.begin(), cands.end(), [](const Cand& a, const Cand& b) { return a.key > b.key || (a.key == b.key && a.idx < b.idx); });
        if (cands.empty()) cands.push_back(stay0);
        if ((int)cands.size() > beam) cands.resize((size_t)beam);
        std::vector<CtcPrefixBiasRefHyp> nxt;
        for (const Cand& c : cands) {
            const int k = (int)(c.idx / V), v = (int)(c.idx % V);
            CtcPrefixBiasRefHyp s = cur[(size_t)k];
            s.h.pb = c.pb; s.h.pnb = c.pnb; s.h.tot = c.tot;
            if (v) {
                s.h.tokens.push_back(v);
                s.h.timestamps.push_back(t);
                s.h.token_log_probs.push_back(row[v]);
                s.h.parent_node = s.h.node;
                s.h.node = next_node++;
                if (tb.next) s.hs = tb.next[(size_t)s.hs * V + v];
                float term = 0.f;
                if (tb.states && v != K2HIP_UNK_ID) ctc_prefix_bias_lm_step(tb, s.ls, v, &term, &s.ls);
                s.ctx = c.cb + term;
            }
            nxt.push_back(std::move(s));
        }
        cur = std::move(nxt);
    }
    for (size_t q = 0; q < cur.size(); q++) {
        const float fv = cur[q].h.tot + cur[q].ctx;
        cur[q].final_score = tb.next ? fv - tb.pending[cur[q].hs] : fv;
        cur[q].slot = (int)q;
    }
    std::stable_sort(cur.begin(), cur.end(), [](const CtcPrefixBiasRefHyp& a, const CtcPrefixBiasRefHyp& b) { return a.final_score > b.final_score; });
    res.hyps = std::move(cur);
    return res;
}

}  // namespace k2hip
