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

// THE FRAME STEP: the live slots `cur` over one frame's row, given the frame's fold table (fold_par[j] = the slot k with y_j = y_k +
// [e_j] as token sequences, or -1).  How the table is decided is the caller's: the whole-row search below compares token lists, the
// resumed search (tests/native/engine_stub_ctc_prefix_stream.cpp) goes through its relation tables.  A hypothesis' last token is
// `last` (-1 for the empty prefix): the resumed form does not hold the carried tokens.
struct CtcPrefixRefSlot {
    CtcPrefixRefHyp h;
    int64_t last = -1;
    int origin = 0;   // the carried slot a resumed search started this hypothesis from (h then holds the chunk's part only)
};
inline std::vector<CtcPrefixRefSlot> ctc_prefix_ref_frame(const std::vector<CtcPrefixRefSlot>& cur, const std::vector<int>& fold_par, const float* row,
                                                          int t, int V, int beam, long long* next_node) {
    const float ninf = -std::numeric_limits<float>::infinity();
    struct Cand {
        float tot, pb, pnb;
        long long idx;
    };
    const int n = (int)cur.size();
    std::vector<Cand> cands;
    for (int k = 0; k < n; k++) {
        const CtcPrefixRefHyp& h = cur[(size_t)k].h;
        const int64_t e = cur[(size_t)k].last;
        Cand s;
        s.idx = (long long)k * V;
        s.pb = h.tot + row[0];
        s.pnb = e >= 0 ? h.pnb + row[e] : ninf;
        if (fold_par[(size_t)k] >= 0) {
            const CtcPrefixRefSlot& p = cur[(size_t)fold_par[(size_t)k]];
            s.pnb = ctc_prefix_logaddexp(s.pnb, (e == p.last ? p.h.pb : p.h.tot) + row[e]);
        }
        s.tot = ctc_prefix_logaddexp(s.pb, s.pnb);
        cands.push_back(s);
        for (int v = 1; v < V; v++) {
            bool folded = false;
            for (int j = 0; j < n; j++) folded = folded || (fold_par[(size_t)j] == k && cur[(size_t)j].last == v);
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
    std::vector<CtcPrefixRefSlot> nxt;
    for (const Cand& c : cands) {
        const int k = (int)(c.idx / V), v = (int)(c.idx % V);
        CtcPrefixRefSlot s = cur[(size_t)k];
        s.h.pb = c.pb; s.h.pnb = c.pnb; s.h.tot = c.tot;
        if (v) {
            s.h.tokens.push_back(v);
            s.h.timestamps.push_back(t);
            s.h.token_log_probs.push_back(row[v]);
            s.h.parent_node = s.h.node;
            s.h.node = (*next_node)++;
            s.last = v;
        }
        nxt.push_back(std::move(s));
    }
    return nxt;
}

// lp: [T][ld] (ld >= V)
inline CtcPrefixRefResult ctc_prefix_ref(const float* lp, int64_t ld, int T, int V, int beam) {
    K2_REQUIRE(T >= 1 && V >= 1 && beam >= 1, "ctc_prefix_ref: T=%d V=%d beam=%d", T, V, beam);
    CtcPrefixRefResult res;
    std::vector<CtcPrefixRefSlot> cur(1);
    cur[0].h.pb = 0.f; cur[0].h.pnb = -std::numeric_limits<float>::infinity(); cur[0].h.tot = 0.f;
    long long next_node = 0;
    for (int t = 0; t < T; t++) {
        const int n = (int)cur.size();
        std::vector<int> fold_par((size_t)n, -1);   // j -> the slot k whose extension by e_j spells j
        for (int j = 0; j < n; j++)
            for (int k = 0; k < n; k++) {
                const CtcPrefixRefHyp &hj = cur[(size_t)j].h, &hk = cur[(size_t)k].h;
                if (j == k || hj.tokens.size() != hk.tokens.size() + 1) continue;
                if (std::equal(hk.tokens.begin(), hk.tokens.end(), hj.tokens.begin())) {
                    fold_par[(size_t)j] = k;
                    if (hj.parent_node != hk.node) res.respelled_folds++;
                }
            }
        cur = ctc_prefix_ref_frame(cur, fold_par, lp + (size_t)t * (size_t)ld, t, V, beam, &next_node);
    }
    for (CtcPrefixRefSlot& s : cur) res.hyps.push_back(std::move(s.h));
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

// The argument rules of the resumed search's chunk (k2hip_ctc_prefix_beam_search_chunk / Engine::ctc_prefix_chunk_host / the debug op),
// checked before any device work; in: [B] blocks of `in_ints` ints laid out as CtcPrefixResumeLayout{K, Tc} (the offsets are passed in:
// this header knows no layout), of which the kernel indexes with n, the last tokens and the relation lengths
inline void ctc_prefix_chunk_check_args(int B, int Tc, int V, const int32_t* n_frames, int K, const int* in, int in_ints, int o_e, int o_rel) {
    K2_REQUIRE(B >= 1 && B <= 65535, "ctc_prefix_beam_search_chunk: B = %d streams outside [1, 65535]", B);
    K2_REQUIRE(Tc >= 1 && V >= 1 && (long long)Tc * kCtcPrefixMaxBeam <= (1 << 30), "ctc_prefix_beam_search_chunk: bad shape Tc=%d V=%d", Tc, V);
    K2_REQUIRE(K >= 1 && K <= kCtcPrefixMaxBeam, "ctc_prefix_beam_search_chunk: beam %d out of range [1,%d]", K, kCtcPrefixMaxBeam);
    if (n_frames)
        for (int b = 0; b < B; b++)
            K2_REQUIRE(n_frames[b] >= 1 && n_frames[b] <= Tc, "ctc_prefix_beam_search_chunk: stream %d has n_frames = %d outside [1, Tc = %d]", b, n_frames[b], Tc);
    K2_REQUIRE(in, "ctc_prefix_beam_search_chunk: null in blocks");
    for (int b = 0; b < B; b++) {
        const int* blk = in + (size_t)b * (size_t)in_ints;
        K2_REQUIRE(blk[0] >= 1 && blk[0] <= K, "ctc_prefix_beam_search_chunk: stream %d carries %d prefixes (beam %d)", b, blk[0], K);
        for (int k = 0; k < K; k++) {
            K2_REQUIRE(blk[o_e + k] >= -1 && blk[o_e + k] < V && blk[o_e + k] != 0, "ctc_prefix_beam_search_chunk: stream %d slot %d ends in token %d", b, k, blk[o_e + k]);
            for (int j = 0; j < K; j++)
                K2_REQUIRE(blk[o_rel + k * K + j] >= -1 && blk[o_rel + k * K + j] <= Tc, "ctc_prefix_beam_search_chunk: stream %d: relation %d", b, blk[o_rel + k * K + j]);
        }
    }
}

}  // namespace k2hip
