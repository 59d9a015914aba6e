// Host reference of the CTC keyword spotter's token passing (ctc_kws.hip k_ctc_trie_dp), float32, header only: what the GPU kernel is
// compared with bit for bit, and what the CPU stand-in of the engine under tests/native runs.  Semantics: include/k2hip.h "Keyword
// spotting for CTC models".
//
// One stream: log-probs lp [T][V] (finite or -inf, blank = column 0), the trie as parent / tok / depth / kw / bar / rc [S], the carried
// block v [2][S] / st [2][S] updated in place.  Plane 0 is n (the path's last frame carried tok(c)), plane 1 is b (the path sits in
// blanks after tok(c)).  The root's n entry is (0, frame count), the root's b entry is (-inf, hold).  A cell whose value is -inf
// carries start = -1, so that the block is one function of the frames seen so far, whatever the chunking.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "kws_ref.h"

namespace k2hip {

inline void ctc_kws_fresh_state(int S, float* v, int32_t* st) {
    for (int s = 0; s < 2 * S; s++) {
        v[s] = s == 0 ? 0.f : -INFINITY;
        st[s] = s == 0 ? 0 : -1;
    }
}

// rc(s): the root's child whose token equals tok(s), or -1 (rc(0) = -1)
inline void ctc_kws_root_children(const int32_t* parent, const int32_t* tok, int S, int32_t* rc) {
    for (int s = 0; s < S; s++) {
        rc[s] = -1;
        for (int r = 1; s > 0 && r < S; r++)
            if (parent[r] == 0 && tok[r] == tok[s]) {
                rc[s] = r;
                break;
            }
    }
}

inline void ctc_kws_dp_ref(const int32_t* parent, const int32_t* tok, const int32_t* depth, const int32_t* kw, const float* bar, const int32_t* rc,
                           int S, const float* lp, int V, int T, float* v, int32_t* st, std::vector<KwsRefEvent>* events) {
    float *n = v, *b = v + S;
    int32_t *sn = st, *sb = st + S;
    std::vector<float> nn((size_t)S), nb((size_t)S);
    std::vector<int32_t> nsn((size_t)S), nsb((size_t)S), entered((size_t)S);
    for (int t = 0; t < T; t++) {
        const float* row = lp + (size_t)t * V;
        const int32_t ta = sn[0];   // the absolute index of this frame
        int32_t hold = sb[0];
        bool closed = false;
        if (hold >= 0) {
            if (row[tok[hold]] >= row[0]) closed = true;
            else hold = -1;
        }
        for (int c = 1; c < S; c++) {
            const int p = parent[c];
            // the predecessors in tie order: n[parent], b[parent], the self loop
            float best = -INFINITY;
            int32_t bs = -1;
            if (p == 0) {
                if (!(closed && c == hold)) { best = 0.f; bs = ta; }
            } else {
                if (tok[p] != tok[c]) { best = n[p]; bs = sn[p]; }
                if (b[p] > best) { best = b[p]; bs = sb[p]; }
            }
            bool self = false;
            if (n[c] > best) { best = n[c]; bs = sn[c]; self = true; }
            nn[(size_t)c] = best + row[tok[c]];
            nsn[(size_t)c] = bs;
            if (!(nn[(size_t)c] > -INFINITY)) nsn[(size_t)c] = -1;
            entered[(size_t)c] = !self && nn[(size_t)c] > -INFINITY;
            const bool from_n = n[c] >= b[c];   // the tie rule: n wins
            nb[(size_t)c] = (from_n ? n[c] : b[c]) + row[0];
            nsb[(size_t)c] = from_n ? sn[c] : sb[c];
            if (!(nb[(size_t)c] > -INFINITY)) nsb[(size_t)c] = -1;
        }
        // the frame's event: largest depth, then largest n, then smallest keyword
        int win = -1;
        for (int c = 1; c < S; c++) {
            if (kw[c] < 0 || !entered[(size_t)c] || !(nn[(size_t)c] >= bar[c])) continue;
            if (win < 0 || depth[c] > depth[win] || (depth[c] == depth[win] && (nn[(size_t)c] > nn[(size_t)win] ||
                                                                                (nn[(size_t)c] == nn[(size_t)win] && kw[c] < kw[win]))))
                win = c;
        }
        if (win >= 0) {
            if (events) events->push_back(KwsRefEvent{kw[win], nsn[(size_t)win], ta, nn[(size_t)win]});
            hold = rc[win];
            for (int c = 1; c < S; c++) {
                nn[(size_t)c] = nb[(size_t)c] = -INFINITY;
                nsn[(size_t)c] = nsb[(size_t)c] = -1;
            }
        }
        for (int c = 1; c < S; c++) {
            n[c] = nn[(size_t)c]; sn[c] = nsn[(size_t)c];
            b[c] = nb[(size_t)c]; sb[c] = nsb[(size_t)c];
        }
        sn[0] = ta + 1;
        sb[0] = hold;
    }
}

}  // namespace k2hip
