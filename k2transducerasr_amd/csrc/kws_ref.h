// Host reference of the keyword spotter's token passing (kws.hip k_trie_dp), float32, header only: what the GPU kernel is compared
// with bit for bit, and what the CPU stand-in of the engine under tests/native runs.  Semantics: include/k2hip.h "Keyword spotting".
//
// One stream: planes stay / emit [T][S] (emit(t, c) is the arc INTO c; column 0 of emit is not read), the trie as parent / depth /
// kw / bar [S], the carried block a / start [S] updated in place.  The carried block of a fresh stream is kws_fresh_state(): a(0) = 0,
// start(0) = 0 (the root's start is the stream's frame count), every other state (-inf, -1).  A state whose value is -inf carries
// start = -1, so that the block is one function of the frames seen so far, whatever the chunking.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace k2hip {

struct KwsRefEvent {
    int32_t keyword, start, end;
    float sum_logp;
};

inline void kws_fresh_state(int S, float* a, int32_t* start) {
    for (int s = 0; s < S; s++) {
        a[s] = s == 0 ? 0.f : -INFINITY;
        start[s] = s == 0 ? 0 : -1;
    }
}

inline void kws_dp_ref(const int32_t* parent, const int32_t* depth, const int32_t* kw, const float* bar, int S, const float* stay,
                       const float* emit, int T, float* a, int32_t* start, std::vector<KwsRefEvent>* events) {
    std::vector<float> na((size_t)S);
    std::vector<int32_t> ns((size_t)S), by_emit((size_t)S);
    for (int t = 0; t < T; t++) {
        const int32_t ta = start[0];   // the absolute index of this frame
        for (int c = 1; c < S; c++) {
            const int p = parent[c];
            const float ap = p == 0 ? 0.f : a[p];
            const int32_t sp = p == 0 ? ta : start[p];
            const float ve = ap + emit[(size_t)t * S + c];
            const float vs = a[c] + stay[(size_t)t * S + c];
            const bool e = ve >= vs;   // the tie rule: emit wins
            na[(size_t)c] = e ? ve : vs;
            ns[(size_t)c] = e ? sp : start[c];
            if (!(na[(size_t)c] > -INFINITY)) ns[(size_t)c] = -1;
            by_emit[(size_t)c] = e;
        }
        // the frame's event: largest depth, then largest a, then smallest keyword
        int win = -1;
        for (int c = 1; c < S; c++) {
            if (kw[c] < 0 || !by_emit[(size_t)c] || !(na[(size_t)c] >= bar[c])) continue;
            if (win < 0 || depth[c] > depth[win] || (depth[c] == depth[win] && (na[(size_t)c] > na[(size_t)win] ||
                                                                                (na[(size_t)c] == na[(size_t)win] && kw[c] < kw[win]))))
                win = c;
        }
        if (win >= 0) {
            if (events) events->push_back(KwsRefEvent{kw[win], ns[(size_t)win], ta, na[(size_t)win]});
            for (int c = 1; c < S; c++) {
                na[(size_t)c] = -INFINITY;
                ns[(size_t)c] = -1;
            }
        }
        for (int c = 1; c < S; c++) {
            a[c] = na[(size_t)c];
            start[c] = ns[(size_t)c];
        }
        start[0] = ta + 1;
    }
}

}  // namespace k2hip
