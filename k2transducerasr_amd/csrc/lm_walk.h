// The n-gram LM's step over the scaled device tables (BeamLm, kernels.h) by one whole wave: shared by the searches that fuse the LM
// (beam.hip, ctc_prefix.hip).  Device code only; every lane of the wave must be active at a call.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace k2hip {

// Step(state, tok) of the n-gram LM (ngram_lm.h) over the scaled device tables, by one whole wave: per level ONE 16-byte load of the
// state, then the 64 lanes search its sorted arcs together -- a 64-ary narrowing while the range is longer than a wave, then one
// compare per lane with the arc's weight and next state loaded beside the token (no load depends on the vote), and a wave vote.  A
// miss adds the back-off weight and moves on; state 0 is a dense row, so every walk ends in one direct load.  At most order - 1 levels.
__device__ __forceinline__ void beam_lm_walk(const BeamLm& lm, int s, int tok, int lane, float* term, int* next) {
    float acc = 0.f;
    for (int lvl = 0; lvl < K2HIP_NGRAM_MAX_ORDER - 1 && s != 0; lvl++) {   // (a state's history is at most order - 1 tokens long)
        const int4 st = lm.states[s];
        int lo = st.x, n = st.y - st.x;
        while (n > 64) {
            const int stride = (n + 63) >> 6, i = lo + lane * stride;
            const unsigned long long le = __ballot(lane * stride < n && lm.arc_tok[i] <= tok);   // (sorted: a prefix of the lanes)
            if (!le) { n = 0; break; }
            const int j = 63 - __clzll(le);
            n = min(stride, n - j * stride);
            lo += j * stride;
        }
        const bool in = lane < n;
        const int tk = in ? lm.arc_tok[lo + lane] : -1;
        const float lpv = in ? lm.arc_lp[lo + lane] : 0.f;
        const int nxv = in ? lm.arc_next[lo + lane] : 0;
        const unsigned long long hit = __ballot(in && tk == tok);
        if (hit) {
            const int src = __ffsll(hit) - 1;
            *term = acc + __shfl(lpv, src);
            *next = __shfl(nxv, src);
            return;
        }
        acc = acc + __int_as_float(st.w);
        s = st.z;
    }
    *term = acc + lm.uni_lp[tok];
    *next = lm.uni_next[tok];
}

}  // namespace k2hip
