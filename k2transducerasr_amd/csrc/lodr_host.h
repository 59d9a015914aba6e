// LODR on the host: the model's copy of the low-order LM's SCALED automaton (ngram_lm.h NgramDeviceForm, every weight multiplied by the
// scale <= 0 once) and the walk over it that the rescoring of an N-best list uses -- the same step, in the same float32 order, as the
// device's beam_lm_walk over the same tables (lm_walk.h), so a total computed here is the sum of the terms a fused search would add.
// Plain C++ (no HIP): tests/native builds it on the CPU.
#pragma once
#include <cstdint>
#include <cstring>

#include "ngram_lm.h"

namespace k2hip {

struct LodrHost {
    NgramDeviceForm d;
    int start = 0, V = 0;

    int num_states() const { return (int)(d.states.size() / 4); }
    // Step(state, tok) over the scaled tables: back-off weights first, then the arc, float32.  Blank, unk and anything outside the
    // vocabulary earn nothing and keep the state.
    void step(int s, int64_t tok, int* next, float* term) const {
        if (tok == K2HIP_BLANK_ID || tok == K2HIP_UNK_ID || tok < 0 || tok >= V || s < 0 || s >= num_states()) {
            *next = s;
            *term = 0.f;
            return;
        }
        float acc = 0.f;
        for (int lvl = 0; lvl < K2HIP_NGRAM_MAX_ORDER - 1 && s != 0; lvl++) {
            const int32_t* st = &d.states[(size_t)s * 4];
            int lo = st[0], hi = st[1];
            while (lo < hi) {   // the arcs of a state are sorted by token
                const int mid = lo + (hi - lo) / 2;
                if (d.arc_tok[(size_t)mid] < tok) lo = mid + 1;
                else hi = mid;
            }
            if (lo < st[1] && d.arc_tok[(size_t)lo] == tok) {
                *term = acc + d.arc_lp[(size_t)lo];
                *next = d.arc_next[(size_t)lo];
                return;
            }
            float bow;
            memcpy(&bow, &st[3], sizeof(float));
            acc = acc + bow;
            s = st[2];
        }
        *term = acc + d.uni_lp[(size_t)tok];
        *next = d.uni_next[(size_t)tok];
    }
    // lodr_i of the rescoring: the float32 sum, in token order from the start state, of the steps of tokens[0 .. n); no eos term
    float total(const int64_t* tokens, size_t n) const {
        volatile float acc = 0.f;   // (every partial sum rounded to float32)
        int s = start;
        for (size_t i = 0; i < n; i++) {
            float term;
            step(s, tokens[i], &s, &term);
            acc = acc + term;
        }
        return acc;
    }
};

}  // namespace k2hip
