// Host plan of one neural-LM scoring call (DESIGN.md "Neural LM rescoring").  Pure host code (no HIP).
//
// Hypothesis i has P_i positions (its length, + 1 with_eos).  The hypotheses are sorted by P descending, stably; rows are laid out
// time-major: a_t = the number of hypotheses with more than t positions, base_t = sum of a_s over s < t, and the row of (position t,
// j-th longest hypothesis) is base_t + j.  The active rows of a step are then one contiguous prefix of the sorted order, and step
// t - 1's h rows are step t's A operand with no gather and no mask.  R = base_T rows in all, T = the longest P.
//
// The input products GX = X . W_ih^T + b of a layer take 4 H floats per row.  When R 4 H floats exceed gx_cap_floats the plan cuts time
// into blocks [block[b], block[b + 1]) whose rows fit the cap (a single step that exceeds it is a block of its own), and GX is formed
// per block.
#pragma once
#include <cstdint>
#include <vector>

namespace k2hip {

constexpr int64_t kRnnLmMaxRows = (int64_t)1 << 22;            // rows (positions of all hypotheses) of one scoring call at most
constexpr int64_t kRnnLmGxCapFloats = (int64_t)1 << 26;        // 256 MiB of GX per time block unless the tunable says otherwise

struct RnnLmPlan {
    int Hn = 0, T = 0;
    int64_t R = 0;
    std::vector<int32_t> order;    // [Hn]: order[j] = the caller's index of the j-th longest hypothesis
    std::vector<int32_t> npos;     // [Hn]: its positions P
    std::vector<int64_t> out_off;  // [Hn]: where its token log-probs start in the caller's packed array
    std::vector<int32_t> active;   // [T]: a_t
    std::vector<int64_t> base;     // [T + 1]: base_t
    std::vector<int32_t> block;    // [n_blocks + 1]: time blocks
};

// offsets [Hn + 1] non-decreasing (checked by the caller); throws Error(K2HIP_ERR_INVALID) when R exceeds kRnnLmMaxRows
RnnLmPlan rnn_lm_plan(const int64_t* offsets, int Hn, bool with_eos, int H, int64_t gx_cap_floats);

}  // namespace k2hip
