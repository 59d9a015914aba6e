// rnn_lm_plan.h: the row layout and time blocks of one neural-LM scoring call.
#include "rnn_lm_plan.h"

#include <algorithm>
#include <numeric>

#include "errors.h"

namespace k2hip {

RnnLmPlan rnn_lm_plan(const int64_t* offsets, int Hn, bool with_eos, int H, int64_t gx_cap_floats) {
    RnnLmPlan p;
    p.Hn = Hn;
    std::vector<int64_t> P((size_t)Hn), off((size_t)Hn);
    int64_t total = 0, longest = 0;
    for (int i = 0; i < Hn; i++) {
        P[(size_t)i] = offsets[i + 1] - offsets[i] + (with_eos ? 1 : 0);
        off[(size_t)i] = total;
        total += P[(size_t)i];
        longest = std::max(longest, P[(size_t)i]);
        K2_REQUIRE(total <= kRnnLmMaxRows, "rnn_lm_score: hypothesis %d brings the call to %lld positions, more than the limit of %lld rows", i,
                   (long long)total, (long long)kRnnLmMaxRows);
    }
    p.R = total;
    p.T = (int)longest;
    p.order.resize((size_t)Hn);
    std::iota(p.order.begin(), p.order.end(), 0);
    std::stable_sort(p.order.begin(), p.order.end(), [&](int32_t a, int32_t b) { return P[(size_t)a] > P[(size_t)b]; });
    p.npos.resize((size_t)Hn);
    p.out_off.resize((size_t)Hn);
    for (int j = 0; j < Hn; j++) {
        p.npos[(size_t)j] = (int32_t)P[(size_t)p.order[(size_t)j]];
        p.out_off[(size_t)j] = off[(size_t)p.order[(size_t)j]];
    }
    p.active.assign((size_t)p.T, 0);
    p.base.assign((size_t)p.T + 1, 0);
    int a = Hn;
    for (int t = 0; t < p.T; t++) {
        while (a > 0 && p.npos[(size_t)a - 1] <= t) a--;
        p.active[(size_t)t] = a;
        p.base[(size_t)t + 1] = p.base[(size_t)t] + a;
    }
    const int64_t cap_rows = std::max<int64_t>(gx_cap_floats / (4 * (int64_t)std::max(H, 1)), 1);
    p.block.push_back(0);
    for (int t = 0; t < p.T; t++)
        if (t > p.block.back() && p.base[(size_t)t + 1] - p.base[(size_t)p.block.back()] > cap_rows) p.block.push_back(t);
    p.block.push_back(p.T);
    if (p.T == 0) p.block.assign(1, 0);
    return p;
}

}  // namespace k2hip
