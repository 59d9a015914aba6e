// Host reference of the sample-rate converter (resample.hip k_resample_gather), float32, header only: what the GPU kernel is compared
// with bit for bit (the sign of a zero aside), and what the CPU stand-in of the engine under tests/native runs.
//
// Per output: acc = +0.0f, then acc = fmaf(w[p][j], x[...], acc) for j ascending; a tap in front of the stream's first sample
// contributes x = 0.  The carried state is the tail of the input that later outputs still read, plus the two running counts; with it
// any chunking of a signal gives the same bits as one push.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "resample_plan.h"

namespace k2hip {

struct ResampleRefState {
    std::vector<float> tail;   // input samples [n_in - tail.size(), n_in)
    int64_t n_in = 0, n_out = 0;
};

// one output from a block of input whose first float is input sample x0
inline float resample_ref_dot(const ResamplePlan& p, int64_t k, const float* x, int64_t x0) {
    const size_t ph = (size_t)(k % p.ou);
    const int64_t s = p.start(k);
    const float* w = p.w.data() + ph * (size_t)p.max_taps;
    float acc = 0.0f;
    for (int j = 0; j < p.ntaps[ph]; j++) acc = fmaf(w[j], s + j < 0 ? 0.0f : x[s + j - x0], acc);
    return acc;
}

// push n samples; the outputs they complete are appended to *out
inline void resample_ref_push(const ResamplePlan& p, ResampleRefState& st, const float* x, int64_t n, std::vector<float>* out) {
    std::vector<float> blk(st.tail);
    blk.insert(blk.end(), x, x + n);
    const int64_t x0 = st.n_in - (int64_t)st.tail.size();
    st.n_in += n;
    const int64_t k1 = p.num_out(st.n_in);
    for (int64_t k = st.n_out; k < k1; k++) out->push_back(resample_ref_dot(p, k, blk.data(), x0));
    st.n_out = k1;
    const int64_t keep = p.keep_from(k1) < st.n_in ? p.keep_from(k1) : st.n_in;
    st.tail.assign(blk.begin() + (keep - x0), blk.end());
}

}  // namespace k2hip
