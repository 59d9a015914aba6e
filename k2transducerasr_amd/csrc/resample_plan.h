// The sample-rate converter's filter as a pure host plan (no GPU): Kaldi's LinearResample written from its definition -- a Hann-windowed
// sinc with num_zeros = 6 and cutoff fc = 0.99 * 0.5 * min(fi, fo), flush = false.  DESIGN.md "Input at other sample rates".
//
// Units: g = gcd(fi, fo), iu = fi / g, ou = fo / g, one second = lcm = fi * ou = fo * iu ticks; input sample j sits at tick j * ou,
// output sample k at tick k * iu.  Output k = u * ou + p (phase p < ou) is
//     y[k] = sum_{j < ntaps[p]} w[p][j] * x[first[p] + u * iu + j],         x = 0 in front of the stream's first sample,
// over the input samples strictly inside the window: |j * ou - p * iu| < ww * lcm = 600 * lcm / (99 * min(fi, fo)) ticks.  Every count
// comes from int64 arithmetic (wmax = the largest whole tick distance strictly inside the window), so the C++, the Python twin of the
// tests and the kernel agree exactly; floating point only enters the weights, computed in double and rounded to float32 once.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace k2hip {

constexpr int kResampleNumZeros = 6;
constexpr int64_t kResampleMaxTable = 65536;   // floats of the weight table, ou * max_taps
constexpr int kResampleMaxTaps = 256;          // per phase
constexpr int kResampleMaxRate = 1 << 24;      // keeps 600 * lcm inside int64

struct ResamplePlan {
    int in_rate = 0, out_rate = 0;
    int iu = 0, ou = 0, max_taps = 0;
    int64_t wmax = 0;              // ticks
    std::vector<int32_t> first;    // [ou]
    std::vector<int32_t> ntaps;    // [ou]
    std::vector<float> w;          // [ou][max_taps], rows zero-filled behind ntaps[p]

    // the absolute input index of output k's first tap (may be negative: zero extension) and one past its last
    int64_t start(int64_t k) const { return (k / ou) * iu + first[(size_t)(k % ou)]; }
    int64_t end(int64_t k) const { return start(k) + ntaps[(size_t)(k % ou)]; }
    // outputs that exist once n input samples have been accepted in all: those whose whole window lies below n
    int64_t num_out(int64_t n) const {
        const int64_t t = n * ou - wmax - 1;
        return t < 0 ? 0 : t / iu + 1;
    }
    // the first input sample that outputs from k on still read: what a stream carries is the input from here
    int64_t keep_from(int64_t k) const {
        const int64_t s = start(k);
        return s < 0 ? 0 : s;
    }
};

// K2HIP_ERR_INVALID for a rate <= 0, K2HIP_ERR_UNSUPPORTED (naming the two rates) for a table beyond kResampleMaxTable floats, more
// than kResampleMaxTaps taps per phase or a rate beyond kResampleMaxRate.  in_rate == out_rate is the caller's business (no plan).
ResamplePlan resample_plan(int in_rate, int out_rate);

}  // namespace k2hip
