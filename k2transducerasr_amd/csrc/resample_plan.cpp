// resample_plan.h: the windowed-sinc plan.  Pure host code (built under the sanitizers as well: make san_resample).
#include "resample_plan.h"

#include <algorithm>
#include <cmath>
#include <numeric>

#include "errors.h"

namespace k2hip {

namespace {
int64_t floor_div(int64_t a, int64_t b) { return a / b - ((a % b != 0) && ((a < 0) != (b < 0))); }
int64_t ceil_div(int64_t a, int64_t b) { return -floor_div(-a, b); }
}  // namespace

ResamplePlan resample_plan(int in_rate, int out_rate) {
    K2_REQUIRE(in_rate > 0 && out_rate > 0, "resample: sample rates %d -> %d", in_rate, out_rate);
    if (in_rate > kResampleMaxRate || out_rate > kResampleMaxRate)
        failf(K2HIP_ERR_UNSUPPORTED, "resample %d -> %d: rates above %d are not supported", in_rate, out_rate, kResampleMaxRate);
    ResamplePlan p;
    p.in_rate = in_rate;
    p.out_rate = out_rate;
    const int64_t g = std::gcd((int64_t)in_rate, (int64_t)out_rate);
    const int64_t iu = in_rate / g, ou = out_rate / g, lcm = (int64_t)in_rate * ou, lo = std::min(in_rate, out_rate);
    // the window's half width in ticks is 600 lcm / (99 lo); wmax = the largest whole number of ticks strictly below it
    const int64_t num = 600 * lcm, den = 99 * lo;
    p.wmax = num % den == 0 ? num / den - 1 : num / den;
    // a bound on the taps of any phase before anything is sized: the window spans 2 wmax + 1 ticks, inputs are ou ticks apart
    const int64_t taps_bound = 2 * p.wmax / ou + 1;
    if (taps_bound > kResampleMaxTaps)
        failf(K2HIP_ERR_UNSUPPORTED, "resample %d -> %d: %lld taps per phase, more than %d", in_rate, out_rate, (long long)taps_bound,
              kResampleMaxTaps);
    if (ou * (taps_bound - 1) > kResampleMaxTable)   // (a phase has taps_bound or taps_bound - 1 taps: a table this long is refused below anyway)
        failf(K2HIP_ERR_UNSUPPORTED, "resample %d -> %d: a filter table of %lld phases x %lld taps exceeds %lld floats", in_rate, out_rate,
              (long long)ou, (long long)taps_bound, (long long)kResampleMaxTable);
    p.iu = (int)iu;
    p.ou = (int)ou;
    p.first.resize((size_t)ou);
    p.ntaps.resize((size_t)ou);
    int mt = 0;
    for (int64_t ph = 0; ph < ou; ph++) {
        const int64_t j0 = ceil_div(ph * iu - p.wmax, ou), j1 = floor_div(ph * iu + p.wmax, ou);
        p.first[(size_t)ph] = (int32_t)j0;
        p.ntaps[(size_t)ph] = (int32_t)(j1 - j0 + 1);
        mt = std::max(mt, (int)(j1 - j0 + 1));
    }
    p.max_taps = mt;
    if (ou * mt > kResampleMaxTable)
        failf(K2HIP_ERR_UNSUPPORTED, "resample %d -> %d: a filter table of %lld phases x %d taps exceeds %lld floats", in_rate, out_rate,
              (long long)ou, mt, (long long)kResampleMaxTable);
    p.w.assign((size_t)(ou * mt), 0.f);
    const double fc = 0.99 * 0.5 * (double)lo, ww = kResampleNumZeros / (2.0 * fc);
    for (int64_t ph = 0; ph < ou; ph++)
        for (int j = 0; j < p.ntaps[(size_t)ph]; j++) {
            const double d = (double)((p.first[(size_t)ph] + j) * ou - ph * iu) / (double)lcm;   // seconds, input minus output
            const double hann = std::fabs(d) < ww ? 0.5 * (1.0 + std::cos(2.0 * M_PI * fc / kResampleNumZeros * d)) : 0.0;
            const double filt = d != 0.0 ? std::sin(2.0 * M_PI * fc * d) / (M_PI * d) : 2.0 * fc;
            p.w[(size_t)(ph * mt + j)] = (float)(filt * hann / (double)in_rate);
        }
    return p;
}

}  // namespace k2hip
