// CPU stand-in of the engine's resampling entry (Engine::resample_host) for the sanitizer builds of the host layer: the float32 host
// reference of csrc/resample_ref.h over the same job descriptions, with the extents the launcher checks on the host checked here too,
// so that the stream bookkeeping of api.cpp (queues, carried tails, counts, erase) runs unmodified.  Never linked into libk2hip.so.
#include <vector>

#include "../../k2transducerasr_amd/csrc/engine.h"
#include "../../k2transducerasr_amd/csrc/resample_ref.h"

namespace k2hip {

void Engine::resample_host(const ResampleJob* jobs, int G) {
    K2_REQUIRE(jobs && G > 0, "resample: empty call");
    for (int g = 0; g < G; g++) {
        const ResampleJob& j = jobs[g];
        K2_REQUIRE(j.plan && j.n_head >= 0 && j.n_tail >= 0 && j.n_out >= 0 && (j.n_out == 0 || j.out), "resample: signal %d: bad arguments", g);
        K2_REQUIRE(j.plan->out_rate == model_->cfg().fbank.sample_rate, "resample: a plan for %d -> %d", j.plan->in_rate, j.plan->out_rate);
        if (j.n_out == 0) continue;
        const int64_t start = j.plan->start(j.k0), end = j.plan->end(j.k0 + j.n_out - 1);
        K2_REQUIRE(j.x0 >= 0 && j.k0 >= 0 && j.x0 <= (start < 0 ? 0 : start) && end <= j.x0 + j.n_head + j.n_tail,
                   "resample: signal %d reads input [%lld, %lld) and holds [%lld, %lld)", g, (long long)start, (long long)end, (long long)j.x0,
                   (long long)(j.x0 + j.n_head + j.n_tail));
        // an exact-size copy: a read past either piece is a heap overflow the sanitizer sees
        std::vector<float> blk;
        blk.reserve((size_t)(j.n_head + j.n_tail));
        if (j.n_head) blk.insert(blk.end(), j.head, j.head + j.n_head);
        if (j.n_tail) blk.insert(blk.end(), j.tail, j.tail + j.n_tail);
        for (int64_t i = 0; i < j.n_out; i++) j.out[i] = resample_ref_dot(*j.plan, j.k0 + i, blk.data(), j.x0);
    }
}

}  // namespace k2hip
