// CPU stand-in of what api.cpp names for the neural LM shallow fusion (k2hip_set_rnn_lm_fusion, k2hip_debug_rnn_lm_fusion_stats) in the
// sanitizer builds of the host layer: the stand-in searches never fuse, so the counters stay 0.  Never linked into libk2hip.so.
#include <vector>

#include "../../k2transducerasr_amd/csrc/engine.h"

namespace k2hip {

void Engine::rnn_lm_fusion_work(int64_t* swept, int64_t* idle) {
    if (swept) *swept = 0;
    if (idle) *idle = 0;
}

// the real layout code over an exact-size buffer (a write past a panel is a heap overflow the sanitizer sees); the "device" block is
// a token allocation the caller owns and frees
void* Engine::rnn_lm_fusion_upload(const RnnLm& m, RnnLmDev* io) {
    K2_REQUIRE(io && io->L == m.L && io->H == m.H && io->V == m.V, "rnn lm fusion: the tables are not those of the attached LM");
    for (int k = 0; k < m.L; k++) {
        std::vector<float> panels((size_t)rnn_lm_panel_floats(m, k));
        rnn_lm_panels(m, k, panels.data());
    }
    void* p = dev_alloc(64);
    io->w_out = static_cast<const float*>(p);
    return p;
}

void Engine::nlm_advance_bench(int, int, int, float*) { failf(K2HIP_ERR_UNSUPPORTED, "nlm_advance_bench: the CPU stand-in has no kernels"); }

long long beam_nlm_launch_count() { return 0; }

}  // namespace k2hip
