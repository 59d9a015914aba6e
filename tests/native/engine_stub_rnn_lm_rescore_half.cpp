// CPU stand-in of what api.cpp names for the half-precision rescoring step (k2hip_set_rnn_lm_rescoring_precision,
// k2hip_debug_rnn_lm_step_f16_bench) in the sanitizer builds of the host layer: the panels are laid out and checked by the real host
// routine (csrc/rnn_lm_fuse_layout.h, input width 0), so an LM that does not fit f16 is refused as on the device; the stand-in's
// scoring stays the float32 host reference.  Never linked into libk2hip.so.
#include <vector>

#include "../../k2transducerasr_amd/csrc/engine.h"

namespace k2hip {

void* Engine::rnn_lm_rescore_upload(const RnnLm& m, RnnLmDev* io) {
    K2_REQUIRE(io && io->L == m.L && io->H == m.H && io->V == m.V, "rnn lm rescoring: the tables are not those of the attached LM");
    std::vector<uint16_t> kh((size_t)4 * m.H * m.H);
    for (int k = 0; k < m.L; k++)
        if (!rnn_lm_panels_f16(m, k, kh.data(), 0))
            failf(K2HIP_ERR_INVALID, "rnn lm rescoring: layer %d has a weight that is not finite in half precision (k2hip_set_rnn_lm_rescoring_precision)", k);
    return dev_alloc(64);   // (what the caller owns and frees)
}
void Engine::rnn_lm_step_bench_f16(int, int, int, float*) { failf(K2HIP_ERR_UNSUPPORTED, "rnn_lm_step_bench_f16: the CPU stand-in has no kernels"); }

}  // namespace k2hip
