// CPU stand-in of what api.cpp names for the half-precision LM weights of the fused searches (k2hip_debug_nlm_advance_f16_bench) in the
// sanitizer builds of the host layer.  Never linked into libk2hip.so.
#include "../../k2transducerasr_amd/csrc/engine.h"

namespace k2hip {

void Engine::nlm_advance_bench_f16(int, int, int, float*) { failf(K2HIP_ERR_UNSUPPORTED, "nlm_advance_bench_f16: the CPU stand-in has no kernels"); }

}  // namespace k2hip
