// CPU stand-in for the engine member behind k2hip_set_ctc_prefix_biasing (Engine::set_ctc_prefix_biasing) -- TEST INFRASTRUCTURE for the
// sanitizer builds of csrc/api.cpp, next to engine_stub_ctc_prefix.cpp.  The switch is a flag on the engine; what it selects on the
// device (k_ctc_prefix<false, true>) has its host reference in csrc/ctc_prefix_bias_ref.h, which tests/native/san_ctc_prefix_bias_driver.cpp
// runs directly.  Never linked into libk2hip.so.
#include "../../k2transducerasr_amd/csrc/engine.h"

namespace k2hip {

void Engine::set_ctc_prefix_biasing(bool on) { ctc_prefix_biasing_ = on; }

}  // namespace k2hip
