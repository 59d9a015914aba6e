// CPU stand-in of what api.cpp names for the neural LM shallow fusion of the STREAMING search (k2hip_set_rnn_lm_stream_fusion,
// k2hip_debug_rnn_lm_stream_fusion_stats) in the sanitizer builds of the host layer.  The stand-in chunk searches (engine_stub_beam.cpp)
// keep every hypothesis and never launch, so the call counter stays 0; the state blocks are real heap allocations of the stand-in
// dev_alloc, taken, flipped, released and freed by the real bookkeeping.  Never linked into libk2hip.so.
#include "../../k2transducerasr_amd/csrc/engine.h"

namespace k2hip {

long long beam_nlm_stream_launch_count() { return 0; }

}  // namespace k2hip
