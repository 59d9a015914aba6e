// CPU stand-in of what api.cpp names for the offline Conformer's half-precision switch (k2hip_set_conformer_precision) in the sanitizer
// builds of the host layer: the model check, the level check and the pack with its refusal are the real host routine's
// (csrc/encoder_half.cpp over csrc/gemm_f16_layout.h); the stand-in's encoder stays what it was.  The counters are read through
// engine_stub_encoder_half.cpp's encoder_f16_stats.  Never linked into libk2hip.so.
#include <vector>

#include "../../k2transducerasr_amd/csrc/engine.h"

namespace k2hip {

void Engine::set_conformer_precision(int level) {
    conformer_half_pack(*model_, nullptr, nullptr);
    K2_REQUIRE(level >= 0 && level <= 2, "set_conformer_precision: level %d (0 = float32, 1 = the linear layers, 2 = the attention core too)", level);
    const int cur = enc_f16_dev_ ? enc_f16_.level : 0;
    if (level == cur) return;
    std::vector<uint16_t> blob;
    std::vector<EncoderHalfEntry> entries;
    if (level != 0) conformer_half_pack(*model_, &blob, &entries);   // (a refusal leaves the level it had)
    enc_f16_ = GemmF16Map();
    enc_f16_bytes_ = 0;
    enc_f16_dev_ = nullptr;
    if (level == 0) return;
    enc_f16_.level = level;
    for (const EncoderHalfEntry& e : entries) enc_f16_.by_weight[e.dev ? e.dev : reinterpret_cast<const float*>(&e)] = {nullptr, e.N, e.K};
    enc_f16_bytes_ = (int64_t)(blob.size() * sizeof(uint16_t));
    enc_f16_dev_ = this;   // (a mark, not an allocation: nothing to free)
}

}  // namespace k2hip
