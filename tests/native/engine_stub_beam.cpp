// CPU stand-in for the engine's streaming beam-search entry points (Engine::online_step_beam, Engine::beam_chunk_host) -- TEST
// INFRASTRUCTURE for the sanitizer builds of csrc/api.cpp, next to engine_stub.cpp.  Each saved hypothesis survives unchanged
// (empty suffix, same score and context): the out block is written exactly as far as the device search writes it, so api.cpp's
// bookkeeping of the beam histories runs under the sanitizers.  Never linked into libk2hip.so.
#include <cstring>

#include "../../k2transducerasr_amd/csrc/engine.h"

namespace k2hip {

namespace {
void keep_hypotheses(int B, int Tp, int K, const int* in, int* out) {
    const BeamResumeLayout L{K, Tp};
    for (int b = 0; b < B; b++) {
        const int* i = in + (size_t)b * L.in_ints();
        int* o = out + (size_t)b * L.out_ints();
        memset(o, 0, sizeof(int) * (size_t)L.out_ints());
        const int nh = i[0];
        K2_REQUIRE(nh >= 1 && nh <= K, "stub: %d saved hypotheses", nh);
        o[0] = nh;
        o[1] = 0;
        for (int k = 0; k < nh; k++) {
            o[L.out_org() + k] = k;
            o[L.out_lp() + k] = i[L.in_lp() + k];
            o[L.out_ctx() + 2 * k] = i[L.in_ctx() + 2 * k];
            o[L.out_ctx() + 2 * k + 1] = i[L.in_ctx() + 2 * k + 1];
        }
    }
}
}  // namespace

void Engine::online_step_beam(const int* slots, const float* const* chunks, const long long*, const int*, int B, int K, const int* beam_in,
                              int* beam_out, const int*) {
    const Config& c = model_->cfg();
    for (int b = 0; b < B; b++) {
        K2_REQUIRE(slots[b] >= 0 && slots[b] < online_cap_, "stub: slot %d", slots[b]);
        volatile float sink = chunks[b][0] + chunks[b][(size_t)c.chunk_T * c.feat - 1];
        (void)sink;
    }
    keep_hypotheses(B, online_frames_per_chunk(), K, beam_in, beam_out);
}
void Engine::beam_chunk_host(const float* enc, int B, int Tp, int K, const int* beam_in, int* beam_out) {
    volatile float sink = enc[0] + enc[(size_t)B * Tp * model_->cfg().J - 1];
    (void)sink;
    keep_hypotheses(B, Tp, K, beam_in, beam_out);
}

}  // namespace k2hip
