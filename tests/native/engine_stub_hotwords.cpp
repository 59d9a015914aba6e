// CPU stand-in for the engine's streaming beam-search entry points with per-stream hotword graphs (Engine::online_step_beam_hw,
// Engine::beam_chunk_host_hw) -- TEST INFRASTRUCTURE for the sanitizer builds of csrc/api.cpp, next to engine_stub_beam.cpp.  Every
// saved hypothesis survives through the unbiased stand-in with its graph state unchanged; the tables of every stream that has a
// graph are READ at their first entries (host allocations stand in for device memory), so a stream that names freed tables shows
// under ASan.  Never linked into libk2hip.so.
#include <atomic>
#include <cstring>

#include "../../k2transducerasr_amd/csrc/engine.h"

namespace k2hip {

namespace {
std::atomic<int> g_fail_next_hw{0};   // (process-wide: the models' locks do not cover them)
std::atomic<long long> g_calls[2];
void keep_states(int B, int K, const Engine::BeamHwIO& hw) {
    if (g_fail_next_hw > 0) {
        g_fail_next_hw--;
        failf(K2HIP_ERR_HIP, "stub: device failure in the biased search");
    }
    for (int b = 0; b < B; b++) {
        const BeamHwStream& g = hw.graphs[b];
        if (g.next) {
            K2_REQUIRE(g.bonus && g.pending, "stub: incomplete tables");
            volatile float sink = (float)g.next[0] + g.bonus[0] + g.pending[0];
            (void)sink;
        }
        for (int k = 0; k < K; k++) hw.st_out[(size_t)b * K + k] = hw.st_in[(size_t)b * K + k];
    }
    g_calls[1]++;
}
}  // namespace
extern "C" void k2hip_stub_fail_next_hotword_search(int n) { g_fail_next_hw = n; }

void beam_launch_counts(long long* plain, long long* hw) {
    *plain = g_calls[0];
    *hw = g_calls[1];
}

void Engine::online_step_beam_hw(const int* slots, const float* const* chunks, const long long* plens, const int* nchunks, int B, int K,
                                 const int* beam_in, int* beam_out, const BeamHwIO& hw, const int* fifo_heads) {
    keep_states(B, K, hw);
    online_step_beam(slots, chunks, plens, nchunks, B, K, beam_in, beam_out, fifo_heads);
}
void Engine::beam_chunk_host_hw(const float* enc, int B, int Tp, int K, const int* beam_in, int* beam_out, const BeamHwIO& hw) {
    keep_states(B, K, hw);
    beam_chunk_host(enc, B, Tp, K, beam_in, beam_out);
}

}  // namespace k2hip
