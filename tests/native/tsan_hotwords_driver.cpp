// ThreadSanitizer driver for the per-stream hotword graphs (csrc/api.cpp) over the CPU stand-ins of the engine.  TEST
// INFRASTRUCTURE (`make -C k2transducerasr_amd/csrc tsan`, tests/test_hotwords_stream.py).
// Two model handles at once, two threads on each: every thread attaches the SAME two graphs to its own streams (the per-model cache
// of resident tables and the process-wide graph identities are shared), steps them, detaches, resets and destroys, while the other
// threads do the same.  Any report or failed check fails the run.
//   tsan_hotwords_driver <offline.k2w> <streaming.k2w>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../../include/k2hip_debug.h"

#define CHECK(cond)                                                                                                          \
    do {                                                                                                                     \
        if (!(cond)) {                                                                                                       \
            fprintf(stderr, "CHECK failed at %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, k2hip_last_error()); \
            exit(3);                                                                                                         \
        }                                                                                                                    \
    } while (0)
#define OK(call) CHECK((call) == K2HIP_OK)

namespace {

void beam_worker(k2hip_model_t* m, k2hip_hotwords_t* const* hw, int J, int rounds) {
    std::vector<float> enc((size_t)2 * 4 * J, 0.25f);
    for (int r = 0; r < rounds; r++) {
        k2hip_beam_stream_t* s[2] = {nullptr, nullptr};
        OK(k2hip_beam_stream_create(m, 4, &s[0]));
        OK(k2hip_beam_stream_create(m, 4, &s[1]));
        OK(k2hip_beam_stream_set_hotwords(s[0], hw[r & 1]));
        if (r % 3) OK(k2hip_beam_stream_set_hotwords(s[1], hw[(r >> 1) & 1]));
        OK(k2hip_beam_search_chunk(m, s, 2, enc.data(), 4));
        OK(k2hip_beam_stream_reset(s[0]));
        OK(k2hip_beam_stream_set_hotwords(s[0], nullptr));
        OK(k2hip_beam_search_chunk(m, s, 2, enc.data(), 4));
        OK(k2hip_beam_stream_destroy(s[0]));
        OK(k2hip_beam_stream_destroy(s[1]));
    }
}
void online_worker(k2hip_model_t* m, k2hip_hotwords_t* const* hw, int rounds) {
    std::vector<float> wav(12000, 0.01f);
    for (size_t i = 0; i < wav.size(); i++) wav[i] = (float)((int)(i * 2654435761u % 2001) - 1000) / 1000.f;
    for (int r = 0; r < rounds; r++) {
        k2hip_online_stream_t* s = nullptr;
        OK(k2hip_online_stream_create(m, &s));
        OK(k2hip_online_stream_set_hotwords(s, hw[r & 1]));
        OK(k2hip_online_stream_accept_samples(s, wav.data(), (int64_t)wav.size()));
        int32_t dec = 0, nn = 0;
        OK(k2hip_online_step(m, &s, 1, &dec, &nn));
        OK(k2hip_online_stream_reset(s));
        if (r & 2) OK(k2hip_online_stream_set_hotwords(s, nullptr));
        OK(k2hip_online_stream_destroy(s));
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s <offline.k2w> <streaming.k2w>\n", argv[0]);
        return 2;
    }
    const int rounds = 200;
    k2hip_model_t *off = nullptr, *on = nullptr;
    OK(k2hip_model_create(argv[1], nullptr, 0, &off));
    OK(k2hip_model_create(argv[2], nullptr, 0, &on));
    OK(k2hip_set_decoding_method(on, "modified_beam_search", 4));
    k2hip_model_info io, in;
    OK(k2hip_model_get_info(off, &io));
    OK(k2hip_model_get_info(on, &in));
    const int64_t ids[] = {4, 5, 6, 7, 8};
    const int32_t lens[] = {2, 3};
    k2hip_hotwords_t *hoff[2], *hon[2];
    for (int i = 0; i < 2; i++) {
        OK(k2hip_hotwords_create(ids, lens, 2, 1.5f + (float)i, io.vocab_size, &hoff[i]));
        OK(k2hip_hotwords_create(ids, lens, 2, 1.5f + (float)i, in.vocab_size, &hon[i]));
    }
    std::vector<std::thread> th;
    for (int t = 0; t < 2; t++) th.emplace_back(beam_worker, off, hoff, io.joiner_dim, rounds);
    for (int t = 0; t < 2; t++) th.emplace_back(online_worker, on, hon, rounds);
    th.emplace_back(beam_worker, on, hon, in.joiner_dim, rounds);   // attach + operator-level step beside the fused ticks of `on`
    for (auto& t : th) t.join();
    int32_t u = 0, r = -1;
    OK(k2hip_debug_stream_hotword_uploads(off, &u, &r));
    CHECK(r == 0 && u >= 2);
    OK(k2hip_debug_stream_hotword_uploads(on, &u, &r));
    CHECK(r == 0);
    for (int i = 0; i < 2; i++) {
        OK(k2hip_hotwords_destroy(hoff[i]));
        OK(k2hip_hotwords_destroy(hon[i]));
    }
    OK(k2hip_model_destroy(off));
    OK(k2hip_model_destroy(on));
    printf("OK\n");
    return 0;
}
