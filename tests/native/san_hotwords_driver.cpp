// AddressSanitizer / UBSan driver for the per-stream hotword graphs of the streaming beam search (csrc/api.cpp:
// k2hip_online_stream_set_hotwords, k2hip_beam_stream_set_hotwords) over the CPU stand-ins of the engine (engine_stub*.cpp; the
// hotword stand-in READS the tables of every stream that names some, so a stream left pointing at freed tables is a report).
// TEST INFRASTRUCTURE (`make -C k2transducerasr_amd/csrc san`, tests/test_hotwords_stream.py).
// Exercised: attach / share / detach / reset, a graph destroyed right after the attach, both destroy orders of stream and model as
// far as the graph is concerned, a call that fails midway (no stream changes), argument errors.
//   san_hotwords_driver <offline.k2w> <streaming.k2w>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

extern "C" void k2hip_stub_fail_next_hotword_search(int n);

namespace {

k2hip_hotwords_t* graph(int V, float c = 1.5f) {
    const int64_t ids[] = {4, 5, 6, 7, 8};
    const int32_t lens[] = {2, 3};
    k2hip_hotwords_t* hw = nullptr;
    OK(k2hip_hotwords_create(ids, lens, 2, c, V, &hw));
    return hw;
}
void resident(k2hip_model_t* m, int uploads, int res) {
    int32_t u = -1, r = -1;
    OK(k2hip_debug_stream_hotword_uploads(m, &u, &r));
    CHECK(u == uploads && r == res);
}

void operator_level(const char* path) {
    k2hip_model_t* m = nullptr;
    OK(k2hip_model_create(path, nullptr, 0, &m));
    k2hip_model_info info;
    OK(k2hip_model_get_info(m, &info));
    const int V = info.vocab_size, J = info.joiner_dim;
    std::vector<float> enc((size_t)3 * 8 * J, 0.25f);
    k2hip_beam_stream_t *a = nullptr, *b = nullptr, *c = nullptr;
    OK(k2hip_beam_stream_create(m, 4, &a));
    OK(k2hip_beam_stream_create(m, 4, &b));
    OK(k2hip_beam_stream_create(m, 4, &c));
    // argument errors, decided before any device work
    CHECK(k2hip_beam_stream_set_hotwords(nullptr, nullptr) == K2HIP_ERR_INVALID);
    k2hip_hotwords_t* other = graph(V + 1);
    CHECK(k2hip_beam_stream_set_hotwords(a, other) == K2HIP_ERR_INVALID);
    CHECK(strstr(k2hip_last_error(), "vocab_size") != nullptr);
    OK(k2hip_hotwords_destroy(other));
    resident(m, 0, 0);
    // attach / share; the graph dies right after the attach
    k2hip_hotwords_t* hw = graph(V);
    OK(k2hip_beam_stream_set_hotwords(a, hw));
    OK(k2hip_beam_stream_set_hotwords(b, hw));
    resident(m, 1, 1);
    k2hip_hotwords_t* hw2 = graph(V, 2.0f);   // (a second graph: its own upload, whatever address it got)
    OK(k2hip_hotwords_destroy(hw));
    OK(k2hip_beam_stream_set_hotwords(c, hw2));
    OK(k2hip_hotwords_destroy(hw2));
    resident(m, 2, 2);
    k2hip_beam_stream_t* all[3] = {a, b, c};
    OK(k2hip_beam_search_chunk(m, all, 3, enc.data(), 8));     // two graphs in one call
    // a call that fails midway changes no stream
    float before = 0.f, after = 0.f;
    OK(k2hip_beam_stream_get_score(a, &before));
    k2hip_stub_fail_next_hotword_search(1);
    CHECK(k2hip_beam_search_chunk(m, all, 3, enc.data(), 8) == K2HIP_ERR_HIP);
    OK(k2hip_beam_stream_get_score(a, &after));
    CHECK(before == after);
    OK(k2hip_beam_search_chunk(m, all, 3, enc.data(), 8));
    // not in the start state: refused; reset keeps the graph; detach frees with the last holder
    CHECK(k2hip_beam_stream_set_hotwords(a, nullptr) == K2HIP_ERR_INVALID);
    CHECK(strstr(k2hip_last_error(), "reset the stream first") != nullptr);
    OK(k2hip_beam_stream_reset(a));
    OK(k2hip_beam_search_chunk(m, all, 1, enc.data(), 8));
    resident(m, 2, 2);
    OK(k2hip_beam_stream_reset(a));
    OK(k2hip_beam_stream_set_hotwords(a, nullptr));
    resident(m, 2, 2);                                         // b still holds the first graph
    OK(k2hip_beam_stream_destroy(b));
    resident(m, 2, 1);
    k2hip_beam_stream_t* mixed[2] = {a, c};
    OK(k2hip_beam_search_chunk(m, mixed, 2, enc.data(), 8));   // a stream with none beside a stream with a graph
    OK(k2hip_beam_search_chunk(m, mixed, 1, enc.data(), 8));   // no graph anywhere: the unbiased entry point
    // the model-level list refuses the streaming search, graphs attached or not
    k2hip_hotwords_t* lvl = graph(V);
    OK(k2hip_set_hotwords(m, lvl));
    OK(k2hip_hotwords_destroy(lvl));
    CHECK(k2hip_beam_search_chunk(m, mixed, 2, enc.data(), 8) == K2HIP_ERR_INVALID);
    CHECK(strstr(k2hip_last_error(), "streaming") != nullptr);
    OK(k2hip_set_hotwords(m, nullptr));
    // destroy orders: a before the model, c (graph attached) after it
    OK(k2hip_beam_stream_destroy(a));
    OK(k2hip_model_destroy(m));
    OK(k2hip_beam_stream_destroy(c));
}

void fused(const char* path) {
    k2hip_model_t* m = nullptr;
    OK(k2hip_model_create(path, nullptr, 0, &m));
    OK(k2hip_set_decoding_method(m, "modified_beam_search", 4));
    k2hip_model_info info;
    OK(k2hip_model_get_info(m, &info));
    k2hip_online_stream_t *a = nullptr, *b = nullptr;
    OK(k2hip_online_stream_create(m, &a));
    OK(k2hip_online_stream_create(m, &b));
    CHECK(k2hip_online_stream_set_hotwords(nullptr, nullptr) == K2HIP_ERR_INVALID);
    k2hip_hotwords_t* hw = graph(info.vocab_size);
    OK(k2hip_online_stream_set_hotwords(a, hw));
    OK(k2hip_hotwords_destroy(hw));
    resident(m, 1, 1);
    std::vector<float> wav(16000, 0.f);
    for (size_t i = 0; i < wav.size(); i++) wav[i] = (float)((int)(i * 2654435761u % 2001) - 1000) / 1000.f;
    k2hip_online_stream_t* both[2] = {a, b};
    int32_t dec[2], nn[2];
    for (int round = 0; round < 3; round++) {
        OK(k2hip_online_stream_accept_samples(a, wav.data(), (int64_t)wav.size()));
        OK(k2hip_online_stream_accept_samples(b, wav.data(), (int64_t)wav.size()));
        OK(k2hip_online_step(m, both, 2, dec, nn));
        CHECK(dec[0] == 1 && dec[1] == 1);
    }
    float sc = 1.f;
    OK(k2hip_online_stream_get_score(a, &sc));
    CHECK(k2hip_online_stream_set_hotwords(a, nullptr) == K2HIP_ERR_INVALID);
    CHECK(strstr(k2hip_last_error(), "reset the stream first") != nullptr);
    // a failed tick poisons the streams but moves no hypothesis
    k2hip_stub_fail_next_hotword_search(1);
    CHECK(k2hip_online_step(m, both, 2, dec, nn) == K2HIP_ERR_HIP);
    float sc2 = 0.f;
    OK(k2hip_online_stream_get_score(a, &sc2));
    CHECK(sc == sc2);
    OK(k2hip_online_stream_reset(a));                          // keeps the graph
    resident(m, 1, 1);
    OK(k2hip_online_stream_reset(b));
    OK(k2hip_online_stream_accept_samples(a, wav.data(), (int64_t)wav.size()));
    int32_t d1, n1;
    OK(k2hip_online_step(m, &a, 1, &d1, &n1));
    OK(k2hip_online_stream_reset(a));
    OK(k2hip_online_stream_set_hotwords(a, nullptr));          // reset-to-none: the tables go
    resident(m, 1, 0);
    // greedy ignores an attached graph
    k2hip_hotwords_t* hw3 = graph(info.vocab_size);
    OK(k2hip_online_stream_set_hotwords(b, hw3));
    OK(k2hip_hotwords_destroy(hw3));
    OK(k2hip_set_decoding_method(m, "greedy_search", 0));
    OK(k2hip_online_stream_accept_samples(b, wav.data(), (int64_t)wav.size()));
    OK(k2hip_online_step(m, &b, 1, &d1, &n1));
    OK(k2hip_online_stream_destroy(b));                        // destroyed with its graph attached
    resident(m, 2, 0);
    OK(k2hip_online_stream_destroy(a));
    OK(k2hip_model_destroy(m));
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s <offline.k2w> <streaming.k2w>\n", argv[0]);
        return 2;
    }
    operator_level(argv[1]);
    fused(argv[2]);
    printf("OK\n");
    return 0;
}
