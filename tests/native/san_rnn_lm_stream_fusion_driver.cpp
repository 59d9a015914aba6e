// AddressSanitizer / UBSan driver for the host side of the neural LM shallow fusion in the STREAMING modified beam search: the state-block
// pool (csrc/rnn_lm_stream_pool.h) over a heap allocator, and the new API paths in csrc/api.cpp (k2hip_set_rnn_lm_stream_fusion, the
// first-chunk rule, the block table of a call, flip after success, reset, the destroy orders) over the CPU stand-ins of the engine
// (engine_stub*.cpp, engine_stub_rnn_lm_stream_fusion.cpp).  TEST INFRASTRUCTURE (`make -C k2transducerasr_amd/csrc
// san_rnn_lm_stream_fusion`, tests/test_rnn_lm_stream_fusion_sanitizers.py, tests/test_rnn_lm_stream_fusion.py).
// Exercised: random orders of create, first chunk, failed call (no flip), flip, reset, LM replaced (another block size), stream destroy
// and model destroy before stream destroy on the pool itself, every half written to its last float and read back; through the ABI the
// switch, a call that fails after its blocks were staged (the stand-in search refuses), the mid-stream refusals, reset, the offline
// switch alone, the recognizer's tick, and both destroy orders.
//   san_rnn_lm_stream_fusion_driver <offline.k2w> <streaming.k2w> <lm.k2w> <lm2.k2w>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/k2hip.h"
#include "../../include/k2hip_debug.h"
#include "../../k2transducerasr_amd/csrc/rnn_lm_stream_pool.h"

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

using k2hip::NlmStreamLayout;
using k2hip::NlmStreamPool;

uint32_t g_rng = 12345;
uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 1664525u + 1013904223u;
    return (g_rng >> 8) % n;
}

// ---- the pool itself ----------------------------------------------------------------------------------------------------------------
struct Stream {
    std::unique_ptr<NlmStreamPool::Handle> h{new NlmStreamPool::Handle()};
    float stamp = 0.f;   // what the current half holds, in every float
    int layout = 0;
};
void fill(float* p, size_t n, float v) {
    for (size_t i = 0; i < n; i++) p[i] = v;
}
bool all_are(const float* p, size_t n, float v) {
    for (size_t i = 0; i < n; i++)
        if (p[i] != v) return false;
    return true;
}

void pool_random_orders(int rounds) {
    const NlmStreamLayout lays[2] = {{4, 2, 32, 37}, {3, 3, 64, 165}};   // (two LMs: the second replaces the first)
    CHECK(lays[0].half_floats() % 4 == 0 && lays[0].half_floats() >= lays[0].state_floats() + 4 * 37 && lays[0].row_off(1) == lays[0].state_floats() + 37);
    CHECK(lays[0].state_off(1, 1, 1) == ((1 * 2 + 1) * 2 + 1) * 32 && lays[1].block_floats() == 2 * lays[1].half_floats());
    for (int round = 0; round < rounds; round++) {
        int64_t allocs = 0, frees = 0;
        auto pool = std::make_shared<NlmStreamPool>(
            [&](size_t n) {
                allocs++;
                void* p = malloc(n);   // exactly n bytes: a write past a half is a heap overflow
                if (!p) throw std::bad_alloc();
                return p;
            },
            [&](void* p) {
                frees++;
                free(p);
            });
        std::vector<Stream> ss;
        int lm = 0;
        bool model_alive = true;
        float next_stamp = 1.f;
        for (int step = 0; step < 200; step++) {
            const uint32_t what = rnd(9);
            if (what == 0 && ss.size() < 12) {   // create
                ss.emplace_back();
                ss.back().layout = lm;
            } else if (ss.empty()) {
                continue;
            } else {
                Stream& s = ss[rnd((uint32_t)ss.size())];
                const size_t half = (size_t)lays[s.layout].half_floats();
                if (what <= 3 && model_alive) {   // a chunk call: first chunk takes; it succeeds (flip) or fails (no flip)
                    if (!s.h->held()) {
                        if (s.layout != lm) continue;   // (the API refuses this stream until it is reset)
                        NlmStreamPool::take(pool, *s.h, lays[lm], (uint64_t)lm + 1);
                        CHECK(s.h->held() && !s.h->has_state() && s.h->read_half() == nullptr && s.h->lm_serial() == (uint64_t)lm + 1);
                        CHECK(s.h->carries((uint64_t)lm + 1) && !s.h->carries((uint64_t)(lm ^ 1) + 1));
                    }
                    if (s.layout != lm) continue;
                    const float* rd = s.h->read_half();
                    float* wr = s.h->write_half();
                    CHECK(wr != nullptr && wr != rd);
                    if (rd) CHECK(all_are(rd, half, s.stamp));
                    fill(wr, half, next_stamp);          // the device writes the other half, every float of it
                    if (rd) CHECK(all_are(rd, half, s.stamp));
                    if (what != 3) {                     // success: flip
                        s.h->flip();
                        s.stamp = next_stamp;
                        CHECK(s.h->has_state() && all_are(s.h->read_half(), half, s.stamp));
                    } else {                             // failure: the state the stream had
                        CHECK(s.h->read_half() == rd);
                    }
                    next_stamp += 1.f;
                } else if (what == 4) {                  // reset: back to the start state
                    s.h->release();
                    s.layout = lm;
                    CHECK(!s.h->held() && s.h->read_half() == nullptr && s.h->write_half() == nullptr);
                } else if (what == 5) {                  // the LM is replaced: streams that carry state are stuck until reset
                    lm ^= 1;
                } else if (what == 6) {                  // stream destroy
                    const size_t i = (size_t)(&s - ss.data());
                    ss.erase(ss.begin() + (long)i);
                } else if (what == 7 && step > 150 && model_alive) {   // model destroy before the streams
                    pool->shutdown();
                    model_alive = false;
                    CHECK(pool->gone() && allocs == frees);
                    for (Stream& t : ss) CHECK(t.h->read_half() == nullptr && t.h->write_half() == nullptr);
                }
                const NlmStreamPool::Stats st = pool->stats();
                int64_t held = 0;
                for (Stream& t : ss) held += t.h->held();
                CHECK(st.live == held && (model_alive || st.bytes == 0));
            }
        }
        if (round & 1) {   // the streams first, or the model first
            ss.clear();
            CHECK(pool->stats().live == 0);
            pool->shutdown();
        } else {
            pool->shutdown();
            ss.clear();
        }
        CHECK(allocs == frees);
        pool->shutdown();   // (twice is harmless)
    }
}

// ---- through the ABI, over the stand-ins ---------------------------------------------------------------------------------------------
void stats(k2hip_model_t* m, int64_t live) {
    int64_t calls = -1, lv = -1, bytes = -1;
    OK(k2hip_debug_rnn_lm_stream_fusion_stats(m, &calls, &lv, &bytes));
    CHECK(calls == 0 && lv == live && bytes >= 0);   // (the stand-in searches launch nothing)
    if (live > 0) CHECK(bytes > 0);
}

void operator_level(const char* path, const char* lm_path, const char* lm2_path, bool model_first) {
    k2hip_model_t* m = nullptr;
    k2hip_rnn_lm_t *lm = nullptr, *lm2 = nullptr;
    OK(k2hip_model_create(path, nullptr, 0, &m));
    OK(k2hip_rnn_lm_load(lm_path, &lm));
    OK(k2hip_rnn_lm_load(lm2_path, &lm2));
    k2hip_model_info info;
    OK(k2hip_model_get_info(m, &info));
    const int J = info.joiner_dim;
    std::vector<float> enc((size_t)3 * 8 * J, 0.25f);
    CHECK(k2hip_set_rnn_lm_stream_fusion(nullptr, 1) != K2HIP_OK);
    OK(k2hip_debug_rnn_lm_stream_fusion_stats(m, nullptr, nullptr, nullptr));
    k2hip_beam_stream_t *a = nullptr, *b = nullptr, *c = nullptr;
    OK(k2hip_beam_stream_create(m, 4, &a));
    OK(k2hip_beam_stream_create(m, 4, &b));
    OK(k2hip_beam_stream_create(m, 4, &c));
    k2hip_beam_stream_t* all[3] = {a, b, c};
    // nothing on: no block.  The offline switch alone enables nothing on a streaming entry
    OK(k2hip_beam_search_chunk(m, all, 1, enc.data(), 8));
    stats(m, 0);
    OK(k2hip_beam_stream_reset(a));
    OK(k2hip_set_rnn_lm(m, lm, 0.5f));
    OK(k2hip_set_rnn_lm_fusion(m, 1));
    OK(k2hip_beam_search_chunk(m, all, 1, enc.data(), 8));
    stats(m, 0);
    OK(k2hip_set_rnn_lm_fusion(m, 0));
    // the streaming switch: a (started unfused) refuses, b starts fused and takes a block
    OK(k2hip_set_rnn_lm_stream_fusion(m, 1));
    CHECK(k2hip_beam_search_chunk(m, all, 2, enc.data(), 8) == K2HIP_ERR_INVALID);   // decided for all streams before any changes
    CHECK(strstr(k2hip_last_error(), "reset the stream first") != nullptr);
    stats(m, 0);
    OK(k2hip_beam_search_chunk(m, all + 1, 2, enc.data(), 8));
    stats(m, 2);
    OK(k2hip_beam_stream_reset(a));
    OK(k2hip_beam_search_chunk(m, all, 3, enc.data(), 8));
    stats(m, 3);
    // a call that fails AFTER its blocks were staged: c is reset (fresh, takes a block in the call), a graph makes the stand-in refuse
    OK(k2hip_beam_stream_reset(c));
    stats(m, 2);
    const int64_t ids[] = {4, 5};
    const int32_t lens[] = {2};
    k2hip_hotwords_t* hw = nullptr;
    OK(k2hip_hotwords_create(ids, lens, 1, 1.5f, info.vocab_size, &hw));
    OK(k2hip_beam_stream_set_hotwords(c, hw));
    OK(k2hip_hotwords_destroy(hw));
    float before = 0.f, after = 1.f;
    OK(k2hip_beam_stream_get_score(a, &before));
    k2hip_stub_fail_next_hotword_search(1);
    CHECK(k2hip_beam_search_chunk(m, all, 3, enc.data(), 8) == K2HIP_ERR_HIP);
    OK(k2hip_beam_stream_get_score(a, &after));
    CHECK(before == after);
    stats(m, 2);                                                 // (the block c took for the failed call went back)
    OK(k2hip_beam_search_chunk(m, all, 3, enc.data(), 8));
    stats(m, 3);
    // mid-stream: the switch, the scale, the LM replaced (the same handle again included) -- INVALID, nothing moves
    OK(k2hip_set_rnn_lm_stream_fusion(m, 0));
    CHECK(k2hip_beam_search_chunk(m, all, 3, enc.data(), 8) == K2HIP_ERR_INVALID);
    OK(k2hip_set_rnn_lm_stream_fusion(m, 1));
    OK(k2hip_beam_search_chunk(m, all, 3, enc.data(), 8));
    OK(k2hip_set_rnn_lm(m, lm, 0.25f));
    CHECK(k2hip_beam_search_chunk(m, all, 3, enc.data(), 8) == K2HIP_ERR_INVALID);
    OK(k2hip_set_rnn_lm(m, lm2, 0.5f));                          // (blocks of another size from here on)
    CHECK(k2hip_beam_search_chunk(m, all, 3, enc.data(), 8) == K2HIP_ERR_INVALID);
    CHECK(strstr(k2hip_last_error(), "reset the stream first") != nullptr);
    stats(m, 3);
    OK(k2hip_beam_stream_reset(a));
    stats(m, 2);
    OK(k2hip_beam_search_chunk(m, all, 1, enc.data(), 8));       // a again, under the new LM: the stale spare block is freed, a new one taken
    stats(m, 3);
    OK(k2hip_set_rnn_lm(m, nullptr, 0.f));                       // cleared: a (fused) refuses, a reset stream runs unfused
    CHECK(k2hip_beam_search_chunk(m, all, 1, enc.data(), 8) == K2HIP_ERR_INVALID);
    OK(k2hip_beam_stream_reset(b));
    OK(k2hip_beam_search_chunk(m, all + 1, 1, enc.data(), 8));
    stats(m, 2);
    OK(k2hip_rnn_lm_destroy(lm));
    OK(k2hip_rnn_lm_destroy(lm2));
    if (model_first) {   // the streams outlive the model: reset and destroy only forget their blocks
        OK(k2hip_model_destroy(m));
        OK(k2hip_beam_stream_reset(a));
        OK(k2hip_beam_stream_destroy(a));
        OK(k2hip_beam_stream_destroy(b));
        OK(k2hip_beam_stream_destroy(c));
    } else {
        OK(k2hip_beam_stream_destroy(a));
        stats(m, 1);
        OK(k2hip_beam_stream_destroy(b));
        OK(k2hip_beam_stream_destroy(c));
        stats(m, 0);
        OK(k2hip_model_destroy(m));
    }
}

void recognizer_level(const char* path, const char* lm_path) {
    k2hip_model_t* m = nullptr;
    k2hip_rnn_lm_t* lm = nullptr;
    OK(k2hip_model_create(path, nullptr, 0, &m));
    OK(k2hip_rnn_lm_load(lm_path, &lm));
    OK(k2hip_set_decoding_method(m, "modified_beam_search", 4));
    OK(k2hip_set_rnn_lm(m, lm, 0.5f));
    OK(k2hip_rnn_lm_destroy(lm));
    OK(k2hip_set_rnn_lm_stream_fusion(m, 1));
    k2hip_online_stream_t *a = nullptr, *b = nullptr;
    OK(k2hip_online_stream_create(m, &a));
    OK(k2hip_online_stream_create(m, &b));
    std::vector<float> wav(16000, 0.f);
    for (size_t i = 0; i < wav.size(); i++) wav[i] = (float)((int)(i * 2654435761u % 2001) - 1000) / 1000.f;
    k2hip_online_stream_t* both[2] = {a, b};
    int32_t dec[2], nn[2];
    OK(k2hip_online_stream_accept_samples(a, wav.data(), (int64_t)wav.size()));
    OK(k2hip_online_step(m, both, 2, dec, nn));
    CHECK(dec[0] == 1 && dec[1] == 0);
    stats(m, 1);
    OK(k2hip_online_stream_accept_samples(b, wav.data(), (int64_t)wav.size()));
    OK(k2hip_online_step(m, both, 2, dec, nn));                 // a carried stream beside a fresh one
    CHECK(dec[0] == 1 && dec[1] == 1);
    stats(m, 2);
    OK(k2hip_set_rnn_lm_stream_fusion(m, 0));                   // mid-stream: refused, nothing moves, the streams are not poisoned
    CHECK(k2hip_online_step(m, both, 2, dec, nn) == K2HIP_ERR_INVALID);
    CHECK(strstr(k2hip_last_error(), "reset the stream first") != nullptr);
    OK(k2hip_set_rnn_lm_stream_fusion(m, 1));
    OK(k2hip_online_step(m, both, 2, dec, nn));
    OK(k2hip_online_stream_reset(a));
    stats(m, 1);
    OK(k2hip_set_rnn_lm_stream_fusion(m, 0));
    OK(k2hip_online_stream_accept_samples(a, wav.data(), (int64_t)wav.size()));
    OK(k2hip_online_step(m, &a, 1, dec, nn));                   // a starts over, unfused: no block
    stats(m, 1);
    OK(k2hip_online_stream_destroy(b));
    stats(m, 0);
    OK(k2hip_online_stream_destroy(a));
    OK(k2hip_model_destroy(m));
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 5) {
        fprintf(stderr, "usage: %s <offline.k2w> <streaming.k2w> <lm.k2w> <lm2.k2w>\n", argv[0]);
        return 2;
    }
    pool_random_orders(40);
    operator_level(argv[1], argv[3], argv[4], false);
    operator_level(argv[1], argv[3], argv[4], true);
    recognizer_level(argv[2], argv[3]);
    printf("san_rnn_lm_stream_fusion_driver ok\n");
    return 0;
}
