// The host layer with an n-gram LM set (csrc/api.cpp k2hip_ngram_lm_* / k2hip_set_ngram_lm) over the CPU stand-ins of the engine
// (engine_stub*.cpp; they keep the hotword states and zero the LM states), under AddressSanitizer / UBSan.  TEST INFRASTRUCTURE (`make -C k2transducerasr_amd/csrc san`,
// tests/test_ngram_sanitizers.py).
//
//   san_ngram_api_driver <offline.k2w>
#include <cmath>
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

static k2hip_ngram_lm_t* lm_for(int V) {
    // unigrams of 3 .. 7, <s>, <unk>; bigrams (<s> 4), (4 5); trigram (<s> 4 5)
    const int64_t ids[] = {K2HIP_NGRAM_BOS, K2HIP_NGRAM_UNK, 3, 4, 5, 6, 7, K2HIP_NGRAM_BOS, 4, 4, 5, K2HIP_NGRAM_BOS, 4, 5};
    const int32_t orders[] = {1, 1, 1, 1, 1, 1, 1, 2, 2, 3};
    const float lps[] = {-99.f, -7.f, -2.f, -2.5f, -3.f, -3.5f, -4.f, -1.f, -0.5f, -0.25f};
    const float bos[] = {-0.25f, 0.f, 0.f, -0.5f, 0.f, 0.f, 0.f, -0.125f, 0.f, 0.f};
    k2hip_ngram_lm_t* lm = nullptr;
    OK(k2hip_ngram_lm_create(ids, orders, lps, bos, 10, V, &lm));
    return lm;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    k2hip_model_t* m = nullptr;
    OK(k2hip_model_create(argv[1], nullptr, 0, &m));
    k2hip_model_info info;
    OK(k2hip_model_get_info(m, &info));
    const int V = info.vocab_size, J = info.joiner_dim;
    k2hip_ngram_lm_t* lm = lm_for(V);
    CHECK(k2hip_ngram_lm_order(lm) == 3 && k2hip_ngram_lm_num_states(lm) == 4 && k2hip_ngram_lm_num_arcs(lm) == 8 && k2hip_ngram_lm_start_state(lm) == 1);
    int32_t n = -1;
    float lp = 0.f;
    OK(k2hip_ngram_lm_step(lm, 1, 4, &n, &lp));
    CHECK(n == 3 && lp == -1.f);
    CHECK(k2hip_ngram_lm_step(lm, 9, 4, &n, &lp) == K2HIP_ERR_INVALID);
    CHECK(k2hip_ngram_lm_step(lm, 0, V, &n, &lp) == K2HIP_ERR_INVALID);
    CHECK(k2hip_ngram_lm_step(nullptr, 0, 4, &n, &lp) == K2HIP_ERR_INVALID);
    // argument errors of the setter, decided before any device work
    CHECK(k2hip_set_ngram_lm(nullptr, lm, 0.5f) == K2HIP_ERR_INVALID);
    CHECK(k2hip_set_ngram_lm(m, lm, -1.f) == K2HIP_ERR_INVALID);
    CHECK(k2hip_set_ngram_lm(m, lm, NAN) == K2HIP_ERR_INVALID);
    k2hip_ngram_lm_t* other = lm_for(V + 1);
    CHECK(k2hip_set_ngram_lm(m, other, 0.5f) == K2HIP_ERR_INVALID);
    CHECK(strstr(k2hip_last_error(), "vocab_size") != nullptr);
    OK(k2hip_ngram_lm_destroy(other));
    // set, replace, scale 0, clear; the LM dies right after the first set (the model keeps its own upload)
    OK(k2hip_set_ngram_lm(m, lm, 0.5f));
    OK(k2hip_ngram_lm_destroy(lm));
    lm = lm_for(V);
    OK(k2hip_set_ngram_lm(m, lm, 0.25f));
    // the streaming search carries the LM states in its side blocks; a stream keeps the LM it started with
    k2hip_beam_stream_t* s = nullptr;
    OK(k2hip_beam_stream_create(m, 4, &s));
    std::vector<float> enc((size_t)8 * J, 0.25f);
    OK(k2hip_beam_search_chunk(m, &s, 1, enc.data(), 8));
    OK(k2hip_beam_search_chunk(m, &s, 1, enc.data(), 8));
    OK(k2hip_set_ngram_lm(m, lm, 0.f));                        // scale 0 = no LM: another setting
    CHECK(k2hip_beam_search_chunk(m, &s, 1, enc.data(), 8) == K2HIP_ERR_INVALID);
    CHECK(strstr(k2hip_last_error(), "reset the stream first") != nullptr);
    OK(k2hip_beam_stream_reset(s));
    OK(k2hip_beam_search_chunk(m, &s, 1, enc.data(), 8));
    OK(k2hip_set_ngram_lm(m, lm, 1.f));
    CHECK(k2hip_beam_search_chunk(m, &s, 1, enc.data(), 8) == K2HIP_ERR_INVALID);
    OK(k2hip_set_ngram_lm(m, nullptr, 0.f));
    OK(k2hip_beam_search_chunk(m, &s, 1, enc.data(), 8));      // (cleared = the setting it started with after the reset)
    OK(k2hip_set_ngram_lm(m, lm, 1.f));        // left set: the model frees the tables
    OK(k2hip_ngram_lm_destroy(lm));
    OK(k2hip_beam_stream_destroy(s));
    OK(k2hip_model_destroy(m));
    printf("san_ngram_api_driver: ok\n");
    return 0;
}
