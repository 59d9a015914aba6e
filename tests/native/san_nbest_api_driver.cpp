// AddressSanitizer / UBSan driver for the host layer of the N-best entry points (csrc/api.cpp: k2hip_set_nbest,
// k2hip_beam_search_nbest, k2hip_*_stream_num_alternatives / _get_alternative / _get_token_log_probs) over the CPU stand-ins of the
// engine (engine_stub*.cpp).  TEST INFRASTRUCTURE (`make -C k2transducerasr_amd/csrc san`, tests/test_nbest.py).
// Exercised: a bad nbest, a small cap (nothing written), greedy / CTC rejection, the pipelined route's and GetResult's refusal, the
// start state before a result, after a reset and after a failed GetResults (the stand-in's search keeps no list, which the host
// layer must report instead of returning one result), a greedy stream's accessors, the side block's lifetime over a streaming step.
//   san_nbest_api_driver <offline.k2w> <streaming.k2w> <ctc.k2w>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/k2hip.h"

#define CHECK(cond)                                                                                                          \
    do {                                                                                                                     \
        if (!(cond)) {                                                                                                       \
            fprintf(stderr, "CHECK failed at %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, k2hip_last_error()); \
            exit(3);                                                                                                         \
        }                                                                                                                    \
    } while (0)
#define OK(call) CHECK((call) == K2HIP_OK)

namespace {

// the start state through one stream kind's three accessors, and the cap rule on it
template <typename S, typename Num, typename Get, typename Yp>
void start_state(const S* s, Num num, Get get, Yp yp) {
    CHECK(num(s) == 1);
    int64_t tok[2] = {-7, -7};
    int32_t ts[2] = {-7, -7}, n = -7;
    float lp[2] = {-7.f, -7.f}, score = -7.f;
    OK(get(s, 0, tok, ts, lp, 2, &n, &score));
    CHECK(n == 0 && score == 0.f && tok[0] == -7 && ts[0] == -7 && lp[0] == -7.f);
    OK(get(s, 0, nullptr, nullptr, nullptr, 0, &n, nullptr));            // every output is optional
    CHECK(get(s, 1, tok, ts, lp, 2, &n, &score) == K2HIP_ERR_INVALID);   // outside the list
    CHECK(get(s, -1, tok, ts, lp, 2, &n, &score) == K2HIP_ERR_INVALID);
    n = -7; score = -7.f;
    CHECK(get(s, 0, tok, ts, lp, -1, &n, &score) == K2HIP_ERR_CAPACITY);  // cap too small: nothing is written, not even the count
    CHECK(n == -7 && score == -7.f && tok[0] == -7);
    CHECK(yp(s, lp, 2) == 0 && lp[0] == -7.f);
    CHECK(yp(s, nullptr, 0) == 0);
    CHECK(yp(s, lp, -1) == K2HIP_ERR_CAPACITY && lp[0] == -7.f);
}

void offline(const char* path) {
    k2hip_model_t* m = nullptr;
    OK(k2hip_model_create(path, nullptr, 0, &m));
    k2hip_model_info info;
    OK(k2hip_model_get_info(m, &info));
    for (int bad : {0, 9, -1}) {
        CHECK(k2hip_set_nbest(m, bad) == K2HIP_ERR_INVALID);
        CHECK(strstr(k2hip_last_error(), "out of range") != nullptr);
    }
    OK(k2hip_set_nbest(m, 1));                                           // off is always allowed
    CHECK(k2hip_set_nbest(m, 4) == K2HIP_ERR_INVALID);                   // greedy_search has no alternatives
    CHECK(strstr(k2hip_last_error(), "modified_beam_search") != nullptr);
    // operator level: bad nbest / beam / shape, decided before any device work
    std::vector<float> enc((size_t)2 * 4 * info.joiner_dim, 0.25f);
    std::vector<int64_t> tok(2 * 8 * 4, -7);
    std::vector<int32_t> ts(2 * 8 * 4, -7), nt(2 * 8, -7), nh(2, -7);
    std::vector<float> lp(2 * 8 * 4, -7.f), sc(2 * 8, -7.f);
    for (int bad : {0, 9})
        CHECK(k2hip_beam_search_nbest(m, enc.data(), 2, 4, 4, bad, tok.data(), ts.data(), lp.data(), nt.data(), nh.data(), sc.data(), 4) == K2HIP_ERR_INVALID);
    CHECK(k2hip_beam_search_nbest(m, enc.data(), 2, 4, 9, 2, tok.data(), ts.data(), lp.data(), nt.data(), nh.data(), sc.data(), 4) == K2HIP_ERR_INVALID);
    CHECK(k2hip_beam_search_nbest(m, enc.data(), 2, 4, 4, 2, tok.data(), ts.data(), lp.data(), nt.data(), nh.data(), sc.data(), 0) == K2HIP_ERR_INVALID);
    CHECK(k2hip_beam_search_nbest(m, enc.data(), 2, 4, 4, 2, tok.data(), ts.data(), nullptr, nt.data(), nh.data(), sc.data(), 4) == K2HIP_ERR_INVALID);
    CHECK(tok[0] == -7 && nh[0] == -7 && sc[0] == -7.f);
    // streams: the start state before any result
    k2hip_offline_stream_t *a = nullptr, *b = nullptr;
    OK(k2hip_offline_stream_create(m, &a));
    OK(k2hip_offline_stream_create(m, &b));
    start_state(a, k2hip_offline_stream_num_alternatives, k2hip_offline_stream_get_alternative, k2hip_offline_stream_get_token_log_probs);
    std::vector<float> wav(16000, 0.f);
    for (size_t i = 0; i < wav.size(); i++) wav[i] = (float)((int)(i * 2654435761u % 2001) - 1000) / 1000.f;
    OK(k2hip_offline_stream_accept_samples(a, wav.data(), (int64_t)wav.size()));
    OK(k2hip_offline_stream_accept_samples(b, wav.data(), (int64_t)wav.size()));
    k2hip_offline_stream_t* both[2] = {a, b};
    // n = 1: GetResults as ever, the streams keep the start state (nothing is kept beyond the result)
    OK(k2hip_set_decoding_method(m, "modified_beam_search", 4));
    OK(k2hip_offline_recognizer_get_results(m, both, 2));
    start_state(a, k2hip_offline_stream_num_alternatives, k2hip_offline_stream_get_alternative, k2hip_offline_stream_get_token_log_probs);
    // n > 1
    OK(k2hip_set_nbest(m, 4));
    int32_t ticket = -1;
    CHECK(k2hip_offline_submit_samples(m, wav.data(), 8000, 2, 16, &ticket) == K2HIP_ERR_INVALID);   // the pipelined route: refused, loudly
    CHECK(strstr(k2hip_last_error(), "k2hip_set_nbest") != nullptr && ticket == -1);
    CHECK(k2hip_offline_submit_samples_dev(m, wav.data(), 8000, 2, 16, &ticket) == K2HIP_ERR_INVALID);
    CHECK(k2hip_offline_wait(m, 0, tok.data(), ts.data(), nt.data()) == K2HIP_ERR_INVALID);
    CHECK(strstr(k2hip_last_error(), "k2hip_set_nbest") != nullptr);
    OK(k2hip_offline_stream_accept_samples(a, wav.data(), (int64_t)wav.size()));
    CHECK(k2hip_offline_recognizer_get_result(m, a) == K2HIP_ERR_INVALID);                        // the single-stream path is greedy search
    CHECK(strstr(k2hip_last_error(), "GetResults") != nullptr);
    start_state(a, k2hip_offline_stream_num_alternatives, k2hip_offline_stream_get_alternative, k2hip_offline_stream_get_token_log_probs);
    // a GetResults that fails (the stand-in's search keeps no list: reported, never one silent result) leaves the start state
    OK(k2hip_offline_stream_accept_samples(b, wav.data(), (int64_t)wav.size()));
    CHECK(k2hip_offline_recognizer_get_results(m, both, 2) == K2HIP_ERR_INVALID);
    CHECK(strstr(k2hip_last_error(), "kept no list") != nullptr);
    start_state(a, k2hip_offline_stream_num_alternatives, k2hip_offline_stream_get_alternative, k2hip_offline_stream_get_token_log_probs);
    start_state(b, k2hip_offline_stream_num_alternatives, k2hip_offline_stream_get_alternative, k2hip_offline_stream_get_token_log_probs);
    // greedy_search while the model keeps alternatives: GetResults is refused
    OK(k2hip_set_decoding_method(m, "greedy_search", 0));
    CHECK(k2hip_offline_recognizer_get_results(m, both, 2) == K2HIP_ERR_INVALID);
    CHECK(strstr(k2hip_last_error(), "greedy_search") != nullptr);
    // off again: everything is as before
    OK(k2hip_set_nbest(m, 1));
    OK(k2hip_offline_recognizer_get_results(m, both, 2));
    OK(k2hip_offline_recognizer_get_result(m, a));
    OK(k2hip_offline_stream_destroy(a));
    OK(k2hip_offline_stream_destroy(b));
    OK(k2hip_model_destroy(m));
}

void streaming(const char* path) {
    k2hip_model_t* m = nullptr;
    OK(k2hip_model_create(path, nullptr, 0, &m));
    k2hip_model_info info;
    OK(k2hip_model_get_info(m, &info));
    OK(k2hip_set_decoding_method(m, "modified_beam_search", 4));
    OK(k2hip_set_nbest(m, 4));
    k2hip_online_stream_t *a = nullptr, *g = nullptr;
    OK(k2hip_online_stream_create(m, &a));
    OK(k2hip_online_stream_create(m, &g));
    start_state(a, k2hip_online_stream_num_alternatives, k2hip_online_stream_get_alternative, k2hip_online_stream_get_token_log_probs);
    std::vector<float> wav(16000, 0.f);
    for (size_t i = 0; i < wav.size(); i++) wav[i] = (float)((int)(i * 2654435761u % 2001) - 1000) / 1000.f;
    int32_t dec = 0, nn = 0;
    for (int round = 0; round < 3; round++) {   // (the side block lives for the call only)
        OK(k2hip_online_stream_accept_samples(a, wav.data(), (int64_t)wav.size()));
        OK(k2hip_online_step(m, &a, 1, &dec, &nn));
        CHECK(dec == 1);
        // the stand-in lets the start hypothesis survive unchanged: one empty alternative, score 0, no token log-probs
        start_state(a, k2hip_online_stream_num_alternatives, k2hip_online_stream_get_alternative, k2hip_online_stream_get_token_log_probs);
    }
    OK(k2hip_online_stream_reset(a));
    start_state(a, k2hip_online_stream_num_alternatives, k2hip_online_stream_get_alternative, k2hip_online_stream_get_token_log_probs);
    // greedy search while the model keeps alternatives: the step is refused and the stream is untouched
    OK(k2hip_set_decoding_method(m, "greedy_search", 0));
    OK(k2hip_online_stream_accept_samples(g, wav.data(), (int64_t)wav.size()));
    CHECK(k2hip_online_step(m, &g, 1, &dec, &nn) == K2HIP_ERR_INVALID);
    CHECK(strstr(k2hip_last_error(), "greedy_search") != nullptr);
    // a stream that decodes with greedy search has no alternatives and no token log-probs
    OK(k2hip_set_decoding_method(m, "modified_beam_search", 4));
    OK(k2hip_set_nbest(m, 1));
    OK(k2hip_set_decoding_method(m, "greedy_search", 0));
    OK(k2hip_online_step(m, &g, 1, &dec, &nn));
    CHECK(dec == 1);
    float lp[1] = {-7.f};
    int32_t n = -7;
    CHECK(k2hip_online_stream_num_alternatives(g) == K2HIP_ERR_INVALID);
    CHECK(k2hip_online_stream_get_alternative(g, 0, nullptr, nullptr, nullptr, 0, &n, nullptr) == K2HIP_ERR_INVALID && n == -7);
    CHECK(k2hip_online_stream_get_token_log_probs(g, lp, 1) == K2HIP_ERR_INVALID && lp[0] == -7.f);
    // operator level of the streaming search
    OK(k2hip_set_decoding_method(m, "modified_beam_search", 4));
    OK(k2hip_set_nbest(m, 8));
    k2hip_beam_stream_t* s = nullptr;
    OK(k2hip_beam_stream_create(m, 4, &s));
    start_state(s, k2hip_beam_stream_num_alternatives, k2hip_beam_stream_get_alternative, k2hip_beam_stream_get_token_log_probs);
    std::vector<float> enc((size_t)5 * info.joiner_dim, 0.25f);
    OK(k2hip_beam_search_chunk(m, &s, 1, enc.data(), 5));
    OK(k2hip_beam_search_chunk(m, &s, 1, enc.data(), 1));
    start_state(s, k2hip_beam_stream_num_alternatives, k2hip_beam_stream_get_alternative, k2hip_beam_stream_get_token_log_probs);
    OK(k2hip_beam_stream_reset(s));
    start_state(s, k2hip_beam_stream_num_alternatives, k2hip_beam_stream_get_alternative, k2hip_beam_stream_get_token_log_probs);
    OK(k2hip_beam_stream_destroy(s));
    OK(k2hip_online_stream_destroy(a));
    OK(k2hip_online_stream_destroy(g));
    OK(k2hip_model_destroy(m));
}

void ctc(const char* path) {
    k2hip_model_t* m = nullptr;
    OK(k2hip_model_create(path, nullptr, 0, &m));
    OK(k2hip_set_nbest(m, 1));
    CHECK(k2hip_set_nbest(m, 2) == K2HIP_ERR_UNSUPPORTED);
    CHECK(strstr(k2hip_last_error(), "CTC") != nullptr);
    k2hip_model_info info;
    OK(k2hip_model_get_info(m, &info));
    std::vector<float> enc((size_t)4 * 600, 0.f);
    int64_t tok[8];
    int32_t ts[8], nt[2], nh[1];
    float lp[8], sc[2];
    CHECK(k2hip_beam_search_nbest(m, enc.data(), 1, 4, 4, 2, tok, ts, lp, nt, nh, sc, 4) == K2HIP_ERR_UNSUPPORTED);
    OK(k2hip_model_destroy(m));
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s <offline.k2w> <streaming.k2w> <ctc.k2w>\n", argv[0]);
        return 2;
    }
    CHECK(k2hip_set_nbest(nullptr, 2) == K2HIP_ERR_INVALID);
    CHECK(k2hip_offline_stream_num_alternatives(nullptr) == -1 && k2hip_online_stream_num_alternatives(nullptr) < 0 &&
          k2hip_beam_stream_num_alternatives(nullptr) == -1);
    offline(argv[1]);
    streaming(argv[2]);
    ctc(argv[3]);
    printf("OK\n");
    return 0;
}
