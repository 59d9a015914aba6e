// AddressSanitizer / UBSan driver of the streaming CTC prefix beam search's host side: the history a stream carries between chunks
// (csrc/ctc_prefix_hist.h), the float32 host reference of the resumed step (engine_stub_ctc_prefix_stream.cpp) and the argument rules
// of k2hip_ctc_prefix_stream_* / k2hip_ctc_prefix_beam_search_chunk (csrc/api.cpp) over the CPU stand-ins of the engine.  TEST
// INFRASTRUCTURE: its own program (`make -C k2transducerasr_amd/csrc san_ctc_prefix_stream`, tests/test_ctc_prefix_stream.py), never
// loaded into another process.
// Exercised: every case of the file the test writes (a row, a beam and a list of chunk lengths) chunked through CtcPrefixHistory and
// the resumed reference; after EVERY chunk the live prefixes equal ctc_prefix_ref.h over all frames so far bit for bit (tokens, absolute
// timestamps, token log-probs, pb, pnb, tot, order) and the live tree nodes are at most beam * (longest live prefix + 1) + 1.  Then,
// through the ABI: the refusals of create and of the chunk call (streams unchanged), a valid call after each, ragged n_frames, reset;
// and the recognizer level over the stand-in of the tick: the per-stream setting's rules, a list mixing settings, a set stream's result.
//   san_ctc_prefix_stream_driver <cases.bin> [<ctc.k2w> <offline.k2w> [<ctc_streaming.k2w>]]
// cases.bin: int32 n_cases, then per case int32 T, V, beam, n_chunks, int32 chunk_len[n_chunks], float32 lp[T][V].
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/k2hip.h"
#include "../../k2transducerasr_amd/csrc/ctc_prefix_hist.h"
#include "../../k2transducerasr_amd/csrc/ctc_prefix_ref.h"

#define CHECK(cond)                                                                                                          \
    do {                                                                                                                     \
        if (!(cond)) {                                                                                                       \
            fprintf(stderr, "CHECK failed at %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, k2hip_last_error()); \
            exit(3);                                                                                                         \
        }                                                                                                                    \
    } while (0)
#define OK(call) CHECK((call) == K2HIP_OK)

namespace k2hip {
void ctc_prefix_chunk_ref(const float* log_probs, int B, int Tc, int V, const int32_t* n_frames, int K, const int* in_all, int* out_all);
}

namespace {

using namespace k2hip;

bool same_bits(float a, float b) { return memcmp(&a, &b, sizeof(float)) == 0; }

int run_cases(const char* path) {
    FILE* f = fopen(path, "rb");
    CHECK(f != nullptr);
    int32_t n_cases = 0;
    CHECK(fread(&n_cases, 4, 1, f) == 1 && n_cases >= 1);
    long long folds_seen = 0;
    for (int c = 0; c < n_cases; c++) {
        int32_t hd[4];
        CHECK(fread(hd, 4, 4, f) == 4);
        const int T = hd[0], V = hd[1], beam = hd[2], nch = hd[3];
        CHECK(T >= 1 && V >= 1 && beam >= 1 && beam <= 8 && nch >= 1 && nch <= T);
        std::vector<int32_t> chunks((size_t)nch);
        CHECK(fread(chunks.data(), 4, (size_t)nch, f) == (size_t)nch);
        std::vector<float> lp((size_t)T * (size_t)V);
        CHECK(fread(lp.data(), 4, lp.size(), f) == lp.size());
        int Tc = 0, sum = 0;
        for (int32_t n : chunks) { CHECK(n >= 1); Tc = n > Tc ? n : Tc; sum += n; }
        CHECK(sum == T);
        const CtcPrefixResumeLayout L{beam, Tc};
        CtcPrefixHistory hist(beam, beam);
        std::vector<int> in((size_t)L.in_ints()), out((size_t)L.out_ints());
        std::vector<float> chunk((size_t)Tc * (size_t)V);
        int done = 0;
        for (int32_t n : chunks) {
            hist.fill_in(in.data(), Tc);
            std::fill(chunk.begin(), chunk.end(), 0.25f);   // (frames behind n_frames: ordinary values that must not be read)
            memcpy(chunk.data(), lp.data() + (size_t)done * (size_t)V, sizeof(float) * (size_t)n * (size_t)V);
            std::fill(out.begin(), out.end(), -7);
            ctc_prefix_chunk_ref(chunk.data(), 1, Tc, V, &n, beam, in.data(), out.data());
            hist.apply_out(out.data(), Tc, n);
            done += n;
            CHECK(hist.frames() == done);
            CHECK(hist.live_nodes() <= (size_t)beam * (size_t)(hist.longest() + 1) + 1);
            const CtcPrefixRefResult want = ctc_prefix_ref(lp.data(), V, done, V, beam);
            if (done == T) folds_seen += want.respelled_folds;
            const std::vector<BeamAlt> got = hist.nbest(beam);
            CHECK(got.size() == want.hyps.size() && hist.slots().size() == want.hyps.size());
            for (size_t i = 0; i < got.size(); i++) {
                const CtcPrefixRefHyp& h = want.hyps[i];
                CHECK(got[i].tokens == h.tokens && got[i].timestamps == h.timestamps && got[i].token_log_probs.size() == h.token_log_probs.size());
                for (size_t u = 0; u < h.tokens.size(); u++) CHECK(same_bits(got[i].token_log_probs[u], h.token_log_probs[u]));
                CHECK(same_bits(got[i].score, h.tot) && same_bits(hist.slots()[i].pb, h.pb) && same_bits(hist.slots()[i].pnb, h.pnb));
            }
            CHECK(hist.tokens() == want.hyps[0].tokens && hist.timestamps() == want.hyps[0].timestamps && same_bits(hist.score(), want.hyps[0].tot));
            CHECK(hist.token_log_probs().size() == want.hyps[0].tokens.size());
        }
        hist.reset();
        CHECK(hist.frames() == 0 && hist.tokens().empty() && hist.live_nodes() == 1 && hist.score() == 0.f);
    }
    fclose(f);
    CHECK(folds_seen >= 1);   // the file holds the re-spelled row: a fold no parent link shows was carried
    return n_cases;
}

struct Snap {
    std::vector<int64_t> tok;
    std::vector<int32_t> ts;
    float score = 0;
    int64_t frames = 0;
    bool operator==(const Snap& o) const { return tok == o.tok && ts == o.ts && same_bits(score, o.score) && frames == o.frames; }
};
Snap snap(const k2hip_ctc_prefix_stream_t* s) {
    Snap r;
    const int n = k2hip_ctc_prefix_stream_num_tokens(s);
    CHECK(n >= 0);
    r.tok.resize((size_t)n); r.ts.resize((size_t)n);
    OK(k2hip_ctc_prefix_stream_get_tokens(s, r.tok.data(), n));
    OK(k2hip_ctc_prefix_stream_get_timestamps(s, r.ts.data(), n));
    OK(k2hip_ctc_prefix_stream_get_score(s, &r.score));
    r.frames = k2hip_ctc_prefix_stream_num_frames(s);
    return r;
}

void abi(const char* ctc_path, const char* transducer_path) {
    k2hip_model_t *m = nullptr, *m2 = nullptr, *tr = nullptr;
    OK(k2hip_model_create(ctc_path, nullptr, 0, &m));
    OK(k2hip_model_create(ctc_path, nullptr, 0, &m2));
    OK(k2hip_model_create(transducer_path, nullptr, 0, &tr));
    k2hip_model_info info;
    OK(k2hip_model_get_info(m, &info));
    const int V = info.vocab_size, Tc = 5, T = 15;
    k2hip_ctc_prefix_stream_t *s4 = nullptr, *t4 = nullptr, *s8 = nullptr, *other = nullptr, *bad = nullptr;
    for (int b : {0, 9, -1}) CHECK(k2hip_ctc_prefix_stream_create(m, b, 1, &bad) == K2HIP_ERR_INVALID && bad == nullptr);
    for (int nb : {0, 5}) CHECK(k2hip_ctc_prefix_stream_create(m, 4, nb, &bad) == K2HIP_ERR_INVALID && bad == nullptr);
    CHECK(k2hip_ctc_prefix_stream_create(tr, 4, 1, &bad) == K2HIP_ERR_UNSUPPORTED && bad == nullptr);
    OK(k2hip_ctc_prefix_stream_create(m, 4, 4, &s4));
    OK(k2hip_ctc_prefix_stream_create(m, 4, 2, &t4));
    OK(k2hip_ctc_prefix_stream_create(m, 8, 8, &s8));
    OK(k2hip_ctc_prefix_stream_create(m2, 4, 4, &other));
    unsigned long long st = 88172645463325252ull;
    std::vector<float> rows((size_t)2 * T * V);   // two rows [T][V] of quarter steps (ties included)
    for (float& x : rows) { st ^= st << 13; st ^= st >> 7; st ^= st << 17; x = -0.25f * (float)((st >> 33) % 40); }
    auto chunk_of = [&](int t0) {   // [2][Tc][V]
        std::vector<float> c((size_t)2 * Tc * V);
        for (int r = 0; r < 2; r++) memcpy(c.data() + (size_t)r * Tc * V, rows.data() + ((size_t)r * T + (size_t)t0) * V, sizeof(float) * (size_t)Tc * V);
        return c;
    };
    k2hip_ctc_prefix_stream_t* pair[2] = {s4, t4};
    const std::vector<float> c0 = chunk_of(0);
    OK(k2hip_ctc_prefix_beam_search_chunk(m, pair, 2, c0.data(), Tc, nullptr));
    const Snap a0 = snap(s4), b0 = snap(t4);
    CHECK(a0.frames == Tc && b0.frames == Tc);
    auto unchanged = [&] { return snap(s4) == a0 && snap(t4) == b0; };
    {   // the refusals, each decided before anything moves
        k2hip_ctc_prefix_stream_t* mixed[2] = {s4, s8};
        CHECK(k2hip_ctc_prefix_beam_search_chunk(m, mixed, 2, c0.data(), Tc, nullptr) == K2HIP_ERR_INVALID && unchanged() && snap(s8).frames == 0);
        k2hip_ctc_prefix_stream_t* twice[2] = {s4, s4};
        CHECK(k2hip_ctc_prefix_beam_search_chunk(m, twice, 2, c0.data(), Tc, nullptr) == K2HIP_ERR_INVALID && unchanged());
        k2hip_ctc_prefix_stream_t* foreign[2] = {s4, other};
        CHECK(k2hip_ctc_prefix_beam_search_chunk(m, foreign, 2, c0.data(), Tc, nullptr) == K2HIP_ERR_INVALID && unchanged() && snap(other).frames == 0);
        for (int32_t nfb : {0, Tc + 1, -3}) {
            const int32_t nf[2] = {Tc, nfb};
            CHECK(k2hip_ctc_prefix_beam_search_chunk(m, pair, 2, c0.data(), Tc, nf) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "n_frames") && unchanged());
        }
        CHECK(k2hip_ctc_prefix_beam_search_chunk(tr, pair, 2, c0.data(), Tc, nullptr) == K2HIP_ERR_UNSUPPORTED && unchanged());
        CHECK(k2hip_ctc_prefix_beam_search_chunk(m, pair, 0, c0.data(), Tc, nullptr) == K2HIP_ERR_INVALID && unchanged());
        CHECK(k2hip_ctc_prefix_beam_search_chunk(m, pair, 2, c0.data(), 0, nullptr) == K2HIP_ERR_INVALID && unchanged());
        CHECK(k2hip_ctc_prefix_beam_search_chunk(m, pair, 2, nullptr, Tc, nullptr) == K2HIP_ERR_INVALID && unchanged());
        CHECK(k2hip_ctc_prefix_beam_search_chunk(m, nullptr, 2, c0.data(), Tc, nullptr) == K2HIP_ERR_INVALID && unchanged());
    }
    // ... and the streams go on as if nothing had happened: chunk 2 ragged (row 1 gets 3 of its 5 frames, the other 2 in a call of its own)
    const std::vector<float> c1 = chunk_of(Tc), c2 = chunk_of(2 * Tc);
    const int32_t nf1[2] = {Tc, 3};
    OK(k2hip_ctc_prefix_beam_search_chunk(m, pair, 2, c1.data(), Tc, nf1));
    {
        std::vector<float> rest((size_t)Tc * V, 0.25f);
        memcpy(rest.data(), rows.data() + ((size_t)T + Tc + 3) * V, sizeof(float) * 2 * (size_t)V);
        const int32_t two = 2;
        OK(k2hip_ctc_prefix_beam_search_chunk(m, &pair[1], 1, rest.data(), Tc, &two));
    }
    OK(k2hip_ctc_prefix_beam_search_chunk(m, pair, 2, c2.data(), Tc, nullptr));
    for (int r = 0; r < 2; r++) {   // against the offline entry over the whole rows
        const k2hip_ctc_prefix_stream_t* s = pair[r];
        const int nb = r == 0 ? 4 : 2;
        std::vector<int64_t> tok((size_t)nb * T, -7);
        std::vector<int32_t> ts((size_t)nb * T, -7), n((size_t)nb, -7);
        std::vector<float> yp((size_t)nb * T, -7.f), sc((size_t)nb, -7.f);
        int32_t nh = -7;
        OK(k2hip_ctc_prefix_beam_search(m, rows.data() + (size_t)r * T * V, 1, T, nullptr, 4, nb, tok.data(), ts.data(), yp.data(), n.data(), &nh, sc.data(), T));
        CHECK(k2hip_ctc_prefix_stream_num_frames(s) == T && k2hip_ctc_prefix_stream_num_alternatives(s) == nh);
        for (int i = 0; i < nh; i++) {
            std::vector<int64_t> gt((size_t)T);
            std::vector<int32_t> gs((size_t)T);
            std::vector<float> gy((size_t)T);
            int32_t gn = -1;
            float gsc = 0;
            OK(k2hip_ctc_prefix_stream_get_alternative(s, i, gt.data(), gs.data(), gy.data(), T, &gn, &gsc));
            CHECK(gn == n[(size_t)i] && same_bits(gsc, sc[(size_t)i]));
            for (int u = 0; u < gn; u++)
                CHECK(gt[(size_t)u] == tok[(size_t)i * T + u] && gs[(size_t)u] == ts[(size_t)i * T + u] && same_bits(gy[(size_t)u], yp[(size_t)i * T + u]));
        }
        CHECK(k2hip_ctc_prefix_stream_get_alternative(s, nh, nullptr, nullptr, nullptr, 0, nullptr, nullptr) == K2HIP_ERR_INVALID);
        const Snap fin = snap(s);
        CHECK((int)fin.tok.size() == n[0] && same_bits(fin.score, sc[0]));
        std::vector<float> y1((size_t)T);
        CHECK(k2hip_ctc_prefix_stream_get_token_log_probs(s, y1.data(), T) == n[0]);
        if (n[0] > 0) CHECK(k2hip_ctc_prefix_stream_get_tokens(s, nullptr, 0) == K2HIP_ERR_CAPACITY);
    }
    OK(k2hip_ctc_prefix_stream_reset(s4));
    CHECK(snap(s4).frames == 0 && snap(s4).tok.empty() && snap(s4).score == 0.f && k2hip_ctc_prefix_stream_num_alternatives(s4) == 1);
    CHECK(k2hip_ctc_prefix_stream_num_tokens(nullptr) == -1 && k2hip_ctc_prefix_stream_num_frames(nullptr) == -1);
    CHECK(k2hip_ctc_prefix_stream_reset(nullptr) == K2HIP_ERR_INVALID);
    for (k2hip_ctc_prefix_stream_t* s : {s4, t4, s8, other}) OK(k2hip_ctc_prefix_stream_destroy(s));
    OK(k2hip_ctc_prefix_stream_destroy(nullptr));
    OK(k2hip_model_destroy(m));
    OK(k2hip_model_destroy(m2));
    OK(k2hip_model_destroy(tr));
}

// recognizer level over the stand-in of the tick: the per-stream setting's rules, a list mixing settings, the result of a set stream
void recognizer(const char* ctc_streaming_path, const char* transducer_path) {
    k2hip_model_t *m = nullptr, *tr = nullptr;
    OK(k2hip_model_create(ctc_streaming_path, nullptr, 0, &m));
    OK(k2hip_model_create(transducer_path, nullptr, 0, &tr));
    k2hip_model_info info;
    OK(k2hip_model_get_info(m, &info));
    int32_t T = 0, shift = 0, Tp = 0;
    OK(k2hip_online_chunk_info(m, &T, &shift, &Tp));
    k2hip_online_stream_t *a = nullptr, *b = nullptr, *g = nullptr;
    OK(k2hip_online_stream_create(m, &a));
    OK(k2hip_online_stream_create(m, &b));
    OK(k2hip_online_stream_create(m, &g));
    for (int bad : {-1, 9}) CHECK(k2hip_online_stream_set_ctc_prefix_beam(a, bad, 1) == K2HIP_ERR_INVALID);
    for (int bad : {0, 5}) CHECK(k2hip_online_stream_set_ctc_prefix_beam(a, 4, bad) == K2HIP_ERR_INVALID);
    CHECK(k2hip_online_stream_set_ctc_prefix_beam(nullptr, 4, 1) == K2HIP_ERR_INVALID);
    OK(k2hip_online_stream_set_ctc_prefix_beam(a, 4, 2));
    OK(k2hip_online_stream_set_ctc_prefix_beam(b, 4, 4));
    float sc = -1;
    OK(k2hip_online_stream_get_score(a, &sc));
    CHECK(sc == 0.f && k2hip_online_stream_num_alternatives(a) == 1);
    std::vector<float> feats((size_t)(T + shift) * (size_t)info.feature_dim);
    for (size_t i = 0; i < feats.size(); i++) feats[i] = -3.f + 0.125f * (float)(i % 41);
    for (k2hip_online_stream_t* s : {a, b, g}) OK(k2hip_online_stream_accept_features(s, feats.data(), T + shift));
    int32_t dec[3] = {-7, -7, -7}, nn[3] = {-7, -7, -7};
    k2hip_online_stream_t* mixed[3] = {a, b, g};
    const int64_t before = k2hip_online_stream_speech_length(a);
    CHECK(k2hip_online_step(m, mixed, 3, dec, nn) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "ctc_prefix_beam") != nullptr);
    CHECK(k2hip_online_stream_speech_length(a) == before && k2hip_online_stream_num_tokens(a) == 2 && k2hip_online_stream_num_tokens(g) == 2);
    k2hip_online_stream_t* set[2] = {a, b};
    for (int tick = 0; tick < 2; tick++) {
        OK(k2hip_online_step(m, set, 2, dec, nn));
        CHECK(dec[0] == 1 && dec[1] == 1);
        const int n = k2hip_online_stream_num_tokens(a), nt = k2hip_online_stream_num_timestamps(a);
        CHECK(n == nt + 2 && n >= 2);
        std::vector<int64_t> tok((size_t)n);
        std::vector<int32_t> ts((size_t)nt + 1);
        OK(k2hip_online_stream_get_tokens(a, tok.data(), n));
        OK(k2hip_online_stream_get_timestamps(a, ts.data(), nt));
        CHECK(tok[0] == K2HIP_BLANK_ID && tok[1] == K2HIP_BLANK_ID);
        for (int i = 0; i < nt; i++) CHECK(ts[(size_t)i] >= 0 && ts[(size_t)i] < (tick + 1) * Tp && (i == 0 || ts[(size_t)i - 1] < ts[(size_t)i]));
        CHECK(k2hip_online_stream_num_alternatives(a) >= 1 && k2hip_online_stream_num_alternatives(a) <= 2 && k2hip_online_stream_num_alternatives(b) <= 4);
        int32_t an = -1;
        std::vector<int64_t> at((size_t)n);
        OK(k2hip_online_stream_get_alternative(a, 0, at.data(), nullptr, nullptr, n, &an, &sc));
        CHECK(an == nt && std::equal(at.begin(), at.begin() + an, tok.begin() + 2));
        float sc1 = 0;
        OK(k2hip_online_stream_get_score(a, &sc1));
        CHECK(same_bits(sc, sc1));
        std::vector<float> yp((size_t)nt + 1);
        CHECK(k2hip_online_stream_get_token_log_probs(a, yp.data(), nt) == nt);
    }
    CHECK(k2hip_online_stream_set_ctc_prefix_beam(a, 8, 1) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "reset") != nullptr);
    OK(k2hip_online_stream_reset(a));
    CHECK(k2hip_online_stream_num_tokens(a) == 2 && k2hip_online_stream_num_alternatives(a) == 1);   // the setting stays, the prefixes went
    OK(k2hip_online_stream_get_score(a, &sc));
    CHECK(sc == 0.f);
    OK(k2hip_online_stream_set_ctc_prefix_beam(a, 0, 0));   // off again: greedy
    k2hip_online_stream_t* one[1] = {g};
    OK(k2hip_online_step(m, one, 1, dec, nn));   // the stream without the setting decodes as before
    CHECK(dec[0] == 1 && k2hip_online_stream_get_score(g, &sc) == K2HIP_ERR_INVALID);
    for (k2hip_online_stream_t* s : {a, b, g}) OK(k2hip_online_stream_destroy(s));
    OK(k2hip_model_destroy(m));
    OK(k2hip_model_destroy(tr));
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: san_ctc_prefix_stream_driver <cases.bin> [<ctc.k2w> <offline.k2w>]\n");
        return 2;
    }
    const int n = run_cases(argv[1]);
    if (argc >= 4) abi(argv[2], argv[3]);
    if (argc >= 5) recognizer(argv[4], argv[3]);
    else fprintf(stderr, "san_ctc_prefix_stream_driver: no model files given, the ABI part is skipped\n");
    printf("san_ctc_prefix_stream_driver ok (%d cases)\n", n);
    return 0;
}
