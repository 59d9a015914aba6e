// AddressSanitizer / UBSan driver of the CTC keyword spotter's host side: the header-only reference of the token passing
// (csrc/ctc_kws_ref.h) and the argument checks of the k2hip_ctc_kws_* entries (csrc/api.cpp) over the CPU stand-ins of the engine
// (engine_stub*.cpp).  TEST INFRASTRUCTURE: its own program (`make -C k2transducerasr_amd/csrc san_ctc_kws`, tests/test_ctc_kws.py),
// never loaded into another process.
// Exercised: ctc_kws_ref.h against an explicit enumeration of frame labellings on tiny tries with -inf cells (values, the entered
// flag, events, the reset, the hold) and any chunking against one call; then every refusal of the entries (a transducer model, a graph
// of another vocabulary size, a stream twice, a stream of another model, n_frames out of range, Tc = 0, NULL arguments), each followed
// by a valid call that shows every stream unchanged; the streams' life cycle with the graph destroyed before its stream and a stream
// outliving its model; the fused entry and its capacity rule.
//   san_ctc_kws_driver <ctc.k2w> <offline.k2w>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/k2hip.h"
#include "../../include/k2hip_debug.h"
#include "../../k2transducerasr_amd/csrc/ctc_kws_ref.h"

#define CHECK(cond)                                                                                                          \
    do {                                                                                                                     \
        if (!(cond)) {                                                                                                       \
            fprintf(stderr, "CHECK failed at %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, k2hip_last_error()); \
            exit(3);                                                                                                         \
        }                                                                                                                    \
    } while (0)
#define OK(call) CHECK((call) == K2HIP_OK)

namespace {

using k2hip::KwsRefEvent;

unsigned long long rng_state = 88172645463325252ull;
unsigned rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 32);
}

struct Trie {
    std::vector<int32_t> parent, tok, depth, kw;
    std::vector<float> bar;
    std::vector<int32_t> rc;
    int S() const { return (int)parent.size(); }
};

Trie make_trie(const std::vector<std::vector<int>>& words, float bar_per_token) {
    Trie g;
    g.parent = {-1}; g.tok = {-1}; g.depth = {0}; g.kw = {-1};
    for (size_t p = 0; p < words.size(); p++) {
        int s = 0;
        for (int v : words[p]) {
            int c = -1;
            for (int k = 1; k < g.S(); k++)
                if (g.parent[(size_t)k] == s && g.tok[(size_t)k] == v) c = k;
            if (c < 0) {
                c = g.S();
                g.parent.push_back(s); g.tok.push_back(v); g.depth.push_back(g.depth[(size_t)s] + 1); g.kw.push_back(-1);
            }
            s = c;
        }
        g.kw[(size_t)s] = (int32_t)p;
    }
    for (int s = 0; s < g.S(); s++) g.bar.push_back(g.kw[(size_t)s] >= 0 ? bar_per_token * (float)g.depth[(size_t)s] : 0.f);
    g.rc.resize((size_t)g.S());
    k2hip::ctc_kws_root_children(g.parent.data(), g.tok.data(), g.S(), g.rc.data());
    return g;
}

struct Best {
    float n = -INFINITY, b = -INFINITY, entry = -INFINITY;   // entry: the best labelling ending on the token that is no self loop
};

// the best labellings of state c over frames s..t for every start s in (R, t]: explicit enumeration over {path tokens, blank}
Best enumerate(const Trie& g, const float* lp, int V, int c, int t, int R, const std::vector<int>& closed) {
    std::vector<int> path;
    for (int s = c; s > 0; s = g.parent[(size_t)s]) path.insert(path.begin(), g.tok[(size_t)s]);
    std::vector<int> sym = {0};
    for (int v : path)
        if (std::find(sym.begin(), sym.end(), v) == sym.end()) sym.push_back(v);
    int first = c;
    while (g.parent[(size_t)first] != 0) first = g.parent[(size_t)first];
    Best best;
    const int K = (int)sym.size();
    for (int s = R + 1; s <= t; s++) {
        if (closed[(size_t)s] == first) continue;
        const int L = t - s + 1;
        long long count = 1;
        for (int i = 0; i < L; i++) count *= K;
        std::vector<int> lab((size_t)L);
        for (long long code = 0; code < count; code++) {
            long long x = code;
            for (int i = 0; i < L; i++) { lab[(size_t)i] = sym[(size_t)(x % K)]; x /= K; }
            if (lab[0] == 0) continue;
            std::vector<int> col;
            int prev = 0;
            for (int v : lab) {
                if (v != 0 && v != prev) col.push_back(v);
                prev = v;
            }
            if (col != path) continue;
            float val = 0.f;   // (multiples of 0.25: exact in any order)
            for (int i = 0; i < L; i++) val += lp[(size_t)(s + i) * V + lab[(size_t)i]];
            if (lab[(size_t)L - 1] == 0) best.b = std::max(best.b, val);
            else {
                best.n = std::max(best.n, val);
                if (!(L >= 2 && lab[(size_t)L - 2] == lab[(size_t)L - 1])) best.entry = std::max(best.entry, val);
            }
        }
    }
    return best;
}

void reference() {
    const int V = 5;
    const std::vector<std::vector<std::vector<int>>> sets = {{{1}}, {{1, 3}}, {{1, 1}}, {{1}, {1, 3}, {3}, {3, 1}}, {{1, 3, 3}}, {{3, 1, 3}, {3, 1}}};
    int fired = 0, held = 0;
    for (const auto& words : sets) {
        const Trie g = make_trie(words, -0.75f);
        const int S = g.S();
        for (int T = 1; T <= 5; T++)
            for (int trial = 0; trial < 4; trial++) {
                std::vector<float> lp((size_t)T * V);
                for (float& x : lp) x = (trial >= 2 && rnd() % 5 == 0) ? -INFINITY : -0.25f * (float)(rnd() % 6);
                std::vector<float> v(2 * (size_t)S), v1(2 * (size_t)S);
                std::vector<int32_t> st(2 * (size_t)S), st1(2 * (size_t)S);
                k2hip::ctc_kws_fresh_state(S, v.data(), st.data());
                k2hip::ctc_kws_fresh_state(S, v1.data(), st1.data());
                std::vector<KwsRefEvent> all;
                k2hip::ctc_kws_dp_ref(g.parent.data(), g.tok.data(), g.depth.data(), g.kw.data(), g.bar.data(), g.rc.data(), S, lp.data(), V, T, v1.data(),
                                      st1.data(), &all);
                int R = -1, hold = -1;
                std::vector<int> closed;
                std::vector<KwsRefEvent> seen;
                for (int t = 0; t < T; t++) {
                    if (hold >= 0 && !(lp[(size_t)t * V + g.tok[(size_t)hold]] >= lp[(size_t)t * V])) hold = -1;
                    closed.push_back(hold);
                    held += hold >= 0;
                    std::vector<KwsRefEvent> ev;
                    k2hip::ctc_kws_dp_ref(g.parent.data(), g.tok.data(), g.depth.data(), g.kw.data(), g.bar.data(), g.rc.data(), S, lp.data() + (size_t)t * V,
                                          V, 1, v.data(), st.data(), &ev);
                    int win = -1;
                    std::vector<Best> want((size_t)S);
                    for (int c = 1; c < S; c++) {
                        const Best w = want[(size_t)c] = enumerate(g, lp.data(), V, c, t, R, closed);
                        if (g.kw[(size_t)c] < 0 || !(w.n > -INFINITY) || w.entry != w.n || !(w.n >= g.bar[(size_t)c])) continue;
                        if (win < 0 || g.depth[(size_t)c] > g.depth[(size_t)win] ||
                            (g.depth[(size_t)c] == g.depth[(size_t)win] &&
                             (w.n > want[(size_t)win].n || (w.n == want[(size_t)win].n && g.kw[(size_t)c] < g.kw[(size_t)win]))))
                            win = c;
                    }
                    if (win >= 0) {
                        CHECK(ev.size() == 1 && ev[0].keyword == g.kw[(size_t)win] && ev[0].end == t && ev[0].sum_logp == want[(size_t)win].n);
                        CHECK(ev[0].start > R && ev[0].start <= t);
                        for (int c = 1; c < S; c++) CHECK(v[(size_t)c] == -INFINITY && v[(size_t)(S + c)] == -INFINITY && st[(size_t)c] == -1 && st[(size_t)(S + c)] == -1);
                        R = t;
                        hold = g.rc[(size_t)win];
                        fired++;
                        seen.push_back(ev[0]);
                    } else {
                        CHECK(ev.empty());
                        for (int c = 1; c < S; c++) {
                            CHECK(v[(size_t)c] == want[(size_t)c].n && v[(size_t)(S + c)] == want[(size_t)c].b);
                            CHECK((st[(size_t)c] == -1) == !(v[(size_t)c] > -INFINITY) && (st[(size_t)(S + c)] == -1) == !(v[(size_t)(S + c)] > -INFINITY));
                        }
                    }
                    CHECK(v[0] == 0.f && st[0] == t + 1 && v[(size_t)S] == -INFINITY && st[(size_t)S] == hold);
                }
                // frame by frame = one call
                CHECK(seen.size() == all.size() && memcmp(v.data(), v1.data(), 8 * (size_t)S) == 0 && st == st1);
                for (size_t i = 0; i < all.size(); i++) CHECK(memcmp(&seen[i], &all[i], sizeof(KwsRefEvent)) == 0);
            }
    }
    CHECK(fired > 20 && held > 5);
}

// ---- the entries over the engine stand-ins ---------------------------------------------------------------------------------------------
void abi(const char* ctc_path, const char* transducer_path) {
    k2hip_model_t *m = nullptr, *m2 = nullptr, *tm = nullptr;
    OK(k2hip_model_create(ctc_path, nullptr, 0, &m));
    OK(k2hip_model_create(ctc_path, nullptr, 0, &m2));
    OK(k2hip_model_create(transducer_path, nullptr, 0, &tm));
    k2hip_model_info info, tinfo;
    OK(k2hip_model_get_info(m, &info));
    OK(k2hip_model_get_info(tm, &tinfo));
    const int V = info.vocab_size;
    const int64_t ids[] = {5, 6, 7, 5, 9, 9};
    const int32_t lens[] = {2, 1, 1, 2};   // [5 6] [7] [5] [9 9]: 6 states
    const std::vector<float> thr(4, 0.02f);
    const int64_t ids2[] = {11};
    const int32_t lens2[] = {1};
    k2hip_keywords_t *kw = nullptr, *kw2 = nullptr, *kw_bad = nullptr, *kw_t = nullptr;
    OK(k2hip_keywords_create(ids, lens, thr.data(), 4, V, &kw));
    OK(k2hip_keywords_create(ids2, lens2, thr.data(), 1, V, &kw2));
    OK(k2hip_keywords_create(ids2, lens2, thr.data(), 1, V + 1, &kw_bad));
    OK(k2hip_keywords_create(ids2, lens2, thr.data(), 1, tinfo.vocab_size, &kw_t));
    CHECK(k2hip_keywords_num_states(kw) == 6);
    k2hip_ctc_kws_stream_t *s[3] = {nullptr, nullptr, nullptr}, *other = nullptr;
    OK(k2hip_ctc_kws_stream_create(m, kw, &s[0]));
    OK(k2hip_ctc_kws_stream_create(m, kw, &s[1]));
    OK(k2hip_ctc_kws_stream_create(m, kw2, &s[2]));
    OK(k2hip_ctc_kws_stream_create(m2, kw, &other));
    k2hip_ctc_kws_stream_t* none = reinterpret_cast<k2hip_ctc_kws_stream_t*>(1);
    CHECK(k2hip_ctc_kws_stream_create(m, kw_bad, &none) == K2HIP_ERR_INVALID && none == nullptr && strstr(k2hip_last_error(), "vocab_size") != nullptr);
    none = reinterpret_cast<k2hip_ctc_kws_stream_t*>(1);
    CHECK(k2hip_ctc_kws_stream_create(tm, kw_t, &none) == K2HIP_ERR_UNSUPPORTED && none == nullptr && strstr(k2hip_last_error(), "CTC") != nullptr);
    CHECK(k2hip_ctc_kws_stream_create(nullptr, kw, &none) == K2HIP_ERR_INVALID && k2hip_ctc_kws_stream_create(m, nullptr, &none) == K2HIP_ERR_INVALID);
    CHECK(k2hip_ctc_kws_stream_create(m, kw, nullptr) == K2HIP_ERR_INVALID);
    OK(k2hip_keywords_destroy(kw_bad));
    OK(k2hip_keywords_destroy(kw));    // the streams keep their own reference
    OK(k2hip_keywords_destroy(kw2));
    const int B = 3, Tc = 16;
    std::vector<float> lp((size_t)B * Tc * V);
    for (int b = 0; b < B; b++)
        for (int t = 0; t < Tc; t++)
            for (int v = 0; v < V; v++) lp[((size_t)b * Tc + t) * V + v] = -0.25f * (float)(((unsigned)(t * 131 + v * 17) * 2654435761u >> 28) & 7);
    auto state = [&](k2hip_ctc_kws_stream_t* st, int S) {
        std::vector<float> a(2 * (size_t)S);
        std::vector<int32_t> b(2 * (size_t)S);
        OK(k2hip_debug_ctc_kws_stream_get_state(st, a.data(), b.data(), 2 * S));
        std::vector<unsigned char> out(16 * (size_t)S);
        memcpy(out.data(), a.data(), 8 * (size_t)S);
        memcpy(out.data() + 8 * (size_t)S, b.data(), 8 * (size_t)S);
        return out;
    };
    CHECK(k2hip_ctc_kws_stream_num_frames(s[0]) == 0 && k2hip_ctc_kws_stream_num_events(s[0]) == 0);
    OK(k2hip_ctc_kws_search_chunk(m, s, B, lp.data(), Tc, nullptr));
    CHECK(k2hip_ctc_kws_stream_num_frames(s[0]) == 16 && k2hip_ctc_kws_stream_num_frames(s[2]) == 16);
    CHECK(state(s[0], 6) == state(s[1], 6));   // one graph, one input: one result
    CHECK(k2hip_debug_ctc_kws_stream_get_state(s[0], nullptr, nullptr, 11) == K2HIP_ERR_CAPACITY);
    const int n0 = k2hip_ctc_kws_stream_num_events(s[0]);
    CHECK(n0 > 0 && n0 == k2hip_ctc_kws_stream_num_events(s[1]));
    {
        std::vector<int32_t> k((size_t)n0), b((size_t)n0), e((size_t)n0);
        std::vector<float> sum((size_t)n0), sc((size_t)n0);
        CHECK(k2hip_ctc_kws_stream_get_events(s[0], k.data(), b.data(), e.data(), sum.data(), sc.data(), n0) == n0);
        for (int i = 0; i < n0; i++) {
            CHECK(k[(size_t)i] >= 0 && k[(size_t)i] < 4 && b[(size_t)i] <= e[(size_t)i] && e[(size_t)i] < 16 && sum[(size_t)i] <= 0.f);
            CHECK(sc[(size_t)i] == sum[(size_t)i] / (float)lens[k[(size_t)i]]);
            if (i) CHECK(b[(size_t)i] > e[(size_t)i - 1]);   // no overlap
        }
        int32_t k1 = -7;
        CHECK(k2hip_ctc_kws_stream_get_events(s[0], &k1, nullptr, nullptr, nullptr, nullptr, 1) == n0 && k1 == k[0]);
        CHECK(k2hip_ctc_kws_stream_get_events(s[0], nullptr, nullptr, nullptr, nullptr, nullptr, 0) == n0);
        CHECK(k2hip_ctc_kws_stream_get_events(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0) == K2HIP_ERR_INVALID);
    }
    // every refused call changes no stream, and a valid call behind it still works
    auto snapshot = [&] {
        std::vector<unsigned char> all;
        const int sizes[3] = {6, 6, 2};
        for (int i = 0; i < 3; i++) {
            const auto x = state(s[i], sizes[i]);
            all.insert(all.end(), x.begin(), x.end());
            all.push_back((unsigned char)k2hip_ctc_kws_stream_num_events(s[i]));
        }
        return all;
    };
    const int32_t nf_none[3] = {0, 0, 0};
    auto before = snapshot();
    auto refused = [&](int32_t rc, int32_t code) {
        CHECK(rc == code);
        CHECK(snapshot() == before);
        OK(k2hip_ctc_kws_search_chunk(m, s, B, lp.data(), Tc, nf_none));   // a valid call that moves nothing
        CHECK(snapshot() == before);
    };
    refused(k2hip_ctc_kws_search_chunk(m, s, B, lp.data(), 0, nullptr), K2HIP_ERR_INVALID);
    refused(k2hip_ctc_kws_search_chunk(m, s, 0, lp.data(), Tc, nullptr), K2HIP_ERR_INVALID);
    refused(k2hip_ctc_kws_search_chunk(m, s, B, nullptr, Tc, nullptr), K2HIP_ERR_INVALID);
    refused(k2hip_ctc_kws_search_chunk(nullptr, s, B, lp.data(), Tc, nullptr), K2HIP_ERR_INVALID);
    refused(k2hip_ctc_kws_search_chunk(m, nullptr, B, lp.data(), Tc, nullptr), K2HIP_ERR_INVALID);
    const int32_t nf_big[3] = {16, 17, 16}, nf_neg[3] = {16, 16, -1};
    refused(k2hip_ctc_kws_search_chunk(m, s, B, lp.data(), Tc, nf_big), K2HIP_ERR_INVALID);
    refused(k2hip_ctc_kws_search_chunk(m, s, B, lp.data(), Tc, nf_neg), K2HIP_ERR_INVALID);
    k2hip_ctc_kws_stream_t* twice[3] = {s[0], s[2], s[0]};
    refused(k2hip_ctc_kws_search_chunk(m, twice, B, lp.data(), Tc, nullptr), K2HIP_ERR_INVALID);
    k2hip_ctc_kws_stream_t* hole[3] = {s[0], nullptr, s[2]};
    refused(k2hip_ctc_kws_search_chunk(m, hole, B, lp.data(), Tc, nullptr), K2HIP_ERR_INVALID);
    k2hip_ctc_kws_stream_t* foreign[3] = {s[0], other, s[2]};
    refused(k2hip_ctc_kws_search_chunk(m, foreign, B, lp.data(), Tc, nullptr), K2HIP_ERR_INVALID);
    refused(k2hip_ctc_kws_search_chunk(tm, s, B, lp.data(), Tc, nullptr), K2HIP_ERR_UNSUPPORTED);
    CHECK(k2hip_ctc_kws_stream_num_frames(other) == 0);
    // n_frames = 0 leaves a stream untouched; the others move on
    const auto before0 = state(s[0], 6);
    const int32_t nf[3] = {0, 7, 16};
    OK(k2hip_ctc_kws_search_chunk(m, s, B, lp.data(), Tc, nf));
    CHECK(state(s[0], 6) == before0 && k2hip_ctc_kws_stream_num_events(s[0]) == n0 && k2hip_ctc_kws_stream_num_frames(s[1]) == 23 &&
          k2hip_ctc_kws_stream_num_frames(s[2]) == 32);
    OK(k2hip_ctc_kws_stream_clear_events(s[1]));
    CHECK(k2hip_ctc_kws_stream_num_events(s[1]) == 0 && k2hip_ctc_kws_stream_num_frames(s[1]) == 23);
    OK(k2hip_ctc_kws_stream_reset(s[2]));
    CHECK(k2hip_ctc_kws_stream_num_frames(s[2]) == 0 && k2hip_ctc_kws_stream_num_events(s[2]) == 0);
    CHECK(k2hip_ctc_kws_stream_reset(nullptr) == K2HIP_ERR_INVALID && k2hip_ctc_kws_stream_clear_events(nullptr) == K2HIP_ERR_INVALID);
    CHECK(k2hip_ctc_kws_stream_num_frames(nullptr) == -1 && k2hip_ctc_kws_stream_num_events(nullptr) == -1);
    // chunking through the entry: 16 + 7 frames in one stream = the 23 frames of s[1], which saw the same rows
    OK(k2hip_ctc_kws_stream_reset(s[0]));
    const int32_t a16[1] = {16}, a7[1] = {7};
    OK(k2hip_ctc_kws_search_chunk(m, s, 1, lp.data(), Tc, a16));
    OK(k2hip_ctc_kws_search_chunk(m, s, 1, lp.data(), Tc, a7));
    CHECK(state(s[0], 6) == state(s[1], 6));
    // the host reference through the debug entry, NULL arguments and a bad table
    {
        const Trie g = make_trie({{1}, {1, 3}}, -1.f);
        std::vector<float> v(2 * (size_t)g.S());
        std::vector<int32_t> st(2 * (size_t)g.S());
        k2hip::ctc_kws_fresh_state(g.S(), v.data(), st.data());
        const float rows[10] = {-2.f, -0.25f, -8.f, -8.f, -8.f, -2.f, -8.f, -8.f, -0.25f, -8.f};
        int32_t ek[2], es[2], ee[2], n = -7;
        float em[2];
        OK(k2hip_debug_ctc_kws_ref_dp(g.parent.data(), g.tok.data(), g.depth.data(), g.kw.data(), g.bar.data(), g.rc.data(), g.S(), rows, 5, 2, v.data(),
                                      st.data(), ek, es, ee, em, 2, &n));
        CHECK(n == 1 && ek[0] == 0 && es[0] == 0 && ee[0] == 0 && em[0] == -0.25f && st[0] == 2 && st[(size_t)g.S()] == -1);   // the hold was released by frame 1
        CHECK(k2hip_debug_ctc_kws_ref_dp(g.parent.data(), g.tok.data(), g.depth.data(), g.kw.data(), g.bar.data(), g.rc.data(), g.S(), rows, 5, 2, v.data(),
                                         st.data(), ek, es, ee, em, 0, &n) == K2HIP_ERR_CAPACITY);   // frame 2 fires again
        CHECK(k2hip_debug_ctc_kws_ref_dp(g.parent.data(), nullptr, g.depth.data(), g.kw.data(), g.bar.data(), g.rc.data(), g.S(), rows, 5, 2, v.data(), st.data(),
                                         ek, es, ee, em, 2, &n) == K2HIP_ERR_INVALID);
        std::vector<int32_t> bad_tok = g.tok;
        bad_tok[1] = 5;
        CHECK(k2hip_debug_ctc_kws_ref_dp(g.parent.data(), bad_tok.data(), g.depth.data(), g.kw.data(), g.bar.data(), g.rc.data(), g.S(), rows, 5, 2, v.data(),
                                         st.data(), ek, es, ee, em, 2, &n) == K2HIP_ERR_INVALID);
    }
    // the fused entry
    OK(k2hip_keywords_create(ids, lens, thr.data(), 4, V, &kw));
    std::vector<float> wav(16000);
    for (size_t i = 0; i < wav.size(); i++) wav[i] = (float)((int)(i * 2654435761u % 2001) - 1000) / 1000.f;
    const float* ptr[2] = {wav.data(), wav.data()};
    const int64_t ns[2] = {16000, 12000};
    int32_t Tpo = -7, ne[2] = {-7, -7};
    const int me = 64;
    std::vector<int32_t> k((size_t)2 * me, -7), b0((size_t)2 * me, -7), e0((size_t)2 * me, -7);
    std::vector<float> sum((size_t)2 * me, -7.f), sc((size_t)2 * me, -7.f);
    OK(k2hip_offline_ctc_spot_keywords_from_samples(m, kw, ptr, ns, 2, k.data(), b0.data(), e0.data(), sum.data(), sc.data(), ne, me, &Tpo));
    CHECK(Tpo > 3 && ne[0] > 1 && ne[1] > 1 && e0[(size_t)ne[0] - 1] < Tpo && k[(size_t)ne[0]] == -7 && k[(size_t)me] >= 0);
    OK(k2hip_offline_ctc_spot_keywords_from_samples(m, kw, ptr, ns, 2, nullptr, nullptr, nullptr, nullptr, nullptr, ne, me, nullptr));
    std::fill(k.begin(), k.end(), -7);
    CHECK(k2hip_offline_ctc_spot_keywords_from_samples(m, kw, ptr, ns, 2, k.data(), b0.data(), e0.data(), sum.data(), sc.data(), ne, 1, &Tpo) ==
              K2HIP_ERR_CAPACITY && k[0] == -7 && strstr(k2hip_last_error(), "max_events") != nullptr);
    const int64_t ns_bad[2] = {16000, 10};
    CHECK(k2hip_offline_ctc_spot_keywords_from_samples(m, kw, ptr, ns_bad, 2, k.data(), b0.data(), e0.data(), sum.data(), sc.data(), ne, me, &Tpo) == K2HIP_ERR_INVALID);
    CHECK(k2hip_offline_ctc_spot_keywords_from_samples(m, nullptr, ptr, ns, 2, k.data(), b0.data(), e0.data(), sum.data(), sc.data(), ne, me, &Tpo) == K2HIP_ERR_INVALID);
    CHECK(k2hip_offline_ctc_spot_keywords_from_samples(m, kw, ptr, ns, 2, k.data(), b0.data(), e0.data(), sum.data(), sc.data(), nullptr, me, &Tpo) == K2HIP_ERR_INVALID);
    CHECK(k2hip_offline_ctc_spot_keywords_from_samples(tm, kw_t, ptr, ns, 2, k.data(), b0.data(), e0.data(), sum.data(), sc.data(), ne, me, &Tpo) == K2HIP_ERR_UNSUPPORTED);
    OK(k2hip_offline_ctc_spot_keywords_from_samples(m, kw, ptr, ns, 2, k.data(), b0.data(), e0.data(), sum.data(), sc.data(), ne, me, &Tpo));
    OK(k2hip_keywords_destroy(kw));
    OK(k2hip_keywords_destroy(kw_t));
    // one stream outlives its model: it holds host data only
    OK(k2hip_ctc_kws_stream_destroy(s[0]));
    OK(k2hip_ctc_kws_stream_destroy(s[2]));
    OK(k2hip_ctc_kws_stream_destroy(other));
    OK(k2hip_model_destroy(m));
    OK(k2hip_model_destroy(m2));
    OK(k2hip_model_destroy(tm));
    OK(k2hip_ctc_kws_stream_destroy(s[1]));
    OK(k2hip_ctc_kws_stream_destroy(nullptr));
}

}  // namespace

int main(int argc, char** argv) {
    reference();
    if (argc >= 3) abi(argv[1], argv[2]);
    else fprintf(stderr, "san_ctc_kws_driver: no model files given, the ABI part is skipped\n");
    printf("san_ctc_kws_driver ok\n");
    return 0;
}
