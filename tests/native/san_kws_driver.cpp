// AddressSanitizer / UBSan driver of the keyword spotter's host side: the graph builder (csrc/keywords.cpp), the header-only reference
// of the token passing (csrc/kws_ref.h) and the argument checks of the k2hip_keywords_* / k2hip_kws_* entries (csrc/api.cpp) over the
// CPU stand-ins of the engine (engine_stub*.cpp).  TEST INFRASTRUCTURE: its own program (`make -C k2transducerasr_amd/csrc san_kws`,
// tests/test_kws.py), never loaded into another process.
// Exercised: the trie, bar and every refusal with its message; kws_ref.h against the enumeration of every path on tiny tries with -inf
// cells, the tie rule, a == bar, the winner order, the reset, and any chunking against one call; then the streams' life cycle: a
// graph destroyed before its stream, a vocab mismatch, Tc = 0, n_frames out of range and 0, a stream twice in a call, NULL
// arguments, a CTC model, the fused entry and its capacity rule, and a valid call after every refused one.
//   san_kws_driver <offline.k2w> <ctc.k2w>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/k2hip.h"
#include "../../include/k2hip_debug.h"
#include "../../k2transducerasr_amd/csrc/keywords.h"
#include "../../k2transducerasr_amd/csrc/kws_ref.h"

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

const int64_t kIds[] = {23, 7, 35, 34, 33, 4, 33, 4, 35, 34, 29, 29, 35, 5, 6, 7, 23, 35, 35, 34, 33};
const int32_t kLens[] = {3, 3, 2, 2, 3, 3, 2, 1, 2};

bool refused(const int64_t* ids, const int32_t* lens, const float* thr, int n, int V, const char* word) {
    k2hip_keywords_t* kw = reinterpret_cast<k2hip_keywords_t*>(1);
    const int32_t rc = k2hip_keywords_create(ids, lens, thr, n, V, &kw);
    return rc == K2HIP_ERR_INVALID && kw == nullptr && strstr(k2hip_last_error(), word) != nullptr;
}

void graph() {
    std::vector<float> thr(9, 0.5f);
    thr[7] = 1.0f;
    k2hip_keywords_t* kw = nullptr;
    OK(k2hip_keywords_create(kIds, kLens, thr.data(), 9, 37, &kw));
    CHECK(k2hip_keywords_num_states(kw) == 18 && k2hip_keywords_num_keywords(kw) == 9);
    int32_t par[18], tok[18], dep[18], kwd[18];
    float bar[18];
    OK(k2hip_debug_keywords_get_tables(kw, par, tok, dep, kwd, bar, 18));
    CHECK(k2hip_debug_keywords_get_tables(kw, par, tok, dep, kwd, bar, 17) == K2HIP_ERR_CAPACITY);
    CHECK(par[0] == -1 && dep[0] == 0 && kwd[0] == -1);
    for (int s = 1; s < 18; s++) CHECK(par[s] >= 0 && par[s] < s && dep[s] == dep[par[s]] + 1);
    // [23,7,35] = states 1,2,3; [34,33,4] = 4,5,6; [33,4] = 7,8; [35,34] = 9,10; [29,29,35] = 11,12,13; [5,6,7] = 14,15,16; [23,35] = 17
    CHECK(tok[1] == 23 && tok[2] == 7 && tok[3] == 35 && kwd[3] == 0 && tok[17] == 35 && par[17] == 1 && kwd[17] == 6);
    CHECK(kwd[9] == 7 && kwd[10] == 3 && kwd[5] == 8 && kwd[6] == 1);   // [35] ends inside [35,34]; [34,33] inside [34,33,4]
    CHECK(bar[3] == 3.f * logf(0.5f) && bar[9] == 0.f && bar[1] == 0.f);
    OK(k2hip_keywords_destroy(kw));
    OK(k2hip_keywords_create(nullptr, nullptr, nullptr, 0, 37, &kw));   // zero keywords: one state
    CHECK(k2hip_keywords_num_states(kw) == 1 && k2hip_keywords_num_keywords(kw) == 0);
    OK(k2hip_keywords_destroy(kw));
    OK(k2hip_keywords_destroy(nullptr));
    const float t2[2] = {0.5f, 0.5f};
    {
        const int64_t ids[] = {5, 6, 7};
        const int32_t l0[] = {2, 0};
        CHECK(refused(ids, l0, t2, 2, 37, "keyword 1 is empty"));
        const int32_t l[] = {2, 1};
        const int64_t big[] = {5, 37, 7}, neg[] = {5, 6, -1}, bl[] = {5, 0, 7}, un[] = {5, 6, 2}, dup[] = {5, 5};
        CHECK(refused(big, l, t2, 2, 37, "keyword 0") && strstr(k2hip_last_error(), "37") != nullptr);
        CHECK(refused(neg, l, t2, 2, 37, "keyword 1"));
        CHECK(refused(bl, l, t2, 2, 37, "keyword 0 contains blank"));
        CHECK(refused(un, l, t2, 2, 37, "keyword 1 contains unk"));
        const int32_t l11[] = {1, 1};
        CHECK(refused(dup, l11, t2, 2, 37, "keyword 1 duplicates keyword 0"));
        for (float bad : {0.f, -0.5f, 1.5f, NAN, INFINITY}) {
            const float tb[2] = {0.5f, bad};
            CHECK(refused(ids, l, tb, 2, 37, "keyword 1: threshold"));
        }
        k2hip_keywords_t* ok = nullptr;   // id 1 is allowed; a keyword may be a proper prefix of another
        const int64_t pre[] = {1, 1, 1};
        const int32_t lpre[] = {1, 2};
        OK(k2hip_keywords_create(pre, lpre, t2, 2, 37, &ok));
        CHECK(k2hip_keywords_num_states(ok) == 3);
        OK(k2hip_keywords_destroy(ok));
    }
    {   // the state limit: chains of 4 tokens, every one a fresh branch
        std::vector<int64_t> ids;
        std::vector<int32_t> lens;
        std::vector<float> th;
        for (int p = 0; p < 300; p++) {
            for (int i = 0; i < 4; i++) ids.push_back(3 + (i == 0 ? p : (p + i) % 300));
            lens.push_back(4);
            th.push_back(0.5f);
        }
        k2hip_keywords_t* ok = nullptr;
        OK(k2hip_keywords_create(ids.data(), lens.data(), th.data(), 255, 400, &ok));
        CHECK(k2hip_keywords_num_states(ok) == 1021);
        OK(k2hip_keywords_destroy(ok));
        CHECK(refused(ids.data(), lens.data(), th.data(), 256, 400, "keyword 255: the trie outgrows 1024 states"));
    }
    CHECK(k2hip_keywords_create(kIds, kLens, thr.data(), 9, 37, nullptr) == K2HIP_ERR_INVALID);
    CHECK(k2hip_keywords_num_states(nullptr) == -1);
}

// ---- kws_ref.h against the enumeration of every path --------------------------------------------------------------------------------
struct Trie {
    std::vector<int32_t> parent, depth, kw;
    std::vector<float> bar;
    int S() const { return (int)parent.size(); }
};
struct Planes {
    int T, S;
    std::vector<float> stay, emit;
};
// the best path that enters c by its emit arc at frame e, every emit after frame R, with the frame of its first emit
void enter(const Trie& g, const Planes& p, int c, int e, int R, double* val, std::vector<int>* starts) {
    const double em = p.emit[(size_t)e * p.S + c];
    if (g.parent[(size_t)c] == 0) {
        *val = em;
        starts->assign(1, e);
        return;
    }
    const int q = g.parent[(size_t)c];
    *val = -INFINITY;
    starts->clear();
    for (int e2 = R + 1; e2 < e; e2++) {
        double v;
        std::vector<int> st;
        enter(g, p, q, e2, R, &v, &st);
        for (int f = e2 + 1; f < e; f++) v += p.stay[(size_t)f * p.S + q];
        v += em;
        if (v > *val) { *val = v; *starts = st; }
        else if (v == *val) starts->insert(starts->end(), st.begin(), st.end());
    }
}

void against_paths(const Trie& g, const Planes& p) {
    const int S = g.S();
    std::vector<float> a((size_t)S);
    std::vector<int32_t> start((size_t)S);
    k2hip::kws_fresh_state(S, a.data(), start.data());
    int R = -1;   // the frame of the last event
    for (int t = 0; t < p.T; t++) {
        std::vector<KwsRefEvent> ev;
        k2hip::kws_dp_ref(g.parent.data(), g.depth.data(), g.kw.data(), g.bar.data(), S, p.stay.data() + (size_t)t * S, p.emit.data() + (size_t)t * S, 1,
                          a.data(), start.data(), &ev);
        CHECK(start[0] == t + 1 && a[0] == 0.f && ev.size() <= 1);
        int win = -1;
        std::vector<double> best((size_t)S, -INFINITY);
        std::vector<std::vector<int>> bstart((size_t)S);
        for (int c = 1; c < S; c++) {
            bool by_emit = false;
            for (int e = R + 1; e <= t; e++) {
                double v;
                std::vector<int> st;
                enter(g, p, c, e, R, &v, &st);
                for (int f = e + 1; f <= t; f++) v += p.stay[(size_t)f * S + c];
                if (v > best[(size_t)c] || (v == best[(size_t)c] && e == t)) {
                    if (v > best[(size_t)c]) bstart[(size_t)c].clear();
                    best[(size_t)c] = v;
                    by_emit = e == t;
                }
                if (v == best[(size_t)c]) bstart[(size_t)c].insert(bstart[(size_t)c].end(), st.begin(), st.end());
            }
            if (g.kw[(size_t)c] >= 0 && by_emit && best[(size_t)c] >= (double)g.bar[(size_t)c]) {
                const bool better = win < 0 || g.depth[(size_t)c] > g.depth[(size_t)win] ||
                                    (g.depth[(size_t)c] == g.depth[(size_t)win] &&
                                     (best[(size_t)c] > best[(size_t)win] || (best[(size_t)c] == best[(size_t)win] && g.kw[(size_t)c] < g.kw[(size_t)win])));
                if (better) win = c;
            }
        }
        if (win >= 0) {
            CHECK(ev.size() == 1 && ev[0].keyword == g.kw[(size_t)win] && ev[0].end == t && (double)ev[0].sum_logp == best[(size_t)win]);
            bool found = false;
            for (int s0 : bstart[(size_t)win]) found |= s0 == ev[0].start;
            CHECK(found);
            for (int c = 1; c < S; c++) CHECK(a[(size_t)c] == -INFINITY && start[(size_t)c] == -1);
            R = t;
        } else {
            CHECK(ev.empty());
            for (int c = 1; c < S; c++) {   // multiples of 0.25: sums are exact in float32
                CHECK((double)a[(size_t)c] == best[(size_t)c]);
                if (best[(size_t)c] == -INFINITY) { CHECK(start[(size_t)c] == -1); continue; }
                bool found = false;
                for (int s0 : bstart[(size_t)c]) found |= s0 == start[(size_t)c];
                CHECK(found);
            }
        }
    }
}

Planes random_planes(int T, int S, int inf_per_16) {
    Planes p{T, S, std::vector<float>((size_t)T * S), std::vector<float>((size_t)T * S)};
    for (size_t i = 0; i < p.stay.size(); i++) {
        p.stay[i] = (int)(rnd() % 16) < inf_per_16 ? -INFINITY : -0.25f * (float)(rnd() % 12);
        p.emit[i] = (int)(rnd() % 16) < inf_per_16 ? -INFINITY : -0.25f * (float)(rnd() % 12);
    }
    return p;
}

void reference() {
    // tiny tries: a chain, a fork under the root, a terminal with a child, two keywords of one depth
    const std::vector<Trie> tries = {
        {{-1, 0, 1, 2}, {0, 1, 2, 3}, {-1, -1, -1, 0}, {0, 0, 0, -3.f}},
        {{-1, 0, 0, 1, 2}, {0, 1, 1, 2, 2}, {-1, -1, -1, 0, 1}, {0, 0, 0, -2.5f, -2.5f}},
        {{-1, 0, 1, 0, 3}, {0, 1, 2, 1, 2}, {-1, 0, 1, 2, -1}, {0, -1.f, -2.5f, -0.75f, 0}},
        {{-1, 0}, {0, 1}, {-1, 0}, {0, -0.5f}},
        {{-1}, {0}, {-1}, {0}},
    };
    for (const Trie& g : tries)
        for (int T = 1; T <= 6; T++)
            for (int inf : {0, 3, 8})
                for (int rep = 0; rep < 6; rep++) against_paths(g, random_planes(T, g.S(), inf));
    // chunking: any split gives the events and the carried block of one call, bit for bit
    for (const Trie& g : tries) {
        const int S = g.S(), T = 40;
        const Planes p = random_planes(T, S, 2);
        std::vector<float> a1((size_t)S), a2((size_t)S);
        std::vector<int32_t> s1((size_t)S), s2((size_t)S);
        std::vector<KwsRefEvent> e1, e2;
        k2hip::kws_fresh_state(S, a1.data(), s1.data());
        k2hip::kws_fresh_state(S, a2.data(), s2.data());
        k2hip::kws_dp_ref(g.parent.data(), g.depth.data(), g.kw.data(), g.bar.data(), S, p.stay.data(), p.emit.data(), T, a1.data(), s1.data(), &e1);
        for (int t = 0; t < T;) {
            const int n = std::min(T - t, 1 + (int)(rnd() % 7));
            k2hip::kws_dp_ref(g.parent.data(), g.depth.data(), g.kw.data(), g.bar.data(), S, p.stay.data() + (size_t)t * S,
                              p.emit.data() + (size_t)t * S, n, a2.data(), s2.data(), &e2);
            t += n;
        }
        CHECK(e1.size() == e2.size() && memcmp(a1.data(), a2.data(), sizeof(float) * (size_t)S) == 0 && s1 == s2);
        for (size_t i = 0; i < e1.size(); i++) CHECK(memcmp(&e1[i], &e2[i], sizeof(KwsRefEvent)) == 0);
    }
    {   // the tie: ve == vs exactly, emit wins and start moves to this frame; then a == bar exactly fires
        const Trie g = {{-1, 0, 1}, {0, 1, 2}, {-1, -1, 0}, {0, 0, -1.5f}};
        // frame 0: state 1 <- -0.5 (start 0); frame 1: state 1: ve = -0.75, vs = -0.5 - 0.25: tie, start 1; state 2 <- -0.5 - 1.0 = -1.5 = bar
        const float stay[6] = {0, 0, 0, 0, -0.25f, 0}, emit[6] = {0, -0.5f, -INFINITY, 0, -0.75f, -1.0f};
        float a[3];
        int32_t st[3];
        std::vector<KwsRefEvent> ev;
        k2hip::kws_fresh_state(3, a, st);
        k2hip::kws_dp_ref(g.parent.data(), g.depth.data(), g.kw.data(), g.bar.data(), 3, stay, emit, 1, a, st, &ev);
        CHECK(ev.empty() && a[1] == -0.5f && st[1] == 0 && a[2] == -INFINITY && st[2] == -1);
        k2hip::kws_dp_ref(g.parent.data(), g.depth.data(), g.kw.data(), g.bar.data(), 3, stay + 3, emit + 3, 1, a, st, &ev);
        CHECK(ev.size() == 1 && ev[0].keyword == 0 && ev[0].start == 0 && ev[0].end == 1 && ev[0].sum_logp == -1.5f);
        CHECK(a[1] == -INFINITY && st[1] == -1 && st[0] == 2);   // the reset took the tied token too
    }
}

// ---- the entries over the engine stand-ins ---------------------------------------------------------------------------------------------
void abi(const char* path, const char* ctc_path) {
    k2hip_model_t* m = nullptr;
    OK(k2hip_model_create(path, nullptr, 0, &m));
    k2hip_model_info info;
    OK(k2hip_model_get_info(m, &info));
    const int V = info.vocab_size, J = info.joiner_dim;
    std::vector<float> thr(9, 0.05f);
    k2hip_keywords_t *kw = nullptr, *kw2 = nullptr, *kw_bad = nullptr;
    OK(k2hip_keywords_create(kIds, kLens, thr.data(), 9, V, &kw));
    const int64_t ids2[] = {5, 9};
    const int32_t lens2[] = {1, 1};
    OK(k2hip_keywords_create(ids2, lens2, thr.data(), 2, V, &kw2));
    OK(k2hip_keywords_create(ids2, lens2, thr.data(), 2, V + 1, &kw_bad));
    k2hip_kws_stream_t* s[3] = {nullptr, nullptr, nullptr};
    OK(k2hip_kws_stream_create(m, kw, &s[0]));
    OK(k2hip_kws_stream_create(m, kw, &s[1]));   // shares the resident graph
    OK(k2hip_kws_stream_create(m, kw2, &s[2]));
    k2hip_kws_stream_t* none = reinterpret_cast<k2hip_kws_stream_t*>(1);
    CHECK(k2hip_kws_stream_create(m, kw_bad, &none) == K2HIP_ERR_INVALID && none == nullptr && strstr(k2hip_last_error(), "vocab_size") != nullptr);
    CHECK(k2hip_kws_stream_create(nullptr, kw, &none) == K2HIP_ERR_INVALID && k2hip_kws_stream_create(m, nullptr, &none) == K2HIP_ERR_INVALID);
    CHECK(k2hip_kws_stream_create(m, kw, nullptr) == K2HIP_ERR_INVALID);
    OK(k2hip_keywords_destroy(kw_bad));
    OK(k2hip_keywords_destroy(kw));    // the streams keep their own reference
    OK(k2hip_keywords_destroy(kw2));
    const int B = 3, Tc = 16;
    std::vector<float> enc((size_t)B * Tc * J, 0.25f);
    auto state = [&](k2hip_kws_stream_t* st, int S) {
        std::vector<float> a((size_t)S);
        std::vector<int32_t> b((size_t)S);
        OK(k2hip_debug_kws_stream_get_state(st, a.data(), b.data(), S));
        std::vector<unsigned char> out(8 * (size_t)S);
        memcpy(out.data(), a.data(), 4 * (size_t)S);
        memcpy(out.data() + 4 * (size_t)S, b.data(), 4 * (size_t)S);
        return out;
    };
    CHECK(k2hip_kws_stream_num_frames(s[0]) == 0 && k2hip_kws_stream_num_events(s[0]) == 0);
    OK(k2hip_kws_search_chunk(m, s, B, enc.data(), Tc, nullptr));
    CHECK(k2hip_kws_stream_num_frames(s[0]) == 16 && k2hip_kws_stream_num_frames(s[2]) == 16);
    CHECK(state(s[0], 18) == state(s[1], 18));   // one graph, one input: one result
    CHECK(k2hip_debug_kws_stream_get_state(s[0], nullptr, nullptr, 17) == K2HIP_ERR_CAPACITY);
    const int n0 = k2hip_kws_stream_num_events(s[0]);
    CHECK(n0 > 0 && n0 == k2hip_kws_stream_num_events(s[1]) && k2hip_kws_stream_num_events(s[2]) > 0);
    {
        std::vector<int32_t> k((size_t)n0), b((size_t)n0), e((size_t)n0);
        std::vector<float> sum((size_t)n0), sc((size_t)n0);
        CHECK(k2hip_kws_stream_get_events(s[0], k.data(), b.data(), e.data(), sum.data(), sc.data(), n0) == n0);
        for (int i = 0; i < n0; i++) {
            CHECK(k[(size_t)i] >= 0 && k[(size_t)i] < 9 && b[(size_t)i] <= e[(size_t)i] && e[(size_t)i] < 16 && sum[(size_t)i] <= 0.f);
            CHECK(sc[(size_t)i] == sum[(size_t)i] / (float)kLens[k[(size_t)i]]);
            if (i) CHECK(b[(size_t)i] > e[(size_t)i - 1]);   // no overlap
        }
        int32_t k1 = -7;
        CHECK(k2hip_kws_stream_get_events(s[0], &k1, nullptr, nullptr, nullptr, nullptr, 1) == n0 && k1 == k[0]);
        CHECK(k2hip_kws_stream_get_events(s[0], nullptr, nullptr, nullptr, nullptr, nullptr, 0) == n0);
        CHECK(k2hip_kws_stream_get_events(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0) == K2HIP_ERR_INVALID);
    }
    // refused calls change no stream
    const auto before0 = state(s[0], 18), before2 = state(s[2], 3);
    const int ev2 = k2hip_kws_stream_num_events(s[2]);
    auto unchanged = [&] {
        return state(s[0], 18) == before0 && state(s[2], 3) == before2 && k2hip_kws_stream_num_events(s[0]) == n0 && k2hip_kws_stream_num_events(s[2]) == ev2;
    };
    CHECK(k2hip_kws_search_chunk(m, s, B, enc.data(), 0, nullptr) == K2HIP_ERR_INVALID && unchanged());
    CHECK(k2hip_kws_search_chunk(m, s, 0, enc.data(), Tc, nullptr) == K2HIP_ERR_INVALID && unchanged());
    CHECK(k2hip_kws_search_chunk(m, s, B, nullptr, Tc, nullptr) == K2HIP_ERR_INVALID && unchanged());
    CHECK(k2hip_kws_search_chunk(nullptr, s, B, enc.data(), Tc, nullptr) == K2HIP_ERR_INVALID && unchanged());
    const int32_t nf_big[3] = {16, 17, 16}, nf_neg[3] = {16, 16, -1};
    CHECK(k2hip_kws_search_chunk(m, s, B, enc.data(), Tc, nf_big) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "stream 1") != nullptr && unchanged());
    CHECK(k2hip_kws_search_chunk(m, s, B, enc.data(), Tc, nf_neg) == K2HIP_ERR_INVALID && unchanged());
    k2hip_kws_stream_t* twice[3] = {s[0], s[2], s[0]};
    CHECK(k2hip_kws_search_chunk(m, twice, B, enc.data(), Tc, nullptr) == K2HIP_ERR_INVALID && unchanged());
    k2hip_kws_stream_t* hole[3] = {s[0], nullptr, s[2]};
    CHECK(k2hip_kws_search_chunk(m, hole, B, enc.data(), Tc, nullptr) == K2HIP_ERR_INVALID && unchanged());
    // n_frames = 0 leaves a stream untouched; the others move on
    const int32_t nf[3] = {0, 7, 16};
    OK(k2hip_kws_search_chunk(m, s, B, enc.data(), Tc, nf));
    CHECK(state(s[0], 18) == before0 && k2hip_kws_stream_num_events(s[0]) == n0 && k2hip_kws_stream_num_frames(s[1]) == 23 &&
          k2hip_kws_stream_num_frames(s[2]) == 32);
    OK(k2hip_kws_stream_clear_events(s[1]));
    CHECK(k2hip_kws_stream_num_events(s[1]) == 0 && k2hip_kws_stream_num_frames(s[1]) == 23);
    OK(k2hip_kws_stream_reset(s[2]));
    CHECK(k2hip_kws_stream_num_frames(s[2]) == 0 && k2hip_kws_stream_num_events(s[2]) == 0);
    CHECK(k2hip_kws_stream_reset(nullptr) == K2HIP_ERR_INVALID && k2hip_kws_stream_clear_events(nullptr) == K2HIP_ERR_INVALID);
    CHECK(k2hip_kws_stream_num_frames(nullptr) == -1 && k2hip_kws_stream_num_events(nullptr) == -1);
    // chunking through the entry: 16 + 7 frames in one stream = 23 frames of s[1], which saw the same cells
    OK(k2hip_kws_stream_reset(s[0]));
    const int32_t a16[1] = {16}, a7[1] = {7};
    OK(k2hip_kws_search_chunk(m, s, 1, enc.data(), Tc, a16));
    OK(k2hip_kws_search_chunk(m, s, 1, enc.data(), Tc, a7));
    CHECK(state(s[0], 18) == state(s[1], 18));
    // the fused entry
    OK(k2hip_keywords_create(kIds, kLens, thr.data(), 9, V, &kw));
    std::vector<float> wav(16000);
    for (size_t i = 0; i < wav.size(); i++) wav[i] = (float)((int)(i * 2654435761u % 2001) - 1000) / 1000.f;
    const float* ptr[2] = {wav.data(), wav.data()};
    const int64_t ns[2] = {16000, 12000};
    int32_t Tpo = -7, ne[2] = {-7, -7};
    const int me = 64;
    std::vector<int32_t> k((size_t)2 * me, -7), b0((size_t)2 * me, -7), e0((size_t)2 * me, -7);
    std::vector<float> sum((size_t)2 * me, -7.f), sc((size_t)2 * me, -7.f);
    OK(k2hip_offline_spot_keywords_from_samples(m, kw, ptr, ns, 2, k.data(), b0.data(), e0.data(), sum.data(), sc.data(), ne, me, &Tpo));
    CHECK(Tpo > 3 && ne[0] > 1 && ne[0] == ne[1] && e0[(size_t)ne[0] - 1] < Tpo && k[(size_t)ne[0]] == -7 && k[(size_t)me] >= 0);
    OK(k2hip_offline_spot_keywords_from_samples(m, kw, ptr, ns, 2, nullptr, nullptr, nullptr, nullptr, nullptr, ne, me, nullptr));
    std::fill(k.begin(), k.end(), -7);
    CHECK(k2hip_offline_spot_keywords_from_samples(m, kw, ptr, ns, 2, k.data(), b0.data(), e0.data(), sum.data(), sc.data(), ne, 1, &Tpo) == K2HIP_ERR_CAPACITY &&
          k[0] == -7 && strstr(k2hip_last_error(), "max_events") != nullptr);
    const int64_t ns_bad[2] = {16000, 10};
    CHECK(k2hip_offline_spot_keywords_from_samples(m, kw, ptr, ns_bad, 2, k.data(), b0.data(), e0.data(), sum.data(), sc.data(), ne, me, &Tpo) == K2HIP_ERR_INVALID);
    CHECK(k2hip_offline_spot_keywords_from_samples(m, nullptr, ptr, ns, 2, k.data(), b0.data(), e0.data(), sum.data(), sc.data(), ne, me, &Tpo) == K2HIP_ERR_INVALID);
    CHECK(k2hip_offline_spot_keywords_from_samples(m, kw, ptr, ns, 2, k.data(), b0.data(), e0.data(), sum.data(), sc.data(), nullptr, me, &Tpo) == K2HIP_ERR_INVALID);
    // a CTC model has no lattice
    k2hip_model_t* c = nullptr;
    OK(k2hip_model_create(ctc_path, nullptr, 0, &c));
    k2hip_model_info ci;
    OK(k2hip_model_get_info(c, &ci));
    k2hip_keywords_t* ckw = nullptr;
    OK(k2hip_keywords_create(ids2, lens2, thr.data(), 2, ci.vocab_size, &ckw));
    CHECK(k2hip_kws_stream_create(c, ckw, &none) == K2HIP_ERR_UNSUPPORTED && none == nullptr && strstr(k2hip_last_error(), "CTC") != nullptr);
    CHECK(k2hip_kws_search_chunk(c, s, 1, enc.data(), 1, nullptr) == K2HIP_ERR_UNSUPPORTED);
    CHECK(k2hip_offline_spot_keywords_from_samples(c, ckw, ptr, ns, 2, k.data(), b0.data(), e0.data(), sum.data(), sc.data(), ne, me, &Tpo) == K2HIP_ERR_UNSUPPORTED);
    CHECK(k2hip_kws_search_chunk(m, s, 1, enc.data(), 1, nullptr) == K2HIP_OK);   // the transducer model's streams still work
    OK(k2hip_keywords_destroy(ckw));
    OK(k2hip_model_destroy(c));
    OK(k2hip_keywords_destroy(kw));
    // one stream outlives the model: it lets go of its graph without touching the model
    OK(k2hip_kws_stream_destroy(s[0]));
    OK(k2hip_kws_stream_destroy(s[2]));
    OK(k2hip_model_destroy(m));
    OK(k2hip_kws_stream_destroy(s[1]));
    OK(k2hip_kws_stream_destroy(nullptr));
}

}  // namespace

int main(int argc, char** argv) {
    graph();
    reference();
    if (argc >= 3) abi(argv[1], argv[2]);
    else fprintf(stderr, "san_kws_driver: no model files given, the ABI part is skipped\n");
    printf("san_kws_driver ok\n");
    return 0;
}
