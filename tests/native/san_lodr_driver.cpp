// The host side of LODR on the CPU under ASan / UBSan -- TEST INFRASTRUCTURE (csrc/beam_hist.h, csrc/lodr_host.h and csrc/ngram_lm.cpp
// are plain C++).
//   1. BeamHistory with LODR states: begin_lodr / fill_lodr_states / apply_out_states over synthetic out blocks (kernels.h
//      BeamResumeLayout) chunk by chunk, beside n-gram LM states of another automaton (two distinct carried planes that must not swap),
//      dead slots, a chunk without the LODR plane, reset, and the setting-change rule the streaming entries apply: a stream that has
//      searched frames is refused under another serial, a fresh or reset one takes the new setting and the new start state.
//   2. The host rescoring walk (LodrHost): every step over the scaled tables against NgramLm::step times the scale on random LMs and
//      random token strings (weights that are powers of two scale exactly, so the comparison is bit for bit), blank / unk / out-of-range
//      tokens, bad states, and total() against the float32 running sum.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../k2transducerasr_amd/csrc/beam_hist.h"
#include "../../k2transducerasr_amd/csrc/lodr_host.h"

using namespace k2hip;

namespace {
int fails = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            fails++;                                                      \
        }                                                                 \
    } while (0)

struct Surv {
    int org;
    std::vector<int> tok;
    float lp;
    int st, lst, dst;
};
// one chunk of Tp frames: the out block and the side planes [graph | LM | LODR], as the device writes them
void apply(BeamHistory& h, int K, int Tp, const std::vector<Surv>& nx, bool with_lm, bool with_lodr) {
    const int o_org = 2, o_n = 2 + K, o_lp = 2 + 2 * K, o_ys = 2 + 5 * K, o_ts = 2 + 5 * K + K * Tp;
    std::vector<int> out((size_t)(2 + 5 * K + 2 * K * Tp), 0), st((size_t)K, 0), lst((size_t)K, 0), dst((size_t)K, 0);
    out[0] = (int)nx.size();
    out[1] = 0;
    for (size_t k = 0; k < nx.size(); k++) {
        out[(size_t)o_org + k] = nx[k].org;
        out[(size_t)o_n + k] = (int)nx[k].tok.size();
        memcpy(&out[(size_t)o_lp + k], &nx[k].lp, sizeof(float));
        for (size_t i = 0; i < nx[k].tok.size(); i++) {
            out[(size_t)o_ys + k * Tp + i] = nx[k].tok[i];
            out[(size_t)o_ts + k * Tp + i] = (int)i;
        }
        st[k] = nx[k].st;
        lst[k] = nx[k].lst;
        dst[k] = nx[k].dst;
    }
    h.apply_out_states(out.data(), Tp, st.data(), nullptr, with_lm ? lst.data() : nullptr, with_lodr ? dst.data() : nullptr);
}
// the rule of k2hip_beam_search_chunk / k2hip_online_step: may this stream search a chunk under setting `serial`?
bool accepts(const BeamHistory& h, uint64_t serial) { return h.frames() == 0 || h.lodr_serial() == serial; }

void history() {
    const int K = 4, Tp = 3;
    BeamHistory h(K, 0);
    std::vector<int> in((size_t)K, -1);
    CHECK(h.lodr_serial() == 0 && accepts(h, 7) && accepts(h, 0));
    h.begin_lm(11, 5);
    h.begin_lodr(7, 3);
    CHECK(h.lodr_serial() == 7 && h.lm_serial() == 11);
    h.fill_lodr_states(in.data());
    CHECK(in[0] == 3 && in[1] == 0 && in[2] == 0 && in[3] == 0);   // the start hypothesis, then dead slots
    h.fill_lm_states(in.data());
    CHECK(in[0] == 5 && in[1] == 0);
    apply(h, K, Tp, {{0, {4, 5}, -1.f, 0, 21, 9}, {0, {4}, -2.f, 0, 22, 8}, {0, {}, -3.f, 0, 5, 3}}, true, true);
    CHECK(h.frames() == Tp && h.hyps().size() == 3);
    h.fill_lodr_states(in.data());
    CHECK(in[0] == 9 && in[1] == 8 && in[2] == 3 && in[3] == 0);
    h.fill_lm_states(in.data());
    CHECK(in[0] == 21 && in[1] == 22 && in[2] == 5 && in[3] == 0);   // the two planes stay apart
    // the setting changed or was cleared: refused while the stream carries states of the old one; the old one still passes
    CHECK(!accepts(h, 8) && !accepts(h, 0) && accepts(h, 7));
    // a second chunk: survivors continue saved hypotheses 1 and 2, one slot fewer
    apply(h, K, Tp, {{1, {6}, -2.5f, 0, 30, 12}, {2, {7, 8, 9}, -3.5f, 0, 31, 13}}, true, true);
    h.fill_lodr_states(in.data());
    CHECK(in[0] == 12 && in[1] == 13 && in[2] == 0 && in[3] == 0);
    CHECK(h.tokens().size() == 2 + 2 && h.tokens()[2] == 4 && h.tokens()[3] == 6);
    // a chunk applied without the LODR plane leaves no stale state behind
    apply(h, K, Tp, {{0, {}, -2.6f, 0, 30, 0}}, true, false);
    h.fill_lodr_states(in.data());
    CHECK(in[0] == 0);
    // reset: the hypotheses are back at the start; the next first chunk notes the setting then set and its start state
    h.reset();
    CHECK(h.frames() == 0 && accepts(h, 8) && accepts(h, 0));
    h.begin_lodr(8, 6);
    h.fill_lodr_states(in.data());
    CHECK(in[0] == 6 && in[1] == 0 && h.lodr_serial() == 8);
    h.reset();
    h.begin_lodr(0, 0);   // cleared (or no active fusion): state 0, serial 0
    h.fill_lodr_states(in.data());
    CHECK(in[0] == 0 && h.lodr_serial() == 0);
    apply(h, K, Tp, {{0, {4}, -1.f, 0, 0, 0}}, false, false);
    CHECK(!accepts(h, 8) && accepts(h, 0));
    // beam 1 and the widest beam
    for (int k : {1, 8}) {
        BeamHistory g(k, 0);
        std::vector<int> s((size_t)k, -1);
        g.begin_lodr(3, 2);
        g.fill_lodr_states(s.data());
        CHECK(s[0] == 2 && s[(size_t)k - 1] == (k == 1 ? 2 : 0));
        std::vector<Surv> nx;
        for (int j = 0; j < k; j++) nx.push_back({0, {j + 3}, -1.f - j, 0, 0, 40 + j});
        apply(g, k, 2, nx, false, true);
        g.fill_lodr_states(s.data());
        for (int j = 0; j < k; j++) CHECK(s[(size_t)j] == 40 + j);
    }
}

// a random back-off LM of `order` over V tokens (2 = unk, 0 = blank): every history has its own entry
NgramLm* random_lm(std::mt19937& rng, int V, int order, int n_high) {
    std::vector<std::vector<int64_t>> ids;
    std::vector<float> lp, bo;
    auto u = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    auto add = [&](std::vector<int64_t> g, float l, float b) {
        for (auto& e : ids)
            if (e == g) return;
        ids.push_back(g);
        lp.push_back(l);
        bo.push_back(b);
    };
    add({kNgramBos}, -99.f, u(-1.f, -0.05f));
    add({kNgramUnk}, -7.5f, 0.f);
    for (int v = 1; v < V; v++)
        if (v != 2 && v % 7 != 3) add({v}, u(-6.f, -3.f), u(-1.f, -0.05f));   // (some tokens have no unigram: the <unk> rule)
    for (int i = 0; i < n_high; i++) {
        const int n = 2 + (int)(rng() % (unsigned)(order - 1));
        std::vector<int64_t> g;
        bool ok = true;
        for (int j = 0; j < n; j++) {
            const int v = (j == 0 && rng() % 5 == 0) ? (int)kNgramBos : 1 + (int)(rng() % (unsigned)(V - 1));
            ok = ok && (v < 0 || (v != 2 && v % 7 != 3));
            g.push_back(v);
        }
        if (!ok) continue;
        for (int m = 2; m <= n; m++) add(std::vector<int64_t>(g.begin(), g.begin() + m), u(-1.5f, -0.1f), m < order ? u(-1.f, -0.05f) : 0.f);
    }
    std::vector<int64_t> flat;
    std::vector<int32_t> orders;
    for (auto& e : ids) {
        flat.insert(flat.end(), e.begin(), e.end());
        orders.push_back((int32_t)e.size());
    }
    return new NgramLm(flat.data(), orders.data(), lp.data(), bo.data(), (int64_t)ids.size(), V);
}

void walk() {
    std::mt19937 rng(20261021);
    long long steps = 0, backed = 0;
    for (int rep = 0; rep < 24; rep++) {
        const int V = 9 + (int)(rng() % 60u), order = 2 + rep % 3;
        std::unique_ptr<NgramLm> lm(random_lm(rng, V, order, 10 + (int)(rng() % 80u)));
        const float scales[] = {-0.25f, -0.5f, -1.f, -2.f};
        const float scale = scales[rep % 4];
        LodrHost h;
        lm->device_form(scale, &h.d);
        h.start = lm->start_state();
        h.V = V;
        CHECK(h.num_states() == lm->num_states());
        for (int seq = 0; seq < 40; seq++) {
            const int n = (int)(rng() % 12u);
            std::vector<int64_t> toks;
            for (int i = 0; i < n; i++) toks.push_back((int64_t)(rng() % (unsigned)V));   // (blank and unk among them)
            int s = h.start, s0 = lm->start_state();
            volatile float acc = 0.f;
            for (int i = 0; i < n; i++) {
                int nx = -1, nx0 = -1;
                float term = NAN, lp0 = 0.f;
                h.step(s, toks[(size_t)i], &nx, &term);
                if (toks[(size_t)i] == K2HIP_BLANK_ID || toks[(size_t)i] == K2HIP_UNK_ID) {
                    CHECK(nx == s && term == 0.f);
                } else {
                    lm->step(s0, toks[(size_t)i], &nx0, &lp0);
                    // a direct hit is ONE scaled weight: bit for bit whatever the scale; a backed-off step sums scaled weights, which a
                    // power-of-two scale keeps bit-equal to the scaled sum
                    const float want = lp0 * scale;
                    CHECK(memcmp(&want, &term, sizeof(float)) == 0);
                    CHECK(nx == nx0);
                    s0 = nx0;
                    backed += nx0 == 0;
                }
                s = nx;
                acc = acc + term;
                steps++;
            }
            const float tot = h.total(toks.data(), toks.size()), want = acc;
            CHECK(memcmp(&tot, &want, sizeof(float)) == 0);
        }
        CHECK(h.total(nullptr, 0) == 0.f);
        // tokens outside the vocabulary and states outside the automaton earn nothing and change nothing
        int nx = -5;
        float term = NAN;
        h.step(h.start, V, &nx, &term);
        CHECK(nx == h.start && term == 0.f);
        h.step(h.start, -1, &nx, &term);
        CHECK(nx == h.start && term == 0.f);
        h.step(h.num_states(), 1, &nx, &term);
        CHECK(nx == h.num_states() && term == 0.f);
        h.step(-1, 1, &nx, &term);
        CHECK(nx == -1 && term == 0.f);
    }
    CHECK(steps > 1000 && backed > 100);
    // a hand case: unigrams at -4, the bigram (6, 7) at -1 with bow(6) = -0.5, weight -0.5
    {
        const int64_t ids[] = {1, 3, 4, 5, 6, 7, 6, 7};
        const int32_t orders[] = {1, 1, 1, 1, 1, 1, 2};
        const float lp[] = {-4, -4, -4, -4, -4, -4, -1}, bo[] = {0, 0, 0, 0, -0.5f, 0, 0};
        NgramLm lm(ids, orders, lp, bo, 7, 8);
        LodrHost h;
        lm.device_form(-0.5f, &h.d);
        h.start = lm.start_state();
        h.V = 8;
        const int64_t a[] = {6, 7}, b[] = {5, 7}, c[] = {6, 0, 2, 7}, d[] = {6, 5};
        CHECK(h.total(a, 2) == 2.5f && h.total(b, 2) == 4.f && h.total(c, 4) == 2.5f);   // (blank and unk keep the state)
        CHECK(h.total(d, 2) == 2.f + 0.25f + 2.f);                                        // (the back-off weight first, then the unigram)
    }
}
}  // namespace

int main() {
    history();
    walk();
    if (fails) {
        fprintf(stderr, "san_lodr_driver: %d checks failed\n", fails);
        return 1;
    }
    printf("san_lodr_driver ok\n");
    return 0;
}
