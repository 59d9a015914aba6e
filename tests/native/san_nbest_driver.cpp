// BeamHistory's N-best and token log-probs on the CPU under ASan / UBSan -- TEST INFRASTRUCTURE (csrc/beam_hist.h is plain C++).
// Synthetic out blocks (kernels.h BeamResumeLayout, with the token log-prob side block) are applied chunk by chunk; after every chunk
// nbest() and the materialised best result are compared with a straightforward whole-sequence model kept here: every hypothesis as
// plain vectors, ordered by (lp - pending(state)) / (length + 2) descending with ties in insertion order.  The script has a merge
// survivor (two hypotheses, one extending the other), a prefix that is pruned and spelled again later with other timestamps and
// log-probs, a hotword pending table that reorders the list, and a reset in the middle.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../k2transducerasr_amd/csrc/beam_hist.h"

using namespace k2hip;

namespace {
struct MHyp {
    std::vector<int> tok, ts;
    std::vector<float> yp;
    float lp = 0.f;
    int st = 0;
};
struct New {   // one survivor of a chunk: saved hypothesis `org` + suffix
    int org;
    std::vector<int> tok, ts;   // ts chunk-relative
    std::vector<float> yp;
    float lp;
    int st;
};
int fails = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            fails++;                                                      \
        }                                                                 \
    } while (0)

void apply(BeamHistory& h, std::vector<MHyp>& model, long long& frames, int K, int Tp, const std::vector<New>& nx, const std::vector<float>* pending,
           bool with_yp) {
    const int o_org = 2, o_n = 2 + K, o_lp = 2 + 2 * K, o_ctx = 2 + 3 * K, o_ys = 2 + 5 * K, o_ts = 2 + 5 * K + K * Tp;
    std::vector<int> out((size_t)(2 + 5 * K + 2 * K * Tp), 0), st((size_t)K, 0);
    std::vector<float> yp((size_t)K * Tp, -77.f);
    std::vector<MHyp> nm;
    for (size_t k = 0; k < nx.size(); k++) {
        const New& n = nx[k];
        MHyp m = model[(size_t)n.org];
        out[(size_t)o_org + k] = n.org;
        out[(size_t)o_n + k] = (int)n.tok.size();
        memcpy(&out[(size_t)o_lp + k], &n.lp, sizeof(float));
        for (size_t i = 0; i < n.tok.size(); i++) {
            out[(size_t)o_ys + k * Tp + i] = n.tok[i];
            out[(size_t)o_ts + k * Tp + i] = n.ts[i];
            yp[k * Tp + i] = n.yp[i];
            m.tok.push_back(n.tok[i]);
            m.ts.push_back((int)frames + n.ts[i]);
            m.yp.push_back(with_yp ? n.yp[i] : 0.f);
        }
        m.lp = n.lp;
        m.st = n.st;
        st[k] = n.st;
        const int L = (int)m.tok.size();
        out[(size_t)o_ctx + 2 * k] = L >= 2 ? m.tok[(size_t)L - 2] : 0;
        out[(size_t)o_ctx + 2 * k + 1] = L >= 1 ? m.tok[(size_t)L - 1] : 0;
        nm.push_back(m);
    }
    // the pick the device makes: first maximum of the normalised finalized log-prob
    auto fin = [&](const MHyp& m) { return pending ? m.lp - (*pending)[(size_t)m.st] : m.lp; };
    int best = 0;
    for (size_t k = 1; k < nm.size(); k++)
        if (fin(nm[k]) / (float)(nm[k].tok.size() + 2) > fin(nm[(size_t)best]) / (float)(nm[(size_t)best].tok.size() + 2)) best = (int)k;
    out[0] = (int)nx.size();
    out[1] = best;
    h.apply_out_states(out.data(), Tp, st.data(), with_yp ? yp.data() : nullptr);
    model.swap(nm);
    frames += Tp;
    // ---- compare
    for (int n = 1; n <= K + 1; n++) {
        std::vector<BeamAlt> got = h.nbest(n);
        std::vector<int> order;
        for (size_t k = 0; k < model.size(); k++) order.push_back((int)k);
        for (size_t i = 0; i < order.size(); i++)   // stable insertion sort, descending
            for (size_t j = i; j > 0; j--) {
                const MHyp &a = model[(size_t)order[j - 1]], &b = model[(size_t)order[j]];
                if (fin(b) / (float)(b.tok.size() + 2) > fin(a) / (float)(a.tok.size() + 2)) std::swap(order[j - 1], order[j]);
                else break;
            }
        CHECK(got.size() == std::min((size_t)n, model.size()));
        for (size_t i = 0; i < got.size(); i++) {
            const MHyp& m = model[(size_t)order[i]];
            CHECK(got[i].tokens.size() == m.tok.size() && got[i].timestamps.size() == m.tok.size() && got[i].token_log_probs.size() == m.tok.size());
            for (size_t j = 0; j < m.tok.size() && j < got[i].tokens.size(); j++) {
                CHECK(got[i].tokens[j] == m.tok[j]);
                CHECK(got[i].timestamps[j] == m.ts[j]);
                CHECK(got[i].token_log_probs[j] == m.yp[j]);
            }
            CHECK(got[i].score == fin(m));
        }
        if (!got.empty()) {   // entry 0 is the materialised best result
            CHECK(got[0].score == h.score());
            CHECK(h.tokens().size() == got[0].tokens.size() + 2 && h.timestamps().size() == got[0].tokens.size());
            CHECK(h.token_log_probs().size() == got[0].tokens.size());
            for (size_t j = 0; j < got[0].tokens.size() && j + 2 < h.tokens().size(); j++) {
                CHECK(h.tokens()[j + 2] == got[0].tokens[j]);
                CHECK(h.timestamps()[j] == got[0].timestamps[j]);
                CHECK(h.token_log_probs()[j] == got[0].token_log_probs[j]);
            }
        }
    }
}
void start_state(const BeamHistory& h) {
    std::vector<BeamAlt> a = h.nbest(8);
    CHECK(a.size() == 1 && a[0].tokens.empty() && a[0].timestamps.empty() && a[0].token_log_probs.empty() && a[0].score == 0.f);
    CHECK(h.token_log_probs().empty() && h.nbest(0).empty());
}
}  // namespace

int main() {
    const int K = 4;
    for (int pass = 0; pass < 3; pass++) {   // 0: plain; 1: with a pending table; 2: chunks applied without the yp block
        BeamHistory h(K, 0);
        auto pending = std::make_shared<std::vector<float>>(std::vector<float>{0.f, 1.5f, 3.0f});
        if (pass == 1) h.set_pending(pending);
        const std::vector<float>* pd = pass == 1 ? pending.get() : nullptr;
        const bool yp = pass != 2;
        std::vector<MHyp> model(1);
        long long frames = 0;
        start_state(h);
        for (int round = 0; round < 2; round++) {
            // chunk 1 (3 frames): [] , [5] , [5 6] (extends [5]) , [7]
            apply(h, model, frames, K, 3, {{0, {}, {}, {}, -0.5f, 0}, {0, {5}, {0}, {-0.25f}, -1.0f, 1}, {0, {5, 6}, {0, 2}, {-0.25f, -0.75f}, -1.5f, 2},
                                          {0, {7}, {1}, {-2.f}, -2.5f, 0}}, pd, yp);
            // chunk 2 (1 frame): [5] is pruned; [5 6] stays, [] -> [8], [7] stays; equal normalised scores of [8] and [7] (a tie: insertion order)
            apply(h, model, frames, K, 1, {{2, {}, {}, {}, -1.75f, 2}, {0, {8}, {0}, {-0.125f}, -3.0f, 0}, {3, {}, {}, {}, -3.0f, 0}}, pd, yp);
            // chunk 3 (2 frames): [5] spelled again from... nothing carries it, so it comes back through [8]'s sibling: [7] -> [7 5],
            // and the prefix [5 6] is extended on both frames; [8] survives unchanged
            apply(h, model, frames, K, 2, {{0, {9, 9}, {0, 1}, {-0.5f, -0.0625f}, -2.0f, 0}, {2, {5}, {1}, {-1.25f}, -3.5f, 1}, {1, {}, {}, {}, -3.25f, 0},
                                          {0, {9}, {1}, {-0.375f}, -2.25f, 2}}, pd, yp);
            // chunk 4 (1 frame): one survivor
            apply(h, model, frames, K, 1, {{3, {4}, {0}, {-0.03125f}, -2.5f, 0}}, pd, yp);
            // the graph may change between steps: the scores follow the table attached when they are read
            if (pass == 1) {
                auto other = std::make_shared<std::vector<float>>(std::vector<float>{0.f, 0.25f, 0.5f});
                h.set_pending(other);
                CHECK(h.nbest(1)[0].score == model[0].lp - (*other)[(size_t)model[0].st]);
                h.set_pending(pending);
            }
            h.reset();
            model.assign(1, MHyp{});
            frames = 0;
            start_state(h);
        }
        CHECK(h.seq_tree().live() == 1);
    }
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("san_nbest_driver: ok\n");
    return 0;
}
