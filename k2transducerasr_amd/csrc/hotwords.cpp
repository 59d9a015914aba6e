// Hotword graph (hotwords.h): trie + Aho-Corasick failure links, the host walk and the dense device form.
#include <algorithm>
#include <cmath>

#include "errors.h"
#include "hotwords.h"

namespace k2hip {

int HotwordGraph::child(int s, int v) const {
    const auto& k = kids_[(size_t)s];
    auto it = std::lower_bound(k.begin(), k.end(), std::make_pair(v, -1));
    return it != k.end() && it->first == v ? it->second : -1;
}

HotwordGraph::HotwordGraph(const int64_t* ids, const int32_t* lens, int n_phrases, float score_per_token, int vocab_size, const char* noun,
                           const int* numbers)
    : V_(vocab_size), c_(score_per_token) {
    K2_REQUIRE(n_phrases >= 0, "hotwords: %d phrases", n_phrases);
    K2_REQUIRE(vocab_size > K2HIP_UNK_ID, "hotwords: vocab_size %d", vocab_size);
    K2_REQUIRE(std::isfinite(score_per_token) && score_per_token >= 0.f, "hotwords: score_per_token %g must be finite and >= 0", (double)score_per_token);
    K2_REQUIRE(n_phrases == 0 || (ids && lens), "hotwords: null phrase arrays");
    depth_.push_back(0);
    fail_.push_back(0);
    end_.push_back(0);
    kids_.emplace_back();
    std::vector<int> owner{-1};   // the first phrase that created the node (for the messages)
    int64_t off = 0;
    for (int p = 0; p < n_phrases; p++) {
        const int num = numbers ? numbers[p] : p;
        K2_REQUIRE(lens[p] > 0, "hotwords: %s %d is empty", noun, num);
        int s = 0;
        for (int i = 0; i < lens[p]; i++) {
            const int64_t v = ids[off + i];
            K2_REQUIRE(v >= 0 && v < V_, "hotwords: %s %d: token id %lld outside [0, %d)", noun, num, (long long)v, V_);
            K2_REQUIRE(v != K2HIP_BLANK_ID && v != K2HIP_UNK_ID, "hotwords: %s %d contains %s (id %lld)", noun, num,
                       v == K2HIP_BLANK_ID ? "blank" : "unk", (long long)v);
            K2_REQUIRE(!end_[(size_t)s], "hotwords: %s %d is a proper prefix of %s %d", noun, owner[(size_t)s], noun, num);
            int n = child(s, (int)v);
            if (n < 0) {
                n = (int)depth_.size();
                if ((int64_t)(n + 1) * V_ > kHotwordMaxEntries)
                    failf(K2HIP_ERR_INVALID, "hotwords: %s %d: the graph outgrows %lld table entries (states x vocab_size %d)", noun, num,
                          (long long)kHotwordMaxEntries, V_);
                depth_.push_back(depth_[(size_t)s] + 1);
                fail_.push_back(0);
                end_.push_back(0);
                kids_.emplace_back();
                owner.push_back(num);
                auto& k = kids_[(size_t)s];
                k.insert(std::lower_bound(k.begin(), k.end(), std::make_pair((int)v, -1)), std::make_pair((int)v, n));
            }
            s = n;
        }
        K2_REQUIRE(!end_[(size_t)s], "hotwords: %s %d duplicates %s %d", noun, num, noun, owner[(size_t)s]);
        K2_REQUIRE(kids_[(size_t)s].empty(), "hotwords: %s %d is a proper prefix of %s %d", noun, num, noun, owner[(size_t)kids_[(size_t)s][0].second]);
        end_[(size_t)s] = 1;
        owner[(size_t)s] = num;
        off += lens[p];
    }
    // failure links, breadth first (states were not created in that order: walk the trie by level)
    std::vector<int> q;
    for (auto& kv : kids_[0]) q.push_back(kv.second);
    for (size_t h = 0; h < q.size(); h++) {
        const int s = q[h];
        for (auto& kv : kids_[(size_t)s]) {
            int f = fail_[(size_t)s];
            int n = child(f, kv.first);
            while (n < 0 && f != 0) {
                f = fail_[(size_t)f];
                n = child(f, kv.first);
            }
            fail_[(size_t)kv.second] = n < 0 ? 0 : n;
            q.push_back(kv.second);
        }
    }
}

int HotwordGraph::delta(int s, int v) const {
    for (;;) {
        const int n = child(s, v);
        if (n >= 0) return n;
        if (s == 0) return 0;
        s = fail_[(size_t)s];
    }
}

void HotwordGraph::step(int state, int64_t token, int* next_state, float* bonus) const {
    K2_REQUIRE(state >= 0 && state < num_states(), "hotwords: state %d outside [0, %d)", state, num_states());
    K2_REQUIRE(token >= 0 && token < V_, "hotwords: token id %lld outside [0, %d)", (long long)token, V_);
    if (token == K2HIP_BLANK_ID || token == K2HIP_UNK_ID) {
        *next_state = state;
        *bonus = 0.f;
        return;
    }
    const int n = delta(state, (int)token);
    *bonus = pending(n) - pending(state);
    *next_state = end_[(size_t)n] ? 0 : n;
}

void HotwordGraph::dense(std::vector<int32_t>* next, std::vector<float>* bonus, std::vector<float>* pend) const {
    const int S = num_states();
    next->assign((size_t)S * V_, 0);
    bonus->assign((size_t)S * V_, 0.f);
    pend->resize((size_t)S);
    for (int s = 0; s < S; s++) {
        (*pend)[(size_t)s] = pending(s);
        for (int v = 0; v < V_; v++) step(s, v, &(*next)[(size_t)s * V_ + v], &(*bonus)[(size_t)s * V_ + v]);
    }
}

}  // namespace k2hip
