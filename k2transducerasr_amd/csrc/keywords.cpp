// Keyword graph (keywords.h): the trie, bar and the sorted child lists.
#include <algorithm>
#include <cmath>
#include <map>

#include "errors.h"
#include "keywords.h"

namespace k2hip {

KeywordGraph::KeywordGraph(const int64_t* ids, const int32_t* lens, const float* thresholds, int n_keywords, int vocab_size, const char* noun,
                           const int* numbers)
    : V_(vocab_size) {
    K2_REQUIRE(n_keywords >= 0, "keywords: %d keywords", n_keywords);
    K2_REQUIRE(vocab_size > K2HIP_UNK_ID, "keywords: vocab_size %d", vocab_size);
    K2_REQUIRE(n_keywords == 0 || (ids && lens && thresholds), "keywords: null keyword arrays");
    parent_.push_back(-1);
    tok_.push_back(-1);
    depth_.push_back(0);
    kw_.push_back(-1);
    std::vector<std::map<int, int>> kids(1);   // token -> child (a map: sorted by token)
    int64_t off = 0;
    for (int p = 0; p < n_keywords; p++) {
        const int num = numbers ? numbers[p] : p;
        K2_REQUIRE(lens[p] > 0, "keywords: %s %d is empty", noun, num);
        const float th = thresholds[p];
        K2_REQUIRE(std::isfinite(th) && th > 0.f && th <= 1.f, "keywords: %s %d: threshold %g outside (0, 1]", noun, num, (double)th);
        int s = 0;
        for (int i = 0; i < lens[p]; i++) {
            const int64_t v = ids[off + i];
            K2_REQUIRE(v >= 0 && v < V_, "keywords: %s %d: token id %lld outside [0, %d)", noun, num, (long long)v, V_);
            K2_REQUIRE(v != K2HIP_BLANK_ID && v != K2HIP_UNK_ID, "keywords: %s %d contains %s (id %lld)", noun, num,
                       v == K2HIP_BLANK_ID ? "blank" : "unk", (long long)v);
            auto it = kids[(size_t)s].find((int)v);
            int n;
            if (it != kids[(size_t)s].end()) {
                n = it->second;
            } else {
                n = (int)parent_.size();
                K2_REQUIRE(n < kKeywordsMaxStates, "keywords: %s %d: the trie outgrows %d states", noun, num, kKeywordsMaxStates);
                parent_.push_back(s);
                tok_.push_back((int)v);
                depth_.push_back(depth_[(size_t)s] + 1);
                kw_.push_back(-1);
                kids.emplace_back();
                kids[(size_t)s][(int)v] = n;
            }
            s = n;
        }
        if (kw_[(size_t)s] >= 0) {
            const int q = kw_[(size_t)s];
            failf(K2HIP_ERR_INVALID, "keywords: %s %d duplicates %s %d", noun, num, noun, numbers ? numbers[q] : q);
        }
        kw_[(size_t)s] = p;
        term_.push_back(s);
        thr_.push_back(th);
        off += lens[p];
    }
    const size_t S = parent_.size();
    bar_.assign(S, 0.f);
    for (size_t s = 0; s < S; s++)
        if (kw_[s] >= 0) bar_[s] = (float)depth_[s] * logf(thr_[(size_t)kw_[s]]);
    child_off_.assign(S + 1, 0);
    for (size_t s = 0; s < S; s++) {
        child_off_[s + 1] = child_off_[s] + (int32_t)kids[s].size();
        for (const auto& kv : kids[s]) {
            child_tok_.push_back(kv.first);
            child_state_.push_back(kv.second);
        }
    }
}

std::vector<int64_t> KeywordGraph::contexts(int cs) const {
    const size_t S = parent_.size();
    std::vector<int64_t> ctx(S * (size_t)cs, K2HIP_BLANK_ID);
    for (size_t s = 1; s < S; s++) {   // parent(s) < s: the parent's row is final
        const size_t p = (size_t)parent_[s];
        for (int i = 0; i + 1 < cs; i++) ctx[s * cs + i] = ctx[p * cs + i + 1];
        ctx[s * cs + cs - 1] = tok_[s];
    }
    return ctx;
}

}  // namespace k2hip
