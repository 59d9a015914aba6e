// Keyword graph of the transducer keyword spotter: the trie of the keywords' token sequences, one threshold per keyword.  Pure host
// code (no HIP, no model): built and read without a GPU (include/k2hip.h "Keyword spotting", DESIGN.md "Keyword spotting").
//
// States are numbered in insertion order, root = 0, parent(s) < s.  State s != root has the token tok(s) of its incoming arc, its
// depth, kw(s) = the keyword that ends there (or -1) and bar(s) = (float)depth(s) * logf(threshold(kw(s))): ONE float32 product,
// rounded once, here (0 where no keyword ends).  A keyword may be a proper prefix of another: a terminal state may have children.
// Every state's children are kept sorted by token (child_off / child_tok / child_state: the form the arc kernel reads).
#pragma once
#include <cstdint>
#include <vector>

namespace k2hip {

constexpr int kKeywordsMaxStates = 1024;   // = K2HIP_KEYWORDS_MAX_STATES (the token-passing kernel keeps 4 rows of S words in LDS)

class KeywordGraph {
  public:
    // keyword p = ids[off .. off + lens[p]), thresholds[p] in (0, 1].  `noun` / numbers[p] (optional) is what an error calls keyword p
    // ("keyword 3" / "line 7"); throws Error(K2HIP_ERR_INVALID) naming the offending keyword
    KeywordGraph(const int64_t* ids, const int32_t* lens, const float* thresholds, int n_keywords, int vocab_size, const char* noun = "keyword",
                 const int* numbers = nullptr);
    int num_states() const { return (int)parent_.size(); }
    int num_keywords() const { return (int)term_.size(); }
    int vocab_size() const { return V_; }
    const std::vector<int32_t>& parent() const { return parent_; }   // [S], parent(0) = -1
    const std::vector<int32_t>& tok() const { return tok_; }         // [S], tok(0) = -1
    const std::vector<int32_t>& depth() const { return depth_; }     // [S]
    const std::vector<int32_t>& kw() const { return kw_; }           // [S], -1 = no keyword ends here
    const std::vector<float>& bar() const { return bar_; }           // [S]
    const std::vector<int32_t>& terminal() const { return term_; }   // [P]: the state keyword p ends in
    const std::vector<float>& thresholds() const { return thr_; }    // [P]
    const std::vector<int32_t>& child_off() const { return child_off_; }      // [S + 1]
    const std::vector<int32_t>& child_tok() const { return child_tok_; }      // [S - 1], sorted inside every state's range
    const std::vector<int32_t>& child_state() const { return child_state_; }  // [S - 1]
    // ctx(s): the last context_size ids of [blank] * context_size + path(s), [S][context_size]
    std::vector<int64_t> contexts(int context_size) const;

  private:
    int V_;
    std::vector<int32_t> parent_, tok_, depth_, kw_, term_, child_off_, child_tok_, child_state_;
    std::vector<float> bar_, thr_;
};

}  // namespace k2hip
