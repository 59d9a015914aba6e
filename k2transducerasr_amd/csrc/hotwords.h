// Hotword (contextual biasing) graph of the modified beam search: the trie of the phrases' token sequences with Aho-Corasick failure
// links.  Pure host code (no HIP): built and walked without a GPU; the model uploads its dense form (include/k2hip.h
// k2hip_set_hotwords, DESIGN.md "Hotword biasing").
//
// State 0 is the root, depth(s) the node's depth, pending(s) = score_per_token * depth(s).  A hypothesis in state s that appends the
// real token v moves to n = delta(s, v) (goto; on a miss the failure links; the root loops) and earns pending(n) - pending(s).  If n
// ends a phrase the match is committed: the bonus stays and the state returns to the root.  No output links: a phrase end that is only
// reachable through a failure link from n is not reported.  Blank and unk append nothing and leave the state alone.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

namespace k2hip {

// dense device form: next / bonus [S][V] (int32 / f32) + pending [S]; S * V entries at most
constexpr int64_t kHotwordMaxEntries = (int64_t)1 << 23;

class HotwordGraph {
  public:
    // phrases: token ids, phrase p = ids[off .. off + lens[p]).  names[p] (optional) is what an error calls phrase p ("phrase 3" /
    // "line 7"); throws Error(K2HIP_ERR_INVALID) naming the offending phrase
    HotwordGraph(const int64_t* ids, const int32_t* lens, int n_phrases, float score_per_token, int vocab_size, const char* noun = "phrase",
                 const int* numbers = nullptr);
    int num_states() const { return (int)depth_.size(); }
    int vocab_size() const { return V_; }
    float score_per_token() const { return c_; }
    float pending(int s) const { return c_ * (float)depth_[(size_t)s]; }
    // one step of the definition above: the state after `token` and the bonus it earns
    void step(int state, int64_t token, int* next_state, float* bonus) const;
    // next[s * V + v] = state after v (the root after a committed match), bonus[s * V + v], pending[s]
    void dense(std::vector<int32_t>* next, std::vector<float>* bonus, std::vector<float>* pending) const;

  private:
    int delta(int s, int v) const;   // the Aho-Corasick transition, before the commit rule
    int child(int s, int v) const;   // goto or -1
    int V_;
    float c_;
    std::vector<int> depth_, fail_;
    std::vector<char> end_;
    std::vector<std::vector<std::pair<int, int>>> kids_;   // per state: (token, child), sorted by token
};

}  // namespace k2hip
