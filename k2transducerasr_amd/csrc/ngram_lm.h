// Back-off n-gram LM of the modified beam search (shallow fusion): the automaton of an ARPA model over the acoustic model's own
// tokens.  Pure host code (no HIP): built, parsed and walked without a GPU; the model uploads its sparse form scaled
// (include/k2hip.h k2hip_set_ngram_lm, DESIGN.md "N-gram LM shallow fusion").
//
// State 0 is the empty history; one state per history of length 1 .. N-1 that is the history of some kept entry, numbered by
// (length, ids lexicographically, <s> = -1 first).  A state has its explicit arcs (token -> log_prob, next state) sorted by token, a
// back-off weight and a back-off state (the longest proper suffix of its history that is a state).  Step(s, w), w a real token:
// acc = 0; while w has no arc in s and s != 0: acc += bow(s), s = backoff(s); result acc + log_prob(arc), in float32 in that order.
// At state 0 a token without a unigram scores the <unk> unigram and moves to state 0.  Blank and unk append nothing.
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../../include/k2hip.h"

namespace k2hip {

// pseudo ids of the array form (include/k2hip.h K2HIP_NGRAM_BOS / _EOS / _UNK)
constexpr int64_t kNgramBos = -1, kNgramEos = -2, kNgramUnk = -3;
constexpr int kNgramMaxOrder = K2HIP_NGRAM_MAX_ORDER;
constexpr int64_t kNgramMaxArcs = (int64_t)1 << 24;

// the sparse device form, every weight multiplied by `scale` once (float32, entry by entry): the device only adds
struct NgramDeviceForm {
    std::vector<int32_t> states;     // [S][4]: arc begin, arc end, back-off state, back-off weight (float bits)
    std::vector<int32_t> arc_tok;    // [A] sorted by token within a state
    std::vector<float> arc_lp;       // [A]
    std::vector<int32_t> arc_next;   // [A]
    std::vector<float> uni_lp;       // [V] state 0 with the <unk> rule resolved (blank / unk: 0)
    std::vector<int32_t> uni_next;   // [V]
};

class NgramLm {
  public:
    // Entry e: ids[off .. off + orders[e]) (real token ids, or the pseudo ids above), natural-log log_probs[e], backoffs[e] (0 where
    // absent).  names an offending entry as "<noun> <numbers[e] or e>"; throws Error(K2HIP_ERR_INVALID).
    NgramLm(const int64_t* ids, const int32_t* orders, const float* log_probs, const float* backoffs, int64_t n_entries, int vocab_size,
            const char* noun = "entry", const int* numbers = nullptr);
    int order() const { return N_; }
    int num_states() const { return (int)bo_state_.size(); }
    int64_t num_arcs() const { return (int64_t)tok_.size(); }
    int start_state() const { return start_; }
    int vocab_size() const { return V_; }
    void step(int state, int64_t token, int* next_state, float* log_prob) const;
    void device_form(float scale, NgramDeviceForm* d) const;

  private:
    int V_, N_ = 1, start_ = 0;
    bool has_unk_ = false;
    float unk_lp_ = 0.f;
    std::vector<int64_t> off_;          // [S + 1]
    std::vector<int32_t> tok_, next_;   // [A]
    std::vector<float> lp_;             // [A]
    std::vector<int32_t> bo_state_;     // [S]
    std::vector<float> bow_;            // [S]
};

// A text ARPA file held in memory (bounds-checked: reads nothing outside [data, data + len)).  Words are looked up in id_of (the
// token strings of tokens.txt); <unk> is always the LM's fallback, <s> / </s> are the sentence marks unless id_of has them.  log10
// values are parsed as double, multiplied by ln 10 in double, then rounded to float32.  Errors are K2HIP_ERR_INVALID and name
// `name` and the line.
NgramLm* ngram_parse_arpa(const char* data, size_t len, const std::map<std::string, int>& id_of, int vocab_size, const char* name);

}  // namespace k2hip
