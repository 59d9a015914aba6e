// Host side of the streaming modified beam search: the hypotheses a stream carries from one chunk to the next.
//
// The device search of a chunk starts from the saved hypotheses (beam.hip, BeamResumeLayout) and never sees their whole token
// sequences; what it needs of them is, per pair (a, b), whether H_a = H_b + x with a short x (|x| <= T' of the chunk).  The histories
// live here as two trees of refcounted nodes:
//   - SeqTree, hash-consed: one node per distinct token sequence ((parent, token) -> node), so node identity IS sequence identity
//     and the relation of a pair costs at most T' parent steps, whatever the length of the transcript.  (Without hash-consing a
//     prefix that was pruned and later spelled again would get a second node: a false "different".)
//   - PathTree, plain: (parent, token, timestamp, token log-prob) per hypothesis -- two hypotheses with the same tokens may carry different
//     timestamps (the first-inserted one's are kept at a merge, but an equal sequence can be spelled again later).
// Nodes no hypothesis reaches any more are freed (and their slot reused), so memory follows the live beam, not the stream's age.
// Plain C++ (no HIP): tests/native builds it on the CPU.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <unordered_map>
#include <vector>

namespace k2hip {

// nodes with parent links and reference counts (children + holders); node 0 is the root (the empty sequence) and is never freed
class RefTree {
  public:
    struct Node {
        int parent, tok, ts, depth, refs;
        float yp;   // PathTree: the token's log-prob at the frame it was emitted (0 where it was not asked for)
    };
    RefTree() { clear(); }
    void clear() {
        nodes_.assign(1, Node{-1, -1, -1, 0, 1, 0.f});
        free_.clear();
    }
    const Node& operator[](int i) const { return nodes_[(size_t)i]; }
    int parent(int i) const { return nodes_[(size_t)i].parent; }
    int depth(int i) const { return nodes_[(size_t)i].depth; }
    void ref(int i) { nodes_[(size_t)i].refs++; }
    // drops one reference; a node nobody refers to is freed, then its parent loses the reference the child held
    template <typename OnFree>
    void unref(int i, OnFree&& on_free) {
        while (i > 0 && --nodes_[(size_t)i].refs == 0) {
            on_free(i);
            const int p = nodes_[(size_t)i].parent;
            free_.push_back(i);
            i = p;
        }
    }
    size_t live() const { return nodes_.size() - free_.size(); }

  protected:
    int make(int parent, int tok, int ts, float yp = 0.f) {
        int id;
        const Node n{parent, tok, ts, nodes_[(size_t)parent].depth + 1, 0, yp};
        if (!free_.empty()) {
            id = free_.back();
            free_.pop_back();
            nodes_[(size_t)id] = n;
        } else {
            id = (int)nodes_.size();
            nodes_.push_back(n);
        }
        nodes_[(size_t)parent].refs++;
        return id;
    }
    std::vector<Node> nodes_;
    std::vector<int> free_;
};

class SeqTree : public RefTree {
  public:
    void clear() {
        RefTree::clear();
        index_.clear();
    }
    // the node of sequence(parent) + [tok], created if it does not exist
    int child(int parent, int tok) {
        const uint64_t key = ((uint64_t)(uint32_t)parent << 32) | (uint32_t)tok;
        auto it = index_.find(key);
        if (it != index_.end()) return it->second;
        const int id = make(parent, tok, -1);
        index_.emplace(key, id);
        return id;
    }
    void unref(int i) {
        RefTree::unref(i, [&](int n) { index_.erase(((uint64_t)(uint32_t)nodes_[(size_t)n].parent << 32) | (uint32_t)nodes_[(size_t)n].tok); });
    }
    // |x| if sequence(a) = sequence(b) + x with 0 < |x| <= cap (x's tokens into x[0..|x|)), else -1
    int extension(int a, int b, int cap, int* x) const {
        const int L = depth(a) - depth(b);
        if (L <= 0 || L > cap) return -1;
        int p = a;
        for (int i = L - 1; i >= 0; i--) {
            x[i] = nodes_[(size_t)p].tok;
            p = nodes_[(size_t)p].parent;
        }
        return p == b ? L : -1;
    }

  private:
    std::unordered_map<uint64_t, int> index_;
};

class PathTree : public RefTree {
  public:
    int child(int parent, int tok, int ts, float yp = 0.f) { return make(parent, tok, ts, yp); }
    void unref(int i) {
        RefTree::unref(i, [](int) {});
    }
};

// One entry of an N-best list: the emitted tokens (no context prefix), their frames and log-probs, the finalized log-prob
struct BeamAlt {
    std::vector<int64_t> tokens;
    std::vector<int32_t> timestamps;
    std::vector<float> token_log_probs;
    float score = 0.f;
    float lm_score = 0.f;   // the neural LM's total of the alternative (k2hip_set_rnn_lm rescoring of an offline list); 0: not rescored
    float lodr_score = 0.f; // the LODR total of the alternative (k2hip_set_lodr_lm, added in that rescoring); 0: not rescored or no LODR LM
};

// One stream's hypotheses between chunks and its result (the best hypothesis, materialised incrementally).
class BeamHistory {
  public:
    struct Hyp {
        int seq, path;     // SeqTree / PathTree nodes
        float lp;
        int ctx[2];        // decoder context: the last two tokens of [blank, blank] + ys
        int st = 0;        // state of the stream's hotword graph (0 = the root; always 0 without a graph)
        int lst = 0;       // state of the model's n-gram LM (always 0 without an LM)
        int dst = 0;       // state of the model's LODR LM (always 0 without one, and outside a fused search)
    };
    explicit BeamHistory(int K = 1, int blank = 0) : K_(K), blank_(blank) { reset(); }
    int beam() const { return K_; }
    void reset() {
        seq_.clear();
        path_.clear();
        hyps_.assign(1, Hyp{0, 0, 0.f, {blank_, blank_}});
        best_ = 0;
        frames_ = 0;
        mat_path_ = 0;
        mat_ids_.clear();
        tokens_.assign(2, blank_);
        timestamps_.clear();
        token_log_probs_.clear();
    }
    const std::vector<Hyp>& hyps() const { return hyps_; }
    int best() const { return best_; }
    long long frames() const { return frames_; }
    // Hotword biasing: pending[s] of the stream's graph (host copy), or null.  The carried log-probs keep the pending bonus of an
    // unfinished match; the result's score is reported without it (the finalize rule of the offline search, applied per step).
    void set_pending(std::shared_ptr<const std::vector<float>> pending) { pending_ = std::move(pending); }
    float score() const {
        const Hyp& h = hyps_[(size_t)best_];
        return pending_ ? h.lp - (*pending_)[(size_t)h.st] : h.lp;
    }
    // Tokens = [blank, blank] + ys of the best hypothesis; Timestamps = its absolute frame indexes
    const std::vector<int64_t>& tokens() const { return tokens_; }
    const std::vector<int32_t>& timestamps() const { return timestamps_; }
    // token log-probs of the best hypothesis, parallel to timestamps() (zeros for chunks applied without the yp block)
    const std::vector<float>& token_log_probs() const { return token_log_probs_; }
    // The current hypotheses, at most n of them, in the order of the final pick: (lp - pending(state)) / (length + 2) descending, ties
    // in insertion order -- entry 0 is the best hypothesis (tokens() / timestamps() / score()).  Each is read off its path node.
    std::vector<BeamAlt> nbest(int n) const {
        const int nh = (int)hyps_.size();
        std::vector<float> fin((size_t)nh), v((size_t)nh);
        for (int k = 0; k < nh; k++) {
            const Hyp& h = hyps_[(size_t)k];
            fin[(size_t)k] = pending_ ? h.lp - (*pending_)[(size_t)h.st] : h.lp;
            v[(size_t)k] = fin[(size_t)k] / (float)(seq_.depth(h.seq) + 2);
        }
        std::vector<BeamAlt> out((size_t)(n < nh ? (n < 0 ? 0 : n) : nh));
        for (int k = 0; k < nh; k++) {
            int rank = 0;
            for (int j = 0; j < nh; j++)
                if (v[(size_t)j] > v[(size_t)k] || (v[(size_t)j] == v[(size_t)k] && j < k)) rank++;
            if (rank >= (int)out.size()) continue;
            BeamAlt& a = out[(size_t)rank];
            const int d = path_.depth(hyps_[(size_t)k].path);
            a.tokens.resize((size_t)d);
            a.timestamps.resize((size_t)d);
            a.token_log_probs.resize((size_t)d);
            int p = hyps_[(size_t)k].path;
            for (int i = d - 1; i >= 0; i--) {
                a.tokens[(size_t)i] = path_[p].tok;
                a.timestamps[(size_t)i] = path_[p].ts;
                a.token_log_probs[(size_t)i] = path_[p].yp;
                p = path_.parent(p);
            }
            a.score = fin[(size_t)k];
        }
        return out;
    }
    const SeqTree& seq_tree() const { return seq_; }

    // the device search's in block (kernels.h BeamResumeLayout{K, Tp}) for the next chunk of Tp frames
    void fill_in(int* in, int Tp) const {
        const int K = K_, nh = (int)hyps_.size();
        const int o_lp = 1, o_ctx = 1 + K, o_len = 1 + 3 * K, o_rel = 1 + 4 * K, o_relx = 1 + 4 * K + K * K;
        memset(in, 0, sizeof(int) * (size_t)(o_relx + K * K * Tp));
        in[0] = nh;
        for (int k = 0; k < K; k++) {
            const bool live = k < nh;
            const float lp = live ? hyps_[(size_t)k].lp : -INFINITY;
            memcpy(&in[o_lp + k], &lp, sizeof(float));
            in[o_ctx + 2 * k] = live ? hyps_[(size_t)k].ctx[0] : blank_;
            in[o_ctx + 2 * k + 1] = live ? hyps_[(size_t)k].ctx[1] : blank_;
            in[o_len + k] = live ? seq_.depth(hyps_[(size_t)k].seq) : 0;
            for (int j = 0; j < K; j++) {
                int& r = in[o_rel + k * K + j];
                if (k == j) r = 0;
                else if (!live || j >= nh) r = -1;
                else r = seq_.extension(hyps_[(size_t)k].seq, hyps_[(size_t)j].seq, Tp, &in[o_relx + (k * K + j) * Tp]);
            }
        }
    }
    // N-gram LM: a stream keeps the LM it decoded its first chunk with.  begin_lm (only while no frame has been searched) notes that
    // LM's serial number (0 = none) and puts the start hypothesis into its start state; lm_serial() is what later chunks compare.
    void begin_lm(uint64_t serial, int start_state) {
        lm_serial_ = serial;
        hyps_[0].lst = start_state;
    }
    uint64_t lm_serial() const { return lm_serial_; }
    void fill_lm_states(int* lst_in) const {
        for (int k = 0; k < K_; k++) lst_in[k] = k < (int)hyps_.size() ? hyps_[(size_t)k].lst : 0;
    }
    // LODR: the same rule for the second automaton, which runs only in a fused search.  begin_lodr (only while no frame has been
    // searched) notes the setting's serial number (0 = none or not active) and puts the start hypothesis into that LM's start state.
    void begin_lodr(uint64_t serial, int start_state) {
        lodr_serial_ = serial;
        hyps_[0].dst = start_state;
    }
    uint64_t lodr_serial() const { return lodr_serial_; }
    void fill_lodr_states(int* dst_in) const {
        for (int k = 0; k < K_; k++) dst_in[k] = k < (int)hyps_.size() ? hyps_[(size_t)k].dst : 0;
    }
    // hotword side block in: the saved hypotheses' graph states [K]
    void fill_states(int* st_in) const {
        for (int k = 0; k < K_; k++) st_in[k] = k < (int)hyps_.size() ? hyps_[(size_t)k].st : 0;
    }
    // apply_out + the hotword side block out: the survivors' graph states [K]
    // (lst_out: the survivors' LM states [K], or null; dst_out: their LODR states [K], or null)
    void apply_out_states(const int* out, int Tp, const int* st_out, const float* yp = nullptr, const int* lst_out = nullptr,
                          const int* dst_out = nullptr) {
        apply_out(out, Tp, yp);
        for (size_t k = 0; k < hyps_.size(); k++) {
            hyps_[k].st = st_out[k];
            if (lst_out) hyps_[k].lst = lst_out[k];
            if (dst_out) hyps_[k].dst = dst_out[k];
        }
    }
    // the device search's out block of that chunk: the new hypotheses, the best one, the result; yp: the side block [K][Tp] with the
    // token log-probs of each survivor's suffix, or null (they are then kept as 0)
    void apply_out(const int* out, int Tp, const float* yp = nullptr) {
        const int K = K_, nh = out[0];
        const int o_org = 2, o_n = 2 + K, o_lp = 2 + 2 * K, o_ctx = 2 + 3 * K, o_ys = 2 + 5 * K, o_ts = 2 + 5 * K + K * Tp;
        std::vector<Hyp> nx((size_t)nh);
        for (int k = 0; k < nh; k++) {
            const Hyp& p = hyps_[(size_t)out[o_org + k]];
            int sq = p.seq, ph = p.path;
            for (int i = 0; i < out[o_n + k]; i++) {
                const int tok = out[o_ys + k * Tp + i];
                sq = seq_.child(sq, tok);
                ph = path_.child(ph, tok, (int)(frames_ + out[o_ts + k * Tp + i]), yp ? yp[k * Tp + i] : 0.f);
            }
            Hyp& h = nx[(size_t)k];
            h.seq = sq;
            h.path = ph;
            memcpy(&h.lp, &out[o_lp + k], sizeof(float));
            h.ctx[0] = out[o_ctx + 2 * k];
            h.ctx[1] = out[o_ctx + 2 * k + 1];
            seq_.ref(sq);
            path_.ref(ph);
        }
        for (const Hyp& h : hyps_) {   // (after the new ones hold their references: shared prefixes survive)
            seq_.unref(h.seq);
            path_.unref(h.path);
        }
        hyps_.swap(nx);
        best_ = out[1];
        frames_ += Tp;
        materialise(hyps_[(size_t)best_].path);
    }
    int hyp_last(int i) const { return hyps_[(size_t)best_].ctx[i]; }

  private:
    // tokens_ / timestamps_ := the path of node `to`; only the part past the longest prefix still shared with the last result is
    // rewritten (the last result's end node is referenced, so ids on its path are not reused while mat_ids_ names them)
    void materialise(int to) {
        std::vector<int> tail;
        int p = to;
        while (p != 0 && !(path_.depth(p) <= (int)mat_ids_.size() && mat_ids_[(size_t)path_.depth(p) - 1] == p)) {
            tail.push_back(p);
            p = path_.parent(p);
        }
        const size_t keep = (size_t)path_.depth(p);
        mat_ids_.resize(keep);
        tokens_.resize(2 + keep);
        timestamps_.resize(keep);
        token_log_probs_.resize(keep);
        for (size_t i = tail.size(); i-- > 0;) {
            mat_ids_.push_back(tail[i]);
            tokens_.push_back(path_[tail[i]].tok);
            timestamps_.push_back(path_[tail[i]].ts);
            token_log_probs_.push_back(path_[tail[i]].yp);
        }
        path_.ref(to);
        path_.unref(mat_path_);
        mat_path_ = to;
    }

    int K_, blank_;
    uint64_t lm_serial_ = 0;
    uint64_t lodr_serial_ = 0;
    std::shared_ptr<const std::vector<float>> pending_;   // (kept across reset(): the graph stays attached)
    SeqTree seq_;
    PathTree path_;
    std::vector<Hyp> hyps_;
    int best_ = 0;
    long long frames_ = 0;
    int mat_path_ = 0;
    std::vector<int> mat_ids_;
    std::vector<int64_t> tokens_;
    std::vector<int32_t> timestamps_;
    std::vector<float> token_log_probs_;
};

}  // namespace k2hip
