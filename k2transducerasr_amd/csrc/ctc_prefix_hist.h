// Host side of the streaming CTC prefix beam search: the live prefixes a stream carries from one chunk to the next.
//
// The device search of a chunk (ctc_prefix.hip, k_ctc_prefix<true>) starts from the carried slots and never sees their token
// sequences; what it needs of them is (pb, pnb, last token, length, its own rolling hashes) per slot and, per pair (a, b), whether
// S_a = S_b + x with a short x (|x| <= Tc of the chunk).  The histories live in the two trees of beam_hist.h: the hash-consed SeqTree
// (node identity IS sequence identity, so the relation of a pair costs at most Tc parent steps) and the PathTree with every slot's own
// (token, absolute frame, token log-prob) -- two slots never spell the same sequence, but a sequence that left the beam and is spelled
// again comes back with the frames of its second spelling, as in the search over the whole row.  Nodes no slot reaches are freed, so
// memory follows the live beam, not the stream's age.  The slots are kept in rank order: slot 0 is the result.
// Plain C++ (no HIP): tests/native builds it on the CPU.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "beam_hist.h"
#include "ctc_prefix_layout.h"
#include "errors.h"

namespace k2hip {

class CtcPrefixHistory {
  public:
    struct Slot {
        int seq, path;   // SeqTree / PathTree nodes
        float pb, pnb;
        uint64_t hash, phash;
    };
    explicit CtcPrefixHistory(int beam = 1, int nbest = 1) : K_(beam), nbest_(nbest) { reset(); }
    int beam() const { return K_; }
    int nbest_limit() const { return nbest_; }
    void reset() {
        seq_.clear();
        path_.clear();
        slots_.assign(1, Slot{0, 0, 0.f, -INFINITY, kCtcPrefixHashSeed, 0});
        tot_.clear();
        ctx_.assign(1, 0.f);
        hs_.assign(1, 0);
        ls_.assign(1, 0);
        fin_.clear();
        ord_.clear();
        lm_serial_ = 0;
        lm_on_ = false;
        frames_ = 0;
        mat_path_ = 0;
        mat_ids_.clear();
        tokens_.clear();
        timestamps_.clear();
        token_log_probs_.clear();
    }
    const std::vector<Slot>& slots() const { return slots_; }
    long long frames() const { return frames_; }
    // the best prefix (slot 0): tokens, absolute frames, token log-probs, score = logaddexp(pb, pnb) in float32 as the device forms it
    const std::vector<int64_t>& tokens() const { return tokens_; }
    const std::vector<int32_t>& timestamps() const { return timestamps_; }
    const std::vector<float>& token_log_probs() const { return token_log_probs_; }
    // (the total the device formed from (pb, pnb), kept as it came out: the host's log1pf / expf may round the sum differently)
    // (a biased stream: the first entry in final order and its final score; tokens() etc. are that entry's)
    float score() const { return tot_.empty() ? 0.f : fin_.empty() ? tot_[0] : fin_[(size_t)ord_[0]]; }
    int longest() const {
        int d = 0;
        for (const Slot& s : slots_) d = seq_.depth(s.seq) > d ? seq_.depth(s.seq) : d;
        return d;
    }
    size_t live_nodes() const { return seq_.live() > path_.live() ? seq_.live() : path_.live(); }
    // the live prefixes in slot (= rank) order -- a biased stream: in final order, read through ord --, at most n of them, each read off
    // its path node
    std::vector<BeamAlt> nbest(int n) const {
        const int nh = (int)slots_.size();
        std::vector<BeamAlt> out((size_t)(n < nh ? (n < 0 ? 0 : n) : nh));
        for (size_t i = 0; i < out.size(); i++) {
            BeamAlt& a = out[i];
            const size_t k = ord_.empty() ? i : (size_t)ord_[i];
            const int d = path_.depth(slots_[k].path);
            a.tokens.resize((size_t)d);
            a.timestamps.resize((size_t)d);
            a.token_log_probs.resize((size_t)d);
            int p = slots_[k].path;
            for (int i = d - 1; i >= 0; i--) {
                a.tokens[(size_t)i] = path_[p].tok;
                a.timestamps[(size_t)i] = path_[p].ts;
                a.token_log_probs[(size_t)i] = path_[p].yp;
                p = path_.parent(p);
            }
            a.score = k >= tot_.size() ? 0.f : fin_.empty() ? tot_[k] : fin_[k];
        }
        return out;
    }

    // ---- biasing (include/k2hip.h "Biasing of the streaming CTC prefix beam search") ----
    // Beside (pb, pnb) every slot carries ctx (the accumulated context score, WITH the pending bonus of a match under way), hs (state of
    // the stream's hotword graph) and ls (LM state); the slots stay in selection-rank order.  fin / ord are the last step's final
    // scores by slot and the slots by (final desc, slot asc): what the stream reports.  An unbiased stream has ctx = hs = ls = 0 and
    // no fin / ord (identity, tot).
    // A stream keeps the LM it searched its first chunk with: begin_lm (only while no frame has been searched) notes that LM's serial
    // number (0 = none), whether this stream runs it, and puts the start prefix into its start state.
    void begin_lm(uint64_t serial, bool on, int start_state) {
        lm_serial_ = serial;
        lm_on_ = on;
        ls_[0] = on ? start_state : 0;
    }
    uint64_t lm_serial() const { return lm_serial_; }
    bool lm_on() const { return lm_on_; }
    const std::vector<float>& ctx() const { return ctx_; }
    const std::vector<int>& hs() const { return hs_; }
    const std::vector<int>& ls() const { return ls_; }
    const std::vector<float>& fin() const { return fin_; }
    const std::vector<int>& ord() const { return ord_; }
    // the side in block (CtcPrefixResumeBiasLayout{K}) for the next chunk.  S: the states of the graph this stream reads (0: none),
    // S_lm: the states of the LM (0: none): every carried state must lie inside its table before anything is launched
    void fill_side_in(int* side, int S, int S_lm) const {
        const CtcPrefixResumeBiasLayout L{K_};
        memset(side, 0, sizeof(int) * (size_t)L.in_ints());
        K2_REQUIRE(!lm_on_ || S_lm >= 1, "ctc prefix stream: the stream runs an n-gram LM and none is set");
        side[0] = lm_on_ ? 1 : 0;
        for (size_t k = 0; k < slots_.size(); k++) {
            K2_REQUIRE(hs_[k] >= 0 && hs_[k] < (S >= 1 ? S : 1), "ctc prefix stream: slot %zu carries the hotword state %d outside [0, %d)", k, hs_[k], S >= 1 ? S : 1);
            K2_REQUIRE(!lm_on_ || (ls_[k] >= 0 && ls_[k] < S_lm), "ctc prefix stream: slot %zu carries the LM state %d outside [0, %d)", k, ls_[k], S_lm);
            memcpy(&side[L.in_ctx() + (int)k], &ctx_[k], sizeof(float));
            side[L.in_hs() + (int)k] = hs_[k];
            side[L.in_ls() + (int)k] = ls_[k];
        }
    }
    // what a side out block must satisfy beside check_out: ord a permutation of the survivors, every state inside its table
    void check_out(const int* out, const int* side, int Tc, int n_frames, int S, int S_lm) const {
        check_out(out, Tc, n_frames);
        const CtcPrefixResumeBiasLayout L{K_};
        const int nh = out[0];
        unsigned seen = 0;
        for (int k = 0; k < nh; k++) {
            const int q = side[L.out_ord() + k], hs = side[L.out_hs() + k], ls = side[L.out_ls() + k];
            K2_REQUIRE(q >= 0 && q < nh && !(seen >> q & 1u), "ctc prefix stream: side out block: the final order is no permutation (entry %d = %d)", k, q);
            seen |= 1u << q;
            K2_REQUIRE(hs >= 0 && hs < (S >= 1 ? S : 1), "ctc prefix stream: side out block slot %d: hotword state %d outside [0, %d)", k, hs, S >= 1 ? S : 1);
            K2_REQUIRE(!lm_on_ || (ls >= 0 && ls < S_lm), "ctc prefix stream: side out block slot %d: LM state %d outside [0, %d)", k, ls, S_lm);
        }
    }
    // the out block and the side out block of a chunk (both checked by the caller)
    void apply_out(const int* out, const int* side, int Tc, int n_frames) {
        const CtcPrefixResumeBiasLayout L{K_};
        const int nh = out[0];
        std::vector<float> ctx((size_t)nh), fin((size_t)nh);
        std::vector<int> hs((size_t)nh), ls((size_t)nh), ord((size_t)nh);
        for (int k = 0; k < nh; k++) {
            memcpy(&ctx[(size_t)k], &side[L.out_ctx() + k], sizeof(float));
            memcpy(&fin[(size_t)k], &side[L.out_fin() + k], sizeof(float));
            hs[(size_t)k] = side[L.out_hs() + k];
            ls[(size_t)k] = side[L.out_ls() + k];
            ord[(size_t)k] = side[L.out_ord() + k];
        }
        apply_slots(out, Tc, n_frames);
        ctx_.swap(ctx); hs_.swap(hs); ls_.swap(ls); fin_.swap(fin); ord_.swap(ord);
        materialise(slots_[(size_t)ord_[0]].path);
    }

    // the device search's in block (CtcPrefixResumeLayout{K, Tc}) for the next chunk of up to Tc frames
    void fill_in(int* in, int Tc) const {
        const CtcPrefixResumeLayout L{K_, Tc};
        const int K = K_, nh = (int)slots_.size();
        memset(in, 0, sizeof(int) * (size_t)L.in_ints());
        in[0] = nh;
        for (int k = 0; k < K; k++) {
            const bool live = k < nh;
            const float pb = live ? slots_[(size_t)k].pb : -INFINITY, pnb = live ? slots_[(size_t)k].pnb : -INFINITY;
            memcpy(&in[L.in_pb() + k], &pb, sizeof(float));
            memcpy(&in[L.in_pnb() + k], &pnb, sizeof(float));
            in[L.in_e() + k] = live ? seq_[slots_[(size_t)k].seq].tok : -1;
            in[L.in_len() + k] = live ? seq_.depth(slots_[(size_t)k].seq) : 0;
            const uint64_t h = live ? slots_[(size_t)k].hash : 0, ph = live ? slots_[(size_t)k].phash : 0;
            in[L.in_hash() + 2 * k] = (int)(uint32_t)h; in[L.in_hash() + 2 * k + 1] = (int)(uint32_t)(h >> 32);
            in[L.in_phash() + 2 * k] = (int)(uint32_t)ph; in[L.in_phash() + 2 * k + 1] = (int)(uint32_t)(ph >> 32);
            for (int j = 0; j < K; j++) {
                int& r = in[L.in_rel() + k * K + j];
                if (k == j) r = 0;
                else if (!live || j >= nh) r = -1;
                else r = seq_.extension(slots_[(size_t)k].seq, slots_[(size_t)j].seq, Tc, &in[L.in_relx() + (k * K + j) * Tc]);
            }
        }
    }
    // what an out block must satisfy before it is applied (a block the device wrote does; a caller-supplied one may not)
    void check_out(const int* out, int Tc, int n_frames) const {
        const CtcPrefixResumeLayout L{K_, Tc};
        const int nh = out[0];
        K2_REQUIRE(n_frames >= 1 && n_frames <= Tc, "ctc prefix stream: n_frames = %d outside [1, Tc = %d]", n_frames, Tc);
        K2_REQUIRE(nh >= 1 && nh <= K_, "ctc prefix stream: out block with %d survivors (beam %d)", nh, K_);
        for (int k = 0; k < nh; k++) {
            const int org = out[L.out_org() + k], na = out[L.out_napp() + k];
            K2_REQUIRE(org >= 0 && org < (int)slots_.size() && na >= 0 && na <= n_frames, "ctc prefix stream: out block slot %d: origin %d, %d appended", k, org, na);
            for (int i = 0; i < na; i++) {
                const int ts = out[L.out_ts() + k * Tc + i];
                K2_REQUIRE(out[L.out_ys() + k * Tc + i] >= 1 && ts >= 0 && ts < n_frames, "ctc prefix stream: out block slot %d: bad token or frame", k);
            }
        }
    }
    // the device search's out block of that chunk of n_frames frames: the survivors in rank order
    void apply_out(const int* out, int Tc, int n_frames) {
        apply_slots(out, Tc, n_frames);
        ctx_.assign(slots_.size(), 0.f);
        hs_.assign(slots_.size(), 0);
        ls_.assign(slots_.size(), 0);
        materialise(slots_[0].path);
    }

  private:
    void apply_slots(const int* out, int Tc, int n_frames) {
        check_out(out, Tc, n_frames);
        const CtcPrefixResumeLayout L{K_, Tc};
        const int nh = out[0];
        std::vector<Slot> nx((size_t)nh);
        std::vector<float> tot((size_t)nh);
        for (int k = 0; k < nh; k++) {
            const Slot& p = slots_[(size_t)out[L.out_org() + k]];
            int sq = p.seq, ph = p.path;
            for (int i = 0; i < out[L.out_napp() + k]; i++) {
                const int tok = out[L.out_ys() + k * Tc + i];
                float yp;
                memcpy(&yp, &out[L.out_yp() + k * Tc + i], sizeof(float));
                sq = seq_.child(sq, tok);
                ph = path_.child(ph, tok, (int)(frames_ + out[L.out_ts() + k * Tc + i]), yp);
            }
            Slot& s = nx[(size_t)k];
            s.seq = sq;
            s.path = ph;
            memcpy(&s.pb, &out[L.out_pb() + k], sizeof(float));
            memcpy(&s.pnb, &out[L.out_pnb() + k], sizeof(float));
            s.hash = (uint64_t)(uint32_t)out[L.out_hash() + 2 * k] | (uint64_t)(uint32_t)out[L.out_hash() + 2 * k + 1] << 32;
            s.phash = (uint64_t)(uint32_t)out[L.out_phash() + 2 * k] | (uint64_t)(uint32_t)out[L.out_phash() + 2 * k + 1] << 32;
            memcpy(&tot[(size_t)k], &out[L.out_tot() + k], sizeof(float));
            seq_.ref(sq);
            path_.ref(ph);
        }
        for (const Slot& s : slots_) {   // (after the new ones hold their references: shared prefixes survive)
            seq_.unref(s.seq);
            path_.unref(s.path);
        }
        slots_.swap(nx);
        tot_.swap(tot);
        frames_ += n_frames;
    }

    // tokens_ / timestamps_ / token_log_probs_ := the path of node `to`; only the part past the longest prefix still shared with the
    // last result is rewritten (BeamHistory::materialise)
    void materialise(int to) {
        std::vector<int> tail;
        int p = to;
        while (p != 0 && !(path_.depth(p) <= (int)mat_ids_.size() && mat_ids_[(size_t)path_.depth(p) - 1] == p)) {
            tail.push_back(p);
            p = path_.parent(p);
        }
        const size_t keep = (size_t)path_.depth(p);
        mat_ids_.resize(keep);
        tokens_.resize(keep);
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

    int K_, nbest_;
    SeqTree seq_;
    PathTree path_;
    std::vector<Slot> slots_;
    std::vector<float> tot_;   // the slots' totals as the device formed them (empty before the first chunk: the start, 0)
    std::vector<float> ctx_, fin_;   // biasing: per slot; fin_ / ord_ empty on an unbiased stream
    std::vector<int> hs_, ls_, ord_;
    uint64_t lm_serial_ = 0;
    bool lm_on_ = false;
    long long frames_ = 0;
    int mat_path_ = 0;
    std::vector<int> mat_ids_;
    std::vector<int64_t> tokens_;
    std::vector<int32_t> timestamps_;
    std::vector<float> token_log_probs_;
};

}  // namespace k2hip
