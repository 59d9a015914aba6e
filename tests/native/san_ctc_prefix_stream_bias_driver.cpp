// AddressSanitizer / UBSan driver of the host side of biasing in the streaming CTC prefix beam search: the history a stream carries
// between chunks with its side blocks (csrc/ctc_prefix_hist.h), the float32 host reference of the resumed biased step
// (engine_stub_ctc_prefix_stream_bias.cpp) and the rules of k2hip_ctc_prefix_stream_set_hotwords / _set_biasing /
// k2hip_online_stream_set_ctc_prefix_biasing (csrc/api.cpp) over the CPU stand-ins of the engine.  TEST INFRASTRUCTURE: its own program
// (`make -C k2transducerasr_amd/csrc san_ctc_prefix_stream_bias`, tests/test_ctc_prefix_stream_bias_sanitizers.py), never loaded into
// another process.
// Exercised: random rows (quarter steps, ties and -inf cells included) with random graphs and LMs at random chunkings through
// CtcPrefixHistory and the resumed biased reference; after EVERY chunk the slots (pb, pnb, ctx, hs, ls in selection order) and the
// entries (tokens, absolute timestamps, token log-probs, final, in final order) equal ctc_prefix_bias_ref.h over all frames so far bit
// for bit, and the live tree nodes are at most beam * (longest live prefix + 1) + 1; rows with null tables beside biased ones equal the
// unbiased resumed reference; side blocks with states out of range are refused.  Then, through the ABI: attach / switch / reset /
// destroy orders, a graph shared between streams and outliving its handle, the setters' start-state rule, the LM-change rule with
// the streams unchanged, a call that mixes biased and unbiased streams; and the recognizer level over the stand-in of the tick.
//   san_ctc_prefix_stream_bias_driver [<ctc.k2w> <offline.k2w> [<ctc_streaming.k2w>]]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../../include/k2hip.h"
#include "../../k2transducerasr_amd/csrc/ctc_prefix_bias_ref.h"
#include "../../k2transducerasr_amd/csrc/ctc_prefix_hist.h"
#include "../../k2transducerasr_amd/csrc/hotwords.h"
#include "../../k2transducerasr_amd/csrc/ngram_lm.h"

#define CHECK(cond)                                                                                                          \
    do {                                                                                                                     \
        if (!(cond)) {                                                                                                       \
            fprintf(stderr, "CHECK failed at %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, k2hip_last_error()); \
            exit(3);                                                                                                         \
        }                                                                                                                    \
    } while (0)
#define OK(call) CHECK((call) == K2HIP_OK)

namespace k2hip {
void ctc_prefix_chunk_ref(const float* log_probs, int B, int Tc, int V, const int32_t* n_frames, int K, const int* in_all, int* out_all);
void ctc_prefix_chunk_bias_ref(const float* log_probs, int B, int Tc, int V, const int32_t* n_frames, int K, const int* in_all, int* out_all,
                               const CtcPrefixBiasTables* tabs, const int* side_in_all, int* side_out_all);
long long ctc_prefix_bias_launch_count();
}  // namespace k2hip

namespace {

using namespace k2hip;

unsigned long long rng_state = 88172645463325252ull;
unsigned rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 32);
}
bool same_bits(float a, float b) { return memcmp(&a, &b, sizeof a) == 0; }

struct Tables {
    std::vector<int32_t> next;
    std::vector<float> bonus, pending;
    NgramDeviceForm lm;
    CtcPrefixBiasTables view;
};
int64_t real_token(int V) {
    for (;;) {
        const int64_t v = 1 + rnd() % (unsigned)(V - 1);
        if (v != K2HIP_UNK_ID) return v;
    }
}
// a random legal phrase list (no duplicate, no phrase a prefix of another) as (ids, lens)
void random_phrases(int V, std::vector<int64_t>* ids, std::vector<int32_t>* lens) {
    std::vector<std::vector<int64_t>> phrases;
    const int n = 1 + (int)(rnd() % 4);
    for (int p = 0; p < n; p++) {
        std::vector<int64_t> ph;
        const int len = 1 + (int)(rnd() % 3);
        for (int i = 0; i < len; i++) ph.push_back(real_token(V));
        bool clash = false;
        for (const auto& q : phrases) {
            const size_t m = std::min(q.size(), ph.size());
            clash = clash || std::equal(q.begin(), q.begin() + (long)m, ph.begin());
        }
        if (clash) continue;
        phrases.push_back(ph);
        ids->insert(ids->end(), ph.begin(), ph.end());
        lens->push_back(len);
    }
}
// random n-gram entries over the real tokens of V: every history of a kept entry has its own entry
void random_lm_entries(int V, std::vector<int64_t>* ids, std::vector<int32_t>* orders, std::vector<float>* lps, std::vector<float>* bos) {
    std::map<std::vector<int64_t>, std::pair<float, float>> ent;
    ent[{kNgramBos}] = {-99.f, -0.25f};
    ent[{kNgramUnk}] = {-7.5f, 0.f};
    std::vector<int64_t> real;
    for (int v = 1; v < V; v++)
        if (v != K2HIP_UNK_ID) real.push_back(v);
    for (size_t i = 0; i < real.size(); i++)
        if (i == 0 || rnd() % 4) ent[{real[i]}] = {-0.25f * (float)(4 + rnd() % 16), -0.125f * (float)(1 + rnd() % 8)};
    const int chains = 2 + (int)(rnd() % 6);
    for (int c = 0; c < chains; c++) {
        std::vector<int64_t> seq;
        const int len = 2 + (int)(rnd() % 2);
        for (int i = 0; i < len; i++) seq.push_back(real_token(V));
        bool has = true;
        for (int64_t v : seq) has = has && ent.count({v});
        if (!has) continue;
        for (size_t nn = 2; nn <= seq.size(); nn++) {
            const std::vector<int64_t> k(seq.begin(), seq.begin() + (long)nn);
            if (!ent.count(k)) ent[k] = {-0.125f * (float)(1 + rnd() % 12), nn < 3 ? -0.125f * (float)(1 + rnd() % 8) : 0.f};
        }
    }
    for (const auto& kv : ent) {
        ids->insert(ids->end(), kv.first.begin(), kv.first.end());
        orders->push_back((int32_t)kv.first.size());
        lps->push_back(kv.second.first);
        bos->push_back(kv.second.second);
    }
}
void random_tables(int V, bool hw, bool lm, Tables* t) {
    t->view = CtcPrefixBiasTables{};
    t->view.V = V;
    if (hw) {
        std::vector<int64_t> ids;
        std::vector<int32_t> lens;
        random_phrases(V, &ids, &lens);
        const HotwordGraph g(ids.data(), lens.data(), (int)lens.size(), 1.5f, V);
        g.dense(&t->next, &t->bonus, &t->pending);
        t->view.S = g.num_states();
        t->view.next = t->next.data(); t->view.bonus = t->bonus.data(); t->view.pending = t->pending.data();
    }
    if (lm) {
        std::vector<int64_t> ids;
        std::vector<int32_t> orders;
        std::vector<float> lps, bos;
        random_lm_entries(V, &ids, &orders, &lps, &bos);
        const NgramLm m(ids.data(), orders.data(), lps.data(), bos.data(), (int64_t)orders.size(), V);
        m.device_form(0.5f, &t->lm);
        t->view.S_lm = m.num_states(); t->view.A = (long long)t->lm.arc_tok.size(); t->view.start = m.start_state();
        t->view.states = t->lm.states.data();
        t->view.arc_tok = t->lm.arc_tok.data(); t->view.arc_lp = t->lm.arc_lp.data(); t->view.arc_next = t->lm.arc_next.data();
        t->view.uni_lp = t->lm.uni_lp.data(); t->view.uni_next = t->lm.uni_next.data();
    }
    ctc_prefix_bias_check_tables(t->view);
}

template <typename F>
bool refused(F&& f) {
    try {
        f();
    } catch (const Error&) {
        return true;
    }
    return false;
}

// ---- 1. the chunked reference against the whole-row reference -------------------------------------------------------------------
long long pending_boundaries = 0, reordered_boundaries = 0;

void chunked_case(int V, int T, int beam, bool hw, bool lm) {
    Tables tb;
    random_tables(V, hw, lm, &tb);
    std::vector<float> lp((size_t)T * (size_t)V);
    for (float& x : lp) x = rnd() % 23 == 0 ? -INFINITY : -0.25f * (float)(rnd() % 24);
    std::vector<int32_t> chunks;
    for (int left = T; left > 0;) {
        const int n = 1 + (int)(rnd() % (unsigned)std::min(left, 7));
        chunks.push_back(n);
        left -= n;
    }
    const int Tc = *std::max_element(chunks.begin(), chunks.end()) + (int)(rnd() % 2);   // (a capacity above the longest chunk, sometimes)
    const CtcPrefixResumeLayout L{beam, Tc};
    const CtcPrefixResumeBiasLayout SL{beam};
    // two streams in every call: the biased one, and the same row with null tables and the LM masked off
    CtcPrefixHistory hist(beam, beam), plain(beam, beam), unbiased(beam, beam);
    hist.begin_lm(lm ? 1 : 0, lm, tb.view.start);
    std::vector<int> in((size_t)2 * L.in_ints()), out((size_t)2 * L.out_ints()), sin((size_t)2 * SL.in_ints()), sout((size_t)2 * SL.out_ints());
    std::vector<int> pin((size_t)L.in_ints()), pout((size_t)L.out_ints());
    std::vector<float> chunk((size_t)2 * Tc * (size_t)V);
    int done = 0;
    for (int32_t n : chunks) {
        hist.fill_in(in.data(), Tc);
        unbiased.fill_in(in.data() + L.in_ints(), Tc);
        hist.fill_side_in(sin.data(), tb.view.S, lm ? tb.view.S_lm : 0);
        unbiased.fill_side_in(sin.data() + SL.in_ints(), 0, 0);
        for (int b = 0; b < 2; b++) ctc_prefix_bias_check_side_in(sin.data() + (size_t)b * SL.in_ints(), beam, b ? 0 : tb.view.S, lm ? tb.view.S_lm : 0, b);
        std::fill(chunk.begin(), chunk.end(), 0.25f);   // (frames behind n_frames: ordinary values that must not be read)
        for (int b = 0; b < 2; b++) memcpy(chunk.data() + (size_t)b * Tc * V, lp.data() + (size_t)done * (size_t)V, sizeof(float) * (size_t)n * (size_t)V);
        std::fill(out.begin(), out.end(), -7);
        std::fill(sout.begin(), sout.end(), -7);
        CtcPrefixBiasTables tabs[2] = {tb.view, tb.view};
        tabs[1].next = nullptr; tabs[1].bonus = nullptr; tabs[1].pending = nullptr;
        const int32_t nf[2] = {n, n};
        ctc_prefix_chunk_bias_ref(chunk.data(), 2, Tc, V, nf, beam, in.data(), out.data(), tabs, sin.data(), sout.data());
        hist.check_out(out.data(), sout.data(), Tc, n, tb.view.S, lm ? tb.view.S_lm : 0);
        hist.apply_out(out.data(), sout.data(), Tc, n);
        // the unbiased neighbour: every word of its out block is the plain resumed reference's
        plain.fill_in(pin.data(), Tc);
        std::fill(pout.begin(), pout.end(), -7);
        ctc_prefix_chunk_ref(chunk.data(), 1, Tc, V, &n, beam, pin.data(), pout.data());
        CHECK(memcmp(pout.data(), out.data() + L.out_ints(), sizeof(int) * (size_t)L.out_ints()) == 0);
        plain.apply_out(pout.data(), Tc, n);
        unbiased.apply_out(out.data() + L.out_ints(), Tc, n);
        CHECK(unbiased.tokens() == plain.tokens() && same_bits(unbiased.score(), plain.score()));
        done += n;
        CHECK(hist.frames() == done);
        CHECK(hist.live_nodes() <= (size_t)beam * (size_t)(hist.longest() + 1) + 1);
        const CtcPrefixBiasRefResult want = ctc_prefix_bias_ref(lp.data(), V, done, beam, tb.view);
        const std::vector<BeamAlt> got = hist.nbest(beam);
        CHECK(got.size() == want.hyps.size() && hist.slots().size() == want.hyps.size());
        bool reordered = false, pending = false;
        for (size_t i = 0; i < got.size(); i++) {
            const CtcPrefixBiasRefHyp& h = want.hyps[i];
            CHECK(got[i].tokens == h.h.tokens && got[i].timestamps == h.h.timestamps && got[i].token_log_probs.size() == h.h.token_log_probs.size());
            for (size_t u = 0; u < h.h.tokens.size(); u++) CHECK(same_bits(got[i].token_log_probs[u], h.h.token_log_probs[u]));
            CHECK(same_bits(got[i].score, h.final_score));
            const size_t q = (size_t)h.slot;   // the carried state, by slot: selection order, ctx with the pending bonus
            CHECK(hist.ord()[i] == h.slot && same_bits(hist.slots()[q].pb, h.h.pb) && same_bits(hist.slots()[q].pnb, h.h.pnb));
            CHECK(same_bits(hist.ctx()[q], h.ctx) && hist.hs()[q] == h.hs && hist.ls()[q] == h.ls && same_bits(hist.fin()[q], h.final_score));
            reordered = reordered || h.slot != (int)i;
            pending = pending || (hw && tb.view.pending[h.hs] != 0.f);
        }
        CHECK(hist.tokens() == want.hyps[0].h.tokens && hist.timestamps() == want.hyps[0].h.timestamps && same_bits(hist.score(), want.hyps[0].final_score));
        CHECK(hist.token_log_probs().size() == want.hyps[0].h.tokens.size());
        if (done < T) { pending_boundaries += pending; reordered_boundaries += reordered; }
    }
    hist.reset();
    CHECK(hist.frames() == 0 && hist.tokens().empty() && hist.live_nodes() == 1 && hist.score() == 0.f && !hist.lm_on() && hist.lm_serial() == 0);
    CHECK(hist.ctx().size() == 1 && hist.ctx()[0] == 0.f && hist.hs()[0] == 0 && hist.ls()[0] == 0 && hist.ord().empty());
}

// ---- 2. side blocks with states out of range ----------------------------------------------------------------------------------------
void side_block_checks() {
    const int K = 4;
    const CtcPrefixResumeBiasLayout SL{K};
    std::vector<int> side((size_t)SL.in_ints(), 0);
    side[0] = 1;
    ctc_prefix_bias_check_side_in(side.data(), K, 3, 5, 0);
    auto bad_in = [&](int off, int v, int S, int S_lm) {
        std::vector<int> b = side;
        b[(size_t)off] = v;
        return refused([&] { ctc_prefix_bias_check_side_in(b.data(), K, S, S_lm, 0); });
    };
    CHECK(bad_in(SL.in_hs(), 3, 3, 5) && bad_in(SL.in_hs() + 2, -1, 3, 5) && bad_in(SL.in_ls() + 1, 5, 3, 5) && bad_in(SL.in_ls(), -1, 3, 5));
    CHECK(bad_in(0, 2, 3, 5) && bad_in(0, 1, 3, 0) && bad_in(SL.in_hs(), 1, 0, 5));
    CHECK(!bad_in(SL.in_hs(), 2, 3, 5) && !bad_in(SL.in_ls(), 4, 3, 5));
    // the history: a side out block is checked before it is applied, the carried states before they are staged
    const int Tc = 2;
    const CtcPrefixResumeLayout L{K, Tc};
    CtcPrefixHistory h(K, K);
    h.begin_lm(7, true, 2);
    std::vector<int> in((size_t)L.in_ints()), out((size_t)L.out_ints(), 0), sin((size_t)SL.in_ints()), sout((size_t)SL.out_ints(), 0);
    CHECK(refused([&] { h.fill_side_in(sin.data(), 0, 2); }));   // the start state of the LM lies outside an LM of two states
    CHECK(refused([&] { h.fill_side_in(sin.data(), 0, 0); }));   // the stream runs an LM and none is given
    h.fill_side_in(sin.data(), 0, 3);
    CHECK(sin[0] == 1 && sin[(size_t)SL.in_ls()] == 2);
    h.fill_in(in.data(), Tc);
    const float lp[2 * 4] = {-1.f, -0.5f, -3.f, -0.75f, -1.f, -2.f, -3.f, -0.25f};
    CtcPrefixBiasTables none;
    const int32_t nf = 2;
    sin[0] = 0;
    ctc_prefix_chunk_bias_ref(lp, 1, Tc, 4, &nf, K, in.data(), out.data(), &none, sin.data(), sout.data());
    const int nh = out[0];
    CHECK(nh >= 2);
    auto bad_out = [&](int off, int v, int S, int S_lm) {
        std::vector<int> b = sout;
        b[(size_t)off] = v;
        return refused([&] { h.check_out(out.data(), b.data(), Tc, 2, S, S_lm); });
    };
    h.check_out(out.data(), sout.data(), Tc, 2, 3, 3);
    CHECK(bad_out(SL.out_hs(), 3, 3, 3) && bad_out(SL.out_hs() + 1, -1, 3, 3) && bad_out(SL.out_ls(), 3, 3, 3) && bad_out(SL.out_hs(), 1, 0, 3));
    CHECK(bad_out(SL.out_ord(), sout[(size_t)SL.out_ord() + 1], 3, 3) && bad_out(SL.out_ord() + 1, nh, 3, 3) && bad_out(SL.out_ord(), -1, 3, 3));
    CHECK(h.frames() == 0);
    h.apply_out(out.data(), sout.data(), Tc, 2);
    CHECK(h.frames() == 2 && (int)h.ord().size() == nh);
}

// ---- 3. the ABI ---------------------------------------------------------------------------------------------------------------------
struct Snap {
    std::vector<int64_t> tok;
    std::vector<int32_t> ts;
    float score = 0;
    int64_t frames = 0;
    bool operator==(const Snap& o) const { return tok == o.tok && ts == o.ts && same_bits(score, o.score) && frames == o.frames; }
};
Snap snap(const k2hip_ctc_prefix_stream_t* s) {
    Snap r;
    const int n = k2hip_ctc_prefix_stream_num_tokens(s);
    CHECK(n >= 0);
    r.tok.resize((size_t)n); r.ts.resize((size_t)n);
    OK(k2hip_ctc_prefix_stream_get_tokens(s, r.tok.data(), n));
    OK(k2hip_ctc_prefix_stream_get_timestamps(s, r.ts.data(), n));
    OK(k2hip_ctc_prefix_stream_get_score(s, &r.score));
    r.frames = k2hip_ctc_prefix_stream_num_frames(s);
    return r;
}

k2hip_ngram_lm_t* make_lm(int V) {
    std::vector<int64_t> ids;
    std::vector<int32_t> orders;
    std::vector<float> lps, bos;
    random_lm_entries(V, &ids, &orders, &lps, &bos);
    k2hip_ngram_lm_t* lm = nullptr;
    OK(k2hip_ngram_lm_create(ids.data(), orders.data(), lps.data(), bos.data(), (int64_t)orders.size(), V, &lm));
    return lm;
}

void abi(const char* ctc_path, const char* transducer_path) {
    k2hip_model_t *m = nullptr, *m2 = nullptr;
    OK(k2hip_model_create(ctc_path, nullptr, 0, &m));
    OK(k2hip_model_create(ctc_path, nullptr, 0, &m2));
    k2hip_model_info info;
    OK(k2hip_model_get_info(m, &info));
    const int V = info.vocab_size, Tc = 5, T = 15, B = 4;
    std::vector<float> rows((size_t)B * T * V);
    for (float& x : rows) x = -0.25f * (float)(rnd() % 40);
    auto chunk_of = [&](int t0) {
        std::vector<float> c((size_t)B * Tc * V);
        for (int r = 0; r < B; r++) memcpy(c.data() + (size_t)r * Tc * V, rows.data() + ((size_t)r * T + (size_t)t0) * V, sizeof(float) * (size_t)Tc * V);
        return c;
    };
    // phrases cut from what the unbiased search finds, so that matches do occur
    k2hip_ctc_prefix_stream_t* s[4] = {};
    for (auto& p : s) OK(k2hip_ctc_prefix_stream_create(m, 4, 4, &p));
    for (int t0 = 0; t0 < T; t0 += Tc) OK(k2hip_ctc_prefix_beam_search_chunk(m, s, B, chunk_of(t0).data(), Tc, nullptr));
    std::vector<Snap> unbiased;
    for (auto* p : s) unbiased.push_back(snap(p));
    CHECK(unbiased[0].tok.size() >= 3 && unbiased[1].tok.size() >= 3);
    const int64_t ph0[2] = {unbiased[0].tok[0], unbiased[0].tok[1]}, ph1[3] = {unbiased[1].tok[0], unbiased[1].tok[1], unbiased[1].tok[2]};
    const int32_t l0 = 2, l1 = 3;
    k2hip_hotwords_t *hw0 = nullptr, *hw1 = nullptr, *hw_small = nullptr;
    OK(k2hip_hotwords_create(ph0, &l0, 1, 1.5f, V, &hw0));
    OK(k2hip_hotwords_create(ph1, &l1, 1, 2.0f, V, &hw1));
    const int64_t ph_small[2] = {3, 4};
    OK(k2hip_hotwords_create(ph_small, &l0, 1, 1.5f, V - 1, &hw_small));
    // setters: only at the start state
    CHECK(k2hip_ctc_prefix_stream_set_hotwords(s[0], hw0) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "reset the stream first") != nullptr);
    CHECK(k2hip_ctc_prefix_stream_set_biasing(s[0], 1) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "reset the stream first") != nullptr);
    CHECK(k2hip_ctc_prefix_stream_set_hotwords(nullptr, hw0) == K2HIP_ERR_INVALID && k2hip_ctc_prefix_stream_set_biasing(nullptr, 1) == K2HIP_ERR_INVALID);
    CHECK(snap(s[0]) == unbiased[0]);
    for (auto* p : s) OK(k2hip_ctc_prefix_stream_reset(p));
    CHECK(k2hip_ctc_prefix_stream_set_hotwords(s[0], hw_small) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "vocab_size") != nullptr);
    // a graph attached with the switch off stays ignored, the launch stays the plain one
    OK(k2hip_ctc_prefix_stream_set_hotwords(s[0], hw0));
    OK(k2hip_ctc_prefix_stream_set_hotwords(s[2], hw0));   // shared between two streams
    OK(k2hip_ctc_prefix_stream_set_hotwords(s[1], hw1));
    const long long launches = ctc_prefix_bias_launch_count();
    for (int t0 = 0; t0 < T; t0 += Tc) OK(k2hip_ctc_prefix_beam_search_chunk(m, s, B, chunk_of(t0).data(), Tc, nullptr));
    for (int b = 0; b < B; b++) CHECK(snap(s[b]) == unbiased[(size_t)b]);
    CHECK(ctc_prefix_bias_launch_count() == launches);
    // switch on for 0 and 1 (different graphs); 2 keeps its graph ignored; 3 has none: a mixed call, in a different order
    for (auto* p : s) OK(k2hip_ctc_prefix_stream_reset(p));   // (a reset keeps the graph)
    OK(k2hip_ctc_prefix_stream_set_biasing(s[0], 1));
    OK(k2hip_ctc_prefix_stream_set_biasing(s[1], 7));
    OK(k2hip_hotwords_destroy(hw0));   // the streams keep the resident graph
    for (int t0 = 0; t0 < T; t0 += Tc) {
        OK(k2hip_ctc_prefix_beam_search_chunk(m, s, B, chunk_of(t0).data(), Tc, nullptr));
        if (t0 == 0) CHECK(k2hip_ctc_prefix_stream_set_biasing(s[0], 0) == K2HIP_ERR_INVALID);
    }
    CHECK(ctc_prefix_bias_launch_count() == launches + T / Tc);
    std::vector<Snap> biased;
    for (auto* p : s) biased.push_back(snap(p));
    CHECK(biased[2] == unbiased[2] && biased[3] == unbiased[3]);
    CHECK(biased[0].score > unbiased[0].score && biased[1].score > unbiased[1].score);   // both phrases are in their stream's best prefix
    // every alternative of a biased stream: finals descending
    for (int b = 0; b < 2; b++) {
        const int na = k2hip_ctc_prefix_stream_num_alternatives(s[b]);
        CHECK(na >= 1 && na <= 4);
        float prev = INFINITY;
        for (int i = 0; i < na; i++) {
            int32_t n = -1;
            float sc = 0;
            std::vector<int64_t> tok((size_t)T);
            OK(k2hip_ctc_prefix_stream_get_alternative(s[b], i, tok.data(), nullptr, nullptr, T, &n, &sc));
            CHECK(sc <= prev && (i > 0 || same_bits(sc, biased[(size_t)b].score)));
            prev = sc;
        }
    }
    // a reset keeps switch and graph: the same biased result again
    for (auto* p : s) OK(k2hip_ctc_prefix_stream_reset(p));
    for (int t0 = 0; t0 < T; t0 += Tc) OK(k2hip_ctc_prefix_beam_search_chunk(m, s, B, chunk_of(t0).data(), Tc, nullptr));
    for (int b = 0; b < B; b++) CHECK(snap(s[b]) == biased[(size_t)b]);
    // the LM rule: a biased stream keeps the setting of its first chunk; unbiased streams are not subject to it
    k2hip_ngram_lm_t* lm = make_lm(V);
    OK(k2hip_set_ngram_lm(m, lm, 0.5f));
    CHECK(k2hip_ctc_prefix_beam_search_chunk(m, s, B, chunk_of(0).data(), Tc, nullptr) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "reset the stream first") != nullptr);
    for (int b = 0; b < B; b++) CHECK(snap(s[b]) == biased[(size_t)b]);
    k2hip_ctc_prefix_stream_t* off_only[2] = {s[2], s[3]};
    std::vector<float> two((size_t)2 * Tc * V, -1.f);
    OK(k2hip_ctc_prefix_beam_search_chunk(m, off_only, 2, two.data(), Tc, nullptr));
    for (auto* p : s) OK(k2hip_ctc_prefix_stream_reset(p));
    OK(k2hip_ctc_prefix_stream_set_hotwords(s[3], nullptr));
    OK(k2hip_ctc_prefix_stream_set_biasing(s[3], 1));   // graph-free, switch on: the LM alone
    for (int t0 = 0; t0 < T; t0 += Tc) OK(k2hip_ctc_prefix_beam_search_chunk(m, s, B, chunk_of(t0).data(), Tc, nullptr));
    std::vector<Snap> with_lm;
    for (auto* p : s) with_lm.push_back(snap(p));
    CHECK(with_lm[2] == unbiased[2] && !(with_lm[3] == unbiased[3]) && !(with_lm[0] == biased[0]));
    OK(k2hip_set_ngram_lm(m, nullptr, 0.f));   // cleared mid-stream
    CHECK(k2hip_ctc_prefix_beam_search_chunk(m, s, B, chunk_of(0).data(), Tc, nullptr) == K2HIP_ERR_INVALID);
    for (int b = 0; b < B; b++) CHECK(snap(s[b]) == with_lm[(size_t)b]);
    OK(k2hip_ngram_lm_destroy(lm));
    // a stream of another model, a transducer model
    k2hip_ctc_prefix_stream_t* other = nullptr;
    OK(k2hip_ctc_prefix_stream_create(m2, 4, 4, &other));
    OK(k2hip_ctc_prefix_stream_set_hotwords(other, hw1));   // one handle, two models: an upload each
    OK(k2hip_ctc_prefix_stream_set_biasing(other, 1));
    std::vector<float> one((size_t)Tc * V, -1.f);
    OK(k2hip_ctc_prefix_beam_search_chunk(m2, &other, 1, one.data(), Tc, nullptr));
    // destroy orders: handle before streams, a stream before its model, a model before its stream
    OK(k2hip_hotwords_destroy(hw1));
    OK(k2hip_hotwords_destroy(hw_small));
    OK(k2hip_ctc_prefix_stream_destroy(s[0]));
    OK(k2hip_ctc_prefix_stream_destroy(s[2]));
    OK(k2hip_model_destroy(m2));
    OK(k2hip_ctc_prefix_stream_destroy(other));
    OK(k2hip_ctc_prefix_stream_destroy(s[1]));
    OK(k2hip_ctc_prefix_stream_destroy(s[3]));
    OK(k2hip_model_destroy(m));
    (void)transducer_path;
}

void recognizer(const char* streaming_path, const char* transducer_path) {
    k2hip_model_t *m = nullptr, *tr = nullptr;
    OK(k2hip_model_create(streaming_path, nullptr, 0, &m));
    OK(k2hip_model_create(transducer_path, nullptr, 0, &tr));
    k2hip_model_info info;
    OK(k2hip_model_get_info(m, &info));
    const int V = info.vocab_size;
    int32_t T = 0, shift = 0, Tp = 0;
    OK(k2hip_online_chunk_info(m, &T, &shift, &Tp));
    k2hip_online_stream_t *a = nullptr, *b = nullptr, *g = nullptr;
    OK(k2hip_online_stream_create(m, &a));
    OK(k2hip_online_stream_create(m, &b));
    OK(k2hip_online_stream_create(m, &g));
    for (k2hip_online_stream_t* st : {a, b, g}) OK(k2hip_online_stream_set_ctc_prefix_beam(st, 4, 4));
    std::vector<float> feats((size_t)(T + 2 * shift) * (size_t)info.feature_dim);
    for (size_t i = 0; i < feats.size(); i++) feats[i] = -3.f + 0.125f * (float)(i % 41);
    auto feed = [&] { for (k2hip_online_stream_t* st : {a, b, g}) OK(k2hip_online_stream_accept_features(st, feats.data(), T + 2 * shift)); };
    auto result = [&](k2hip_online_stream_t* st) {
        Snap r;
        const int n = k2hip_online_stream_num_tokens(st), nt = k2hip_online_stream_num_timestamps(st);
        CHECK(n == nt + 2);
        r.tok.resize((size_t)n); r.ts.resize((size_t)nt + 1);
        OK(k2hip_online_stream_get_tokens(st, r.tok.data(), n));
        OK(k2hip_online_stream_get_timestamps(st, r.ts.data(), nt));
        r.ts.resize((size_t)nt);
        OK(k2hip_online_stream_get_score(st, &r.score));
        return r;
    };
    int32_t dec[3], nn[3];
    k2hip_online_stream_t* all[3] = {a, b, g};
    feed();
    for (int tick = 0; tick < 3; tick++) OK(k2hip_online_step(m, all, 3, dec, nn));
    const Snap plain = result(a);
    CHECK(plain.tok.size() >= 5 && result(b) == plain);
    const int64_t ph[2] = {plain.tok[2], plain.tok[3]};
    const int32_t len = 2;
    k2hip_hotwords_t* hw = nullptr;
    OK(k2hip_hotwords_create(ph, &len, 1, 1.5f, V, &hw));
    CHECK(k2hip_online_stream_set_ctc_prefix_biasing(a, 1) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "reset the stream first") != nullptr);
    CHECK(k2hip_online_stream_set_ctc_prefix_biasing(nullptr, 1) == K2HIP_ERR_INVALID);
    k2hip_online_stream_t* trs = nullptr;
    OK(k2hip_online_stream_create(tr, &trs));
    CHECK(k2hip_online_stream_set_ctc_prefix_biasing(trs, 1) == K2HIP_ERR_UNSUPPORTED && strstr(k2hip_last_error(), "CTC") != nullptr);
    OK(k2hip_online_stream_destroy(trs));
    for (k2hip_online_stream_t* st : all) OK(k2hip_online_stream_reset(st));
    OK(k2hip_online_stream_set_hotwords(a, hw));
    OK(k2hip_online_stream_set_hotwords(b, hw));     // attached, switch off: ignored
    OK(k2hip_online_stream_set_ctc_prefix_biasing(a, 1));
    OK(k2hip_hotwords_destroy(hw));
    feed();
    for (int tick = 0; tick < 3; tick++) {
        OK(k2hip_online_step(m, all, 3, dec, nn));
        CHECK(dec[0] == 1 && dec[1] == 1 && dec[2] == 1);
    }
    CHECK(result(b) == plain && result(g) == plain);
    const Snap biased = result(a);
    CHECK(biased.score > plain.score);   // the phrase is in the best prefix: its bonus is in the reported final
    CHECK(k2hip_online_stream_num_alternatives(a) >= 1);
    // the LM rule at the recognizer level; a reset keeps the switch and the graph
    k2hip_ngram_lm_t* lm = make_lm(V);
    OK(k2hip_set_ngram_lm(m, lm, 0.5f));
    feed();
    const int64_t before = k2hip_online_stream_speech_length(a);
    CHECK(k2hip_online_step(m, all, 3, dec, nn) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "reset the stream first") != nullptr);
    CHECK(k2hip_online_stream_speech_length(a) == before && result(a) == biased && result(b) == plain);
    k2hip_online_stream_t* off_only[2] = {b, g};
    OK(k2hip_online_step(m, off_only, 2, dec, nn));   // streams with the switch off are not subject to the rule
    OK(k2hip_set_ngram_lm(m, nullptr, 0.f));
    OK(k2hip_ngram_lm_destroy(lm));
    for (k2hip_online_stream_t* st : all) OK(k2hip_online_stream_reset(st));
    feed();
    for (int tick = 0; tick < 3; tick++) OK(k2hip_online_step(m, all, 3, dec, nn));
    CHECK(result(a) == biased && result(b) == plain);
    for (k2hip_online_stream_t* st : all) OK(k2hip_online_stream_destroy(st));
    OK(k2hip_model_destroy(m));
    OK(k2hip_model_destroy(tr));
}

}  // namespace

int main(int argc, char** argv) {
    int cases = 0;
    for (int round = 0; round < 60; round++)
        for (int kind = 0; kind < 3; kind++) {
            const int V = 3 + (int)(rnd() % 7), T = 1 + (int)(rnd() % 24), beam = 1 + (int)(rnd() % 8);
            chunked_case(V, T, beam, kind != 1, kind != 0);
            cases++;
        }
    CHECK(pending_boundaries >= 10 && reordered_boundaries >= 10);   // the random cases do cross boundaries in the ways that matter
    side_block_checks();
    if (argc >= 3) abi(argv[1], argv[2]);
    else fprintf(stderr, "san_ctc_prefix_stream_bias_driver: no model files given, the ABI part is skipped\n");
    if (argc >= 4) recognizer(argv[3], argv[2]);
    printf("san_ctc_prefix_stream_bias_driver ok (%d cases, %lld pending and %lld reordered boundaries)\n", cases, pending_boundaries, reordered_boundaries);
    return 0;
}
