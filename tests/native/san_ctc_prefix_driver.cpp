// AddressSanitizer / UBSan driver of the CTC prefix beam search's host side: the header-only reference (csrc/ctc_prefix_ref.h) and the
// argument checks of k2hip_ctc_prefix_beam_search and k2hip_set_decoding_method("ctc_prefix_beam_search") / k2hip_set_nbest
// (csrc/api.cpp) over the CPU stand-ins of the engine (engine_stub*.cpp).  TEST INFRASTRUCTURE: its own program
// (`make -C k2transducerasr_amd/csrc san_ctc_prefix`, tests/test_ctc_prefix.py), never loaded into another process.
// Exercised: the reference against brute-force enumeration of every frame labelling (V = 3, T <= 6, a beam that prunes nothing: every
// surviving prefix's pb / pnb / score is its full sum), -inf cells and an all -inf row; the three tie rules and `a a`; the fold rule
// on a re-spelled prefix (a small-vocabulary search until the reference counts one: the N-best stays pairwise distinct); then,
// through the ABI: beam, nbest, n_frames and R out of range, max_tokens too small (nothing written), NULL arguments, a transducer
// model, the method / N-best rules of a CTC handle, and a valid call after every refused one.
//   san_ctc_prefix_driver <ctc.k2w> <offline.k2w>
//   san_ctc_prefix_driver row <file>      one row through ctc_prefix_ref.h, printed for tests/test_ctc_prefix_tie_cases_ref.py: the file
//                                         holds the text line "V T beam" and then T x V raw float32 values.  Per frame a line
//                                         "picks t i0 i1 ..." (the selected flat indexes in rank order), per surviving hypothesis a line
//                                         "hyp i score-bits n tok0 .. | ts0 .. | token-log-prob-bits0 .." (bits as unsigned decimals)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../../include/k2hip.h"
#include "../../k2transducerasr_amd/csrc/ctc_prefix_ref.h"

#define CHECK(cond)                                                                                                          \
    do {                                                                                                                     \
        if (!(cond)) {                                                                                                       \
            fprintf(stderr, "CHECK failed at %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, k2hip_last_error()); \
            exit(3);                                                                                                         \
        }                                                                                                                    \
    } while (0)
#define OK(call) CHECK((call) == K2HIP_OK)

namespace {

using k2hip::ctc_prefix_ref;
using k2hip::CtcPrefixRefResult;

unsigned long long rng_state = 88172645463325252ull;
unsigned rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 32);
}

double lae(double a, double b) {
    if (a == -INFINITY) return b;
    if (b == -INFINITY) return a;
    const double m = a > b ? a : b;
    return m + std::log(std::exp(a - m) + std::exp(b - m));
}

bool close_to(float got, double want) {
    if (want == -INFINITY) return got == -INFINITY;
    return std::fabs((double)got - want) <= 1e-5 * std::fmax(1.0, std::fabs(want));
}

// every labelling of T frames over 3 symbols: collapsed prefix -> (sum over paths ending in blank, ending in the last token)
void brute_case(int T, int inf_per_16) {
    constexpr int V = 3;
    std::vector<float> lp((size_t)T * V);
    for (float& x : lp) x = (int)(rnd() % 16) < inf_per_16 ? -INFINITY : -0.25f * (float)(rnd() % 24);
    std::map<std::vector<int64_t>, std::pair<double, double>> acc;
    int n = 1;
    for (int t = 0; t < T; t++) n *= V;
    for (int code = 0; code < n; code++) {
        std::vector<int64_t> got;
        double s = 0;
        int64_t prev = -1, last = 0;
        for (int t = 0, c = code; t < T; t++, c /= V) {
            const int64_t v = c % V;
            s += lp[(size_t)t * V + (size_t)v];
            if (v != 0 && v != prev) got.push_back(v);
            prev = v;
            last = v;
        }
        auto it = acc.emplace(got, std::make_pair(-INFINITY, -INFINITY)).first;
        (last == 0 ? it->second.first : it->second.second) = lae(last == 0 ? it->second.first : it->second.second, s);
    }
    const CtcPrefixRefResult r = ctc_prefix_ref(lp.data(), V, T, V, 1000);   // nothing is pruned
    size_t finite = 0;
    for (const auto& kv : acc) finite += lae(kv.second.first, kv.second.second) > -INFINITY;
    CHECK(r.respelled_folds == 0);   // (nothing leaves a beam that prunes nothing)
    if (finite == 0) {
        CHECK(r.hyps.size() == 1 && r.hyps[0].tot == -INFINITY);
        return;
    }
    CHECK(r.hyps.size() == finite);
    for (size_t i = 0; i < r.hyps.size(); i++) {
        const auto& h = r.hyps[i];
        const auto it = acc.find(h.tokens);
        CHECK(it != acc.end());
        CHECK(!std::isnan(h.tot) && close_to(h.pb, it->second.first) && close_to(h.pnb, it->second.second));
        CHECK(close_to(h.tot, lae(it->second.first, it->second.second)));
        if (i) CHECK(r.hyps[i - 1].tot >= h.tot && r.hyps[i - 1].tokens != h.tokens);
        CHECK(h.timestamps.size() == h.tokens.size() && h.token_log_probs.size() == h.tokens.size());
        for (size_t u = 0; u < h.tokens.size(); u++) {
            CHECK(h.timestamps[u] >= 0 && h.timestamps[u] < T && (u == 0 || h.timestamps[u - 1] < h.timestamps[u]));
            CHECK(h.token_log_probs[u] == lp[(size_t)h.timestamps[u] * V + (size_t)h.tokens[u]]);
        }
    }
}

void rules() {
    const float ninf = -INFINITY;
    using Tok = std::vector<int64_t>;
    {   // equal tokens: the lower id wins (columns: blank, a, b)
        const float lp[3] = {-4.f, -0.5f, -0.5f};
        const CtcPrefixRefResult r = ctc_prefix_ref(lp, 3, 1, 3, 2);
        CHECK(r.hyps.size() == 2 && r.hyps[0].tokens == Tok{1} && r.hyps[1].tokens == Tok{2} && r.hyps[0].tot == -0.5f);
    }
    {   // stay against extension: stay (flat index 0) wins
        const float lp[3] = {-0.5f, -0.5f, -4.f};
        const CtcPrefixRefResult r = ctc_prefix_ref(lp, 3, 1, 3, 1);
        CHECK(r.hyps.size() == 1 && r.hyps[0].tokens.empty() && r.hyps[0].tot == -0.5f);
    }
    {   // equal candidates of two slots: the lower slot wins.  After frame 0 the slots are [a] (-0.25) and [] (-0.25 -- blank ties
        // with a, the stay has the lower index: slot 0 = [], slot 1 = [a]); frame 1: [] + b = -0.25 + -1 and [a] + b = the same.
        const float lp[6] = {-0.25f, -0.25f, -8.f, -8.f, -8.f, -1.f};
        const CtcPrefixRefResult r = ctc_prefix_ref(lp, 3, 2, 3, 2);
        CHECK(r.hyps.size() == 2 && r.hyps[0].tokens == Tok{2} && (r.hyps[1].tokens == Tok{1, 2}) && r.hyps[0].tot == r.hyps[1].tot);
    }
    {   // a a: peaky a, blank, a gives [a, a] at frames 0 and 2; peaky a, a, a gives [a] at frame 0
        const float aba[9] = {-20.f, 0.f, -20.f, 0.f, -20.f, -20.f, -20.f, 0.f, -20.f};
        CtcPrefixRefResult r = ctc_prefix_ref(aba, 3, 3, 3, 4);
        CHECK(r.hyps[0].tokens == (Tok{1, 1}) && r.hyps[0].timestamps == (std::vector<int32_t>{0, 2}));
        const float aaa[9] = {-20.f, 0.f, -20.f, -20.f, 0.f, -20.f, -20.f, 0.f, -20.f};
        r = ctc_prefix_ref(aaa, 3, 3, 3, 4);
        CHECK(r.hyps[0].tokens == Tok{1} && r.hyps[0].timestamps == std::vector<int32_t>{0} && r.hyps[0].token_log_probs[0] == 0.f);
    }
    {   // all -inf: the empty prefix survives with score -inf; -inf from frame 1 on: slot 0 stays what it was
        const float lp[6] = {ninf, ninf, ninf, ninf, ninf, ninf};
        CtcPrefixRefResult r = ctc_prefix_ref(lp, 3, 2, 3, 4);
        CHECK(r.hyps.size() == 1 && r.hyps[0].tokens.empty() && r.hyps[0].tot == ninf);
        const float lp2[6] = {-4.f, -0.5f, -1.f, ninf, ninf, ninf};
        r = ctc_prefix_ref(lp2, 3, 2, 3, 4);
        CHECK(r.hyps.size() == 1 && r.hyps[0].tokens == Tok{1} && r.hyps[0].tot == ninf && r.hyps[0].timestamps[0] == 0);
    }
}

// a re-spelled prefix: small vocabularies until the reference counts one; the survivors stay pairwise distinct throughout
void respelled() {
    long long found = 0;
    for (int trial = 0; trial < 400; trial++) {
        const int V = 3 + (int)(rnd() % 2), T = 6 + (int)(rnd() % 5), beam = 3 + (int)(rnd() % 6);
        std::vector<float> lp((size_t)T * V);
        for (float& x : lp) x = -0.125f * (float)(1 + rnd() % 48);
        const CtcPrefixRefResult r = ctc_prefix_ref(lp.data(), V, T, V, beam);
        found += r.respelled_folds;
        CHECK((int)r.hyps.size() <= beam);
        for (size_t i = 0; i < r.hyps.size(); i++)
            for (size_t j = i + 1; j < r.hyps.size(); j++) CHECK(r.hyps[i].tokens != r.hyps[j].tokens);
    }
    CHECK(found > 0);
}

void abi(const char* ctc_path, const char* transducer_path) {
    k2hip_model_t* m = nullptr;
    OK(k2hip_model_create(ctc_path, nullptr, 0, &m));
    k2hip_model_info info;
    OK(k2hip_model_get_info(m, &info));
    const int Vm = info.vocab_size, R = 2, Tp = 6, mt = 6, beam = 4, nbest = 3;
    CHECK(Vm > 8);
    std::vector<float> lp((size_t)R * Tp * Vm);
    for (float& x : lp) x = -0.25f * (float)(1 + rnd() % 12);
    int32_t nf[2] = {6, 3};
    const size_t NB = (size_t)R * nbest;
    std::vector<int64_t> tok(NB * mt, -7);
    std::vector<int32_t> ts(NB * mt, -7), n(NB, -7), nh(R, -7);
    std::vector<float> yp(NB * mt, -7.f), sc(NB, -7.f);
    auto untouched = [&] { return tok[0] == -7 && ts[0] == -7 && yp[0] == -7.f && n[0] == -7 && nh[1] == -7 && sc[0] == -7.f; };
    auto wipe = [&] {
        std::fill(tok.begin(), tok.end(), -7); std::fill(ts.begin(), ts.end(), -7); std::fill(n.begin(), n.end(), -7);
        std::fill(nh.begin(), nh.end(), -7); std::fill(yp.begin(), yp.end(), -7.f); std::fill(sc.begin(), sc.end(), -7.f);
    };
    auto call = [&](int rows, int frames, const int32_t* n_frames, int k, int nb, int max_tokens) {
        return k2hip_ctc_prefix_beam_search(m, lp.data(), rows, frames, n_frames, k, nb, tok.data(), ts.data(), yp.data(), n.data(), nh.data(), sc.data(),
                                            max_tokens);
    };
    auto valid = [&] {
        OK(call(R, Tp, nf, beam, nbest, mt));
        const CtcPrefixRefResult r1 = ctc_prefix_ref(lp.data() + (size_t)Tp * Vm, Vm, 3, Vm, beam);
        CHECK(nh[0] == nbest && nh[1] == nbest && sc[0] >= sc[1] && sc[1] >= sc[2]);
        for (int i = 0; i < nbest; i++) {
            const auto& h = r1.hyps[(size_t)i];
            const size_t en = (size_t)nbest + (size_t)i;
            CHECK(n[en] == (int32_t)h.tokens.size() && sc[en] == h.tot);
            for (size_t u = 0; u < h.tokens.size(); u++)
                CHECK(tok[en * mt + u] == h.tokens[u] && ts[en * mt + u] == h.timestamps[u] && ts[en * mt + u] < 3 && yp[en * mt + u] == h.token_log_probs[u]);
            CHECK(h.tokens.size() == (size_t)mt || tok[en * mt + h.tokens.size()] == -7);
        }
        wipe();
    };
    valid();
    for (int bad : {0, 9, -1}) {
        CHECK(call(R, Tp, nf, bad, 1, mt) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "beam") != nullptr && untouched());
        valid();
    }
    for (int bad : {0, beam + 1}) {
        CHECK(call(R, Tp, nf, beam, bad, mt) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "nbest") != nullptr && untouched());
        valid();
    }
    for (int32_t bad : {0, 7}) {
        int32_t nf_bad[2] = {6, bad};
        CHECK(call(R, Tp, nf_bad, beam, nbest, mt) == K2HIP_ERR_INVALID && strstr(k2hip_last_error(), "n_frames") != nullptr && untouched());
        valid();
    }
    for (int bad : {0, 65536}) CHECK(call(bad, Tp, nullptr, beam, nbest, mt) == K2HIP_ERR_INVALID && untouched());   // (decided before anything is read)
    CHECK(call(R, 0, nullptr, beam, nbest, mt) == K2HIP_ERR_INVALID && untouched());
    CHECK(call(R, Tp, nf, beam, nbest, 0) == K2HIP_ERR_INVALID && untouched());
    valid();
    {   // max_tokens below an entry's length: K2HIP_ERR_CAPACITY.  Peaky rows spell a b a b a b
        std::vector<float> peaky((size_t)R * Tp * Vm, -20.f);
        for (int r = 0; r < R; r++)
            for (int t = 0; t < Tp; t++) peaky[((size_t)r * Tp + (size_t)t) * Vm + (size_t)(3 + t % 2)] = 0.f;
        CHECK(k2hip_ctc_prefix_beam_search(m, peaky.data(), R, Tp, nullptr, beam, 1, tok.data(), ts.data(), yp.data(), n.data(), nh.data(), sc.data(), 5) ==
              K2HIP_ERR_CAPACITY && untouched());
        OK(k2hip_ctc_prefix_beam_search(m, peaky.data(), R, Tp, nullptr, beam, 1, tok.data(), ts.data(), yp.data(), n.data(), nh.data(), sc.data(), 6));
        CHECK(n[0] == 6 && tok[0] == 3 && tok[5] == 4 && ts[5] == 5 && nh[0] == 1);
        wipe();
    }
    OK(call(R, Tp, nullptr, 1, 1, mt));   // n_frames NULL = T'; beam 1
    CHECK(nh[0] == 1 && nh[1] == 1);
    wipe();
    CHECK(k2hip_ctc_prefix_beam_search(nullptr, lp.data(), R, Tp, nf, beam, nbest, tok.data(), ts.data(), yp.data(), n.data(), nh.data(), sc.data(), mt) == K2HIP_ERR_INVALID);
    CHECK(k2hip_ctc_prefix_beam_search(m, nullptr, R, Tp, nf, beam, nbest, tok.data(), ts.data(), yp.data(), n.data(), nh.data(), sc.data(), mt) == K2HIP_ERR_INVALID);
    CHECK(k2hip_ctc_prefix_beam_search(m, lp.data(), R, Tp, nf, beam, nbest, nullptr, ts.data(), yp.data(), n.data(), nh.data(), sc.data(), mt) == K2HIP_ERR_INVALID);
    CHECK(k2hip_ctc_prefix_beam_search(m, lp.data(), R, Tp, nf, beam, nbest, tok.data(), ts.data(), yp.data(), n.data(), nullptr, sc.data(), mt) == K2HIP_ERR_INVALID && untouched());
    valid();
    // the method and the N-best setting of a CTC handle
    CHECK(k2hip_set_nbest(m, 2) == K2HIP_ERR_UNSUPPORTED);                              // greedy_search: as before
    OK(k2hip_set_decoding_method(m, "modified_beam_search", 4));
    CHECK(k2hip_set_nbest(m, 2) == K2HIP_ERR_UNSUPPORTED);                              // modified_beam_search: as before
    for (int bad : {0, 9}) CHECK(k2hip_set_decoding_method(m, "ctc_prefix_beam_search", bad) == K2HIP_ERR_INVALID);
    CHECK(k2hip_set_nbest(m, 2) == K2HIP_ERR_UNSUPPORTED);                              // a refused setting set nothing
    OK(k2hip_set_decoding_method(m, "ctc_prefix_beam_search", 4));
    CHECK(k2hip_set_nbest(m, 5) == K2HIP_ERR_INVALID);                                  // above the beam
    OK(k2hip_set_nbest(m, 4));
    CHECK(k2hip_set_decoding_method(m, "ctc_prefix_beam_search", 2) == K2HIP_ERR_INVALID);   // a beam below the list kept
    OK(k2hip_set_decoding_method(m, "ctc_prefix_beam_search", 8));
    valid();                                                                            // the operator entry is independent of both
    OK(k2hip_set_decoding_method(m, "greedy_search", 0));                               // leaving resets the list to 1
    CHECK(k2hip_set_nbest(m, 2) == K2HIP_ERR_UNSUPPORTED);
    OK(k2hip_set_nbest(m, 1));
    OK(k2hip_set_decoding_method(m, "ctc_prefix_beam_search", 4));
    OK(k2hip_set_nbest(m, 2));
    OK(k2hip_set_decoding_method(m, "modified_beam_search", 4));
    CHECK(k2hip_set_nbest(m, 2) == K2HIP_ERR_UNSUPPORTED);
    CHECK(k2hip_set_decoding_method(m, "no_such_search", 4) == K2HIP_ERR_UNSUPPORTED);
    OK(k2hip_set_decoding_method(m, "greedy_search", 0));
    OK(k2hip_model_destroy(m));
    // a transducer model has no CTC head: both entries refuse it
    k2hip_model_t* tr = nullptr;
    OK(k2hip_model_create(transducer_path, nullptr, 0, &tr));
    k2hip_model_info ti;
    OK(k2hip_model_get_info(tr, &ti));
    std::vector<float> tlp((size_t)R * Tp * (size_t)ti.vocab_size, -1.f);
    CHECK(k2hip_ctc_prefix_beam_search(tr, tlp.data(), R, Tp, nf, beam, nbest, tok.data(), ts.data(), yp.data(), n.data(), nh.data(), sc.data(), mt) ==
              K2HIP_ERR_UNSUPPORTED && untouched());
    CHECK(k2hip_set_decoding_method(tr, "ctc_prefix_beam_search", 4) == K2HIP_ERR_UNSUPPORTED);
    OK(k2hip_set_decoding_method(tr, "modified_beam_search", 4));
    OK(k2hip_set_nbest(tr, 2));   // a transducer's N-best is untouched
    OK(k2hip_model_destroy(tr));
}

unsigned bits_of(float x) {
    unsigned u;
    memcpy(&u, &x, sizeof u);
    return u;
}

// the whole-row search stepped frame by frame (the fold table of ctc_prefix_ref: token lists compared), so that every frame's picks show:
// a new slot's flat index is (the slot it came from) V + (the token it appended, 0 for a stay); the result must be ctc_prefix_ref's
int row_from_file(const char* path) {
    FILE* f = fopen(path, "rb");
    CHECK(f != nullptr);
    int V = 0, T = 0, beam = 0;
    CHECK(fscanf(f, "%d %d %d", &V, &T, &beam) == 3 && fgetc(f) == '\n');
    CHECK(V >= 1 && V <= 100000 && T >= 1 && T <= 100000 && beam >= 1 && beam <= 64);
    std::vector<float> lp((size_t)T * (size_t)V);
    CHECK(fread(lp.data(), sizeof(float), lp.size(), f) == lp.size());
    fclose(f);
    std::vector<k2hip::CtcPrefixRefSlot> cur(1);
    cur[0].h.pb = 0.f; cur[0].h.pnb = -INFINITY; cur[0].h.tot = 0.f;
    long long next_node = 0;
    for (int t = 0; t < T; t++) {
        const int n = (int)cur.size();
        std::vector<int> fold_par((size_t)n, -1);
        for (int j = 0; j < n; j++) {
            cur[(size_t)j].origin = j;
            for (int k = 0; k < n; k++) {
                const auto &tj = cur[(size_t)j].h.tokens, &tk = cur[(size_t)k].h.tokens;
                if (j != k && tj.size() == tk.size() + 1 && std::equal(tk.begin(), tk.end(), tj.begin())) fold_par[(size_t)j] = k;
            }
        }
        std::vector<k2hip::CtcPrefixRefSlot> nxt = k2hip::ctc_prefix_ref_frame(cur, fold_par, lp.data() + (size_t)t * (size_t)V, t, V, beam, &next_node);
        printf("picks %d", t);
        for (const auto& s : nxt) {
            const bool grew = s.h.tokens.size() > cur[(size_t)s.origin].h.tokens.size();
            printf(" %lld", (long long)s.origin * V + (grew ? (long long)s.h.tokens.back() : 0));
        }
        printf("\n");
        cur = std::move(nxt);
    }
    const CtcPrefixRefResult r = ctc_prefix_ref(lp.data(), V, T, V, beam);
    CHECK(r.hyps.size() == cur.size());
    for (size_t i = 0; i < r.hyps.size(); i++) {
        const auto& h = r.hyps[i];
        CHECK(h.tokens == cur[i].h.tokens && h.timestamps == cur[i].h.timestamps && bits_of(h.tot) == bits_of(cur[i].h.tot));
        printf("hyp %zu %u %zu", i, bits_of(h.tot), h.tokens.size());
        for (int64_t v : h.tokens) printf(" %lld", (long long)v);
        printf(" |");
        for (int32_t x : h.timestamps) printf(" %d", x);
        printf(" |");
        for (float x : h.token_log_probs) printf(" %u", bits_of(x));
        printf("\n");
    }
    printf("san_ctc_prefix_driver row ok\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 3 && strcmp(argv[1], "row") == 0) return row_from_file(argv[2]);
    for (int T = 1; T <= 6; T++)
        for (int inf : {0, 0, 0, 2, 6, 16}) brute_case(T, inf);
    rules();
    respelled();
    if (argc >= 3) abi(argv[1], argv[2]);
    else fprintf(stderr, "san_ctc_prefix_driver: no model files given, the ABI part is skipped\n");
    printf("san_ctc_prefix_driver ok\n");
    return 0;
}
