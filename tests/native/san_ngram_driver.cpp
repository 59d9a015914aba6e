// The n-gram LM's host code (csrc/ngram_lm.cpp: the text ARPA parser and the back-off automaton) under AddressSanitizer / UBSan.
// TEST INFRASTRUCTURE (`make -C k2transducerasr_amd/csrc san`, tests/test_ngram_sanitizers.py).  No engine, no GPU.
//
//   san_ngram_driver
//
// A valid file is parsed and walked at random; then every truncation of it and seeded byte mutations go through the parser: each
// either gives an LM that can be walked from every state, or a k2hip::Error -- never a crash, an out-of-bounds read or an overflow.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <string>

#include "../../k2transducerasr_amd/csrc/errors.h"
#include "../../k2transducerasr_amd/csrc/ngram_lm.h"

using namespace k2hip;

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                    \
        }                                                                \
    } while (0)

static const char* kArpa =
    "\\data\\\nngram 1=8\nngram 2=4\nngram 3=2\n\n"
    "\\1-grams:\n-2.0\t<unk>\n-99\t<s>\t-0.5\n-1.0\t</s>\n-1.5\tA\t-0.25\n-2.0\tB\t-0.3\n-2.5\tC\t-0.1\n-1.75\tD\n-3\tE\t-0.2\n\n"
    "\\2-grams:\n-0.5\t<s> A\t-0.1\n-0.25\tA B\t-0.2\n-0.4\tB C\n-0.6\tB </s>\n\n"
    "\\3-grams:\n-0.1\t<s> A B\n-0.2\tA B C\n\n\\end\\\n";

// walks the automaton from every state with every token, then a long random walk; sums what it sees so nothing is optimised away
static double exercise(const NgramLm& lm, std::mt19937& rng) {
    double sum = 0;
    for (int s = 0; s < lm.num_states(); s++)
        for (int v = 0; v < lm.vocab_size(); v++) {
            int n = -1;
            float lp = 0;
            lm.step(s, v, &n, &lp);
            if (n < 0 || n >= lm.num_states()) abort();
            sum += lp;
        }
    int s = lm.start_state();
    for (int i = 0; i < 2000; i++) {
        float lp = 0;
        lm.step(s, (int)(rng() % (unsigned)lm.vocab_size()), &s, &lp);
        sum += lp;
    }
    NgramDeviceForm d;
    lm.device_form(0.5f, &d);
    for (size_t i = 0; i < d.states.size(); i += 4) {
        if (d.states[i] < 0 || d.states[i + 1] < d.states[i] || (size_t)d.states[i + 1] > d.arc_tok.size()) abort();
        if (d.states[i + 2] < 0 || d.states[i + 2] >= lm.num_states()) abort();
    }
    for (int32_t n : d.arc_next)
        if (n < 0 || n >= lm.num_states()) abort();
    for (int32_t n : d.uni_next)
        if (n < 0 || n >= lm.num_states()) abort();
    return sum;
}

int main() {
    const std::map<std::string, int> id_of{{"<blk>", 0}, {"<sos/eos>", 1}, {"<unk2>", 2}, {"A", 3}, {"B", 4}, {"C", 5}, {"D", 6}, {"E", 7}};
    const int V = 8;
    std::mt19937 rng(12345);
    const std::string good(kArpa);
    double sink = 0;
    {
        std::unique_ptr<NgramLm> lm(ngram_parse_arpa(good.data(), good.size(), id_of, V, "good"));
        CHECK(lm->order() == 3 && lm->start_state() == 1 && lm->num_arcs() == 5 + 3 + 2);
        sink += exercise(*lm, rng);
    }
    int parsed = 0, refused = 0;
    auto attempt = [&](const std::string& text) {
        // (an exact-size heap copy: a read past the end is a report, not a lucky zero)
        std::unique_ptr<char[]> buf(new char[text.size() ? text.size() : 1]);
        std::copy(text.begin(), text.end(), buf.get());
        try {
            std::unique_ptr<NgramLm> lm(ngram_parse_arpa(buf.get(), text.size(), id_of, V, "mutant"));
            sink += exercise(*lm, rng);
            parsed++;
        } catch (const Error& e) {
            if (e.code != K2HIP_ERR_INVALID) abort();
            refused++;
        }
    };
    for (size_t n = 0; n < good.size(); n++) attempt(good.substr(0, n));
    const char alphabet[] = "\\\n\t -=0123456789.eE<>/sABCZ:gramsdtun";
    for (int i = 0; i < 4000; i++) {
        std::string m = good;
        const int edits = 1 + (int)(rng() % 3);
        for (int e = 0; e < edits; e++) {
            const size_t at = rng() % m.size();
            switch (rng() % 3) {
                case 0: m[at] = alphabet[rng() % (sizeof alphabet - 1)]; break;
                case 1: m.erase(at, 1 + rng() % 4); break;
                default: m.insert(at, 1, alphabet[rng() % (sizeof alphabet - 1)]); break;
            }
            if (m.empty()) m = "x";
        }
        attempt(m);
    }
    CHECK(refused > 1000 && parsed > 50);
    // the array form's own checks
    {
        const int64_t ids[] = {3, 3, 4, kNgramUnk};
        const int32_t orders[] = {1, 2, 1};
        const float lps[] = {-1.f, -0.5f, -2.f}, bos[] = {-0.1f, 0.f, 0.f};
        try {
            NgramLm lm(ids, orders, lps, bos, 2, V);   // (3, 4) has its history, but 4 has no unigram and there is no <unk>
            CHECK(false);
        } catch (const Error&) {
        }
        const int32_t orders2[] = {1, 2, 1};
        const int64_t ids2[] = {3, 3, 3, kNgramUnk};
        NgramLm lm(ids2, orders2, lps, bos, 3, V);
        sink += exercise(lm, rng);
    }
    printf("san_ngram_driver: ok (%d mutants parsed, %d refused, sink %g)\n", parsed, refused, sink);
    return 0;
}
