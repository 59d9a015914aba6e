// Back-off n-gram LM (ngram_lm.h): the automaton, the host walk, the scaled sparse device form and the text ARPA parser.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "errors.h"
#include "ngram_lm.h"

namespace k2hip {
namespace {

using Key = std::vector<int>;
struct Entry {
    float lp, bo;
    bool arc;   // false: kept only as a history's own entry (<s>, or an ignored </s> / <s> prediction)
    int num;
};
struct Arc {
    int s, tok;
    float lp;
    int next;
};

}  // namespace

NgramLm::NgramLm(const int64_t* ids, const int32_t* orders, const float* log_probs, const float* backoffs, int64_t n_entries, int vocab_size,
                 const char* noun, const int* numbers)
    : V_(vocab_size) {
    K2_REQUIRE(n_entries >= 0, "ngram lm: %lld entries", (long long)n_entries);
    K2_REQUIRE(vocab_size > K2HIP_UNK_ID, "ngram lm: vocab_size %d", vocab_size);
    K2_REQUIRE(n_entries == 0 || (ids && orders && log_probs && backoffs), "ngram lm: null entry arrays");
    if (n_entries > kNgramMaxArcs)
        failf(K2HIP_ERR_INVALID, "ngram lm: %lld entries, the model outgrows %lld arcs", (long long)n_entries, (long long)kNgramMaxArcs);
    std::map<Key, Entry> ents;
    int64_t off = 0;
    for (int64_t e = 0; e < n_entries; e++) {
        const int num = numbers ? numbers[e] : (int)e, n = orders[e];
        K2_REQUIRE(n >= 1 && n <= kNgramMaxOrder, "ngram lm: %s %d: order %d outside [1, %d]", noun, num, n, kNgramMaxOrder);
        K2_REQUIRE(std::isfinite(log_probs[e]) && std::isfinite(backoffs[e]), "ngram lm: %s %d: non-finite number", noun, num);
        N_ = std::max(N_, n);
        Key key((size_t)n);
        bool unk = false, arc = true;
        for (int i = 0; i < n; i++) {
            const int64_t v = ids[off + i];
            if (v == kNgramUnk) {
                unk = true;
            } else if (v == kNgramEos) {
                K2_REQUIRE(i == n - 1, "ngram lm: %s %d: </s> inside a history", noun, num);
                arc = false;   // </s> as a predicted word is ignored
            } else if (v == kNgramBos) {
                K2_REQUIRE(i == 0 || i == n - 1, "ngram lm: %s %d: <s> inside a history", noun, num);
                if (i == n - 1) arc = false;   // <s> as a predicted word is ignored (the unigram carries the back-off of history <s>)
            } else {
                K2_REQUIRE(v >= 0 && v < V_, "ngram lm: %s %d: token id %lld outside [0, %d)", noun, num, (long long)v, V_);
                K2_REQUIRE(v != K2HIP_BLANK_ID && v != K2HIP_UNK_ID, "ngram lm: %s %d contains %s (id %lld)", noun, num,
                           v == K2HIP_BLANK_ID ? "blank" : "unk", (long long)v);
            }
            key[(size_t)i] = (int)v;
        }
        off += n;
        if (unk) {
            if (n > 1) continue;   // contexts with <unk> are never reached: a token without a unigram returns to state 0
            K2_REQUIRE(!has_unk_, "ngram lm: %s %d duplicates the <unk> unigram", noun, num);
            has_unk_ = true;
            unk_lp_ = log_probs[e];
            continue;
        }
        auto ins = ents.emplace(std::move(key), Entry{log_probs[e], backoffs[e], arc, num});
        K2_REQUIRE(ins.second, "ngram lm: %s %d duplicates %s %d", noun, num, noun, ins.first->second.num);
    }
    // every history has an entry of its own; the histories of the kept entries are the states
    std::vector<Key> hist;
    for (auto& kv : ents) {
        if (kv.first.size() < 2) continue;
        Key h(kv.first.begin(), kv.first.end() - 1);
        K2_REQUIRE(ents.count(h), "ngram lm: %s %d: its history has no entry of its own", noun, kv.second.num);
        if (kv.second.arc) hist.push_back(std::move(h));
    }
    std::sort(hist.begin(), hist.end(), [](const Key& a, const Key& b) { return a.size() != b.size() ? a.size() < b.size() : a < b; });
    hist.erase(std::unique(hist.begin(), hist.end()), hist.end());
    std::map<Key, int> state_of;
    state_of[Key()] = 0;
    for (size_t i = 0; i < hist.size(); i++) state_of[hist[i]] = (int)i + 1;
    const int S = (int)hist.size() + 1;
    auto longest_suffix = [&](const Key& k, int max_len) {
        for (int len = std::min((int)k.size(), max_len); len >= 1; len--) {
            auto it = state_of.find(Key(k.end() - len, k.end()));
            if (it != state_of.end()) return it->second;
        }
        return 0;
    };
    bo_state_.assign((size_t)S, 0);
    bow_.assign((size_t)S, 0.f);
    for (size_t i = 0; i < hist.size(); i++) {
        bo_state_[i + 1] = longest_suffix(hist[i], (int)hist[i].size() - 1);
        bow_[i + 1] = ents.at(hist[i]).bo;
    }
    std::vector<Arc> arcs;
    std::vector<char> has_uni((size_t)V_, 0);
    for (auto& kv : ents) {
        if (!kv.second.arc) continue;
        const Key& k = kv.first;
        const int s = state_of.at(Key(k.begin(), k.end() - 1));
        if (s == 0) has_uni[(size_t)k.back()] = 1;
        arcs.push_back(Arc{s, k.back(), kv.second.lp, longest_suffix(k, N_ - 1)});
    }
    for (int v = 0; v < V_; v++)
        if (v != K2HIP_BLANK_ID && v != K2HIP_UNK_ID && !has_uni[(size_t)v] && !has_unk_)
            failf(K2HIP_ERR_INVALID, "ngram lm: token id %d has no unigram and the model has no <unk> unigram to fall back on", v);
    std::sort(arcs.begin(), arcs.end(), [](const Arc& a, const Arc& b) { return a.s != b.s ? a.s < b.s : a.tok < b.tok; });
    off_.assign((size_t)S + 1, 0);
    for (auto& a : arcs) off_[(size_t)a.s + 1]++;
    for (int s = 0; s < S; s++) off_[(size_t)s + 1] += off_[(size_t)s];
    tok_.reserve(arcs.size()); lp_.reserve(arcs.size()); next_.reserve(arcs.size());
    for (auto& a : arcs) {
        tok_.push_back(a.tok);
        lp_.push_back(a.lp);
        next_.push_back(a.next);
    }
    auto it = state_of.find(Key{(int)kNgramBos});
    start_ = it != state_of.end() ? it->second : 0;
}

void NgramLm::step(int state, int64_t token, int* next_state, float* log_prob) const {
    K2_REQUIRE(state >= 0 && state < num_states(), "ngram lm: state %d outside [0, %d)", state, num_states());
    K2_REQUIRE(token >= 0 && token < V_, "ngram lm: token id %lld outside [0, %d)", (long long)token, V_);
    if (token == K2HIP_BLANK_ID || token == K2HIP_UNK_ID) {
        *next_state = state;
        *log_prob = 0.f;
        return;
    }
    float acc = 0.f;
    int s = state;
    for (;;) {
        const int32_t* b = tok_.data() + off_[(size_t)s];
        const int32_t* e = tok_.data() + off_[(size_t)s + 1];
        const int32_t* p = std::lower_bound(b, e, (int32_t)token);
        if (p != e && *p == token) {
            const size_t a = (size_t)(p - tok_.data());
            *log_prob = acc + lp_[a];
            *next_state = next_[a];
            return;
        }
        if (s == 0) {   // (the constructor made sure the fallback exists)
            *log_prob = acc + unk_lp_;
            *next_state = 0;
            return;
        }
        acc = acc + bow_[(size_t)s];
        s = bo_state_[(size_t)s];
    }
}

void NgramLm::device_form(float scale, NgramDeviceForm* d) const {
    const int S = num_states();
    const size_t A = tok_.size();
    auto bits = [](float f) {
        int32_t i;
        memcpy(&i, &f, sizeof i);
        return i;
    };
    d->states.resize((size_t)S * 4);
    for (int s = 0; s < S; s++) {
        d->states[(size_t)s * 4 + 0] = (int32_t)off_[(size_t)s];
        d->states[(size_t)s * 4 + 1] = (int32_t)off_[(size_t)s + 1];
        d->states[(size_t)s * 4 + 2] = bo_state_[(size_t)s];
        d->states[(size_t)s * 4 + 3] = bits(bow_[(size_t)s] * scale);
    }
    d->arc_tok = tok_;
    d->arc_next = next_;
    d->arc_lp.resize(A);
    for (size_t a = 0; a < A; a++) d->arc_lp[a] = lp_[a] * scale;
    d->uni_lp.assign((size_t)V_, 0.f);
    d->uni_next.assign((size_t)V_, 0);
    for (int v = 0; v < V_; v++) {
        if (v == K2HIP_BLANK_ID || v == K2HIP_UNK_ID) continue;
        d->uni_lp[(size_t)v] = (has_unk_ ? unk_lp_ : 0.f) * scale;
    }
    for (int64_t a = off_[0]; a < off_[1]; a++) {
        d->uni_lp[(size_t)tok_[(size_t)a]] = lp_[(size_t)a] * scale;
        d->uni_next[(size_t)tok_[(size_t)a]] = next_[(size_t)a];
    }
}

// ---- text ARPA ------------------------------------------------------------------------------------------------------------------
namespace {

struct Line {
    const char* p;
    size_t n;
};
// fields of a line (blanks, tabs and a trailing carriage return separate)
std::vector<std::string> fields(const Line& l) {
    std::vector<std::string> out;
    size_t i = 0;
    auto sep = [](char c) { return c == ' ' || c == '\t' || c == '\r'; };
    while (i < l.n) {
        while (i < l.n && sep(l.p[i])) i++;
        size_t j = i;
        while (j < l.n && !sep(l.p[j])) j++;
        if (j > i) out.emplace_back(l.p + i, j - i);
        i = j;
    }
    return out;
}
// log10 text -> natural log float32; false for anything but one finite number
bool parse_log10(const std::string& s, float* out) {
    if (s.empty() || s.size() > 64) return false;
    char* end = nullptr;
    const double v = strtod(s.c_str(), &end);
    if (end != s.c_str() + s.size() || !std::isfinite(v)) return false;
    const float f = (float)(v * 2.302585092994045684);
    if (!std::isfinite(f)) return false;
    *out = f;
    return true;
}

// a non-negative decimal integer that is all of [p, p + n) and at most `max`; -1 otherwise
long long parse_count(const char* p, size_t n, long long max) {
    if (n == 0 || n > 18) return -1;
    long long v = 0;
    for (size_t i = 0; i < n; i++) {
        if (p[i] < '0' || p[i] > '9') return -1;
        v = v * 10 + (p[i] - '0');   // (at most 18 digits: no overflow)
    }
    return v <= max ? v : -1;
}

}  // namespace

NgramLm* ngram_parse_arpa(const char* data, size_t len, const std::map<std::string, int>& id_of, int vocab_size, const char* name) {
    std::vector<int64_t> ids;
    std::vector<int32_t> orders;
    std::vector<float> lps, bos;
    std::vector<int> line_of;
    std::vector<long long> declared;   // [order - 1]
    enum { HEAD, COUNTS, GRAMS, DONE } where = HEAD;
    int cur = 0;            // the open \k-grams: section
    long long seen = 0;     // its entries so far
    int ln = 0;
    auto close_section = [&](int at) {
        if (cur > 0 && seen != declared[(size_t)cur - 1])
            failf(K2HIP_ERR_INVALID, "ngram lm file %s line %d: the %d-gram section has %lld entries, \\data\\ declares %lld", name, at, cur, seen,
                  declared[(size_t)cur - 1]);
    };
    for (size_t pos = 0; pos < len && where != DONE;) {
        const char* nl = static_cast<const char*>(memchr(data + pos, '\n', len - pos));
        const Line l{data + pos, nl ? (size_t)(nl - (data + pos)) : len - pos};
        pos += l.n + 1;
        ln++;
        const std::vector<std::string> f = fields(l);
        if (f.empty()) continue;
        if (where == HEAD) {
            if (f.size() == 1 && f[0] == "\\data\\") where = COUNTS;
            continue;
        }
        if (f[0][0] == '\\') {
            if (f.size() == 1 && f[0] == "\\end\\") {
                close_section(ln);
                if (cur != (int)declared.size())
                    failf(K2HIP_ERR_INVALID, "ngram lm file %s line %d: \\end\\ after %d of %d declared sections", name, ln, cur, (int)declared.size());
                where = DONE;
                continue;
            }
            // "\<k>-grams:"
            const std::string& h = f[0];
            const size_t dash = h.find('-');
            const int k = (f.size() == 1 && dash != std::string::npos && h.compare(dash, std::string::npos, "-grams:") == 0)
                              ? (int)parse_count(h.data() + 1, dash - 1, 1 << 20) : -1;
            if (k < 0)
                failf(K2HIP_ERR_INVALID, "ngram lm file %s line %d: unknown section '%.40s'", name, ln, f[0].c_str());
            close_section(ln);
            if (k != cur + 1 || k > (int)declared.size())
                failf(K2HIP_ERR_INVALID, "ngram lm file %s line %d: section %d-grams out of order (\\data\\ declares %d orders)", name, ln, k, (int)declared.size());
            where = GRAMS;
            cur = k;
            seen = 0;
            continue;
        }
        if (where == COUNTS) {
            // "ngram <k>=<count>"
            const std::string rest = f.size() == 2 ? f[1] : "";
            const size_t eq = rest.find('=');
            const int k = (f[0] == "ngram" && eq != std::string::npos) ? (int)parse_count(rest.data(), eq, 1 << 20) : -1;
            const long long c = k >= 0 ? parse_count(rest.data() + eq + 1, rest.size() - eq - 1, (long long)1 << 60) : -1;
            if (k < 0 || c < 0)
                failf(K2HIP_ERR_INVALID, "ngram lm file %s line %d: expected 'ngram <order>=<count>'", name, ln);
            if (k > kNgramMaxOrder) failf(K2HIP_ERR_INVALID, "ngram lm file %s line %d: order %d above %d", name, ln, k, kNgramMaxOrder);
            if (k != (int)declared.size() + 1) failf(K2HIP_ERR_INVALID, "ngram lm file %s line %d: order %d out of sequence", name, ln, k);
            declared.push_back(c);
            long long total = 0;
            for (long long d : declared) total += d;
            if (total > kNgramMaxArcs)
                failf(K2HIP_ERR_INVALID, "ngram lm file %s line %d: %lld entries, the model outgrows %lld arcs", name, ln, total, (long long)kNgramMaxArcs);
            continue;
        }
        // an entry of the open section: log10(p), cur words, an optional log10(back-off)
        if ((int)f.size() != cur + 1 && (int)f.size() != cur + 2)
            failf(K2HIP_ERR_INVALID, "ngram lm file %s line %d: a %d-gram line has %zu fields", name, ln, cur, f.size());
        if (++seen > declared[(size_t)cur - 1])
            failf(K2HIP_ERR_INVALID, "ngram lm file %s line %d: the %d-gram section has more entries than the %lld \\data\\ declares", name, ln, cur,
                  declared[(size_t)cur - 1]);
        float lp = 0.f, bo = 0.f;
        if (!parse_log10(f[0], &lp) || ((int)f.size() == cur + 2 && !parse_log10(f.back(), &bo)))
            failf(K2HIP_ERR_INVALID, "ngram lm file %s line %d: not a finite number", name, ln);
        for (int i = 1; i <= cur; i++) {
            const std::string& w = f[(size_t)i];
            auto it = id_of.find(w);
            if (w == "<unk>") ids.push_back(kNgramUnk);   // always the LM's own fallback, never the acoustic unk id
            else if (it != id_of.end()) ids.push_back(it->second);
            else if (w == "<s>") ids.push_back(kNgramBos);
            else if (w == "</s>") ids.push_back(kNgramEos);
            else failf(K2HIP_ERR_INVALID, "ngram lm file %s line %d: word '%.60s' is not in the token table", name, ln, w.c_str());
        }
        orders.push_back(cur);
        lps.push_back(lp);
        bos.push_back(bo);
        line_of.push_back(ln);
    }
    if (where == HEAD) failf(K2HIP_ERR_INVALID, "ngram lm file %s line %d: no \\data\\ section", name, ln);
    if (where != DONE) failf(K2HIP_ERR_INVALID, "ngram lm file %s line %d: no \\end\\", name, ln);
    try {
        return new NgramLm(ids.data(), orders.data(), lps.data(), bos.data(), (int64_t)orders.size(), vocab_size, "line", line_of.data());
    } catch (const Error& e) {
        failf(e.code, "ngram lm file %s: %s", name, e.what());
    }
}

}  // namespace k2hip
