// CPU sanitizer driver (AddressSanitizer + UBSan, see `make -C k2transducerasr_amd/csrc san`) for the pure-host units of
// libk2hip that read untrusted bytes: the .k2w container parser and the token -> text stage.  Test infrastructure.
//   san_driver k2w  <file>                 parse once; prints "OK <n_meta> <n_tensors>" or "ERR <code> <message>"
//   san_driver fuzz <file> <seed> <iters>  parse <iters> mutated copies (truncations, byte flips, field overwrites in the header);
//                                          prints the OK / ERR counts.  Any crash or sanitizer report fails the process.
//   san_driver text <tokens.txt> <online 0|1> <id> ...   decode ids to text
//   san_driver searchout                   the arithmetic of SearchOut (csrc/search_out.h), the one layout of a search's token outputs
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <string>
#include <vector>

#include "../../k2transducerasr_amd/csrc/errors.h"
#include "../../k2transducerasr_amd/csrc/k2w_file.h"
#include "../../k2transducerasr_amd/csrc/search_out.h"
#include "../../k2transducerasr_amd/csrc/text.h"

using namespace k2hip;

static int parse(const std::string& path, bool verbose) {
    try {
        K2wFile f(path);
        // touch every tensor's first and last byte: the range checks promised they are inside the mapping
        unsigned long long sum = 0;
        for (const auto& t : f.tensors)
            if (t.nbytes) sum += f.data()[t.off] + f.data()[t.off + t.nbytes - 1];
        if (verbose) printf("OK %zu %zu %llu\n", f.meta.size(), f.tensors.size(), sum);
        return 0;
    } catch (const Error& e) {
        if (verbose) printf("ERR %d %s\n", e.code, e.what());
        return e.code == K2HIP_ERR_IO ? 1 : 2;
    }
}

struct OneBlockArena {   // hands out one 256-aligned block of exactly the bytes asked for, as the engine's arena would
    char* p = nullptr;
    int64_t n = 0;
    template <typename T>
    T* take(int64_t count) {
        n = count * (int64_t)sizeof(T);
        p = static_cast<char*>(aligned_alloc(256, (size_t)((n + 255) / 256 * 256)));
        return reinterpret_cast<T*>(p);
    }
    ~OneBlockArena() { free(p); }
};

// SearchOut: the four parts in order, without overlap, aligned to 16 / 8 / 4 / 4 bytes from a 256-aligned base, summing to bytes();
// the form taken from an arena equal to the form placed at the same address; every byte of the block writable through the accessors
// and none beyond (the allocation is exactly bytes() long, AddressSanitizer watches its end).
static int check_search_out() {
    static const int shapes[][2] = {{1, 1}, {3, 7}, {32, 250}, {128, 16}};
    for (const auto& sh : shapes) {
        const int B = sh[0], mt = sh[1];
        OneBlockArena ar;
        const SearchOut o(ar, B, mt);
        const char *f = reinterpret_cast<const char*>(o.flag()), *t = reinterpret_cast<const char*>(o.tokens()),
                   *s = reinterpret_cast<const char*>(o.timestamps()), *c = reinterpret_cast<const char*>(o.counts());
        const int64_t want = 16 + (int64_t)B * mt * 8 + (int64_t)B * mt * 4 + (int64_t)B * 4;
        bool ok = o.base == ar.p && ar.n == o.bytes() && o.bytes() == want && o.bytes() == SearchOut::bytes_for(B, mt);
        ok = ok && ((uintptr_t)ar.p % 256) == 0 && f == ar.p;
        ok = ok && t == f + 16 && s == t + (int64_t)B * mt * 8 && c == s + (int64_t)B * mt * 4 && c + (int64_t)B * 4 == f + o.bytes();   // in order, gapless
        ok = ok && o.tokens_bytes() == s - t && o.timestamps_bytes() == c - s && o.counts_bytes() == (int64_t)B * 4;
        ok = ok && (uintptr_t)f % 16 == 0 && (uintptr_t)t % 8 == 0 && (uintptr_t)s % 4 == 0 && (uintptr_t)c % 4 == 0;
        const SearchOut q(static_cast<void*>(ar.p), B, mt);
        ok = ok && q.B == o.B && q.max_tokens == o.max_tokens && q.base == o.base && q.flag() == o.flag() && q.tokens() == o.tokens() &&
             q.timestamps() == o.timestamps() && q.counts() == o.counts() && q.bytes() == o.bytes();
        if (!ok) { printf("searchout FAILED at B=%d max_tokens=%d\n", B, mt); return 6; }
        // write every element through the accessors, read it back through copy_out
        *o.flag() = 0;
        for (int64_t i = 0; i < (int64_t)B * mt; i++) { o.tokens()[i] = 1000 + i; o.timestamps()[i] = (int)(7 * i); }
        for (int b = 0; b < B; b++) o.counts()[b] = b % (mt + 1);
        std::vector<int64_t> ht((size_t)B * mt);
        std::vector<int32_t> hs((size_t)B * mt), hn((size_t)B);
        q.copy_out(ht.data(), hs.data(), hn.data());
        for (int64_t i = 0; i < (int64_t)B * mt; i++)
            if (ht[(size_t)i] != 1000 + i || hs[(size_t)i] != (int)(7 * i)) return 7;
        for (int b = 0; b < B; b++)
            if (hn[(size_t)b] != b % (mt + 1)) return 7;
    }
    printf("searchout OK\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "searchout")) return check_search_out();
    if (argc >= 3 && !strcmp(argv[1], "k2w")) {
        int r = parse(argv[2], true);
        return r == 2 ? 3 : 0;  // a wrong error class is a failure; OK and K2HIP_ERR_IO are both valid outcomes
    }
    if (argc >= 5 && !strcmp(argv[1], "fuzz")) {
        std::ifstream in(argv[2], std::ios::binary);
        std::vector<char> orig((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        if (orig.size() < 24) { fprintf(stderr, "cannot read %s\n", argv[2]); return 4; }
        uint64_t data_off = 0;
        memcpy(&data_off, orig.data() + 16, 8);
        const size_t hdr = (size_t)std::min<uint64_t>(data_off, orig.size());
        std::mt19937_64 rng((uint64_t)atoll(argv[3]));
        const int iters = atoi(argv[4]);
        std::string tmp = std::string(argv[2]) + ".fuzz";
        int ok = 0, err = 0, other = 0;
        for (int it = 0; it < iters; it++) {
            std::vector<char> m = orig;
            switch (it % 4) {
                case 0: m.resize(rng() % (it % 8 == 0 ? orig.size() : hdr + 64)); break;          // truncation
                case 1: for (int k = 0; k < 1 + (int)(rng() % 4); k++) m[rng() % hdr] = (char)rng(); break;   // byte flips in the header
                case 2: {   // overwrite a 4- or 8-byte field with an extreme value
                    static const uint64_t ext[] = {0, 1, 0x7fffffffull, 0xffffffffull, 0x7fffffffffffffffull, 0xffffffffffffffffull, 1ull << 40};
                    const uint64_t v = ext[rng() % 7];
                    const size_t w = (rng() & 1) ? 4 : 8, at = rng() % (hdr - w);
                    memcpy(m.data() + at, &v, w);
                    break;
                }
                default: {  // header counts / data offset
                    uint32_t v = (uint32_t)rng();
                    memcpy(m.data() + 8 + 4 * (rng() % 2), &v, 4);
                    if (rng() & 1) { uint64_t d = rng() % (2 * orig.size()); memcpy(m.data() + 16, &d, 8); }
                }
            }
            std::ofstream(tmp, std::ios::binary).write(m.data(), (std::streamsize)m.size());
            int r = parse(tmp, false);
            (r == 0 ? ok : r == 1 ? err : other)++;
        }
        unlink(tmp.c_str());
        printf("fuzz ok=%d err=%d other=%d\n", ok, err, other);
        return other ? 3 : 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "text")) {
        try {
            struct Tab {
                TokenTable* t;
                ~Tab() { token_table_free(t); }
            } tab{token_table_load(argv[2])};
            TokenTable* t = tab.t;
            std::vector<int64_t> ids;
            for (int i = 4; i < argc; i++) ids.push_back(atoll(argv[i]));
            std::string s = decode_tokens(*t, ids.data(), (int)ids.size(), atoi(argv[3]) != 0);
            printf("%s\n", s.c_str());
            for (int b = 0; b < 256; b++)
                if (bbpe_byte_of_char((uint32_t)bbpe_char_of_byte(b)) != b) return 5;
        } catch (const Error& e) {
            printf("ERR %d %s\n", e.code, e.what());
        }
        return 0;
    }
    fprintf(stderr, "usage: san_driver k2w|fuzz|text|searchout ...\n");
    return 64;
}
