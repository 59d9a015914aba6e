// SearchOut = the token outputs of one search (greedy, CTC collapse, modified beam search) as ONE block of device memory:
//   [flag: 16 B | tokens: B x max_tokens x 8 | timestamps: B x max_tokens x 4 | counts: B x 4]
// so that a call downloads them with one copy and every entry point agrees on where they are.  The flag's first word is the search's
// status (0 = fine, 1 = a stream outgrew max_tokens, 2 = the vocabulary-parallel exchange timed out).  The writers store single
// elements, so the 16 / 8 / 4 / 4-byte alignment that a 16-aligned base gives is all they need.  The same struct placed over the
// pinned copy of the block reads the results on the host.  No HIP in here: the arithmetic is checked by tests/native/san_driver.cpp.
#pragma once
#include <cstdint>
#include <cstring>
#include <utility>

namespace k2hip {

struct SearchOut {
    int B = 0, max_tokens = 0;
    char* base = nullptr;

    SearchOut() = default;
    // the block at `at` (16-byte aligned): the streaming tick's flag is the last 16 bytes of its uploaded input block
    SearchOut(void* at, int B_, int max_tokens_) : B(B_), max_tokens(max_tokens_), base(static_cast<char*>(at)) {}
    // the block taken from an arena (anything with take<char>(bytes); a dry arena gives a null base, to be sized only)
    template <typename ArenaT, typename = decltype(std::declval<ArenaT&>().template take<char>(int64_t{}))>
    SearchOut(ArenaT& arena, int B_, int max_tokens_) : SearchOut(arena.template take<char>(bytes_for(B_, max_tokens_)), B_, max_tokens_) {}

    static int64_t bytes_for(int B, int max_tokens) { return 16 + (int64_t)B * max_tokens * 12 + (int64_t)B * 4; }
    int64_t tokens_bytes() const { return (int64_t)B * max_tokens * 8; }
    int64_t timestamps_bytes() const { return (int64_t)B * max_tokens * 4; }
    int64_t counts_bytes() const { return (int64_t)B * 4; }
    int64_t bytes() const { return bytes_for(B, max_tokens); }

    int* flag() const { return reinterpret_cast<int*>(base); }
    long long* tokens() const { return reinterpret_cast<long long*>(base + 16); }
    int* timestamps() const { return reinterpret_cast<int*>(base + 16 + tokens_bytes()); }
    int* counts() const { return reinterpret_cast<int*>(base + 16 + tokens_bytes() + timestamps_bytes()); }
    // (a block in host memory) the results into the caller's three arrays
    void copy_out(int64_t* tok, int32_t* ts, int32_t* n) const {
        memcpy(tok, tokens(), (size_t)tokens_bytes());
        memcpy(ts, timestamps(), (size_t)timestamps_bytes());
        memcpy(n, counts(), (size_t)counts_bytes());
    }
};

}  // namespace k2hip
