// Host reference of the RNN-T lattice recursions of align.hip (k_lattice_dp) and the argument rules of the align entry points.
// No HIP in here: tests/native/engine_stub_align.cpp (the CPU stand-in of Engine::align_*) and tests/native/san_align_driver.cpp
// build it with a plain C++ compiler under AddressSanitizer / UBSan, and engine.cpp uses the same argument check.
//
// One stream: frames t = 0 .. T-1, target positions u = 0 .. U, two planes [T][U+1] of float32
//   stay(t,u): (t,u) -> (t+1,u)          emit(t,u): (t,u) -> (t+1,u+1), u < U      (modified topology: at most one symbol per frame)
// total = logsumexp over all paths (0,0) -> (T,U), best = their maximum.  A cell is only read inside the reachable band
// u <= t and U-u <= T-t; everything outside it counts as -inf whatever the planes hold.
// Tie rule of the Viterbi step: on equal float32 values the emit predecessor (t-1,u-1) wins over the stay predecessor (t-1,u).
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "errors.h"

namespace k2hip {

// logaddexp(a, b) = m + log1p(exp(min - m)); a -inf operand gives the other one, two give -inf (never NaN)
inline float lattice_logaddexp(float a, float b) {
    const float m = a > b ? a : b, n = a > b ? b : a;
    if (n == -std::numeric_limits<float>::infinity()) return m;
    return m + log1pf(expf(n - m));
}

inline bool lattice_in_band(int t, int u, int T, int U) { return u <= t && U - u <= T - t; }

struct LatticeRefResult {
    float total = 0, best = 0;
    std::vector<int32_t> timestamps;      // [U]: frame of the best path's emit arc of y_{u+1}, strictly increasing
    std::vector<float> token_log_probs;   // [U]: that arc's emit value
};

inline LatticeRefResult lattice_dp_ref(const float* stay, const float* emit, int T, int U) {
    K2_REQUIRE(T >= 1 && U >= 0 && U <= T, "lattice_dp_ref: T=%d U=%d", T, U);
    const float ninf = -std::numeric_limits<float>::infinity();
    const int U1 = U + 1;
    std::vector<float> fa((size_t)U1, ninf), va((size_t)U1, ninf), fb((size_t)U1), vb((size_t)U1);
    std::vector<uint8_t> bp((size_t)T * U1, 0);   // bp[(t-1) U1 + u]: the best path enters (t,u) by an emit arc
    fa[0] = va[0] = 0.f;
    for (int t = 0; t < T; t++) {   // (t, .) -> (t+1, .)
        for (int u = 0; u < U1; u++) {
            float fs = ninf, vs = ninf, fe = ninf, ve = ninf;
            if (lattice_in_band(t, u, T, U)) {
                const float s = stay[(size_t)t * U1 + u];
                fs = fa[(size_t)u] + s;
                vs = va[(size_t)u] + s;
            }
            if (u > 0 && lattice_in_band(t, u - 1, T, U)) {
                const float e = emit[(size_t)t * U1 + u - 1];
                fe = fa[(size_t)u - 1] + e;
                ve = va[(size_t)u - 1] + e;
            }
            fb[(size_t)u] = lattice_logaddexp(fs, fe);
            const bool by_emit = u > 0 && ve >= vs;
            vb[(size_t)u] = by_emit ? ve : vs;
            bp[(size_t)t * U1 + u] = by_emit;
        }
        fa.swap(fb);
        va.swap(vb);
    }
    LatticeRefResult r;
    r.total = fa[(size_t)U];
    r.best = va[(size_t)U];
    r.timestamps.assign((size_t)U, 0);
    r.token_log_probs.assign((size_t)U, 0.f);
    int u = U;
    for (int t = T; t >= 1 && u > 0; t--) {
        // on the diagonal u == t the stay predecessor is outside the band, so the bit is set and u reaches 0 with t
        if (bp[(size_t)(t - 1) * U1 + u]) {
            r.timestamps[(size_t)u - 1] = t - 1;
            r.token_log_probs[(size_t)u - 1] = emit[(size_t)(t - 1) * U1 + u - 1];
            u--;
        }
    }
    return r;
}

// The argument rules of Engine::align_host / align_samples, checked before any device work.  ids: the targets back to back.
inline void lattice_check_targets(int V, int B, int Tp, const int32_t* n_frames, const int64_t* ids, const int32_t* lens) {
    K2_REQUIRE(B > 0 && Tp > 0, "align: bad shape B=%d T'=%d", B, Tp);
    K2_REQUIRE(lens != nullptr, "align: lens is null");
    size_t o = 0;
    for (int b = 0; b < B; b++) {
        const int T = n_frames ? n_frames[b] : Tp, U = lens[b];
        K2_REQUIRE(T >= 1 && T <= Tp, "align: stream %d has n_frames = %d outside [1, T' = %d]", b, T, Tp);
        K2_REQUIRE(U >= 0, "align: stream %d has a negative target length %d", b, U);
        K2_REQUIRE(U <= T, "align: stream %d has %d target tokens but only %d frames: no alignment exists (one symbol per frame at most)", b, U, T);
        K2_REQUIRE(U == 0 || ids != nullptr, "align: ids is null");
        for (int u = 0; u < U; u++) {
            const int64_t y = ids[o + (size_t)u];
            K2_REQUIRE(y >= 0 && y < V, "align: stream %d target %d is id %lld, outside the vocabulary [0, %d)", b, u, (long long)y, V);
            K2_REQUIRE(y != K2HIP_BLANK_ID && y != K2HIP_UNK_ID, "align: stream %d target %d is %s (id %lld), which the search never emits", b, u,
                       y == K2HIP_BLANK_ID ? "blank" : "unk", (long long)y);
        }
        o += (size_t)U;
    }
}

}  // namespace k2hip
