// Host reference of the CTC trellis recursions of ctc_align.hip (k_ctc_lattice) and the argument rules of the CTC align entry points
// (semantics: include/k2hip.h, DESIGN.md "CTC forced alignment and full-sum scoring").  No HIP in here:
// tests/native/engine_stub_ctc_align.cpp (the CPU stand-in of Engine::ctc_align_*) and tests/native/san_ctc_align_driver.cpp build it with
// a plain C++ compiler under AddressSanitizer / UBSan, and engine.cpp uses the same argument check.
//
// One target y_1 .. y_U against T frames of log_probs [T][V]: the extended sequence z = [blank, y_1, blank, .., y_U, blank], S = 2U + 1
// states; state s at frame t is reached from s, s-1 and -- when z_s is not blank and z_s != z_{s-2} -- s-2; every arrival pays
// lp(t, z_s); frame 0 starts in state 0 or 1; the path ends after frame T-1 in state S-1 or S-2.
// A cell is computed only inside the reachable band s <= 2t + 1 and S-1-s <= 2 (T-1-t) + 1; outside it a cell counts as -inf.
// THE TIE RULE (written down here once; the twin tests/ctc_align_twin.py and the kernel follow it): a state's Viterbi predecessor is the
// maximum over the predecessors the topology allows (s always, s-1 when s > 0, s-2 under the condition above); on equal float32 values
// the LOWEST state index wins -- s-2 over s-1 over s; at the end S-2 wins over S-1.  The back-pointer of a cell outside the band is 1
// (only a backtrace whose best score is -inf can reach one: it then walks down one state per frame and stays inside every array).
// The forward sum of a cell is logaddexp(logaddexp(a_s, a_{s-1}), a_{s-2}) + lp, in that order.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "errors.h"

namespace k2hip {

// U + (number of adjacent equal pairs) frames are the least a target needs; 4 ping-pong rows of S = 2U + 1 floats live in LDS
constexpr int kCtcAlignMaxU = 4095;

// logaddexp(a, b) = m + log1p(exp(min - m)); a -inf operand gives the other one, two give -inf (never NaN)
inline float ctc_logaddexp(float a, float b) {
    const float m = a > b ? a : b, n = a > b ? b : a;
    if (n == -std::numeric_limits<float>::infinity()) return m;
    return m + log1pf(expf(n - m));
}

inline bool ctc_in_band(int t, int s, int T, int S) { return s <= 2 * t + 1 && S - 1 - s <= 2 * (T - 1 - t) + 1; }

// the frames a target needs at least: one per token and one blank between two equal neighbours
inline int ctc_min_frames(const int64_t* y, int U) {
    int n = U;
    for (int u = 1; u < U; u++) n += y[u] == y[u - 1];
    return n;
}

struct CtcLatticeRefResult {
    float total = 0, best = 0;
    std::vector<int32_t> timestamps, end_frames;   // [U]: first / last frame the best path spends in y_{u+1}'s state
    std::vector<float> token_log_probs;            // [U]: lp(timestamps[u], y_{u+1})
};

// lp: [T][ld] (ld >= V), y: U ids in [1, V)
inline CtcLatticeRefResult ctc_lattice_ref(const float* lp, int64_t ld, const int64_t* y, int T, int U) {
    K2_REQUIRE(T >= 1 && U >= 0 && ctc_min_frames(y, U) <= T, "ctc_lattice_ref: T=%d U=%d", T, U);
    const float ninf = -std::numeric_limits<float>::infinity();
    const int S = 2 * U + 1;
    auto z = [&](int s) -> int64_t { return (s & 1) ? y[(s - 1) / 2] : 0; };
    auto skip = [&](int s) { return (s & 1) && s >= 3 && y[(s - 1) / 2] != y[(s - 3) / 2]; };
    std::vector<float> fa((size_t)S, ninf), va((size_t)S, ninf), fb((size_t)S, ninf), vb((size_t)S, ninf);
    std::vector<uint8_t> bp((size_t)T * S, 1);
    for (int s = 0; s < S && s < 2; s++)
        if (ctc_in_band(0, s, T, S)) fa[(size_t)s] = va[(size_t)s] = lp[z(s)];
    for (int t = 1; t < T; t++) {
        for (int s = 0; s < S; s++) {
            if (!ctc_in_band(t, s, T, S)) {
                fb[(size_t)s] = vb[(size_t)s] = ninf;
                continue;
            }
            const float x = lp[(size_t)t * (size_t)ld + (size_t)z(s)];
            const float f0 = fa[(size_t)s], v0 = va[(size_t)s];
            const float f1 = s > 0 ? fa[(size_t)s - 1] : ninf, v1 = s > 0 ? va[(size_t)s - 1] : ninf;
            const bool sk = skip(s);
            const float f2 = sk ? fa[(size_t)s - 2] : ninf, v2 = sk ? va[(size_t)s - 2] : ninf;
            fb[(size_t)s] = ctc_logaddexp(ctc_logaddexp(f0, f1), f2) + x;
            float m = v0;
            uint8_t p = 0;
            if (s > 0 && v1 >= m) { m = v1; p = 1; }
            if (sk && v2 >= m) { m = v2; p = 2; }
            vb[(size_t)s] = m + x;
            bp[(size_t)t * S + s] = p;
        }
        fa.swap(fb);
        va.swap(vb);
    }
    CtcLatticeRefResult r;
    int s = S - 1;
    if (U == 0) {
        r.total = fa[0];
        r.best = va[0];
    } else {
        r.total = ctc_logaddexp(fa[(size_t)S - 2], fa[(size_t)S - 1]);
        if (va[(size_t)S - 2] >= va[(size_t)S - 1]) s = S - 2;
        r.best = va[(size_t)s];
    }
    r.timestamps.assign((size_t)U, 0);
    r.end_frames.assign((size_t)U, 0);
    r.token_log_probs.assign((size_t)U, 0.f);
    for (int t = T - 1, last = -1; t >= 0; t--) {
        if (s & 1) {
            const size_t u = (size_t)(s - 1) / 2;
            if (s != last) r.end_frames[u] = t;
            r.timestamps[u] = t;
            r.token_log_probs[u] = lp[(size_t)t * (size_t)ld + (size_t)y[u]];
        }
        last = s;
        if (t > 0) {
            const int step = ctc_in_band(t, s, T, S) ? bp[(size_t)t * S + s] : 1;
            s = s - step < 0 ? 0 : s - step;
        }
    }
    return r;
}

// The argument rules of Engine::ctc_align_host / ctc_align_samples, checked before any device work.  log_probs has R rows of Tp frames;
// n_frames [R] or null (= Tp); H targets back to back in ids, lens [H]; stream_of [H] or null (then H == R, the identity).
inline void ctc_check_targets(int V, int R, int Tp, const int32_t* n_frames, int H, const int32_t* stream_of, const int64_t* ids, const int32_t* lens) {
    K2_REQUIRE(R > 0 && Tp > 0 && H > 0, "ctc_align: bad shape R=%d T'=%d H=%d", R, Tp, H);
    K2_REQUIRE(lens != nullptr, "ctc_align: lens is null");
    K2_REQUIRE(stream_of != nullptr || H == R, "ctc_align: %d targets for %d rows and no stream_of", H, R);
    if (n_frames)
        for (int r = 0; r < R; r++)
            K2_REQUIRE(n_frames[r] >= 1 && n_frames[r] <= Tp, "ctc_align: row %d has n_frames = %d outside [1, T' = %d]", r, n_frames[r], Tp);
    size_t o = 0;
    for (int h = 0; h < H; h++) {
        const int r = stream_of ? stream_of[h] : h, U = lens[h];
        K2_REQUIRE(r >= 0 && r < R, "ctc_align: target %d has stream_of = %d outside [0, %d)", h, r, R);
        const int T = n_frames ? n_frames[r] : Tp;
        K2_REQUIRE(U >= 0, "ctc_align: target %d has a negative length %d", h, U);
        K2_REQUIRE(U == 0 || ids != nullptr, "ctc_align: ids is null");
        for (int u = 0; u < U; u++) {
            const int64_t y = ids[o + (size_t)u];
            K2_REQUIRE(y != K2HIP_BLANK_ID, "ctc_align: target %d token %d is blank (id %lld)", h, u, (long long)y);
            K2_REQUIRE(y >= 1 && y < V, "ctc_align: target %d token %d is id %lld, outside the vocabulary [1, %d)", h, u, (long long)y, V);
        }
        const int need = ctc_min_frames(ids + o, U);
        K2_REQUIRE(need <= T, "ctc_align: target %d needs %d frames (%d tokens and a blank between equal neighbours) but row %d has %d: no alignment exists",
                   h, need, U, r, T);
        o += (size_t)U;
    }
}

}  // namespace k2hip
