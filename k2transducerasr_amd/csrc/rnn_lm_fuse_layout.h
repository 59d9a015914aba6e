// Neural LM shallow fusion: the weight layout k_nlm_advance reads (rnn_lm_fuse.hip; kernels.h RnnLmDev::wcat).  Pure host code: built
// from the loaded LM without a GPU, exercised under the sanitizers by tests/native/san_rnn_lm_fusion_driver.cpp.
//
// Layer k's [W_ih ; W_hh] concatenated along k -- W_ih's `in` columns, zeros up to Ip = in rounded up to 32, W_hh's H columns: Kc = Ip +
// H -- in H / 8 panels.  Panel jb holds the four gates of the hidden columns 8 jb .. 8 jb + 7: its column c (0 .. 31) is row
// (c / 8) H + 8 jb + c % 8 of the torch matrices, stored as [Kc / 4][32][4], so element (k, c) sits at ((k / 4) 32 + c) 4 + k % 4.
#pragma once
#include <cstdint>
#include <cstring>

#include "rnn_lm_ref.h"

namespace k2hip {

inline int rnn_lm_panel_k(const RnnLm& m, int k) { return (m.in_dim(k) + 31) / 32 * 32 + m.H; }
inline int64_t rnn_lm_panel_floats(const RnnLm& m, int k) { return (int64_t)4 * m.H * rnn_lm_panel_k(m, k); }
// out: rnn_lm_panel_floats(m, k) floats, every one of them written
inline void rnn_lm_panels(const RnnLm& m, int k, float* out) {
    const int H = m.H, I = m.in_dim(k), Ip = (I + 31) / 32 * 32, Kc = Ip + H;
    const float *wi = m.w_ih[(size_t)k].data(), *wh = m.w_hh[(size_t)k].data();
    for (int64_t i = 0, n = rnn_lm_panel_floats(m, k); i < n; i++) out[i] = 0.f;
    for (int jb = 0; jb < H / 8; jb++) {
        float* panel = out + (size_t)jb * Kc * 32;
        for (int c = 0; c < 32; c++) {
            const size_t row = (size_t)(c >> 3) * H + (size_t)jb * 8 + (c & 7);
            for (int i = 0; i < I; i++) panel[((size_t)(i / 4) * 32 + c) * 4 + i % 4] = wi[row * I + i];
            for (int i = 0; i < H; i++) panel[((size_t)((Ip + i) / 4) * 32 + c) * 4 + (Ip + i) % 4] = wh[row * H + i];
        }
    }
}

// ---- the half-precision panels k_nlm_advance_f16 reads (rnn_lm_fuse_f16.hip; kernels.h RnnLmDev::wcat_h) ------------------------------
// The same concatenation along k and the same H / 8 panels of 32 columns, every weight rounded to f16 (nearest even, subnormals kept,
// as numpy.astype(float16) rounds).  k runs in chunks of 32, the chunk one wave sums with two v_mfma_f32_32x32x16_f16: instruction j of
// chunk q takes from the lane half hh its eight k = 32 q + 16 hh + 8 j + e, e = 0 .. 7 -- so that the A side of both instructions is ONE
// run of 16 consecutive floats per lane -- and the panel is [Kc / 32][j: 2][hh: 2][32 columns][e: 8]: element (k, c) sits at
// ((((k / 32) 2 + k % 16 / 8) 2 + k % 32 / 16) 32 + c) 8 + k % 8.  A lane's B operand of one instruction is one 16-byte load, a wave's
// load 1 KiB contiguous, a chunk 2 KiB.
inline uint16_t rnn_lm_f16_bits(float f) {
    uint32_t x;
    memcpy(&x, &f, sizeof x);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);    // NaN
    if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);   // 65520 and up (and infinity) round to infinity
    if (x < 0x33000000u) return (uint16_t)sign;                // below 2^-25: zero
    uint32_t q, rem, half;
    if (x < 0x38800000u) {   // below 2^-14: a multiple of 2^-24 (the implicit bit shifted down with the mantissa)
        const int shift = 126 - (int)(x >> 23);   // 14 .. 24
        const uint32_t m = (x & 0x7fffffu) | 0x800000u;
        q = m >> shift; rem = m & ((1u << shift) - 1u); half = 1u << (shift - 1);
    } else {
        q = (x - 0x38000000u) >> 13; rem = x & 0x1fffu; half = 0x1000u;
    }
    if (rem > half || (rem == half && (q & 1u))) q++;   // (a carry into the exponent is the right encoding)
    return (uint16_t)(sign | q);
}
inline int64_t rnn_lm_panel_halves(const RnnLm& m, int k) { return rnn_lm_panel_floats(m, k); }
inline size_t rnn_lm_panel_f16_at(int k, int c) { return ((((size_t)(k / 32) * 2 + (size_t)(k % 16 / 8)) * 2 + (size_t)(k % 32 / 16)) * 32 + (size_t)c) * 8 + (size_t)(k % 8); }
// out: rnn_lm_panel_halves(m, k) f16 bit patterns, every one of them written.  False: a weight is not finite in f16 (the caller refuses
// the LM); out is then unspecified.
// I: the input width that is laid out in front of W_hh -- the layer's (the fused searches) or 0 (the rescoring step, whose input
// products are a GEMM of their own: the panels are then W_hh's alone, [H / 32][j][hh][32][e], 4 H H halves)
inline bool rnn_lm_panels_f16(const RnnLm& m, int k, uint16_t* out, int I) {
    const int H = m.H, Ip = (I + 31) / 32 * 32, Kc = Ip + H;
    const float *wi = m.w_ih[(size_t)k].data(), *wh = m.w_hh[(size_t)k].data();
    for (int64_t i = 0, n = (int64_t)4 * H * Kc; i < n; i++) out[i] = 0;
    bool finite = true;
    auto put = [&](uint16_t* panel, int kk, int c, float w) {
        const uint16_t h = rnn_lm_f16_bits(w);
        finite = finite && (h & 0x7c00u) != 0x7c00u;
        panel[rnn_lm_panel_f16_at(kk, c)] = h;
    };
    for (int jb = 0; jb < H / 8; jb++) {
        uint16_t* panel = out + (size_t)jb * Kc * 32;
        for (int c = 0; c < 32; c++) {
            const size_t row = (size_t)(c >> 3) * H + (size_t)jb * 8 + (c & 7);
            for (int i = 0; i < I; i++) put(panel, i, c, wi[row * I + i]);
            for (int i = 0; i < H; i++) put(panel, Ip + i, c, wh[row * H + i]);
        }
    }
    return finite;
}
inline bool rnn_lm_panels_f16(const RnnLm& m, int k, uint16_t* out) { return rnn_lm_panels_f16(m, k, out, m.in_dim(k)); }

}  // namespace k2hip
