// Neural LM shallow fusion: the weight layout k_nlm_advance reads (rnn_lm_fuse.hip; kernels.h RnnLmDev::wcat).  Pure host code: built
// from the loaded LM without a GPU, exercised under the sanitizers by tests/native/san_rnn_lm_fusion_driver.cpp.
//
// Layer k's [W_ih ; W_hh] concatenated along k -- W_ih's `in` columns, zeros up to Ip = in rounded up to 32, W_hh's H columns: Kc = Ip +
// H -- in H / 8 panels.  Panel jb holds the four gates of the hidden columns 8 jb .. 8 jb + 7: its column c (0 .. 31) is row
// (c / 8) H + 8 jb + c % 8 of the torch matrices, stored as [Kc / 4][32][4], so element (k, c) sits at ((k / 4) 32 + c) 4 + k % 4.
#pragma once
#include <cstdint>

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

}  // namespace k2hip
