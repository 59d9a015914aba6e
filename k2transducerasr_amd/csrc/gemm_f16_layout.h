// Half-precision weight panels of the encoder's linear layers: the layout gemm_f16_mfma reads (gemm_f16.hip).  Pure host code.
//
// A [N, K] torch Linear matrix (K % 32 == 0) rounded to f16 (nearest even, subnormals kept, as numpy.astype(float16) rounds), in blocks
// of 32 columns -- N padded with zero columns to a multiple of 32 -- by chunks of 32 k.  A (block, chunk) is 2 KiB in the k order of
// rnn_lm_fuse_layout.h: [j: 2][hh: 2][32 columns][e: 8], element e of instruction j and lane half hh being k = 32 q + 16 hh + 8 j + e, so
// that a lane's B operand of one v_mfma_f32_32x32x16_f16 is one 16-byte read and the chunks of a column block follow each other in
// memory.  Element (n, k) sits at (n / 32) 32 K + rnn_lm_panel_f16_at(k, n % 32).
#pragma once
#include <cstddef>
#include <cstdint>

#include "rnn_lm_fuse_layout.h"

namespace k2hip {

inline int64_t gemm_f16_panel_halves(int N, int K) { return (int64_t)((N + 31) / 32) * 32 * K; }
inline size_t gemm_f16_panel_at(int n, int k, int K) { return (size_t)(n / 32) * 32 * (size_t)K + rnn_lm_panel_f16_at(k, n % 32); }
// out: gemm_f16_panel_halves(N, K) f16 bit patterns, every one of them written.  False: a weight is not finite in f16 (the caller refuses
// the matrix); out is then unspecified.
inline bool gemm_f16_pack(const float* W, int N, int K, uint16_t* out) {
    for (int64_t i = 0, n = gemm_f16_panel_halves(N, K); i < n; i++) out[i] = 0;
    bool finite = true;
    for (int n = 0; n < N; n++)
        for (int k = 0; k < K; k++) {
            const uint16_t h = rnn_lm_f16_bits(W[(size_t)n * K + k]);
            finite = finite && (h & 0x7c00u) != 0x7c00u;
            out[gemm_f16_panel_at(n, k, K)] = h;
        }
    return finite;
}

}  // namespace k2hip
