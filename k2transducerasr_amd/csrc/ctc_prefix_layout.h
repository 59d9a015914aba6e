// The in / out blocks of the resumed CTC prefix beam search (ctc_prefix.hip k_ctc_prefix<true>; described in kernels.h beside
// CtcPrefixResumeArgs).  Plain C++ as well as HIP: the host history (ctc_prefix_hist.h) builds on the CPU without the HIP headers.
#pragma once
#if defined(__HIPCC__)
#define K2HIP_LAYOUT_HD __host__ __device__
#else
#define K2HIP_LAYOUT_HD
#endif

namespace k2hip {

// the rolling hash of a prefix: seed for the empty one, h * mul + (token + 1) per token; a chunk passes its hashes on as they came out
constexpr unsigned long long kCtcPrefixHashSeed = 0x243F6A8885A308D3ull, kCtcPrefixHashMul = 0x9E3779B97F4A7C15ull;

struct CtcPrefixResumeLayout {
    int K, Tc;
    K2HIP_LAYOUT_HD int in_ints() const { return 1 + 8 * K + K * K + K * K * Tc; }
    K2HIP_LAYOUT_HD int in_pb() const { return 1; }
    K2HIP_LAYOUT_HD int in_pnb() const { return 1 + K; }
    K2HIP_LAYOUT_HD int in_e() const { return 1 + 2 * K; }
    K2HIP_LAYOUT_HD int in_len() const { return 1 + 3 * K; }
    K2HIP_LAYOUT_HD int in_hash() const { return 1 + 4 * K; }
    K2HIP_LAYOUT_HD int in_phash() const { return 1 + 6 * K; }
    K2HIP_LAYOUT_HD int in_rel() const { return 1 + 8 * K; }
    K2HIP_LAYOUT_HD int in_relx() const { return 1 + 8 * K + K * K; }
    K2HIP_LAYOUT_HD int out_ints() const { return 1 + 9 * K + 3 * K * Tc; }
    K2HIP_LAYOUT_HD int out_org() const { return 1; }
    K2HIP_LAYOUT_HD int out_napp() const { return 1 + K; }
    K2HIP_LAYOUT_HD int out_pb() const { return 1 + 2 * K; }
    K2HIP_LAYOUT_HD int out_pnb() const { return 1 + 3 * K; }
    K2HIP_LAYOUT_HD int out_hash() const { return 1 + 4 * K; }
    K2HIP_LAYOUT_HD int out_phash() const { return 1 + 6 * K; }
    K2HIP_LAYOUT_HD int out_tot() const { return 1 + 8 * K; }
    K2HIP_LAYOUT_HD int out_ys() const { return 1 + 9 * K; }
    K2HIP_LAYOUT_HD int out_ts() const { return 1 + 9 * K + K * Tc; }
    K2HIP_LAYOUT_HD int out_yp() const { return 1 + 9 * K + 2 * K * Tc; }
};

// The side blocks of the resumed BIASED search (k_ctc_prefix<true, true>), beside the blocks above, which keep every offset:
//   in  (ints): [flags | ctx[K] (float bits) | hs[K] | ls[K]]   flags bit 0: this row runs the n-gram LM.  ctx is the accumulated
//               context score WITH the pending bonus of a match under way (it may complete in the next chunk); slots in selection order
//   out (ints): [ctx[K] | hs[K] | ls[K] | fin[K] (float bits) | ord[K]]   the survivors' values by slot; fin[q] = (tot + ctx) -
//               pending[hs] of slot q; ord[i] = the slot that is i-th by (fin desc, slot asc)
struct CtcPrefixResumeBiasLayout {
    int K;
    K2HIP_LAYOUT_HD int in_ints() const { return 1 + 3 * K; }
    K2HIP_LAYOUT_HD int in_ctx() const { return 1; }
    K2HIP_LAYOUT_HD int in_hs() const { return 1 + K; }
    K2HIP_LAYOUT_HD int in_ls() const { return 1 + 2 * K; }
    K2HIP_LAYOUT_HD int out_ints() const { return 5 * K; }
    K2HIP_LAYOUT_HD int out_ctx() const { return 0; }
    K2HIP_LAYOUT_HD int out_hs() const { return K; }
    K2HIP_LAYOUT_HD int out_ls() const { return 2 * K; }
    K2HIP_LAYOUT_HD int out_fin() const { return 3 * K; }
    K2HIP_LAYOUT_HD int out_ord() const { return 4 * K; }
};

}  // namespace k2hip
