// The shared GEMM epilogue and tile order of the MFMA kernels with a 32x32 (or 16x16) float32 C/D layout: gemm.hip's float32 kernels and
// gemm_f16.hip's half-precision-operand kernel (v_mfma_f32_32x32x16_f16 has the C/D layout of v_mfma_f32_32x32x2_f32).  Device code,
// included by those two files only; every function is internal to its translation unit.
#pragma once
#include "act.h"
#include "kernels.h"

namespace k2hip {

namespace {

// Activations with the hardware transcendental units (v_exp_f32 / v_log_f32, ~1e-6
// relative): the accurate libm forms cost ~100 VALU instructions per element, which
// for K <= 256 made the epilogue longer than the MFMA loop.  Swoosh's softplus is act.h's lean form.
__device__ __forceinline__ float apply_act(float v, int act) {
    switch (act) {
        case ACT_SWOOSH_L: return swoosh_l(v);
        case ACT_SWOOSH_R: return swoosh_r(v);
        case ACT_TANH: {
            float e = __expf(-2.0f * fabsf(v));
            float t = (1.0f - e) / (1.0f + e);
            return v < 0.f ? -t : t;
        }
        case ACT_SIGMOID: return 1.0f / (1.0f + __expf(-v));
        case ACT_RELU: return fmaxf(v, 0.f);
        case ACT_DOUBLE_SWISH: return v / (1.0f + __expf(1.0f - v));  // v * sigmoid(v - 1)
        default: return v;
    }
}

// ---- shared epilogue ------------------------------------------------------------------------------------------------------
// One lane's NV accumulator values of output column `col`, rows row0 + ROWS::off(n).  v = act(acc + bias) (+ residual) [* mul]
// [bypass] -> C.  Written so that the NV stores issue BACK TO BACK: every optional per-element load (residual when it was not
// prefetched, mul, the bypass original) is batched in front of the arithmetic, the activation is chosen by ONE wave-uniform switch
// around the element loop, and nothing loads between two stores.  (With the loads and a per-element activation switch inside the
// element loop the compiler drains vmcnt(0) in front of every element, so each store waited for the previous store's round trip:
// ~500 cycles x 16 per 32x32 block -- 8.6k of the 50k cycles a 128x64 tile with K = 512 takes; in-kernel stamps,
// tools/gemm_dma_trace.py.)
struct Rows32 {  // C/D layout of v_mfma_f32_32x32x2_f32: register r of lane (li, lh) is row (r & 3) + 8 (r >> 2) + 4 lh
    static __device__ __forceinline__ int off(int r) { return (r & 3) + 8 * (r >> 2); }
};
struct Rows16 {  // v_mfma_f32_16x16x4_f32: register e of lane (r, q) is row 4 q + e
    static __device__ __forceinline__ int off(int e) { return e; }
};
// residual: prefetched by the caller (rres, when use_rres) or loaded here from R
template <int NV, typename ROWS>
__device__ __forceinline__ void epilogue_rows(const GemmArgs& g, float (&v)[NV], int row0, int col, float* __restrict__ C,
                                              const float* __restrict__ R, const float (&rres)[NV], bool use_rres,
                                              const float* __restrict__ mulp, const float* __restrict__ biasp, bool bias_loaded = false,
                                              float bias_value = 0.f) {
    if (col >= g.N) return;
    // (bias_loaded: the caller fetched this column's bias before its K loop -- the load's latency is then not part of the epilogue)
    const float bv = bias_loaded ? bias_value : (biasp ? biasp[col] : 0.f);
    const bool act_on = g.act_cols == 0 || col < g.act_cols;
    float rv[NV], mv[NV], ov[NV];
    float bs = 0.f;
    const bool has_res = R != nullptr || use_rres;
    if (use_rres) {
#pragma unroll
        for (int n = 0; n < NV; n++) rv[n] = rres[n];
    } else if (R) {
#pragma unroll
        for (int n = 0; n < NV; n++) {
            const int row = min(row0 + ROWS::off(n), g.M - 1);
            rv[n] = R[(long long)(g.res_div > 1 ? row / g.res_div : row) * g.ldr + col];
        }
    }
    if (mulp) {
#pragma unroll
        for (int n = 0; n < NV; n++) mv[n] = mulp[(long long)min(row0 + ROWS::off(n), g.M - 1) * g.ldm + col];
    }
    if (g.byp_orig) {
        bs = g.byp_scale[col];
#pragma unroll
        for (int n = 0; n < NV; n++) ov[n] = g.byp_orig[(long long)min(row0 + ROWS::off(n), g.M - 1) * g.ld_orig + col];
    }
#pragma unroll
    for (int n = 0; n < NV; n++) v[n] += bv;
    if (g.glu) {
        // The first glu_cols columns (all N when 0) come in blocks of 32 = 16 values | their 16 gates (weights interleaved at load):
        // the partner is 16 lanes away (col = lane & 31 in these layouts); value * sigmoid(gate) (1) or value * tanh(gate) (2) goes
        // to column 16 q + p of C.  Columns from glu_cols on pass through to C columns glu_cols / 2 + (col - glu_cols).
        const int gc = g.glu_cols > 0 ? g.glu_cols : g.N;
        const bool paired = col < gc;  // uniform over a 32-column block (gc % 32 == 0)
        const bool is_value = (col & 16) == 0;
        const int ccol = paired ? ((col >> 5) << 4) + (col & 15) : (gc >> 1) + (col - gc);
        float* cp = C + (long long)row0 * g.ldc + ccol;
#pragma unroll
        for (int n = 0; n < NV; n++) {
            const float other = __shfl_xor(v[n], 16, 64);
            const float gate = g.glu == 2 ? apply_act(other, ACT_TANH) : 1.0f / (1.0f + __expf(-other));
            v[n] = paired ? v[n] * gate : v[n];
        }
        if ((paired && !is_value) || (g.ablate & 4)) return;
#pragma unroll
        for (int n = 0; n < NV; n++)
            if (row0 + ROWS::off(n) < g.M) cp[(long long)ROWS::off(n) * g.ldc] = v[n];
        return;
    }
    if (g.act_after_res && has_res) {
#pragma unroll
        for (int n = 0; n < NV; n++) v[n] += rv[n];
    }
    switch (g.act) {  // wave-uniform; the lanes of columns >= act_cols keep their value
#define K2_ACT_CASE(A_)                                                        \
    case A_:                                                                   \
        _Pragma("unroll") for (int n = 0; n < NV; n++) {                       \
            const float t = apply_act(v[n], A_);                               \
            v[n] = act_on ? t : v[n];                                          \
        }                                                                      \
        break;
        K2_ACT_CASE(ACT_SWOOSH_L)
        K2_ACT_CASE(ACT_SWOOSH_R)
        K2_ACT_CASE(ACT_TANH)
        K2_ACT_CASE(ACT_SIGMOID)
        K2_ACT_CASE(ACT_RELU)
        K2_ACT_CASE(ACT_DOUBLE_SWISH)
#undef K2_ACT_CASE
        default: break;
    }
    if (!g.act_after_res && has_res) {
#pragma unroll
        for (int n = 0; n < NV; n++) v[n] += rv[n];
    }
    if (mulp) {
#pragma unroll
        for (int n = 0; n < NV; n++) v[n] *= mv[n];
    }
    if (g.byp_orig) {
#pragma unroll
        for (int n = 0; n < NV; n++) v[n] = ov[n] + (v[n] - ov[n]) * bs;
    }
    if (g.ablate & 4) return;
    // address = (uniform 64-bit base + the row's uniform byte offset) + a 32-bit per-lane offset: the row offsets are scalar work and
    // the store can take its SGPR-base form; when the lane's last row is inside M (all but the bottom tiles) no row is tested
    const unsigned lane_off = (unsigned)(((long long)row0 * g.ldc + col) * 4);  // < 2^32: checked by the launchers that matter (M * ldc < 2^29)
    const bool small = (long long)g.M * g.ldc < (1ll << 29);
    if (small && row0 + ROWS::off(NV - 1) < g.M) {
#pragma unroll
        for (int n = 0; n < NV; n++) {
            char* ub = reinterpret_cast<char*>(C) + (long long)ROWS::off(n) * g.ldc * 4;
            *reinterpret_cast<float*>(ub + lane_off) = v[n];
        }
        return;
    }
    float* cp = C + (long long)row0 * g.ldc + col;
#pragma unroll
    for (int n = 0; n < NV; n++)
        if (row0 + ROWS::off(n) < g.M) cp[(long long)ROWS::off(n) * g.ldc] = v[n];
}

// XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs (b and b+8 share an L2), so the natural x-fastest order
// makes every XCD read all of A and all of W.  Remap so that each XCD owns a contiguous run of a linear tile order in which runs are
// compact blocks: the N tiles are cut into PN panels (1, 2, 4 or 8), a panel is walked row-major, panels follow each other.  PN = 1 is a
// band of M per XCD (its L2 holds A / 8 + W: the right cut while the rows outweigh the columns); with PN panels an XCD holds ~A PN / 8 +
// W / PN, and the cut that minimises the fabric traffic PN x A + (8 / PN) x W -- PN M + (8 / PN) N in rows and columns, K cancels -- is
// taken (round 4: the wide feed-forward GEMMs of the 6.25 / 12.5 Hz stacks used to pull W, the larger operand there, once per XCD).
// Any (M tiles, N tiles, PN) is a bijection: run boundaries need not coincide with panel boundaries.
__device__ __forceinline__ void xcd_tile(int& mb, int& nb, int M = 0, int N = 0) {
    const int gx = gridDim.x, gy = gridDim.y, nwg = gx * gy;
    if (gridDim.z != 1 || nwg < 16) {  // batched launches keep the natural order
        mb = blockIdx.y;
        nb = blockIdx.x;
        return;
    }
    const int orig = blockIdx.x + blockIdx.y * gx;
    const int xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
    int t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
    int pn = 1;
    // (launches of more than a round of the chip only: on the streaming tick's GEMMs of 100 - 250 workgroups the panels cost 0.06 ms per
    // tick -- there the next launch reads what this one's XCD just wrote, band by band)
    if (M > 0 && N > 0 && nwg >= 320) {
        long long best = (long long)M + 8ll * N;
        const long long worth = best - best / 8;   // (a cut has to save an eighth of the band form's traffic to be taken)
#pragma unroll
        for (int c = 2; c <= 8; c *= 2) {
            const long long cost = (long long)c * M + (8ll / c) * N;
            if (cost < best && cost <= worth && gx >= c) {
                best = cost;
                pn = c;
            }
        }
    }
    // panel p holds columns [n0, n0 + w): widths gx / pn, the first gx % pn panels one wider
    const int wq = gx / pn, wr = gx % pn;
    int n0 = 0, w = wq + (wr > 0);
    for (int p = 0; p < pn - 1 && t >= gy * w; p++) {
        t -= gy * w;
        n0 += w;
        w = wq + (p + 1 < wr);
    }
    mb = t / w;
    nb = n0 + (t - mb * w);
}

}  // namespace

}  // namespace k2hip
