// Neural LM rescoring: an LSTM language model over the rows of rnn_lm_plan.h (semantics: include/k2hip.h, DESIGN.md "Neural LM
// rescoring"; host reference: rnn_lm_ref.h).
//
//   k_lm_embed       X0[row] = E[x(row)], float4 per thread.
//   k_lm_lstm_step   the hot path, one launch per (layer, position): a workgroup owns a strip of LS = 32 active rows x 32 hidden
//                    columns x all four gates, one gate per wave.  h_{t-1} of the strip is staged k-major in LDS in chunks of LKC k (the
//                    A operand of v_mfma_f32_32x32x2_f32 is then one conflict-free ds_read per lane), the wave sweeps its gate's 32
//                    columns of W_hh [H][4H] (the B operand straight from global memory / L2: 128 contiguous bytes per half-wave and k
//                    row), k ascending in ONE accumulator chain per output -- the f32 MFMA is an exact fmaf chain, so a row's product
//                    does not depend on its strip-mates.  The epilogue adds GX, exchanges the four gates of a cell through LDS, applies
//                    the cell, updates c in place and stores h into the row of the layer's output.  Gates never reach memory.
//   k_lm_score       strips of 32 rows of the last layer's output against out_kn [H][Vp] in 32-column tiles, four tiles (waves) in
//                    flight, with the online log-sum-exp of align.hip's k_lattice_logprobs; the target's logit is picked as its column
//                    passes.  The [R, V] logits are never stored; columns >= V never enter the sum.
//   k_lm_totals      one wave per hypothesis: its lp summed sequentially in position order by one lane, the token log-probs and the total
//                    scattered to the caller's order.
// No workgroup waits for another anywhere: no grid barrier, no spin, no persistent loop over t; all stores are ordinary vector stores.
#include "kernels.h"

namespace k2hip {
namespace {

constexpr int LS = 32;     // rows per strip = rows of the 32x32 tile
constexpr int LT = 256;    // threads per workgroup (4 waves)
constexpr int LKC = 256;   // k staged in LDS at a time: [LKC][LS] floats = 32 KiB
constexpr int LPF = 8;     // weight k-pairs requested ahead per lane

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float ninf() { return -__builtin_inff(); }
__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
    const float M = fmaxf(m, om);
    if (M == ninf()) return;   // both empty
    s = s * expf(m - M) + os * expf(om - M);
    m = M;
}

__global__ void k_lm_embed(const float* __restrict__ emb, const int* __restrict__ ids, float* __restrict__ x0, long long R, int E4) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R * E4) return;
    const long long row = i / E4;
    const int q = (int)(i - row * E4);
    reinterpret_cast<float4*>(x0)[i] = reinterpret_cast<const float4*>(emb)[(long long)ids[row] * E4 + q];
}

// rows [row0, row0 + LS) (clamped to n_rows - 1) x k [k0, k0 + kc) of src (rows of H floats) into dst [kc][LS], k-major
__device__ __forceinline__ void stage_strip(float* dst, const float* __restrict__ src, long long row0, long long n_rows, int H, int k0, int kc, int tid) {
    const int i = tid & (LS - 1), kq = tid / LS;
    const long long row = row0 + i < n_rows ? row0 + i : n_rows - 1;
    const float* p = src + row * H + k0;
    for (int k4 = kq; k4 < kc / 4; k4 += LT / LS) {
        const float4 v = *reinterpret_cast<const float4*>(p + 4 * k4);
        dst[(4 * k4 + 0) * LS + i] = v.x;
        dst[(4 * k4 + 1) * LS + i] = v.y;
        dst[(4 * k4 + 2) * LS + i] = v.z;
        dst[(4 * k4 + 3) * LS + i] = v.w;
    }
}
// acc += strip [nk pairs of k] . B, lane l holding A[row l & 31][k = 2 kk + (l >> 5)] = strip[64 kk + l] and B[k][column l & 31] =
// wp[kk ld2] (wp already points at the lane's k row and column); nk is a multiple of LPF
__device__ __forceinline__ f32x16 sweep_k(f32x16 acc, const float* strip, const float* __restrict__ wp, long long ld2, int nk, int lane) {
    const float* ap = strip + lane;
    float bv[LPF];
#pragma unroll
    for (int i = 0; i < LPF; i++) bv[i] = wp[(long long)i * ld2];
    for (int kk0 = 0; kk0 < nk; kk0 += LPF) {
        float av[LPF], bn[LPF];
#pragma unroll
        for (int i = 0; i < LPF; i++) av[i] = ap[64 * (kk0 + i)];
        if (kk0 + LPF < nk) {
#pragma unroll
            for (int i = 0; i < LPF; i++) bn[i] = wp[(long long)(kk0 + LPF + i) * ld2];
        }
#pragma unroll
        for (int i = 0; i < LPF; i++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[i], acc, 0, 0, 0);
        if (kk0 + LPF < nk) {
#pragma unroll
            for (int i = 0; i < LPF; i++) bv[i] = bn[i];
        }
    }
    return acc;
}

__global__ __launch_bounds__(LT) void k_lm_lstm_step(const float* __restrict__ h_prev, const float* __restrict__ whh_kn, const float* __restrict__ gx,
                                                     float* __restrict__ c, float* __restrict__ h_out, int a, int H) {
    __shared__ float hT[LKC * LS];
    __shared__ float gs[4][LS][LS + 1];
    const int row0 = blockIdx.x * LS, j0 = blockIdx.y * 32;
    const int tid = threadIdx.x, lane = tid & 63, gate = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const long long G = 4LL * H;
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; g++) acc[g] = 0.f;
    if (h_prev) {   // (the first position has h = 0: no product)
        for (int k0 = 0; k0 < H; k0 += LKC) {
            const int kc = min(LKC, H - k0);   // H % 32 == 0: whole groups of 16 k pairs
            if (k0) __syncthreads();
            stage_strip(hT, h_prev, row0, a, H, k0, kc, tid);
            __syncthreads();
            acc = sweep_k(acc, hT, whh_kn + (long long)(k0 + hh) * G + (long long)gate * H + j0 + r, 2 * G, kc / 2, lane);
        }
    }
#pragma unroll
    for (int g = 0; g < 16; g++) {
        const int rt = (g & 3) + 8 * (g >> 2) + 4 * hh;
        gs[gate][rt][r] = row0 + rt < a ? acc[g] + gx[(long long)(row0 + rt) * G + (long long)gate * H + j0 + r] : 0.f;
    }
    __syncthreads();
    for (int e = tid; e < LS * 32; e += LT) {
        const int rt = e >> 5, col = e & 31;
        if (row0 + rt >= a) continue;
        const long long o = (long long)(row0 + rt) * H + j0 + col;
        const float ig = sigmoid_f(gs[0][rt][col]), fg = sigmoid_f(gs[1][rt][col]), gg = tanhf(gs[2][rt][col]), og = sigmoid_f(gs[3][rt][col]);
        const float cn = fg * c[o] + ig * gg;
        c[o] = cn;
        h_out[o] = og * tanhf(cn);
    }
}

__global__ __launch_bounds__(LT) void k_lm_score(const float* __restrict__ y, const float* __restrict__ out_kn, const float* __restrict__ out_b,
                                                 const int* __restrict__ target, float* __restrict__ lp, long long R, int H, int V, int Vp) {
    __shared__ float aT[LKC * LS];
    __shared__ float wm[4 * LS], ws[4 * LS], pick[LS];
    const long long row0 = (long long)blockIdx.x * LS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    int tg[16];
    float m[16], s[16];
#pragma unroll
    for (int g = 0; g < 16; g++) {
        const long long row = row0 + (g & 3) + 8 * (g >> 2) + 4 * hh;
        tg[g] = target[row < R ? row : R - 1];
        m[g] = ninf();
        s[g] = 0.f;
    }
    const int ntiles = Vp / 32, rounds = (ntiles + 3) / 4, nchunks = (H + LKC - 1) / LKC;
    for (int rd = 0; rd < rounds; rd++) {
        const int ct = rd * 4 + wave;
        const bool live = ct < ntiles;
        const int col = ct * 32 + r;
        f32x16 acc;
#pragma unroll
        for (int g = 0; g < 16; g++) acc[g] = 0.f;
        for (int ch = 0; ch < nchunks; ch++) {
            const int k0 = ch * LKC, kc = min(LKC, H - k0);
            if (nchunks > 1 || rd == 0) {   // (a strip that fits one chunk is staged once)
                if (rd || ch) __syncthreads();
                stage_strip(aT, y, row0, R, H, k0, kc, tid);
                __syncthreads();
            }
            if (live) acc = sweep_k(acc, aT, out_kn + (long long)(k0 + hh) * Vp + col, 2LL * Vp, kc / 2, lane);
        }
        if (live && col < V) {   // padded columns V .. Vp-1 never enter the sum
            const float bias = out_b[col];
#pragma unroll
            for (int g = 0; g < 16; g++) {
                const float x = acc[g] + bias;
                if (x > m[g]) {
                    s[g] = s[g] * expf(m[g] - x) + 1.f;
                    m[g] = x;
                } else {
                    s[g] += expf(x - m[g]);
                }
                if (col == tg[g]) pick[(g & 3) + 8 * (g >> 2) + 4 * hh] = x;
            }
        }
    }
    // every lane's column states -> one per row and wave
#pragma unroll
    for (int g = 0; g < 16; g++) {
#pragma unroll
        for (int off = 1; off < 32; off <<= 1) {
            const float om = __shfl_xor(m[g], off), os = __shfl_xor(s[g], off);
            lse_merge(m[g], s[g], om, os);
        }
        if (r == 0) {
            const int row = (g & 3) + 8 * (g >> 2) + 4 * hh;
            wm[wave * LS + row] = m[g];
            ws[wave * LS + row] = s[g];
        }
    }
    __syncthreads();
    if (tid < LS && row0 + tid < R) {
        float M = wm[tid], S = ws[tid];
#pragma unroll
        for (int v = 1; v < 4; v++) lse_merge(M, S, wm[v * LS + tid], ws[v * LS + tid]);
        lp[row0 + tid] = pick[tid] - (M + logf(S));
    }
}

__global__ __launch_bounds__(64) void k_lm_totals(const float* __restrict__ lp, const RnnLmHyp* __restrict__ hyps, const long long* __restrict__ base,
                                                  float* __restrict__ token_log_probs, float* __restrict__ totals) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const RnnLmHyp h = hyps[j];
    if (token_log_probs)
        for (int t = lane; t < h.npos; t += 64) token_log_probs[h.out_off + t] = lp[base[t] + j];
    if (lane == 0) {
        float total = 0.f;
        for (int t = 0; t < h.npos; t++) total += lp[base[t] + j];
        totals[h.orig] = total;
    }
}

}  // namespace

void rnn_lm_embed(const Ctx& ctx, const float* emb, const int* ids, float* x0, long long R, int E) {
    K2_REQUIRE(R > 0 && E > 0 && E % 4 == 0, "rnn_lm_embed: %lld rows of %d floats", R, E);
    if (ctx.dry) return;
    hipLaunchKernelGGL(k_lm_embed, dim3(cdiv(R * (E / 4), 256)), dim3(256), 0, ctx.stream, emb, ids, x0, R, E / 4);
    K2_HIP(hipGetLastError());
}

void rnn_lm_step(const Ctx& ctx, const float* h_prev, const float* whh_kn, const float* gx, float* c, float* h_out, int a, int H) {
    K2_REQUIRE(a > 0 && H > 0 && H % 32 == 0, "rnn_lm_step: %d rows, hidden_dim %d (a multiple of 32)", a, H);
    if (ctx.dry) return;
    hipLaunchKernelGGL(k_lm_lstm_step, dim3(cdiv(a, LS), H / 32), dim3(LT), 0, ctx.stream, h_prev, whh_kn, gx, c, h_out, a, H);
    K2_HIP(hipGetLastError());
}

void rnn_lm_score_rows(const Ctx& ctx, const float* y, const float* out_kn, const float* out_b, const int* target, float* lp, long long R, int H,
                       int V, int Vp) {
    K2_REQUIRE(R > 0 && R <= (long long)LS * 0x7fffffff && H > 0 && H % 32 == 0 && V > 0 && Vp >= V && Vp % 32 == 0,
               "rnn_lm_score: %lld rows, hidden_dim %d, V = %d in %d columns", R, H, V, Vp);
    if (ctx.dry) return;
    hipLaunchKernelGGL(k_lm_score, dim3(cdiv(R, LS)), dim3(LT), 0, ctx.stream, y, out_kn, out_b, target, lp, R, H, V, Vp);
    K2_HIP(hipGetLastError());
}

void rnn_lm_totals(const Ctx& ctx, const float* lp, const RnnLmHyp* hyps, const long long* base, int Hn, float* token_log_probs, float* totals) {
    K2_REQUIRE(Hn > 0, "rnn_lm_totals: %d hypotheses", Hn);
    if (ctx.dry) return;
    hipLaunchKernelGGL(k_lm_totals, dim3(Hn), dim3(64), 0, ctx.stream, lp, hyps, base, token_log_probs, totals);
    K2_HIP(hipGetLastError());
}

}  // namespace k2hip
