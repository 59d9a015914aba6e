// Forced alignment and full-sum scoring of a transcript on the RNN-T lattice (semantics: include/k2hip.h, DESIGN.md "Forced alignment
// and full-sum scoring"; host reference: lattice_ref.h).
//
//   k_lattice_logprobs  the hot path: for every stream and every cell (t,u) of the reachable band the two arc weights
//                       stay = logaddexp(lp(blank), lp(unk)) and emit = lp(y_{u+1}), lp = log_softmax(out(tanh(enc[t] + dec[u]))).
//                       A workgroup owns a strip of AF = 32 frames x one u: tanh(enc + dec) is formed once in LDS (k-major, so the
//                       A operand of v_mfma_f32_32x32x2_f32 is one conflict-free ds_read per lane), its four waves sweep out_kn
//                       [J, Vp] in 32-column tiles (the B operand straight from global memory / L2: 128 contiguous bytes per
//                       half-wave and k row), and every lane keeps the running (maximum, sum) of its own column of each of its 16
//                       accumulator rows across the tiles -- the online log-sum-exp needs no cross-lane traffic until the sweep is
//                       over.  The three logits a cell needs are picked out of the accumulators as their columns pass.  Logits are
//                       never stored: 32 x 10 s with 40-token targets would be 0.7 GB of them.
//   k_lattice_dp        one workgroup per stream: u across lanes (looping when U + 1 exceeds the workgroup), t sequential with one
//                       barrier per frame; the forward (logaddexp) and the Viterbi (max) recursion share the loads; one back-pointer
//                       bit per cell (a wave's 64 bits are one ballot, stored by one lane); one lane backtraces.
// No workgroup waits for another anywhere; all stores are ordinary vector stores.
#include "kernels.h"

namespace k2hip {
namespace {

constexpr int AF = 32;    // frames per strip = rows of the 32x32 tile
constexpr int AT = 256;   // threads per workgroup (4 waves: 4 column tiles in flight)
constexpr int APF = 8;    // weight k-pairs requested ahead per lane
constexpr int DT = 256;   // threads of the DP workgroup

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float ninf() { return -__builtin_inff(); }

// logaddexp(a, b) = m + log1p(exp(min - m)); -inf operands never make a NaN
__device__ __forceinline__ float logaddexp_f(float a, float b) {
    const float m = fmaxf(a, b), n = fminf(a, b);
    if (n == ninf()) return m;
    return m + log1pf(expf(n - m));
}
// (m, s) <- the log-sum-exp state of both: sum = s exp(m)
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
    const float M = fmaxf(m, om);
    if (M == ninf()) return;   // both empty
    s = s * expf(m - M) + os * expf(om - M);
    m = M;
}

__global__ __launch_bounds__(AT) void k_lattice_logprobs(DecJoinW w, AlignArgs a) {
    extern __shared__ float sm[];
    const AlignStream st = a.streams[blockIdx.z];
    const int u = blockIdx.y, t0 = blockIdx.x * AF, T = st.T, U = st.U;
    if (u > U || t0 >= T) return;
    // the reachable band of this u: u <= t <= T - U + u
    const int t_hi = T - U + u;
    if (t0 + AF - 1 < u || t0 > t_hi) return;
    const int J = w.J, V = w.V;
    float* actT = sm;               // [J][AF]
    float* wm = sm + (size_t)J * AF;   // [4 waves][AF]
    float* ws = wm + 4 * AF;
    float* pick = ws + 4 * AF;      // [3][AF]: the blank, unk and target logits of every row
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {
        const int i = tid & (AF - 1), kq = tid / AF;
        const int t = min(t0 + i, T - 1);   // (rows past the stream's last frame repeat it and are not stored)
        const float* e = a.enc + ((long long)blockIdx.z * a.Tp + t) * J;
        const float* d = a.dec + (long long)(st.ctx_off + u) * J;
        for (int k4 = kq; k4 < J / 4; k4 += AT / AF) {
            const float4 ev = *reinterpret_cast<const float4*>(e + 4 * k4), dv = *reinterpret_cast<const float4*>(d + 4 * k4);
            actT[(4 * k4 + 0) * AF + i] = tanhf(ev.x + dv.x);
            actT[(4 * k4 + 1) * AF + i] = tanhf(ev.y + dv.y);
            actT[(4 * k4 + 2) * AF + i] = tanhf(ev.z + dv.z);
            actT[(4 * k4 + 3) * AF + i] = tanhf(ev.w + dv.w);
        }
    }
    __syncthreads();
    const int y = u < U ? a.ids[st.id_off + u] : -1;
    const int r = lane & 31, h = lane >> 5;
    float m[16], s[16];
#pragma unroll
    for (int g = 0; g < 16; g++) { m[g] = ninf(); s[g] = 0.f; }
    const int ntiles = (V + 31) / 32, nk = J / 2;
    const long long ld2 = 2LL * w.Vp;
    for (int ct = wave; ct < ntiles; ct += AT / 64) {
        const int col = ct * 32 + r;
        // lane l holds A[row l & 31][k = 2 kk + (l >> 5)] = actT[64 kk + l] and B[k][column l & 31]; columns past Vp re-read the last one
        const float* wp = w.out_kn + (long long)h * w.Vp + min(col, w.Vp - 1);
        const float* ap = actT + lane;
        f32x16 acc;
#pragma unroll
        for (int g = 0; g < 16; g++) acc[g] = 0.f;
        float bv[APF];
#pragma unroll
        for (int i = 0; i < APF; i++) bv[i] = wp[(long long)i * ld2];
        for (int kk0 = 0; kk0 < nk; kk0 += APF) {
            float av[APF], bn[APF];
#pragma unroll
            for (int i = 0; i < APF; i++) av[i] = ap[64 * (kk0 + i)];
            if (kk0 + APF < nk) {
#pragma unroll
                for (int i = 0; i < APF; i++) bn[i] = wp[(long long)(kk0 + APF + i) * ld2];
            }
#pragma unroll
            for (int i = 0; i < APF; i++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[i], acc, 0, 0, 0);
            if (kk0 + APF < nk) {
#pragma unroll
                for (int i = 0; i < APF; i++) bv[i] = bn[i];
            }
        }
        if (col < V) {   // padded columns V .. Vp-1 (and the tile's columns past them) never enter the sum
            const float bias = w.out_b[col];
#pragma unroll
            for (int g = 0; g < 16; g++) {
                const float x = acc[g] + bias;
                const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
                if (x > m[g]) {
                    s[g] = s[g] * expf(m[g] - x) + 1.f;
                    m[g] = x;
                } else {
                    s[g] += expf(x - m[g]);
                }
                if (col == K2HIP_BLANK_ID) pick[row] = x;
                if (col == K2HIP_UNK_ID) pick[AF + row] = x;
                if (col == y) pick[2 * AF + row] = x;
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
            const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
            wm[wave * AF + row] = m[g];
            ws[wave * AF + row] = s[g];
        }
    }
    __syncthreads();
    if (tid < AF) {
        const int t = t0 + tid;
        float M = wm[tid], S = ws[tid];
#pragma unroll
        for (int v = 1; v < AT / 64; v++) lse_merge(M, S, wm[v * AF + tid], ws[v * AF + tid]);
        if (t < T && t >= u && t <= t_hi) {
            const float lse = M + logf(S);
            const long long o = st.plane_off + (long long)t * (U + 1) + u;
            a.stay[o] = logaddexp_f(pick[tid] - lse, pick[AF + tid] - lse);
            a.emit[o] = u < U ? pick[2 * AF + tid] - lse : ninf();
        }
    }
}

__global__ __launch_bounds__(DT) void k_lattice_dp(AlignArgs a) {
    extern __shared__ float sm[];
    const int b = blockIdx.x;
    const AlignStream st = a.streams[b];
    const int T = st.T, U = st.U, U1 = U + 1, W = (U1 + 63) / 64, up = a.max_U + 1;
    float* f[2] = {sm, sm + up};
    float* v[2] = {sm + 2 * up, sm + 3 * up};
    const float* stay = a.stay + st.plane_off;
    const float* emit = a.emit + st.plane_off;
    unsigned long long* bp = a.bp + st.bp_off;
    const int tid = threadIdx.x, lane = tid & 63;
    auto in_band = [&](int t, int u) { return u >= 0 && u <= t && U - u <= T - t; };
    auto load_stay = [&](int t, int u) { return in_band(t, u) ? stay[(long long)t * U1 + u] : ninf(); };
    auto load_emit = [&](int t, int u) { return in_band(t, u - 1) ? emit[(long long)t * U1 + u - 1] : ninf(); };   // the arc INTO u
    for (int u = tid; u < U1; u += DT) f[0][u] = v[0][u] = u == 0 ? 0.f : ninf();
    if (a.tokens)
        for (int u = tid; u < U; u += DT) a.tokens[(long long)b * a.max_tokens + u] = a.ids[st.id_off + u];
    // the first chunk's arc weights of frame t + 1 are requested before frame t's barrier
    float ps = tid < U1 ? load_stay(0, tid) : ninf(), pe = tid < U1 ? load_emit(0, tid) : ninf();
    __syncthreads();
    int cur = 0;
    for (int t = 0; t < T; t++) {   // (t, .) -> (t + 1, .)
        const float *fa = f[cur], *va = v[cur];
        float *fb = f[cur ^ 1], *vb = v[cur ^ 1];
        const float cs = ps, ce = pe;
        if (t + 1 < T && tid < U1) {
            ps = load_stay(t + 1, tid);
            pe = load_emit(t + 1, tid);
        }
        for (int u0 = 0; u0 < U1; u0 += DT) {   // (uniform: every lane reaches the ballot)
            const int u = u0 + tid;
            bool by_emit = false;
            if (u < U1) {
                const float s = u0 == 0 ? cs : load_stay(t, u), e = u0 == 0 ? ce : load_emit(t, u);
                const float fs = fa[u] + s, vs = va[u] + s;
                const float fe = u > 0 ? fa[u - 1] + e : ninf(), ve = u > 0 ? va[u - 1] + e : ninf();
                fb[u] = logaddexp_f(fs, fe);
                by_emit = u > 0 && ve >= vs;   // the tie rule: emit wins
                vb[u] = by_emit ? ve : vs;
            }
            const unsigned long long bits = __ballot(by_emit);
            if (lane == 0 && u < U1) bp[(long long)t * W + (u >> 6)] = bits;
        }
        __syncthreads();
        cur ^= 1;
    }
    if (tid == 0) {
        a.scores[2 * b] = f[cur][U];
        a.scores[2 * b + 1] = v[cur][U];
        if (a.n_tokens) a.n_tokens[b] = U;
        // on the diagonal u == t the stay predecessor is outside the band and the bit is set: u reaches 0 with t, whatever the planes hold
        int u = U;
        for (int t = T; t >= 1 && u > 0; t--) {
            if (bp[(long long)(t - 1) * W + (u >> 6)] >> (u & 63) & 1ull) {
                a.timestamps[(long long)b * a.max_tokens + u - 1] = t - 1;
                a.token_log_probs[(long long)b * a.max_tokens + u - 1] = emit[(long long)(t - 1) * U1 + u - 1];
                u--;
            }
        }
    }
}

}  // namespace

void lattice_logprobs(const Ctx& ctx, const DecJoinW& w, const AlignArgs& a) {
    if (ctx.dry) return;
    K2_REQUIRE(a.B > 0 && a.max_T > 0 && a.max_U >= 0, "lattice_logprobs: bad shape B=%d T=%d U=%d", a.B, a.max_T, a.max_U);
    K2_REQUIRE(w.J % (2 * APF) == 0 && w.J <= 1024, "lattice_logprobs: joiner_dim %d is not a multiple of %d up to 1024", w.J, 2 * APF);
    K2_REQUIRE(a.max_U + 1 <= 65535 && a.B <= 65535, "lattice_logprobs: B=%d / U=%d exceed the launch grid", a.B, a.max_U);
    const size_t lds = sizeof(float) * ((size_t)w.J * AF + 11 * AF);
    static LdsAttrOnce lds_attr;
    lds_attr.ensure(k_lattice_logprobs, 150 * 1024);
    hipLaunchKernelGGL(k_lattice_logprobs, dim3(cdiv(a.max_T, AF), a.max_U + 1, a.B), dim3(AT), lds, ctx.stream, w, a);
    K2_HIP(hipGetLastError());
}

void lattice_dp(const Ctx& ctx, const AlignArgs& a) {
    if (ctx.dry) return;
    K2_REQUIRE(a.B > 0 && a.max_U >= 0 && a.max_U <= kAlignMaxU, "lattice_dp: bad shape B=%d U=%d (at most %d tokens)", a.B, a.max_U, kAlignMaxU);
    const size_t lds = sizeof(float) * 4 * ((size_t)a.max_U + 1);
    static LdsAttrOnce lds_attr;
    lds_attr.ensure(k_lattice_dp, 64 * 1024);
    hipLaunchKernelGGL(k_lattice_dp, dim3(a.B), dim3(DT), lds, ctx.stream, a);
    K2_HIP(hipGetLastError());
}

}  // namespace k2hip
