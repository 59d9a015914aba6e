// Keyword spotting for transducer models: trie Viterbi (token passing) on the lattice (semantics: include/k2hip.h "Keyword spotting",
// DESIGN.md "Keyword spotting"; host reference: kws_ref.h).  The forced-alignment lattice of align.hip with "position u, predecessor
// u - 1" generalised to "state s, predecessor parent(s)".
//
//   k_trie_logprobs  the hot path: for every stream, frame and trie state s the arc weight stay(t,s) = logaddexp(lp(blank), lp(unk)) and
//                    the emit(t,c) = lp(tok(c)) of every child c of s, lp = log_softmax(out(tanh(enc[t] + dec[s]))).  A workgroup owns
//                    32 frames x ONE state (k_lattice_logprobs' tile: tanh(enc + dec) once in LDS, k-major; four waves sweep out_kn in
//                    32-column tiles on v_mfma_f32_32x32x2_f32 with one online log-sum-exp per row; no logit is stored).  The children's
//                    logits are NOT picked out of the passing tiles: after the sweep they are taken from the LDS activation by direct dot
//                    products, one child per wave at a time -- lane = (row, k parity), the child's weight column is one address per
//                    half-wave -- so a root with hundreds of children needs no pick buffer and no second code path.
//                    Every row's arithmetic (the MFMA row, the merge order of its column states, the dot products) is a function of
//                    that row's frame and state alone, never of its place in a tile or of its neighbours: the chunking rule rests on it.
//   k_trie_dp        one workgroup per stream: states across lanes (four per lane at most: S <= 1024), frames sequential, the (a, start)
//                    rows ping-pong in LDS.  A frame's event is decided by a two-level reduction (wave_best.h, then the four waves'
//                    results through LDS), first over the depth, then over (a, keyword); frames without a candidate pay one barrier.
//                    The reset after an event is applied before the rows are stored for the next frame.
// No workgroup waits for another anywhere; all stores are ordinary vector stores.
#include "kernels.h"
#include "wave_best.h"

namespace k2hip {
namespace {

constexpr int AF = 32;    // frames per strip = rows of the 32x32 tile
constexpr int AT = 256;   // threads per workgroup (4 waves: 4 column tiles in flight)
constexpr int APF = 8;    // weight k-pairs requested ahead per lane
constexpr int DT = 256;   // threads of the DP workgroup
constexpr int DS = kKwsMaxStates / DT;   // states per lane of the DP

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float ninf() { return -__builtin_inff(); }

__device__ __forceinline__ float logaddexp_f(float a, float b) {
    const float m = fmaxf(a, b), n = fminf(a, b);
    if (n == ninf()) return m;
    return m + log1pf(expf(n - m));
}
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
    const float M = fmaxf(m, om);
    if (M == ninf()) return;
    s = s * expf(m - M) + os * expf(om - M);
    m = M;
}

__global__ __launch_bounds__(AT) void k_trie_logprobs(DecJoinW w, KwsArgs a) {
    extern __shared__ float sm[];
    const KwsStream st = a.streams[blockIdx.z];
    const int s = blockIdx.y, t0 = blockIdx.x * AF, T = st.T, S = st.g.S;
    if (s >= S || t0 >= T) return;
    const int J = w.J, V = w.V;
    float* actT = sm;                  // [J][AF]
    float* wm = sm + (size_t)J * AF;   // [4 waves][AF]
    float* ws = wm + 4 * AF;
    float* pick = ws + 4 * AF;         // [2][AF]: the blank and unk logits of every row
    float* lse = pick + 2 * AF;        // [AF]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {
        const int i = tid & (AF - 1), kq = tid / AF;
        const int t = min(t0 + i, T - 1);   // (rows past the stream's last frame repeat it and are not stored)
        const float* e = a.enc + ((long long)blockIdx.z * a.Tp + t) * J;
        const float* d = st.g.dec + (long long)s * J;
        for (int k4 = kq; k4 < J / 4; k4 += AT / AF) {
            const float4 ev = *reinterpret_cast<const float4*>(e + 4 * k4), dv = *reinterpret_cast<const float4*>(d + 4 * k4);
            actT[(4 * k4 + 0) * AF + i] = tanhf(ev.x + dv.x);
            actT[(4 * k4 + 1) * AF + i] = tanhf(ev.y + dv.y);
            actT[(4 * k4 + 2) * AF + i] = tanhf(ev.z + dv.z);
            actT[(4 * k4 + 3) * AF + i] = tanhf(ev.w + dv.w);
        }
    }
    __syncthreads();
    const int r = lane & 31, h = lane >> 5;
    float m[16], sum[16];
#pragma unroll
    for (int g = 0; g < 16; g++) { m[g] = ninf(); sum[g] = 0.f; }
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
                    sum[g] = sum[g] * expf(m[g] - x) + 1.f;
                    m[g] = x;
                } else {
                    sum[g] += expf(x - m[g]);
                }
                if (col == K2HIP_BLANK_ID) pick[row] = x;
                if (col == K2HIP_UNK_ID) pick[AF + row] = x;
            }
        }
    }
    // every lane's column states -> one per row and wave
#pragma unroll
    for (int g = 0; g < 16; g++) {
#pragma unroll
        for (int off = 1; off < 32; off <<= 1) {
            const float om = __shfl_xor(m[g], off), os = __shfl_xor(sum[g], off);
            lse_merge(m[g], sum[g], om, os);
        }
        if (r == 0) {
            const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
            wm[wave * AF + row] = m[g];
            ws[wave * AF + row] = sum[g];
        }
    }
    __syncthreads();
    float* stay = a.stay + st.plane_off;
    float* emit = a.emit + st.plane_off;
    if (tid < AF) {
        const int t = t0 + tid;
        float M = wm[tid], Sm = ws[tid];
#pragma unroll
        for (int v = 1; v < AT / 64; v++) lse_merge(M, Sm, wm[v * AF + tid], ws[v * AF + tid]);
        const float l = M + logf(Sm);
        lse[tid] = l;
        if (t < T) {
            stay[(long long)t * S + s] = logaddexp_f(pick[tid] - l, pick[AF + tid] - l);
            if (s == 0) emit[(long long)t * S] = ninf();   // no arc enters the root
        }
    }
    __syncthreads();
    // the children's logits by direct dot products: lane (row r, parity h) sums k = h, h + 2, ... in four interleaved chains of a fixed
    // order, the two parities are added once
    const int c_lo = st.g.child_off[s], c_hi = st.g.child_off[s + 1];
    for (int j = c_lo + wave; j < c_hi; j += AT / 64) {
        const int tok = st.g.child_tok[j], child = st.g.child_state[j];
        const float* wp = w.out_kn + (long long)h * w.Vp + tok;
        const float* ap = actT + lane;
        float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
        for (int kk = 0; kk < nk; kk += 4) {
            p0 = fmaf(ap[64 * (kk + 0)], wp[(long long)(kk + 0) * ld2], p0);
            p1 = fmaf(ap[64 * (kk + 1)], wp[(long long)(kk + 1) * ld2], p1);
            p2 = fmaf(ap[64 * (kk + 2)], wp[(long long)(kk + 2) * ld2], p2);
            p3 = fmaf(ap[64 * (kk + 3)], wp[(long long)(kk + 3) * ld2], p3);
        }
        const float part = (p0 + p1) + (p2 + p3);
        const float other = __shfl_xor(part, 32);
        const float even = h == 0 ? part : other, odd = h == 0 ? other : part;
        const int t = t0 + r;
        if (h == 0 && t < T) emit[(long long)t * S + child] = ((even + odd) + w.out_b[tok]) - lse[r];
    }
}

__global__ __launch_bounds__(DT) void k_trie_dp(KwsArgs a) {
    extern __shared__ float sm[];
    const int b = blockIdx.x;
    const KwsStream st = a.streams[b];
    const int S = st.g.S, T = st.T, up = a.max_S;
    float* av[2] = {sm, sm + up};
    int* sv[2] = {reinterpret_cast<int*>(sm + 2 * up), reinterpret_cast<int*>(sm + 3 * up)};
    float* red_v = sm + 4 * up;                               // [2 passes][4 waves]
    int* red_i = reinterpret_cast<int*>(sm + 4 * up + 8);     // [2 passes][4 waves]
    const float* stay = a.stay + st.plane_off;
    const float* emit = a.emit + st.plane_off;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int par[DS], dep[DS], kwd[DS];
    float bar[DS];
#pragma unroll
    for (int i = 0; i < DS; i++) {
        const int c = tid + i * DT;
        const bool on = c >= 1 && c < S;
        par[i] = on ? st.g.parent[c] : 0;
        dep[i] = on ? st.g.depth[c] : 0;
        kwd[i] = on ? st.g.kw[c] : -1;
        bar[i] = on ? st.g.bar[c] : 0.f;
        if (c < S) {
            av[0][c] = a.a_in[st.state_off + c];
            sv[0][c] = a.start_in[st.state_off + c];
        }
    }
    float ps[DS], pe[DS];   // the arc weights of the next frame, requested one frame ahead
#pragma unroll
    for (int i = 0; i < DS; i++) {
        const int c = tid + i * DT;
        const bool on = c >= 1 && c < S && T > 0;
        ps[i] = on ? stay[c] : ninf();
        pe[i] = on ? emit[c] : ninf();
    }
    __syncthreads();
    int cur = 0, n_ev = 0;
    for (int t = 0; t < T; t++) {
        const float* ao = av[cur];
        const int* so = sv[cur];
        const int ta = so[0];   // the absolute index of this frame
        float na[DS];
        int ns[DS];
        bool cand[DS];
        bool any = false;
#pragma unroll
        for (int i = 0; i < DS; i++) {
            const int c = tid + i * DT;
            const float cs = ps[i], ce = pe[i];
            if (t + 1 < T && c >= 1 && c < S) {
                ps[i] = stay[(long long)(t + 1) * S + c];
                pe[i] = emit[(long long)(t + 1) * S + c];
            }
            na[i] = ninf(); ns[i] = -1; cand[i] = false;
            if (c >= 1 && c < S) {
                const int p = par[i];
                const float ap = p == 0 ? 0.f : ao[p];
                const int sp = p == 0 ? ta : so[p];
                const float ve = ap + ce, vs = ao[c] + cs;
                const bool e = ve >= vs;   // the tie rule: emit wins
                na[i] = e ? ve : vs;
                ns[i] = e ? sp : so[c];
                if (!(na[i] > ninf())) ns[i] = -1;
                cand[i] = kwd[i] >= 0 && e && na[i] >= bar[i];
                any |= cand[i];
            }
        }
        if (__syncthreads_or(any)) {   // (uniform: every lane of every wave reaches the reductions)
            // the largest depth among the candidates
            float bv = 0.f;
            int bi = -1;
#pragma unroll
            for (int i = 0; i < DS; i++)
                if (cand[i]) best_merge(bv, bi, (float)dep[i], tid + i * DT);
            wave_best(bv, bi);
            if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; }
            __syncthreads();
            bv = red_v[0]; bi = red_i[0];
#pragma unroll
            for (int v = 1; v < DT / 64; v++) best_merge(bv, bi, red_v[v], red_i[v]);
            const float D = bv;
            // among those: the largest a, then the smallest keyword
            bv = 0.f; bi = -1;
#pragma unroll
            for (int i = 0; i < DS; i++)
                if (cand[i] && (float)dep[i] == D) best_merge(bv, bi, na[i], kwd[i]);
            wave_best(bv, bi);
            if (lane == 0) { red_v[4 + wave] = bv; red_i[4 + wave] = bi; }
            __syncthreads();
            bv = red_v[4]; bi = red_i[4];
#pragma unroll
            for (int v = 1; v < DT / 64; v++) best_merge(bv, bi, red_v[4 + v], red_i[4 + v]);
            const int win = bi;
#pragma unroll
            for (int i = 0; i < DS; i++) {
                if (cand[i] && kwd[i] == win && n_ev < a.max_events) {
                    const long long o = (long long)b * a.max_events + n_ev;
                    a.ev_keyword[o] = win;
                    a.ev_start[o] = ns[i];
                    a.ev_end[o] = ta;
                    a.ev_sum[o] = na[i];
                }
                na[i] = ninf();   // overlapping matches are suppressed: every token dies with the event
                ns[i] = -1;
            }
            n_ev++;
        }
        float* an = av[cur ^ 1];
        int* sn = sv[cur ^ 1];
#pragma unroll
        for (int i = 0; i < DS; i++) {
            const int c = tid + i * DT;
            if (c >= 1 && c < S) { an[c] = na[i]; sn[c] = ns[i]; }
        }
        if (tid == 0) { an[0] = 0.f; sn[0] = ta + 1; }
        __syncthreads();
        cur ^= 1;
    }
#pragma unroll
    for (int i = 0; i < DS; i++) {
        const int c = tid + i * DT;
        if (c < S) {
            a.a_out[st.state_off + c] = av[cur][c];
            a.start_out[st.state_off + c] = sv[cur][c];
        }
    }
    if (tid == 0) a.n_events[b] = n_ev;
}

}  // namespace

void trie_logprobs(const Ctx& ctx, const DecJoinW& w, const KwsArgs& a) {
    if (ctx.dry) return;
    K2_REQUIRE(a.B > 0 && a.max_T >= 0 && a.max_S >= 1, "trie_logprobs: bad shape B=%d T=%d S=%d", a.B, a.max_T, a.max_S);
    K2_REQUIRE(w.J % (2 * APF) == 0 && w.J <= 1024, "trie_logprobs: joiner_dim %d is not a multiple of %d up to 1024", w.J, 2 * APF);
    K2_REQUIRE(a.max_S <= kKwsMaxStates && a.B <= 65535, "trie_logprobs: B=%d / S=%d exceed the launch grid", a.B, a.max_S);
    if (a.max_T == 0) return;
    const size_t lds = sizeof(float) * ((size_t)w.J * AF + 11 * AF);
    static LdsAttrOnce lds_attr;
    lds_attr.ensure(k_trie_logprobs, 150 * 1024);
    hipLaunchKernelGGL(k_trie_logprobs, dim3(cdiv(a.max_T, AF), a.max_S, a.B), dim3(AT), lds, ctx.stream, w, a);
    K2_HIP(hipGetLastError());
}

void trie_dp(const Ctx& ctx, const KwsArgs& a) {
    if (ctx.dry) return;
    K2_REQUIRE(a.B > 0 && a.max_S >= 1 && a.max_S <= kKwsMaxStates, "trie_dp: bad shape B=%d S=%d (at most %d states)", a.B, a.max_S, kKwsMaxStates);
    K2_REQUIRE(a.max_events >= a.max_T && a.max_events >= 1, "trie_dp: %d event slots for %d frames", a.max_events, a.max_T);
    const size_t lds = sizeof(float) * (4 * (size_t)a.max_S + 16);
    hipLaunchKernelGGL(k_trie_dp, dim3(a.B), dim3(DT), lds, ctx.stream, a);
    K2_HIP(hipGetLastError());
}

}  // namespace k2hip
