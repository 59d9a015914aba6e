// CTC forced alignment and full-sum scoring of given transcripts (semantics: include/k2hip.h, DESIGN.md "CTC forced alignment and
// full-sum scoring"; host reference and THE tie rule: ctc_lattice_ref.h).
//
//   k_ctc_gather    parallel over (t, k): copies the U + 1 columns a target needs out of its row of log_probs [Tp][V] into the target's
//                   compact plane [T][U + 1] (column 0: blank, column k: y_k), so the serial part reads contiguous rows instead of
//                   2U + 1 words scattered over V per frame.
//   k_ctc_lattice   one workgroup per target: the S = 2U + 1 states of the extended sequence across lanes (a loop when S exceeds the
//                   workgroup), t sequential with one barrier per frame; the forward (logaddexp) and the Viterbi (max) recursion share
//                   their loads; both recursions' rows ping-pong in LDS; the first chunk's plane row of frame t + 1 is requested
//                   before frame t's barrier; only the reachable band s <= 2t + 1, S-1-s <= 2 (T-1-t) + 1 is touched; two
//                   back-pointer bits per cell (a wave's 64 states are two ballots, stored by lane 0 as two 64-bit words); one lane
//                   backtraces and writes the first / last frame and the log-prob of every token.
// No workgroup waits for another anywhere; all stores are ordinary vector stores.
#include "kernels.h"

namespace k2hip {
namespace {

constexpr int CT = 256;   // threads of both kernels' workgroups

__device__ __forceinline__ float ninf() { return -__builtin_inff(); }

// logaddexp(a, b) = m + log1p(exp(min - m)); -inf operands never make a NaN
__device__ __forceinline__ float logaddexp_f(float a, float b) {
    const float m = fmaxf(a, b), n = fminf(a, b);
    if (n == ninf()) return m;
    return m + log1pf(expf(n - m));
}

// the plane column of state s: blank for the even states, y_{(s+1)/2} for the odd ones
__device__ __forceinline__ int col_of(int s) { return (s & 1) ? (s + 1) >> 1 : 0; }

__global__ __launch_bounds__(CT) void k_ctc_gather(CtcAlignArgs a) {
    const CtcAlignTarget tg = a.targets[blockIdx.y];
    const int U1 = tg.U + 1;
    const long long n = (long long)tg.T * U1;
    const float* lp = a.log_probs + (long long)tg.row * a.Tp * a.V;
    float* plane = a.plane + tg.plane_off;
    for (long long i = (long long)blockIdx.x * CT + threadIdx.x; i < n; i += (long long)gridDim.x * CT) {
        const int t = (int)(i / U1), k = (int)(i - (long long)t * U1);
        const int id = k ? a.ids[tg.id_off + k - 1] : K2HIP_BLANK_ID;
        plane[i] = lp[(long long)t * a.V + id];
    }
}

__global__ __launch_bounds__(CT) void k_ctc_lattice(CtcAlignArgs a) {
    extern __shared__ float sm[];
    const int h = blockIdx.x;
    const CtcAlignTarget tg = a.targets[h];
    const int T = tg.T, U = tg.U, U1 = U + 1, S = 2 * U + 1, W = (S + 63) / 64, Sp = 2 * a.max_U + 1;
    float* f[2] = {sm, sm + Sp};
    float* v[2] = {sm + 2 * Sp, sm + 3 * Sp};
    const float* plane = a.plane + tg.plane_off;
    unsigned long long* bp = a.bp + tg.bp_off;
    const int* y = a.ids + tg.id_off;
    const int tid = threadIdx.x, lane = tid & 63;
    // bit j: state j CT + tid has the s-2 predecessor (z_s is a token and differs from z_{s-2}); S <= 8191 gives at most 32 chunks
    unsigned skipm = 0;
    for (int j = 0, s = tid; s < S; j++, s += CT) {
        if ((s & 1) && s >= 3 && y[(s - 1) >> 1] != y[(s - 3) >> 1]) skipm |= 1u << j;
        f[0][s] = f[1][s] = v[0][s] = v[1][s] = ninf();
    }
    auto lo_of = [&](int t) { return max(0, S - 2 * (T - t)); };
    auto hi_of = [&](int t) { return min(S - 1, 2 * t + 1); };
    auto load = [&](int t, int s) { return s < S && s >= lo_of(t) && s <= hi_of(t) ? plane[(long long)t * U1 + col_of(s)] : ninf(); };
    if (tid < 2) {   // frame 0 starts in state 0 or 1 (the same thread wrote the -inf above)
        const float x = load(0, tid);
        if (tid < S) f[0][tid] = v[0][tid] = x;
    }
    if (a.tokens)
        for (int u = tid; u < U; u += CT) a.tokens[(long long)h * a.max_tokens + u] = y[u];
    // the first chunk's plane row of frame t + 1 is requested before frame t's barrier
    float px = T > 1 ? load(1, (lo_of(1) & ~(CT - 1)) + tid) : ninf();
    __syncthreads();
    for (int t = 1; t < T; t++) {   // (t - 1, .) -> (t, .)
        const float *fa = f[(t - 1) & 1], *va = v[(t - 1) & 1];
        float *fb = f[t & 1], *vb = v[t & 1];
        const int lo = lo_of(t), hi = hi_of(t), c0 = lo & ~(CT - 1);
        const float cx = px;
        if (t + 1 < T) px = load(t + 1, (lo_of(t + 1) & ~(CT - 1)) + tid);
        for (int s0 = c0; s0 <= hi; s0 += CT) {   // (uniform: every lane reaches the ballots)
            const int s = s0 + tid;
            int p = 0;
            if (s >= lo && s <= hi) {
                const float x = s0 == c0 ? cx : plane[(long long)t * U1 + col_of(s)];
                const bool sk = skipm >> (s0 / CT) & 1u;
                const float f0 = fa[s], v0 = va[s];
                const float f1 = s > 0 ? fa[s - 1] : ninf(), v1 = s > 0 ? va[s - 1] : ninf();
                const float f2 = sk ? fa[s - 2] : ninf(), v2 = sk ? va[s - 2] : ninf();
                fb[s] = logaddexp_f(logaddexp_f(f0, f1), f2) + x;
                // the tie rule: the lowest state index wins -- s-2 over s-1 over s
                float m = v0;
                if (s > 0 && v1 >= m) { m = v1; p = 1; }
                if (sk && v2 >= m) { m = v2; p = 2; }
                vb[s] = m + x;
            }
            const unsigned long long b0 = __ballot(p & 1), b1 = __ballot(p >> 1);
            if (lane == 0 && s < S) {
                unsigned long long* w = bp + ((long long)t * W + (s >> 6)) * 2;
                w[0] = b0;
                w[1] = b1;
            }
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const float *fe = f[(T - 1) & 1], *ve = v[(T - 1) & 1];
    int s = S - 1;
    if (U == 0) {
        a.scores[2 * h] = fe[0];
        a.scores[2 * h + 1] = ve[0];
    } else {
        a.scores[2 * h] = logaddexp_f(fe[S - 2], fe[S - 1]);
        if (ve[S - 2] >= ve[S - 1]) s = S - 2;   // at the end S-2 wins over S-1
        a.scores[2 * h + 1] = ve[s];
    }
    if (a.n_tokens) a.n_tokens[h] = U;
    // backwards over the frames: a token's last frame is where its state is entered from above, its first frame where it is left.  A
    // cell outside the band (reachable only when best is -inf) steps down one state, so s stays inside [0, S) whatever bp holds.
    const long long o = (long long)h * a.max_tokens;
    auto leave = [&](int st, int t_first) {
        if (!(st & 1)) return;
        const int u = (st - 1) >> 1;
        a.timestamps[o + u] = t_first;
        a.token_log_probs[o + u] = plane[(long long)t_first * U1 + u + 1];
    };
    int last = -1;
    for (int t = T - 1; t >= 0; t--) {
        if (s != last) {
            if (last >= 0) leave(last, t + 1);
            if (s & 1) a.end_frames[o + ((s - 1) >> 1)] = t;
        }
        last = s;
        if (t > 0) {
            int step = 1;
            if (s >= lo_of(t) && s <= hi_of(t)) {
                const unsigned long long* w = bp + ((long long)t * W + (s >> 6)) * 2;
                step = (int)(w[0] >> (s & 63) & 1ull) | (int)(w[1] >> (s & 63) & 1ull) << 1;
            }
            s = max(0, s - step);
        }
    }
    leave(last, 0);
}

}  // namespace

void ctc_lattice(const Ctx& ctx, const CtcAlignArgs& a) {
    if (ctx.dry) return;
    K2_REQUIRE(a.H > 0 && a.H <= 65535 && a.max_T > 0 && a.max_U >= 0 && a.max_U <= kCtcAlignMaxTokens && a.V > 0,
               "ctc_lattice: bad shape H=%d T=%d U=%d (at most %d tokens, 65535 targets)", a.H, a.max_T, a.max_U, kCtcAlignMaxTokens);
    const long long cells = (long long)a.max_T * (a.max_U + 1);
    hipLaunchKernelGGL(k_ctc_gather, dim3((unsigned)std::min<long long>((cells + CT - 1) / CT, 1024), a.H), dim3(CT), 0, ctx.stream, a);
    K2_HIP(hipGetLastError());
    const size_t lds = sizeof(float) * 4 * (2 * (size_t)a.max_U + 1);
    static LdsAttrOnce lds_attr;
    lds_attr.ensure(k_ctc_lattice, 136 * 1024);
    hipLaunchKernelGGL(k_ctc_lattice, dim3(a.H), dim3(CT), lds, ctx.stream, a);
    K2_HIP(hipGetLastError());
}

}  // namespace k2hip
