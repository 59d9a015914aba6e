// Keyword spotting for CTC models: trie Viterbi (token passing) on the CTC trellis (semantics: include/k2hip.h "Keyword spotting for CTC
// models", DESIGN.md "CTC keyword spotting"; host reference: ctc_kws_ref.h).  kws.hip's k_trie_dp with two cells per trie state -- n (the
// last frame carried the state's token) and b (blanks after it) -- and the model's own log-probs as arc weights: no arc kernel.
//
//   k_ctc_trie_dp   one workgroup of 256 per stream: states across lanes (DS = 1, 2 or 4 per lane: S <= 1024), frames sequential, the
//                   four rows (n, b, start_n, start_b) ping-pong in LDS.  The log-probs are taken in blocks of F = 16 frames: a lane
//                   requests the F values lp(t, tok(c)) of each of its states (column 0 of the staged block: lp(t, blank)) in one go,
//                   all independent, keeps them in registers while the workgroup walks the current block out of LDS, and stores them
//                   to LDS when that block is done -- a frame of the recursion is far shorter than a trip to memory, so a request
//                   one frame ahead (k_trie_dp's) would leave the workgroup waiting on every frame.  The hold test reads two staged
//                   values.  A frame without a candidate pays one barrier; an event's winner is found by k_trie_dp's two two-level
//                   reductions (wave_best.h, then the four waves' results through LDS), and the reset overwrites the rows just stored.
//                   Every cell's float32 operations and their order are those of ctc_kws_ref.h: the chunking rule rests on it.
// No workgroup waits for another; all stores are ordinary vector stores.
#include "kernels.h"
#include "wave_best.h"

namespace k2hip {
namespace {

constexpr int DT = 256;   // threads of the workgroup
constexpr int F = 16;     // frames per staged block of log-probs
static_assert(kKwsMaxStates == 4 * DT, "at most four states per lane");

__device__ __forceinline__ float ninf() { return -__builtin_inff(); }

template <int DS>
__global__ __launch_bounds__(DT) void k_ctc_trie_dp(CtcKwsArgs a) {
    extern __shared__ float sm[];
    const int b = blockIdx.x;
    const CtcKwsStream st = a.streams[b];
    const int S = st.S, T = st.T, up = a.max_S;
    const int* g_parent = a.tables + st.table_off;
    const int *g_tok = g_parent + S, *g_depth = g_parent + 2 * S, *g_kw = g_parent + 3 * S, *g_rc = g_parent + 5 * S;
    const float* g_bar = reinterpret_cast<const float*>(g_parent + 4 * S);
    // buffer k: [n | b | start_n | start_b], each `up` words; then the staged block [F][up] and the reductions' [2 passes][4 waves] x 2
    float* col = sm + 8 * up;
    float* red_v = col + F * up;
    int* red_i = reinterpret_cast<int*>(red_v + 8);
    const float* lp = a.log_probs + (long long)st.row * a.Tp * a.V;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int par[DS], gcol[DS], dep[DS], kwd[DS], rcv[DS];
    bool via_n[DS];   // n[parent] may precede n[c]: the parent is no root and carries another token
    float bar[DS];
    const long long so = 2LL * st.state_off;
#pragma unroll
    for (int i = 0; i < DS; i++) {
        const int c = tid + i * DT;
        const bool on = c >= 1 && c < S;
        par[i] = on ? g_parent[c] : 0;
        gcol[i] = on ? g_tok[c] : 0;
        dep[i] = on ? g_depth[c] : 0;
        kwd[i] = on ? g_kw[c] : -1;
        rcv[i] = on ? g_rc[c] : -1;
        bar[i] = on ? g_bar[c] : 0.f;
        via_n[i] = on && par[i] != 0 && g_tok[par[i]] != gcol[i];
        if (c < S) {
            sm[c] = a.v_in[so + c];
            sm[up + c] = a.v_in[so + S + c];
            reinterpret_cast<int*>(sm)[2 * up + c] = a.st_in[so + c];
            reinterpret_cast<int*>(sm)[3 * up + c] = a.st_in[so + S + c];
        }
    }
    float pf[F][DS];   // the next block's log-probs, requested a whole block ahead
    auto request = [&](int t0) {
#pragma unroll
        for (int f = 0; f < F; f++)
#pragma unroll
            for (int i = 0; i < DS; i++) {
                const int c = tid + i * DT;
                pf[f][i] = (c < S && t0 + f < T) ? lp[(long long)(t0 + f) * a.V + gcol[i]] : ninf();
            }
    };
    request(0);
    int cur = 0, n_ev = 0;
    for (int t0 = 0; t0 < T; t0 += F) {
        // (the barrier that ended the last frame of the previous block lies behind every read of `col`)
#pragma unroll
        for (int f = 0; f < F; f++)
#pragma unroll
            for (int i = 0; i < DS; i++) {
                const int c = tid + i * DT;
                if (c < S) col[f * up + c] = pf[f][i];
            }
        __syncthreads();
        if (t0 + F < T) request(t0 + F);
        const int nf = min(F, T - t0);
        for (int f = 0; f < nf; f++) {
            const float* on_ = sm + cur * 4 * up;
            const float* ob = on_ + up;
            const int* osn = reinterpret_cast<const int*>(on_ + 2 * up);
            const int* osb = osn + up;
            float* nn_ = sm + (cur ^ 1) * 4 * up;
            float* nb_ = nn_ + up;
            int* nsn_ = reinterpret_cast<int*>(nn_ + 2 * up);
            int* nsb_ = nsn_ + up;
            const float* row = col + f * up;
            const int ta = osn[0];   // the absolute index of this frame
            const float lpb = row[0];
            int hold = osb[0];
            bool closed = false;
            if (hold >= 0) {
                if (row[hold] >= lpb) closed = true;
                else hold = -1;
            }
            float vn[DS];
            int sn[DS];
            bool cand[DS];
            bool any = false;
#pragma unroll
            for (int i = 0; i < DS; i++) {
                const int c = tid + i * DT;
                vn[i] = ninf(); sn[i] = -1; cand[i] = false;
                if (c >= 1 && c < S) {
                    const int p = par[i];
                    const float nc = on_[c], bc = ob[c];
                    const int snc = osn[c], sbc = osb[c];
                    // the predecessors in tie order: n[parent], b[parent], the self loop
                    float best = ninf();
                    int bs = -1;
                    if (p == 0) {
                        if (!(closed && c == hold)) { best = 0.f; bs = ta; }
                    } else {
                        if (via_n[i]) { best = on_[p]; bs = osn[p]; }
                        const float bp = ob[p];
                        if (bp > best) { best = bp; bs = osb[p]; }
                    }
                    bool self = false;
                    if (nc > best) { best = nc; bs = snc; self = true; }
                    vn[i] = best + row[c];
                    sn[i] = vn[i] > ninf() ? bs : -1;
                    cand[i] = kwd[i] >= 0 && !self && vn[i] > ninf() && vn[i] >= bar[i];
                    any |= cand[i];
                    const bool from_n = nc >= bc;   // the tie rule: n wins
                    const float vb = (from_n ? nc : bc) + lpb;
                    nn_[c] = vn[i];
                    nsn_[c] = sn[i];
                    nb_[c] = vb;
                    nsb_[c] = vb > ninf() ? (from_n ? snc : sbc) : -1;
                }
            }
            if (tid == 0) {
                nn_[0] = 0.f; nsn_[0] = ta + 1;
                nb_[0] = ninf(); nsb_[0] = hold;
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
                // among those: the largest n, then the smallest keyword
                bv = 0.f; bi = -1;
#pragma unroll
                for (int i = 0; i < DS; i++)
                    if (cand[i] && (float)dep[i] == D) best_merge(bv, bi, vn[i], kwd[i]);
                wave_best(bv, bi);
                if (lane == 0) { red_v[4 + wave] = bv; red_i[4 + wave] = bi; }
                __syncthreads();
                bv = red_v[4]; bi = red_i[4];
#pragma unroll
                for (int v = 1; v < DT / 64; v++) best_merge(bv, bi, red_v[4 + v], red_i[4 + v]);
                const int win = bi;
#pragma unroll
                for (int i = 0; i < DS; i++) {
                    const int c = tid + i * DT;
                    if (cand[i] && kwd[i] == win) {
                        if (n_ev < a.max_events) {
                            const long long o = (long long)b * a.max_events + n_ev;
                            a.ev_keyword[o] = win;
                            a.ev_start[o] = sn[i];
                            a.ev_end[o] = ta;
                            a.ev_sum[o] = vn[i];
                        }
                        nsb_[0] = rcv[i];   // the hold, from the next frame on (lane 0's store lies behind the barrier above)
                    }
                    if (c >= 1 && c < S) {   // overlapping matches are suppressed: every token dies with the event
                        nn_[c] = ninf(); nb_[c] = ninf();
                        nsn_[c] = -1; nsb_[c] = -1;
                    }
                }
                n_ev++;
                __syncthreads();
            }
            cur ^= 1;
        }
    }
    if (T == 0) __syncthreads();
#pragma unroll
    for (int i = 0; i < DS; i++) {
        const int c = tid + i * DT;
        if (c < S) {
            const float* v = sm + cur * 4 * up;
            const int* s = reinterpret_cast<const int*>(v + 2 * up);
            a.v_out[so + c] = v[c];
            a.v_out[so + S + c] = v[up + c];
            a.st_out[so + c] = s[c];
            a.st_out[so + S + c] = s[up + c];
        }
    }
    if (tid == 0) a.n_events[b] = n_ev;
}

template <int DS>
void launch(const Ctx& ctx, const CtcKwsArgs& a, size_t lds) {
    static LdsAttrOnce lds_attr;
    lds_attr.ensure(k_ctc_trie_dp<DS>, 150 * 1024);
    hipLaunchKernelGGL(k_ctc_trie_dp<DS>, dim3(a.B), dim3(DT), lds, ctx.stream, a);
}

}  // namespace

void ctc_trie_dp(const Ctx& ctx, const CtcKwsArgs& a) {
    if (ctx.dry) return;
    K2_REQUIRE(a.B > 0 && a.max_S >= 1 && a.max_S <= kKwsMaxStates, "ctc_trie_dp: bad shape B=%d S=%d (at most %d states)", a.B, a.max_S, kKwsMaxStates);
    K2_REQUIRE(a.max_T >= 0 && a.max_T <= a.Tp && a.V >= 1, "ctc_trie_dp: bad shape T=%d T'=%d V=%d", a.max_T, a.Tp, a.V);
    K2_REQUIRE(a.max_events >= a.max_T && a.max_events >= 1, "ctc_trie_dp: %d event slots for %d frames", a.max_events, a.max_T);
    const size_t lds = sizeof(float) * ((8 + F) * (size_t)a.max_S + 16);
    if (a.max_S <= DT) launch<1>(ctx, a, lds);
    else if (a.max_S <= 2 * DT) launch<2>(ctx, a, lds);
    else launch<4>(ctx, a, lds);
    K2_HIP(hipGetLastError());
}

}  // namespace k2hip
