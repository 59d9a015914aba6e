// Modified beam search on device (BASELINE.json configs[2]: "modified-beam-search beam=4").
//
// The reference has no beam search (OfflineRecognizer.cs:54-68 only dispatches "greedy_search"); the
// semantics are icefall's beam_search.py modified_beam_search, restated and tie-broken in
// DESIGN.md.  Frame-synchronous, so the whole search is enqueued up front (4 launches
// per frame, no host round trip): for frame t
//   h = relu(conv(emb(ctx)))  of every hypothesis  k_beam_embconv      [B*K rows]
//   act = tanh(enc[b,t] + decoder_proj(h)[b,k])   one GEMM, the encoder frame added (row / K) before the tanh in its epilogue
//   logits = act . W^T + bias                     gemm_f32_mfma       [B*K, V]
//   per stream: log_softmax + hyp score, top-K over K*V by (score desc, flat index asc), expand,
//   merge equal token sequences by logaddexp (first-inserted hypothesis keeps its timestamps)   k_beam_step
// Hypotheses live in double-buffered device arrays [2][B][K][cap]; ys excludes the ctx-blank prefix.
// Streaming (BeamArgs::rin / rout, kernels.h BeamResumeLayout): the search starts from a stream's saved hypotheses instead of
// [blank, blank]; a hypothesis is then (saved index org, suffix ys of this chunk), its decoder context falls back to the saved
// context while the suffix is shorter than 2, and the merge test of two candidates from different saved hypotheses goes through the
// host's relation table.  With rin == null every one of these is the offline search's own behaviour.
// Hotword biasing (BeamArgs::hw_*): every hypothesis carries the state of the hotword graph; the bonus of a selected
// candidate is looked up after the frame's selection and added before the merges, the new state is written with the hypothesis, and
// the final pick takes back the pending bonus of an unfinished match.  The kernels are templates on HW: HW = false is the unbiased
// search, with nothing added to its code.  Streaming with hotwords (HW and resume): every stream of the call brings its own tables
// (BeamArgs::hw_streams; none = no bonus, state 0), the saved hypotheses' states come in with st_in and the survivors' go out with
// st_out, and the out block's `best` follows the same final pick while the log-probs written keep the pending bonus.
// N-gram LM shallow fusion (BeamArgs::lm; resumed: lst_in / lst_out beside st_in / st_out): every hypothesis also carries the state of the LM's back-off automaton; the
// selected candidates' walks (beam_lm_walk, a wave per candidate) run beside the pair comparisons, before the barrier in front of the
// merge section, which reads term and next state from LDS.  It lives in the HW instantiations behind a null check, as hw_bonus does.
// Neural LM shallow fusion (BeamArgs::nlm; rnn_lm_fuse.hip): in the per-frame launch form only, offline and resumed (the streams' LM
// state then lives in device blocks between the calls: BeamArgs::nlm_io).  The NLM instantiation of the
// step reads the parent's row of the LM's log-probs for a selected real token, adds the scaled term after the n-gram term, and leaves
// for the LM launches behind it each new slot's parent slot and appended token and the frame's "something appended" flag.
// LODR (BeamArgs::lodr; dst_in / dst_out resumed): a second automaton with a state of its own per hypothesis, in the NLM instantiation
// only and behind a null check there: a second pass of beam_lm_walk beside the first, its term added last in the merge section.
#include <type_traits>

#include <atomic>

#include "kernels.h"
#include "sweep.h"
#include "lm_walk.h"
#include "wave_best.h"

namespace k2hip {
namespace {

std::atomic<long long> g_launches[2];   // searches enqueued with HW = false / true (beam_launch_counts)

constexpr int BT = 256;  // threads per stream workgroup

__global__ void k_beam_init(BeamState s, int B) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * s.K) return;
    int k = i % s.K;
    s.lp[i] = k == 0 ? 0.f : -INFINITY;
    s.n[i] = 0;
    s.n[B * s.K + i] = 0;
    s.ctx[2 * i] = K2HIP_BLANK_ID;
    s.ctx[2 * i + 1] = K2HIP_BLANK_ID;
    if (s.st) {
        s.st[i] = 0;
        s.st[B * s.K + i] = 0;
    }
    if (s.lst) {
        s.lst[i] = s.lm.start;
        s.lst[B * s.K + i] = s.lm.start;
    }
    if (s.dst) {
        s.dst[i] = s.lodr.start;
        s.dst[B * s.K + i] = s.lodr.start;
    }
    if (k == 0) s.nhyp[i / s.K] = 1;
}
// the saved hypotheses of every stream (resume): hypothesis k = saved hypothesis k with an empty suffix
__global__ void k_beam_resume_init(BeamState s, int B) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * s.K) return;
    const int K = s.K, k = i % K, b = i / K;
    const BeamResumeLayout L{K, s.Tp};
    const int* in = s.rin + (long long)b * L.in_ints();
    const int nh = in[0];
    s.lp[i] = k < nh ? __int_as_float(in[L.in_lp() + k]) : -INFINITY;
    s.n[i] = 0;
    s.n[B * K + i] = 0;
    s.org[i] = k;
    s.org[B * K + i] = 0;
    s.ctx[2 * i] = k < nh ? in[L.in_ctx() + 2 * k] : K2HIP_BLANK_ID;
    s.ctx[2 * i + 1] = k < nh ? in[L.in_ctx() + 2 * k + 1] : K2HIP_BLANK_ID;
    if (s.st) {
        s.st[i] = (s.st_in && k < nh) ? s.st_in[i] : 0;
        s.st[B * K + i] = 0;
    }
    if (s.lst) {
        s.lst[i] = (s.lst_in && k < nh) ? s.lst_in[i] : 0;
        s.lst[B * K + i] = 0;
    }
    if (s.dst) {
        s.dst[i] = (s.dst_in && k < nh) ? s.dst_in[i] : 0;
        s.dst[B * K + i] = 0;
    }
    if (k == 0) s.nhyp[b] = nh;
}

// relu(Conv1d(k = 2) over (emb[y0], emb[y1]))[co]  (id < 0 -> zero embedding)
__device__ __forceinline__ float embconv1(const DecJoinW& w, long long y0, long long y1, int co) {
    float s = 0.f;
    if (w.cpg <= 4) {
        const int g0 = (co / w.cpg) * w.cpg;
        for (int ci = 0; ci < w.cpg; ci++) {
            const float e0 = y0 >= 0 ? w.emb[y0 * w.DD + g0 + ci] : 0.f;
            const float e1 = y1 >= 0 ? w.emb[y1 * w.DD + g0 + ci] : 0.f;
            s += w.conv[(co * w.cpg + ci) * 2 + 0] * e0;
            s += w.conv[(co * w.cpg + ci) * 2 + 1] * e1;
        }
    } else {
        s = (y0 >= 0 ? w.ptab[y0 * w.DD + co] : 0.f) + (y1 >= 0 ? w.ptab[((long long)w.V + y1) * w.DD + co] : 0.f);
    }
    return fmaxf(s, 0.f);
}
// h[m][co] for every hypothesis row m
__global__ void k_beam_embconv(DecJoinW w, const long long* __restrict__ y, float* __restrict__ h, int M) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)M * w.DD) return;
    const int m = (int)(i / w.DD), co = (int)(i - (long long)m * w.DD);
    h[i] = embconv1(w, y[2 * m], y[2 * m + 1], co);
}

__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, dpp_f<kDppXor1>(v));
    v = fmaxf(v, dpp_f<kDppXor2>(v));
    v = fmaxf(v, dpp_f<kDppHalfMirror>(v));
    v = fmaxf(v, dpp_f<kDppMirror>(v));
    float r = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
#pragma unroll
    for (int row = 1; row < 4; row++) r = fmaxf(r, __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16 * row)));
    return r;
}

// One stream's hypotheses as the step sees them: frame t's input buffers (_c), the other parity's (_n), and the in-place state.
// Global memory (k_beam_step: one launch per frame) or LDS (k_beam_loop: the whole search in one kernel).
struct HypView {
    int K, cap;
    const int *ys_c, *ts_c, *n_c;
    int *ys_n, *ts_n, *n_n;
    float* lp;         // [K] in place: every read of it precedes (barrier-separated) tid 0's write
    long long* ctx;    // [K][2]
    int* nhyp;
    // debug tap (k2hip_debug.h, K2HIP_BEAM_TRACE) or null: this frame's record of this stream, 2 K + 1 words = the selected candidates'
    // flat indexes (slot * V + token) in rank order, their scores (float bits), the number of hypotheses after the merges
    int* trace = nullptr;
    // resume (null: the offline search): saved-hypothesis index of each hypothesis at frame t / t + 1, the stream's in block
    const int* org_c = nullptr;
    int* org_n = nullptr;
    const int* rin = nullptr;
    int Tp = 0;
    // hotword biasing (HW instantiations only): graph state of each hypothesis at frame t / t + 1, the stream's tables [S][V] (null:
    // a stream without a graph in a call that has one -- no bonus, the states stay 0)
    const int* st_c = nullptr;
    int* st_n = nullptr;
    const int* hw_next = nullptr;
    const float* hw_bonus = nullptr;
    // n-gram LM (HW instantiations only; lm.states null: none): LM state of each hypothesis at frame t / t + 1
    const int* lst_c = nullptr;
    int* lst_n = nullptr;
    BeamLm lm;
    // token log-probs (null: not kept, the search does what it does without them): parallel to ts, the unbiased log-softmax term
    // of each emitted token at the frame it was emitted
    const float* yp_c = nullptr;
    float* yp_n = nullptr;
    // neural LM shallow fusion (the NLM instantiation only): the stream's rows of the LM's next-token log-probs at frame t [K][V]; what
    // the step leaves for the LM launches behind it -- for each new slot the GLOBAL slot (nbase + parent) it continues and the token
    // it appended (-1: none) -- and the frame's "some slot appended" flag
    const float* nq_c = nullptr;
    int* npar = nullptr;
    int* ntok = nullptr;
    int* nflag = nullptr;
    int nbase = 0;
    float nscale = 0.f;
    // LODR (the NLM instantiation only; lodr.states null: none): the state of each hypothesis in the second automaton at frame t / t + 1
    const int* dst_c = nullptr;
    int* dst_n = nullptr;
    BeamLm lodr;
};
// a + fl32(s q): the product rounded on its own (no contraction into an fma)
__device__ __forceinline__ float add_scaled(float a, float s, float q) {
#pragma clang fp contract(off)
    const float t = s * q;
    return a + t;
}
constexpr int kStepScratchInts = 4 * kMaxBeam + 4 + 2 * kMaxBeam * kMaxBeam;
constexpr int kYpScratchFloats = kMaxBeam * kMaxBeam + kMaxBeam;
// one workgroup of NT threads per stream; lg: the hypotheses' logits, ldl floats per row; scratch: kStepScratchInts ints of LDS
// pscratch: kYpScratchFloats floats of LDS when hv.yp_n is set (the candidates' unbiased terms beside candv / candi, the top K's)
template <int NT, bool HW, bool NLM = false>
__device__ void beam_step_body(const HypView& hv, const float* lg, int ldl, int V, int t, int* scratch, float* pscratch = nullptr) {
    constexpr int BT = NT;
    float* candp = hv.yp_n ? pscratch : nullptr;
    float* topp = candp ? pscratch + kMaxBeam * kMaxBeam : nullptr;
    int* taken = scratch;
    float* topv = reinterpret_cast<float*>(scratch + kMaxBeam);
    int* topi = scratch + 2 * kMaxBeam;
    float* candv = reinterpret_cast<float*>(scratch + 4 * kMaxBeam + 4);
    int* candi = scratch + 4 * kMaxBeam + 4 + kMaxBeam * kMaxBeam;
    const int tid = threadIdx.x, K = hv.K;
    const int nA = *hv.nhyp;
    // ---- one wave per hypothesis (4 waves, K <= 8): log_softmax statistics, then the hypothesis' own top `want` candidates by
    //      (score desc, token asc) with wave shuffles only; the global top `want` is the top of the union (no block-wide
    //      reductions, which is what made this step cost more than the joiner GEMM)
    const int nc = nA * V, want = min(K, nc);
    const int lane = tid & 63, wave = tid >> 6;
    if (V <= 64 * 16) {
        // the hypothesis' logits, V / 64 per lane, are read ONCE into registers: the max, the sum and the `want` selection rounds below
        // went through global memory 2 + want times before (a chain of dependent loads that made this step 20 us)
        auto select = [&](auto ne_tag) {
            constexpr int NE = decltype(ne_tag)::value;   // elements per lane
            for (int k = wave; k < nA; k += BT / 64) {
                const float* l = lg + (long long)k * ldl;
                float lv[NE];
#pragma unroll
                for (int i = 0; i < NE; i++) lv[i] = lane + 64 * i < V ? l[lane + 64 * i] : -INFINITY;
                float mx = -INFINITY;
#pragma unroll
                for (int i = 0; i < NE; i++) mx = fmaxf(mx, lv[i]);
                mx = wave_max(mx);
                float sm = 0.f;
#pragma unroll
                for (int i = 0; i < NE; i++)
                    if (lane + 64 * i < V) sm += expf(lv[i] - mx);
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) sm += __shfl_xor(sm, o);
                const float lse = logf(sm), lpk = hv.lp[k];
#pragma unroll
                for (int i = 0; i < NE; i++) lv[i] = (lv[i] - mx - lse) + lpk;  // the scores, in the oracle's order of operations
                unsigned used = 0;  // bit i: this lane's element i was already selected
                for (int r = 0; r < want; r++) {
                    float bv = -INFINITY;
                    int bi = -1;
#pragma unroll
                    for (int i = 0; i < NE; i++) {
                        const int v = lane + 64 * i;
                        if (v >= V || (used >> i & 1)) continue;
                        if (bi < 0 || lv[i] > bv) { bv = lv[i]; bi = v; }   // ascending v per lane: first maximum wins
                    }
                    wave_best(bv, bi);
                    if (bi >= 0 && (bi & 63) == lane) used |= 1u << (bi >> 6);
                    if (lane == 0) { candv[k * kMaxBeam + r] = bv; candi[k * kMaxBeam + r] = bi < 0 ? -1 : k * V + bi; }
                    // the unbiased term of the winner, formed from its logit exactly as the score's first two operations were
                    if (candp && lane == 0 && bi >= 0) candp[k * kMaxBeam + r] = (l[bi] - mx) - lse;
                }
            }
        };
        if (V <= 64 * 8) select(std::integral_constant<int, 8>{});
        else select(std::integral_constant<int, 16>{});
    } else
    for (int k = wave; k < nA; k += BT / 64) {
        const float* l = lg + (long long)k * ldl;
        float mx = -INFINITY;
        for (int v = lane; v < V; v += 64) mx = fmaxf(mx, l[v]);
        mx = wave_max(mx);
        float sm = 0.f;
        for (int v = lane; v < V; v += 64) sm += expf(l[v] - mx);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sm += __shfl_xor(sm, o);
        const float lse = logf(sm), lpk = hv.lp[k];
        int excl[kMaxBeam];
        for (int r = 0; r < want; r++) {
            float bv = -INFINITY;
            int bi = -1;
            for (int v = lane; v < V; v += 64) {
                bool tk = false;
                for (int q = 0; q < r; q++) tk |= (excl[q] == v);
                if (tk) continue;
                const float sc = (l[v] - mx - lse) + lpk;  // the oracle's order of operations
                if (bi < 0 || sc > bv) { bv = sc; bi = v; }   // ascending v per lane: first maximum wins
            }
            wave_best(bv, bi);
            excl[r] = bi;
            if (lane == 0) { candv[k * kMaxBeam + r] = bv; candi[k * kMaxBeam + r] = bi < 0 ? -1 : k * V + bi; }
            if (candp && lane == 0 && bi >= 0) candp[k * kMaxBeam + r] = (l[bi] - mx) - lse;
        }
    }
    __syncthreads();
    if (wave == 0) {  // merge the nA x want candidates: lane = k * kMaxBeam + r
        // Each candidate's RANK among all of them (how many beat it: higher score, then lower flat index -- a total order, flat
        // indexes are unique): every candidate is broadcast in turn with v_readlane and compared by all lanes at once, no dependent
        // rounds (`want` rounds of a wave-wide best, each waiting for the one before, were 2 us of the step).
        const bool has = (lane / kMaxBeam) < nA && (lane % kMaxBeam) < want;
        const float myv = has ? candv[lane] : -INFINITY;
        const int myi = has ? candi[lane] : -1;
        int rank = 0;
        for (int k = 0; k < nA; k++)
            for (int r = 0; r < want; r++) {
                const int src = k * kMaxBeam + r;   // (uniform)
                const float ov = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, myv), src));
                const int oi = __builtin_amdgcn_readlane(myi, src);
                if (oi >= 0 && (ov > myv || (ov == myv && oi < myi))) rank++;
            }
        if (myi >= 0 && rank < want) {
            topv[rank] = myv; topi[rank] = myi; taken[rank] = myi;
            if (candp) topp[rank] = candp[lane];
        }
    }
    __syncthreads();
    // ---- expand + merge (HypothesisList.add) into the other buffer
    const int *ys_c = hv.ys_c, *ts_c = hv.ts_c, *n_c = hv.n_c;
    int *ys_n = hv.ys_n, *ts_n = hv.ts_n, *n_n = hv.n_n;
    // sequence of candidate r = ys_c[parent_r][0..n) (+ tok_r if real).  Which candidates spell the same sequence: every pair (r, q < r)
    // compared by a wave of its own (one barrier for all pairs; a loop over the pairs with three block barriers each was a third of
    // the step), then tid 0 resolves the merges in insertion order
    int* eq = candi;   // [r][q] (the per-hypothesis candidates are used up)
    // n-gram LM: term and next state of every selected candidate, a wave each, into LDS for the merge section (candv is used up too)
    float* lmterm = candv;
    int* lmnext = reinterpret_cast<int*>(candv) + kMaxBeam;
    // LODR: the same of the second automaton, behind them
    static_assert(4 * kMaxBeam <= kMaxBeam * kMaxBeam, "the LM and LODR terms and next states live in candv");
    [[maybe_unused]] float* dterm = candv + 2 * kMaxBeam;
    [[maybe_unused]] int* dnext = reinterpret_cast<int*>(candv) + 3 * kMaxBeam;
    if constexpr (HW) {
        if (hv.lm.states)
            for (int r = wave; r < want; r += BT / 64) {
                const int hr = topi[r] / V, tr = topi[r] % V;
                float term = 0.f;
                int nx = hv.lst_c[hr];
                if (tr != K2HIP_BLANK_ID && tr != K2HIP_UNK_ID) beam_lm_walk(hv.lm, nx, tr, lane, &term, &nx);
                if (lane == 0) { lmterm[r] = term; lmnext[r] = nx; }
            }
    }
    if constexpr (NLM) {
        if (hv.lodr.states)
            for (int r = wave; r < want; r += BT / 64) {
                const int hr = topi[r] / V, tr = topi[r] % V;
                float term = 0.f;
                int nx = hv.dst_c[hr];
                if (tr != K2HIP_BLANK_ID && tr != K2HIP_UNK_ID) beam_lm_walk(hv.lodr, nx, tr, lane, &term, &nx);
                if (lane == 0) { dterm[r] = term; dnext[r] = nx; }
            }
    }
    {
        const int npairs = want * (want - 1) / 2;
        for (int pi = wave; pi < npairs; pi += BT / 64) {
            int r = 1, base = 0;
            while (base + r <= pi) { base += r; r++; }
            const int q = pi - base;
            int hr = topi[r] / V, tr = topi[r] % V, hq = topi[q] / V, tq = topi[q] % V;
            // resume: candidates from different saved hypotheses -- r's saved sequence must be q's plus x (or the other way round, then
            // the two swap roles): the sequences are equal iff x + suffix_r == suffix_q
            int xl = 0;
            const int* xp = nullptr;
            bool e = true;
            if (hv.org_c) {
                const BeamResumeLayout L{K, hv.Tp};
                const int orr = hv.org_c[hr], oq = hv.org_c[hq];
                if (orr != oq) {
                    const int lrq = hv.rin[L.in_rel() + orr * K + oq], lqr = hv.rin[L.in_rel() + oq * K + orr];
                    if (lrq > 0) {
                        xl = lrq;
                        xp = hv.rin + L.in_relx() + (orr * K + oq) * hv.Tp;
                    } else if (lqr > 0) {
                        xl = lqr;
                        xp = hv.rin + L.in_relx() + (oq * K + orr) * hv.Tp;
                        const int h = hr, tk = tr;
                        hr = hq; tr = tq; hq = h; tq = tk;
                    } else {
                        e = false;
                    }
                }
            }
            const bool realr = tr != K2HIP_BLANK_ID && tr != K2HIP_UNK_ID, realq = tq != K2HIP_BLANK_ID && tq != K2HIP_UNK_ID;
            const int lenr = n_c[hr] + (realr ? 1 : 0), lenq = n_c[hq] + (realq ? 1 : 0);
            e = e && xl + lenr == lenq;
            if (e) {
                for (int i = lane; i < lenq; i += 64) {
                    const int j = i - xl;
                    const int x = j < 0 ? xp[i] : (j < n_c[hr]) ? ys_c[(long long)hr * hv.cap + j] : tr;
                    const int y = (i < n_c[hq]) ? ys_c[(long long)hq * hv.cap + i] : tq;
                    e = e && x == y;
                }
            }
            e = __all(e);
            if (lane == 0) eq[r * kMaxBeam + q] = e ? 1 : 0;
        }
    }
    __syncthreads();
    if (tid == 0) {
        // One thread resolves the merges in insertion order.  Everything it needs is read up front (independent LDS loads) and kept in
        // registers -- fully unrolled, selects instead of indexed arrays: as a loop over LDS this was a chain of ~40 dependent
        // accesses, 2 us of the step.
        float tv[kMaxBeam], lpn[kMaxBeam];
        unsigned eqm[kMaxBeam];   // bit q of eqm[r]: candidates r and q < r spell the same sequence
#pragma unroll
        for (int r = 0; r < kMaxBeam; r++) {
            tv[r] = r < want ? topv[r] : -INFINITY;
            if constexpr (HW) {
                // the selected candidate's bonus (the selection itself and the tap's `val` stay unbiased): independent loads
                if (r < want) {
                    const int hr = topi[r] / V, tr = topi[r] % V;
                    if (hv.hw_bonus && tr != K2HIP_BLANK_ID && tr != K2HIP_UNK_ID) tv[r] += hv.hw_bonus[(long long)hv.st_c[hr] * V + tr];
                    if (hv.lm.states) tv[r] += lmterm[r];   // (sum + hotword bonus) + LM term
                    if constexpr (NLM) {   // ... + fl32(scale q_parent[token])
                        if (tr != K2HIP_BLANK_ID && tr != K2HIP_UNK_ID) tv[r] = add_scaled(tv[r], hv.nscale, hv.nq_c[(long long)hr * V + tr]);
                        if (hv.lodr.states) tv[r] += dterm[r];   // ... + Step_lodr(state, token), last
                    }
                }
            }
            lpn[r] = -INFINITY;
            eqm[r] = 0;
#pragma unroll
            for (int q = 0; q < r; q++)
                if (r < want && eq[r * kMaxBeam + q]) eqm[r] |= 1u << q;
        }
        unsigned merged = 0;      // bit q: candidate q was merged into an earlier one
        int slot_of[kMaxBeam];
        int nN = 0;
#pragma unroll
        for (int r = 0; r < kMaxBeam; r++) {
            if (r < want) {
                // the earliest earlier entry with the same sequence that was not merged away itself, or none
                const unsigned cand = eqm[r] & ~merged;
                const int found = cand ? __ffs(cand) - 1 : -1;
                int sl = nN;
                if (found >= 0) {
                    merged |= 1u << r;
#pragma unroll
                    for (int q = 0; q < r; q++)
                        if (q == found) sl = slot_of[q];
                }
                slot_of[r] = sl;
                // slot assignment in insertion order; merged scores accumulate in candidate order (logaddexp)
                float cur = -INFINITY;
#pragma unroll
                for (int q = 0; q < kMaxBeam; q++)
                    if (q == sl) cur = lpn[q];
                float nv = tv[r];
                if (found >= 0) {
                    const float mx = fmaxf(cur, tv[r]);
                    nv = (isinf(mx) && mx < 0) ? mx : mx + log1pf(expf(-fabsf(cur - tv[r])));
                } else {
                    nN++;
                }
#pragma unroll
                for (int q = 0; q < kMaxBeam; q++)
                    if (q == sl) lpn[q] = nv;
                taken[r] = found < 0 ? sl : -1;  // reuse: destination slot of a fresh hypothesis
            }
        }
#pragma unroll
        for (int q = 0; q < kMaxBeam; q++)
            if (q < nN) hv.lp[q] = lpn[q];
        for (int k = nN; k < K; k++) {
            hv.lp[k] = -INFINITY;
            // empty slots still go through the batched decoder launch: give them a valid context
            hv.ctx[2 * k] = K2HIP_BLANK_ID;
            hv.ctx[2 * k + 1] = K2HIP_BLANK_ID;
            n_n[k] = 0;
            if (hv.org_n) hv.org_n[k] = 0;
            if constexpr (HW) {
                hv.st_n[k] = 0;
                if (hv.lst_n) hv.lst_n[k] = 0;
            }
            if constexpr (NLM) {   // (empty slots still go through the LM launches: a valid parent, nothing appended)
                hv.npar[k] = hv.nbase;
                hv.ntok[k] = -1;
                if (hv.dst_n) hv.dst_n[k] = 0;
            }
        }
        *hv.nhyp = nN;
        if (hv.trace) hv.trace[2 * K] = nN;
    }
    if (hv.trace && tid < K) {
        hv.trace[tid] = tid < want ? topi[tid] : -1;
        hv.trace[K + tid] = __float_as_int(tid < want ? topv[tid] : -INFINITY);
    }
    __syncthreads();
    for (int r = wave; r < want; r += BT / 64) {   // a wave per surviving candidate (distinct destination slots)
        const int slot = taken[r];
        if (slot < 0) continue;
        const int hr = topi[r] / V, tr = topi[r] % V;
        const bool realr = tr != K2HIP_BLANK_ID && tr != K2HIP_UNK_ID;
        const int n0 = n_c[hr];
        for (int i = lane; i < n0; i += 64) {
            ys_n[(long long)slot * hv.cap + i] = ys_c[(long long)hr * hv.cap + i];
            ts_n[(long long)slot * hv.cap + i] = ts_c[(long long)hr * hv.cap + i];
        }
        if (hv.yp_n)
            for (int i = lane; i < n0; i += 64) hv.yp_n[(long long)slot * hv.cap + i] = hv.yp_c[(long long)hr * hv.cap + i];
        if (lane == 0) {
            int nn = n0;
            if (realr) {
                if (nn < hv.cap) {
                    ys_n[(long long)slot * hv.cap + nn] = tr;
                    ts_n[(long long)slot * hv.cap + nn] = t;
                    if (hv.yp_n) hv.yp_n[(long long)slot * hv.cap + nn] = topp[r];
                }
                nn++;
            }
            n_n[slot] = nn;
            if constexpr (HW) {
                hv.st_n[slot] = (realr && hv.hw_next) ? hv.hw_next[(long long)hv.st_c[hr] * V + tr] : hv.st_c[hr];
                if (hv.lst_n) hv.lst_n[slot] = lmnext[r];
            }
            if constexpr (NLM) {
                hv.npar[slot] = hv.nbase + hr;
                hv.ntok[slot] = realr ? tr : -1;
                if (realr) *hv.nflag = 1;
                if (hv.dst_n) hv.dst_n[slot] = dnext[r];
            }
            // decoder context of the new hypothesis: last two of [c0, c1] + ys, [c0, c1] = the saved hypothesis' context (resume) or
            // [blank, blank]
            long long c0 = K2HIP_BLANK_ID, c1 = K2HIP_BLANK_ID;
            if (hv.org_c) {
                const int o = hv.org_c[hr];
                hv.org_n[slot] = o;
                c0 = hv.rin[BeamResumeLayout{K, hv.Tp}.in_ctx() + 2 * o];
                c1 = hv.rin[BeamResumeLayout{K, hv.Tp}.in_ctx() + 2 * o + 1];
            }
            long long y1 = nn >= 1 ? (realr ? tr : ys_c[(long long)hr * hv.cap + n0 - 1]) : c1;
            long long y0 = nn == 1 ? c1 : c0;
            if (nn >= 2) y0 = realr ? ys_c[(long long)hr * hv.cap + n0 - 1] : ys_c[(long long)hr * hv.cap + n0 - 2];
            hv.ctx[2 * slot] = y0;
            hv.ctx[2 * slot + 1] = y1;
        }
    }
}

// one workgroup per stream; `cur` = buffer holding frame t's input hypotheses
template <bool HW, bool NLM = false>
__global__ __launch_bounds__(BT) void k_beam_step(BeamState s, const float* __restrict__ logits, int V, int t, int cur, int B, int* trace, int Tp) {
    __shared__ int scratch[kStepScratchInts];
    __shared__ float pscratch[kYpScratchFloats];
    const int b = blockIdx.x, K = s.K, nxt = cur ^ 1;
    const long long BK = (long long)B * K;
    HypView hv;
    hv.K = K; hv.cap = s.cap;
    hv.ys_c = s.ys + ((long long)cur * BK + (long long)b * K) * s.cap;
    hv.ts_c = s.ts + ((long long)cur * BK + (long long)b * K) * s.cap;
    hv.ys_n = s.ys + ((long long)nxt * BK + (long long)b * K) * s.cap;
    hv.ts_n = s.ts + ((long long)nxt * BK + (long long)b * K) * s.cap;
    hv.n_c = s.n + cur * BK + b * K;
    hv.n_n = s.n + nxt * BK + b * K;
    hv.lp = s.lp + b * K;
    hv.ctx = s.ctx + 2 * (long long)b * K;
    hv.nhyp = s.nhyp + b;
    hv.trace = trace ? trace + ((long long)b * Tp + t) * (2 * K + 1) : nullptr;
    if (s.org) {
        hv.org_c = s.org + cur * BK + b * K;
        hv.org_n = s.org + nxt * BK + b * K;
        hv.rin = s.rin + (long long)b * BeamResumeLayout{K, s.Tp}.in_ints();
        hv.Tp = s.Tp;
    }
    if constexpr (HW) {
        hv.st_c = s.st + cur * BK + b * K;
        hv.st_n = s.st + nxt * BK + b * K;
        hv.hw_next = s.hw_streams ? s.hw_streams[b].next : s.hw_next;
        hv.hw_bonus = s.hw_streams ? s.hw_streams[b].bonus : s.hw_bonus;
        if (s.lst) {
            hv.lst_c = s.lst + cur * BK + b * K;
            hv.lst_n = s.lst + nxt * BK + b * K;
            hv.lm = s.lm;
        }
    }
    if (s.yp) {
        hv.yp_c = s.yp + ((long long)cur * BK + (long long)b * K) * s.cap;
        hv.yp_n = s.yp + ((long long)nxt * BK + (long long)b * K) * s.cap;
    }
    if constexpr (NLM) {
        hv.nq_c = s.nq + ((long long)cur * BK + (long long)b * K) * V;
        hv.npar = s.npar + b * K;
        hv.ntok = s.ntok + b * K;
        hv.nflag = s.nflag + t;
        hv.nbase = b * K;
        hv.nscale = s.nscale;
        if (s.dst) {
            hv.dst_c = s.dst + cur * BK + b * K;
            hv.dst_n = s.dst + nxt * BK + b * K;
            hv.lodr = s.lodr;
        }
    }
    beam_step_body<BT, HW, NLM>(hv, logits + (long long)b * K * V, V, V, t, scratch, pscratch);
}

// resume: every surviving hypothesis of the stream into its out block, and the best one (get_most_probable over the WHOLE
// sequences: length = |saved| + |suffix| + the 2 ctx blanks, first maximum).  ys / ts / n / org: the final parity's [K][cap] / [K]
// arrays of the stream.  Called by all threads of a workgroup.
// HW: st = the hypotheses' graph states, pending = the stream's table or null; the pick is made on lp - pending(state) (an unfinished
// match earns nothing), the log-probs go out as they are, the states to st_out [K].
template <bool HW>
__device__ void beam_resume_write(const int* in, int* out, int K, int Tp, int cap, int nh, const float* lp, const long long* ctx,
                                  const int* n, const int* org, const int* ys, const int* ts, const int* st = nullptr,
                                  const float* pending = nullptr, int* st_out = nullptr, const float* yp = nullptr, float* yp_out = nullptr,
                                  const int* lst = nullptr, int* lst_out = nullptr, const int* dst = nullptr, int* dst_out = nullptr) {
    const BeamResumeLayout L{K, Tp};
    const int tid = threadIdx.x;
    if (tid == 0) {
        int best = 0;
        float bs = -INFINITY;
        for (int k = 0; k < nh; k++) {
            float l = lp[k];
            if constexpr (HW) {
                if (pending) l -= pending[st[k]];
            }
            const float v = l / (float)(in[L.in_len() + org[k]] + n[k] + 2);
            if (k == 0 || v > bs) { bs = v; best = k; }
        }
        out[0] = nh;
        out[1] = best;
    }
    for (int k = tid; k < K; k += blockDim.x) {
        const bool live = k < nh;
        out[L.out_org() + k] = live ? org[k] : 0;
        out[L.out_n() + k] = live ? n[k] : 0;
        out[L.out_lp() + k] = __float_as_int(live ? lp[k] : -INFINITY);
        out[L.out_ctx() + 2 * k] = live ? (int)ctx[2 * k] : K2HIP_BLANK_ID;
        out[L.out_ctx() + 2 * k + 1] = live ? (int)ctx[2 * k + 1] : K2HIP_BLANK_ID;
        if constexpr (HW) {
            if (st_out) st_out[k] = live ? st[k] : 0;
            if (lst_out) lst_out[k] = live ? lst[k] : 0;
            if (dst_out) dst_out[k] = live ? dst[k] : 0;
        }
    }
    for (int i = tid; i < nh * Tp; i += blockDim.x) {
        const int k = i / Tp, j = i - k * Tp;
        if (j < n[k] && j < cap) {
            out[L.out_ys() + i] = ys[(long long)k * cap + j];
            out[L.out_ts() + i] = ts[(long long)k * cap + j];
            if (yp_out) yp_out[i] = yp[(long long)k * cap + j];   // side block [K][Tp]: the suffixes' token log-probs
        }
    }
}
template <bool HW>
__global__ void k_beam_resume_final(BeamState s, int fin, int B, int* __restrict__ rout) {
    const int b = blockIdx.x, K = s.K;
    const long long BK = (long long)B * K;
    const BeamResumeLayout L{K, s.Tp};
    if constexpr (HW)
        beam_resume_write<true>(s.rin + (long long)b * L.in_ints(), rout + (long long)b * L.out_ints(), K, s.Tp, s.cap, s.nhyp[b], s.lp + b * K,
                                s.ctx + 2 * (long long)b * K, s.n + fin * BK + b * K, s.org + fin * BK + b * K,
                                s.ys + (fin * BK + (long long)b * K) * s.cap, s.ts + (fin * BK + (long long)b * K) * s.cap,
                                s.st + fin * BK + b * K, s.hw_streams ? s.hw_streams[b].pending : s.hw_pending,
                                s.st_out ? s.st_out + b * K : nullptr, s.yp ? s.yp + (fin * BK + (long long)b * K) * s.cap : nullptr,
                                s.yp_out ? s.yp_out + (long long)b * K * s.Tp : nullptr, s.lst ? s.lst + fin * BK + b * K : nullptr,
                                s.lst_out ? s.lst_out + b * K : nullptr, s.dst ? s.dst + fin * BK + b * K : nullptr,
                                (s.dst && s.dst_out) ? s.dst_out + b * K : nullptr);
    else
        beam_resume_write<false>(s.rin + (long long)b * L.in_ints(), rout + (long long)b * L.out_ints(), K, s.Tp, s.cap, s.nhyp[b], s.lp + b * K,
                                 s.ctx + 2 * (long long)b * K, s.n + fin * BK + b * K, s.org + fin * BK + b * K,
                                 s.ys + (fin * BK + (long long)b * K) * s.cap, s.ts + (fin * BK + (long long)b * K) * s.cap, nullptr, nullptr,
                                 nullptr, s.yp ? s.yp + (fin * BK + (long long)b * K) * s.cap : nullptr,
                                 s.yp_out ? s.yp_out + (long long)b * K * s.Tp : nullptr);
}

// N-best: up to nb.nbest of the stream's nh final hypotheses in the order of the final pick -- (final log-prob) / (length + 2)
// descending, ties in insertion order, so entry 0 is the hypothesis the single-result code picks.  Called by all threads of a
// workgroup; n / ys / ts / yp: the final parity's [K] / [K][cap] arrays of the stream, final_lp(k): the finalized log-prob.
template <typename FinalLp>
__device__ void beam_nbest_write(const BeamNbest& nb, int b, int nh, int cap, int max_tokens, const int* n, const int* ys, const int* ts,
                                 const float* yp, FinalLp final_lp, int* overflow) {
    float v[kMaxBeam];
#pragma unroll
    for (int k = 0; k < kMaxBeam; k++) v[k] = k < nh ? final_lp(k) / (float)(n[k] + 2) : -INFINITY;
    for (int k = 0; k < nh; k++) {
        int rank = 0;
#pragma unroll
        for (int j = 0; j < kMaxBeam; j++)
            if (j < nh && (v[j] > v[k] || (v[j] == v[k] && j < k))) rank++;
        if (rank >= nb.nbest) continue;
        const int len = n[k];
        if (len > max_tokens || len > cap) {   // (the single result's rule, per entry)
            if (threadIdx.x == 0) *overflow = 1;
            continue;
        }
        const long long o = ((long long)b * nb.nbest + rank) * max_tokens;
        for (int i = threadIdx.x; i < len; i += blockDim.x) {
            nb.tokens[o + i] = ys[(long long)k * cap + i];
            nb.timestamps[o + i] = ts[(long long)k * cap + i];
            nb.token_log_probs[o + i] = yp[(long long)k * cap + i];
        }
        if (threadIdx.x == 0) {
            nb.n_tokens[b * nb.nbest + rank] = len;
            nb.scores[b * nb.nbest + rank] = final_lp(k);
        }
    }
    if (threadIdx.x == 0) nb.n_hyps[b] = min(nh, nb.nbest);
}

// ---- the whole search of a stream in one kernel (small vocabularies: the model's all-contexts decoder table) -----------------
// One workgroup of GT threads per stream walks the T' frames: the K hypotheses' decoder outputs are rows of the table, their
// joiner inputs tanh(enc_t + dec_k) take the place of k_greedy's 8 speculated frames in the same sweep of the joiner matrix on the
// matrix pipe (mfma_sweep_rows: 8 hypotheses x 256 columns per pass), the logits stay in LDS, and the step (log-softmax, top K,
// expand, merge) is beam_step_body on hypotheses that live in LDS as well.  Replaces 4 launches per frame (1012 for the headline
// batch, each waiting for slots between the next batch's encoder GEMMs) by one launch per batch.
// Forms of the sweep: beam <= 4 uses the lower 4 x 4 half of each MFMA; with V <= 512 both 256-column chunks go through one pass
// (mfma_sweep_rows_2c), or -- when 2 B workgroups fit the co-residency budget -- each chunk gets a workgroup of its own and the two
// exchange their 4 x 256 logits per frame as tagged granules (BeamLoopArgs::xg; bounded waits, *overflow = 2 on a timeout and a repeat
// with one workgroup per stream, as for k_greedy's parts).
typedef __attribute__((address_space(1))) unsigned long long bgu64;
__device__ __forceinline__ void bstore_granule(unsigned long long* g, unsigned epoch, unsigned value) {
    __hip_atomic_store((bgu64*)g, ((unsigned long long)epoch << 32) | value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long bload_granule(const unsigned long long* g) {
    return __hip_atomic_load((bgu64*)g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// LDS (floats): actT[J GF] | psum | lg[GF][Vp] | ctx[2 GF] (long long) | lp[GF] | n[2][GF] | org[2][GF] | st[2][GF], lst[2][GF] (biased only) |
// nhyp, pad | scratch | ys[2][K][cap] | ts[2][K][cap]
// with token log-probs (yp): ... | scratch | yp scratch | ys | ts | yp[2][K][cap]
__host__ __device__ inline size_t beam_loop_lds_floats(int J, int Vp, int K, int cap, bool hyp_in_lds, bool hw, bool yp) {
    return (size_t)J * GF + kPsumFloats + (size_t)GF * Vp + 4 * GF + GF + 2 * GF + 2 * GF + (hw ? 4 * GF : 0) + 4 + kStepScratchInts + 4 +
           (yp ? kYpScratchFloats : 0) + (hyp_in_lds ? (yp ? 6 : 4) * (size_t)K * cap : 0);
}
template <int NH, bool HW>   // NH = 1: beam <= 4, the sweep forms only rows 0..3; HW: hotword biasing
__global__ __launch_bounds__(GT) void k_beam_loop(DecJoinW w, BeamLoopArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* actT = sm;
    float* psum = actT + w.J * GF;
    float* lg = psum + kPsumFloats;
    long long* ctx = reinterpret_cast<long long*>(lg + GF * w.Vp);   // (J GF, the psum size and GF Vp are multiples of 4 floats)
    float* lp = reinterpret_cast<float*>(ctx + 2 * GF);
    int* nbuf = reinterpret_cast<int*>(lp + GF);       // [2][GF]
    int* orgb = nbuf + 2 * GF;                          // [2][GF] (resume)
    int* stb = orgb + 2 * GF;                           // [2][GF] (hotwords)
    int* lstb = stb + 2 * GF;                           // [2][GF] (n-gram LM)
    int* nhyp = stb + (HW ? 4 * GF : 0);
    int* scratch = nhyp + 4;
    // token log-probs (a.want_yp; the whole launch takes one side of this branch): the step's extra scratch, and yp beside ys / ts
    float* pscratch = a.want_yp ? reinterpret_cast<float*>(scratch + kStepScratchInts + 4) : nullptr;
    int* ys = a.ys_g ? a.ys_g + (size_t)blockIdx.x * 2 * a.K * a.cap : scratch + kStepScratchInts + 4 + (a.want_yp ? kYpScratchFloats : 0);
    int* ts = a.ys_g ? a.ts_g + (size_t)blockIdx.x * 2 * a.K * a.cap : ys + 2 * a.K * a.cap;
    float* yp = !a.want_yp ? nullptr : a.ys_g ? a.yp_g + (size_t)blockIdx.x * 2 * a.K * a.cap : reinterpret_cast<float*>(ts + 2 * a.K * a.cap);
    __shared__ int xfail;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, K = a.K;
    if (tid == 0) xfail = 0;
    const int b = a.xg ? blockIdx.x >> 1 : blockIdx.x, slab = a.xg ? blockIdx.x & 1 : 0;
    const float* enc = a.enc + (long long)b * a.Tp * w.J;
    const BeamResumeLayout RL{K, a.Tp};
    const int* rin = a.rin ? a.rin + (long long)b * RL.in_ints() : nullptr;
    // this stream's hotword tables: its own (streaming) or the call's one graph
    BeamHwStream hws;
    if constexpr (HW) {
        if (a.hw_streams) hws = a.hw_streams[b];
        else hws = BeamHwStream{a.hw_next, a.hw_bonus, a.hw_pending};
    }
    if (tid < GF) {   // k_beam_init / k_beam_resume_init
        nbuf[tid] = 0;
        nbuf[GF + tid] = 0;
        orgb[tid] = tid;
        orgb[GF + tid] = 0;
        if constexpr (HW) {
            stb[tid] = 0;
            stb[GF + tid] = 0;
            lstb[tid] = a.lm.start;
            lstb[GF + tid] = a.lm.start;
        }
        if (rin) {
            const int nh = rin[0];
            const bool live = tid < nh && tid < K;
            lp[tid] = live ? __int_as_float(rin[RL.in_lp() + tid]) : -INFINITY;
            ctx[2 * tid] = live ? rin[RL.in_ctx() + 2 * tid] : K2HIP_BLANK_ID;
            ctx[2 * tid + 1] = live ? rin[RL.in_ctx() + 2 * tid + 1] : K2HIP_BLANK_ID;
            if constexpr (HW) {
                if (a.st_in && live) stb[tid] = a.st_in[b * K + tid];   // the saved hypotheses' graph states
                lstb[tid] = (a.lst_in && live) ? a.lst_in[b * K + tid] : 0;     // ... and LM states
                lstb[GF + tid] = 0;
            }
            if (tid == 0) *nhyp = nh;
        } else {
            lp[tid] = tid == 0 ? 0.f : -INFINITY;
            ctx[2 * tid] = K2HIP_BLANK_ID;
            ctx[2 * tid + 1] = K2HIP_BLANK_ID;
            if (tid == 0) *nhyp = 1;
        }
    }
    __syncthreads();
    const int kper = w.J >> 3, ncg = w.Vp >> 2;
    for (int t = 0; t < a.Tp; t++) {
        const int nA = *nhyp, cur = t & 1;
        // joiner inputs of the live hypotheses (row q of the sweep = hypothesis q); rows past nA are zero and ignored
        for (int k = tid; k < w.J; k += GT) {
            const float e = enc[(long long)t * w.J + k];
            float d[4 * NH];
#pragma unroll
            for (int q = 0; q < 4 * NH; q++) {
                const long long y0 = ctx[2 * min(q, K - 1)], y1 = ctx[2 * min(q, K - 1) + 1];   // (empty slots hold [blank, blank])
                d[q] = w.dec_table[((y0 + 1) * w.V + y1) * (long long)w.J + k];
            }
#pragma unroll
            for (int q = 0; q < GF; q++) actT[k * GF + q] = (q < 4 * NH && q < nA) ? tanhf(e + d[q < 4 * NH ? q : 0]) : 0.f;
        }
        __syncthreads();
        if (NH == 1 && a.xg) {
            // two slabs: this workgroup's 256-column chunk, then the peer's logits through tagged granules
            f32x4 c[2][4];
#pragma unroll
            for (int hh = 0; hh < 2; hh++)
#pragma unroll
                for (int q = 0; q < 4; q++) c[hh][q] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int cg = 64 * slab + lane;
            mfma_sweep_rows<1>(w.out_kn + (long long)(wave * kper) * w.Vp + 4 * min(cg, ncg - 1), w.Vp, actT + (wave * kper) * GF + (lane & 3), kper, c);
            psum_store<1>(psum, wave, lane, c);
            __syncthreads();
            unsigned long long* xo = a.xg + ((((long long)b * 2 + (t & 1)) * 2 + slab) * 4) * 256;
            const unsigned long long* xi = a.xg + ((((long long)b * 2 + (t & 1)) * 2 + (slab ^ 1)) * 4) * 256;
            if (wave < 4) {   // wave q: hypothesis q's 256 logits of this slab (computed for every slot: the peer must not wait on nA)
                float4 ps[8];
#pragma unroll
                for (int sl = 0; sl < 8; sl++) ps[sl] = *reinterpret_cast<const float4*>(psum + (sl * GF + wave) * 256 + 4 * lane);
                float sj[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const float p0 = (&ps[0].x)[j], p1 = (&ps[1].x)[j], p2 = (&ps[2].x)[j], p3 = (&ps[3].x)[j];
                    const float p4 = (&ps[4].x)[j], p5 = (&ps[5].x)[j], p6 = (&ps[6].x)[j], p7 = (&ps[7].x)[j];
                    const int col = 4 * min(cg, ncg - 1) + j;
                    sj[j] = (((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7))) + (col < w.V ? w.out_b[col] : 0.f);
                }
                if (cg < ncg) *reinterpret_cast<float4*>(lg + wave * w.Vp + 4 * cg) = make_float4(sj[0], sj[1], sj[2], sj[3]);
#pragma unroll
                for (int j = 0; j < 4; j++) bstore_granule(xo + wave * 256 + 4 * lane + j, (unsigned)(t + 1), __float_as_uint(sj[j]));
            }
            // every thread collects 2 of the peer's 1024 granules
            for (int e = tid; e < 4 * 256; e += GT) {
                unsigned long long x = bload_granule(xi + e);
                for (unsigned spins = 0; (unsigned)(x >> 32) != (unsigned)(t + 1) && spins < (1u << 22); spins++) {
                    __builtin_amdgcn_s_sleep(1);
                    x = bload_granule(xi + e);
                }
                if ((unsigned)(x >> 32) != (unsigned)(t + 1)) xfail = 1;
                const int q = e >> 8, col = 256 * (slab ^ 1) + (e & 255);
                if (col < w.Vp) lg[q * w.Vp + col] = __uint_as_float((unsigned)x);
            }
            __syncthreads();
            if (xfail) {
                if (tid == 0) *a.overflow = 2;
                return;
            }
        } else if (NH == 1 && ncg <= 128) {
            // beam <= 4 and V <= 512: both 256-column chunks in ONE pass -- the 4 live rows leave half of the accumulators and of the
            // exchange area free, so the second chunk rides along: one LDS exchange and one pair of barriers per frame instead of two
            f32x4 c[2][4];
#pragma unroll
            for (int hh = 0; hh < 2; hh++)
#pragma unroll
                for (int q = 0; q < 4; q++) c[hh][q] = f32x4{0.f, 0.f, 0.f, 0.f};
            const float* wrow = w.out_kn + (long long)(wave * kper) * w.Vp;
            mfma_sweep_rows_2c(wrow + 4 * min(lane, ncg - 1), wrow + 4 * min(64 + lane, ncg - 1), w.Vp, actT + (wave * kper) * GF + (lane & 3), kper, c);
            // psum[slice][row 0..3][512 columns]
#pragma unroll
            for (int ch = 0; ch < 2; ch++)
#pragma unroll
                for (int i = 0; i < 4; i++)
                    *reinterpret_cast<float4*>(psum + ((wave * 4) + i) * 512 + 256 * ch + 4 * lane) = make_float4(c[ch][0][i], c[ch][1][i], c[ch][2][i], c[ch][3][i]);
            __syncthreads();
            {
                const int q = wave & 3, ch = wave >> 2, cg = 64 * ch + lane;   // wave: hypothesis q's chunk ch
                if (cg < ncg && q < nA) {
                    float4 ps[8];
#pragma unroll
                    for (int sl = 0; sl < 8; sl++) ps[sl] = *reinterpret_cast<const float4*>(psum + ((sl * 4) + q) * 512 + 256 * ch + 4 * lane);
                    float sj[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const float p0 = (&ps[0].x)[j], p1 = (&ps[1].x)[j], p2 = (&ps[2].x)[j], p3 = (&ps[3].x)[j];
                        const float p4 = (&ps[4].x)[j], p5 = (&ps[5].x)[j], p6 = (&ps[6].x)[j], p7 = (&ps[7].x)[j];
                        const int col = 4 * cg + j;
                        sj[j] = (((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7))) + (col < w.V ? w.out_b[col] : 0.f);
                    }
                    *reinterpret_cast<float4*>(lg + q * w.Vp + 4 * cg) = make_float4(sj[0], sj[1], sj[2], sj[3]);
                }
            }
            __syncthreads();
        } else
        for (int cgb = 0; cgb < ncg; cgb += 64) {
            const int cg = cgb + lane;
            f32x4 c[2][4];
#pragma unroll
            for (int hh = 0; hh < 2; hh++)
#pragma unroll
                for (int q = 0; q < 4; q++) c[hh][q] = f32x4{0.f, 0.f, 0.f, 0.f};
            mfma_sweep_rows<NH>(w.out_kn + (long long)(wave * kper) * w.Vp + 4 * min(cg, ncg - 1), w.Vp, actT + (wave * kper) * GF + (lane & 3), kper, c);
            psum_store<NH>(psum, wave, lane, c);
            __syncthreads();
            if (cg < ncg && wave < nA) {   // wave q: hypothesis q's 256 logits of this pass, slices added in k_greedy's order
                float4 ps[8];
#pragma unroll
                for (int q = 0; q < 8; q++) ps[q] = *reinterpret_cast<const float4*>(psum + (q * GF + wave) * 256 + 4 * lane);
                float sj[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const float p0 = (&ps[0].x)[j], p1 = (&ps[1].x)[j], p2 = (&ps[2].x)[j], p3 = (&ps[3].x)[j];
                    const float p4 = (&ps[4].x)[j], p5 = (&ps[5].x)[j], p6 = (&ps[6].x)[j], p7 = (&ps[7].x)[j];
                    const int col = 4 * cg + j;
                    sj[j] = (((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7))) + (col < w.V ? w.out_b[col] : 0.f);
                }
                *reinterpret_cast<float4*>(lg + wave * w.Vp + 4 * cg) = make_float4(sj[0], sj[1], sj[2], sj[3]);
            }
            __syncthreads();
        }
        HypView hv;
        hv.K = K; hv.cap = a.cap;
        hv.ys_c = ys + (size_t)cur * K * a.cap; hv.ts_c = ts + (size_t)cur * K * a.cap; hv.n_c = nbuf + cur * GF;
        hv.ys_n = ys + (size_t)(cur ^ 1) * K * a.cap; hv.ts_n = ts + (size_t)(cur ^ 1) * K * a.cap; hv.n_n = nbuf + (cur ^ 1) * GF;
        hv.lp = lp; hv.ctx = ctx; hv.nhyp = nhyp;
        hv.trace = (a.trace && slab == 0) ? a.trace + ((long long)b * a.Tp + t) * (2 * K + 1) : nullptr;
        if (rin) {
            hv.org_c = orgb + cur * GF;
            hv.org_n = orgb + (cur ^ 1) * GF;
            hv.rin = rin;
            hv.Tp = a.Tp;
        }
        if constexpr (HW) {
            hv.st_c = stb + cur * GF;
            hv.st_n = stb + (cur ^ 1) * GF;
            hv.hw_next = hws.next;
            hv.hw_bonus = hws.bonus;
            if (a.lm.states) {
                hv.lst_c = lstb + cur * GF;
                hv.lst_n = lstb + (cur ^ 1) * GF;
                hv.lm = a.lm;
            }
        }
        if (yp) {
            hv.yp_c = yp + (size_t)cur * K * a.cap;
            hv.yp_n = yp + (size_t)(cur ^ 1) * K * a.cap;
        }
        beam_step_body<GT, HW>(hv, lg, w.Vp, w.V, t, scratch, pscratch);
        __syncthreads();
    }
    // k_beam_final: max of log_prob / len(ys) (len counts the 2 ctx blanks), first maximum
    const int fin = a.Tp & 1;
    const int* n_f = nbuf + fin * GF;
    if (rin) {   // (resume runs one workgroup per stream: no slabs)
        if constexpr (HW)
            beam_resume_write<true>(rin, a.rout + (long long)b * RL.out_ints(), K, a.Tp, a.cap, *nhyp, lp, ctx, n_f, orgb + fin * GF,
                                    ys + (size_t)fin * K * a.cap, ts + (size_t)fin * K * a.cap, stb + fin * GF, hws.pending,
                                    a.st_out ? a.st_out + b * K : nullptr, yp ? yp + (size_t)fin * K * a.cap : nullptr,
                                    a.yp_out ? a.yp_out + (long long)b * K * a.Tp : nullptr, lstb + fin * GF,
                                    a.lst_out ? a.lst_out + b * K : nullptr);
        else
            beam_resume_write<false>(rin, a.rout + (long long)b * RL.out_ints(), K, a.Tp, a.cap, *nhyp, lp, ctx, n_f, orgb + fin * GF,
                                     ys + (size_t)fin * K * a.cap, ts + (size_t)fin * K * a.cap, nullptr, nullptr, nullptr,
                                     yp ? yp + (size_t)fin * K * a.cap : nullptr, a.yp_out ? a.yp_out + (long long)b * K * a.Tp : nullptr);
        return;
    }
    // (hotwords: an unfinished match earns nothing -- every hypothesis' log-prob loses its state's pending bonus first)
    const int* st_f = stb + fin * GF;
    auto final_lp = [&](int k) {
        if constexpr (HW) return hws.pending ? lp[k] - hws.pending[st_f[k]] : lp[k];   // (an LM alone: nothing is pending)
        else return lp[k];
    };
    if (a.nb.tokens && slab == 0)
        beam_nbest_write(a.nb, b, *nhyp, a.cap, a.max_tokens, n_f, ys + (size_t)fin * K * a.cap, ts + (size_t)fin * K * a.cap,
                         yp + (size_t)fin * K * a.cap, final_lp, a.overflow);
    int best = 0;
    float bs = final_lp(0) / (float)(n_f[0] + 2);
    for (int k = 1; k < *nhyp; k++) {
        const float v = final_lp(k) / (float)(n_f[k] + 2);
        if (v > bs) { bs = v; best = k; }
    }
    const int n = n_f[best];
    if (n > a.max_tokens || n > a.cap) {
        if (tid == 0) *a.overflow = 1;
        return;
    }
    const int* ysf = ys + ((size_t)fin * K + best) * a.cap;
    const int* tsf = ts + ((size_t)fin * K + best) * a.cap;
    if (slab != 0) return;
    for (int i = tid; i < n; i += GT) {
        a.tokens[(long long)b * a.max_tokens + i] = ysf[i];
        a.timestamps[(long long)b * a.max_tokens + i] = tsf[i];
    }
    if (tid == 0) {
        a.n_tokens[b] = n;
        if (a.scores) a.scores[b] = final_lp(best);
    }
}

// get_most_probable(length_norm=True): max of log_prob / len(ys) (len counts the 2 ctx blanks), first maximum
template <bool HW>
__global__ void k_beam_final(BeamState s, int fin, int B, long long* __restrict__ tokens, int* __restrict__ timestamps,
                             int* __restrict__ n_tokens, float* __restrict__ scores, int max_tokens, int* __restrict__ overflow, BeamNbest nb) {
    const int b = blockIdx.x, K = s.K;
    const long long BK = (long long)B * K;
    const int* n_f = s.n + fin * BK + b * K;
    // (hotwords: every hypothesis' log-prob loses its state's pending bonus first)
    auto final_lp = [&](int k) {
        if constexpr (HW) return s.hw_pending ? s.lp[b * K + k] - s.hw_pending[s.st[fin * BK + b * K + k]] : s.lp[b * K + k];
        else return s.lp[b * K + k];
    };
    if (nb.tokens)
        beam_nbest_write(nb, b, s.nhyp[b], s.cap, max_tokens, n_f, s.ys + (fin * BK + (long long)b * K) * s.cap,
                         s.ts + (fin * BK + (long long)b * K) * s.cap, s.yp + (fin * BK + (long long)b * K) * s.cap, final_lp, overflow);
    int best = 0;
    float bs = final_lp(0) / (float)(n_f[0] + 2);
    for (int k = 1; k < s.nhyp[b]; k++) {
        float v = final_lp(k) / (float)(n_f[k] + 2);
        if (v > bs) { bs = v; best = k; }
    }
    const int n = n_f[best];
    if (n > max_tokens || n > s.cap) {
        if (threadIdx.x == 0) *overflow = 1;
        return;
    }
    const int* ys = s.ys + (fin * BK + (long long)b * K + best) * s.cap;
    const int* ts = s.ts + (fin * BK + (long long)b * K + best) * s.cap;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        tokens[(long long)b * max_tokens + i] = ys[i];
        timestamps[(long long)b * max_tokens + i] = ts[i];
    }
    if (threadIdx.x == 0) {
        n_tokens[b] = n;
        if (scores) scores[b] = final_lp(best);
    }
}

}  // namespace

void beam_search(const Ctx& ctx, const DecJoinW& w, const BeamArgs& a) {
    K2_REQUIRE(a.beam >= 1 && a.beam <= kMaxBeam, "beam search: beam %d out of range [1,%d]", a.beam, kMaxBeam);
    K2_REQUIRE(a.B > 0 && a.Tp > 0, "beam search: bad shape");
    // neural LM shallow fusion: the biased instantiation with the neural term, always in the per-frame launch form
    const bool nlm = a.nlm.dev.emb != nullptr;
    const bool hw = a.hw_next != nullptr || a.hw_streams != nullptr || a.lm.states != nullptr || nlm;
    K2_REQUIRE(!nlm || (a.nlm.scale > 0.f && a.nlm.dev.V == w.V && a.nlm.dev.L >= 1 && a.nlm.dev.L <= 8 && a.nlm.dev.w_out && a.nlm.dev.out_b &&
                        a.nlm.dev.h0 && a.nlm.dev.c0 && a.nlm.dev.q0),
               "beam search: neural LM fusion needs a complete LM over the model's %d tokens and a scale > 0", w.V);
    K2_REQUIRE(!nlm || ctx.dry || (a.rin != nullptr) == (a.nlm_io != nullptr), "beam search: neural LM fusion: the resumed search, and only it, takes the streams' state blocks");
    for (int k = 0; nlm && k < a.nlm.dev.L; k++) K2_REQUIRE(a.nlm.dev.wcat[k] && a.nlm.dev.bias[k], "beam search: neural LM fusion: layer %d has no weights", k);
    K2_REQUIRE(!a.lm.states || (a.lm.arc_tok && a.lm.arc_lp && a.lm.arc_next && a.lm.uni_lp && a.lm.uni_next), "beam search: incomplete n-gram LM tables");
    K2_REQUIRE(!(a.lm.states && a.rin) || (a.lst_in && a.lst_out), "beam search: the resumed search with an n-gram LM needs its LM state blocks");
    K2_REQUIRE(!a.lodr.states || nlm, "beam search: LODR runs only beside the neural LM fusion");
    K2_REQUIRE(!a.lodr.states || (a.lodr.arc_tok && a.lodr.arc_lp && a.lodr.arc_next && a.lodr.uni_lp && a.lodr.uni_next), "beam search: incomplete LODR tables");
    K2_REQUIRE(!(a.lodr.states && a.rin) || ctx.dry || (a.dst_in && a.dst_out), "beam search: the resumed search with LODR needs its LODR state blocks");
    K2_REQUIRE(!a.hw_next || (a.hw_bonus && a.hw_pending), "beam search: incomplete hotword tables");
    K2_REQUIRE(!(a.hw_next && a.hw_streams), "beam search: one hotword graph or one per stream, not both");
    K2_REQUIRE(!a.hw_streams || (a.rin && a.st_in && a.st_out), "beam search: per-stream hotword graphs belong to the resumed search and need its state blocks");
    K2_REQUIRE(!(a.hw_next && a.rin), "beam search: the resumed search takes its hotword graphs per stream");
    // token log-probs / N-best: the offline search writes nb (which needs them), the resumed one the side block yp_out
    // (keep_yp: the sizing pass sees null pointers for both)
    const bool yp = a.keep_yp || a.nb.tokens != nullptr || a.yp_out != nullptr;
    K2_REQUIRE(!a.nb.tokens || (!a.rin && a.nb.nbest >= 1 && a.nb.nbest <= kMaxBeam && a.nb.timestamps && a.nb.token_log_probs && a.nb.n_tokens &&
                                a.nb.scores && a.nb.n_hyps),
               "beam search: incomplete N-best outputs (nbest %d, range [1,%d])", a.nb.nbest, kMaxBeam);
    K2_REQUIRE(!a.yp_out || a.rin, "beam search: the token log-prob side block belongs to the resumed search");
    if (!ctx.dry) {
        if (nlm && a.rin) nlm_note_stream_search();
        else if (nlm) nlm_note_search();
        else g_launches[hw ? 1 : 0]++;
    }
    Arena& ar = *ctx.arena;
    const int B = a.B, K = a.beam, M = B * K, cap = a.Tp + 1;
    if (!nlm) {
        // the one-kernel form: needs the decoder table (small vocabulary) and the stream's logits and hypotheses in LDS
        // hypotheses in LDS when they fit beside the logits (T' <= ~600 at beam 4 with the large-en shapes), else in device memory
        const bool hyp_in_lds = sizeof(float) * beam_loop_lds_floats(w.J, w.Vp, K, cap, true, hw, yp) <= 150 * 1024 && !tunables().beam_hyp_global;
        const size_t lds = sizeof(float) * beam_loop_lds_floats(w.J, w.Vp, K, cap, hyp_in_lds, hw, yp);
        if (w.dec_table && !tunables().beam_launches && lds <= 150 * 1024 && w.J % 8 == 0 && w.Vp % 4 == 0 && K <= GF) {
            // Two column slabs per stream where one workgroup would sweep two chunks (beam <= 4, 256 < V <= 512) and 2 B workgroups fit
            // the offline co-residency budget: the frame's sweep is bound by ONE CU's fetch of the 1 MB matrix, two CUs halve it, and the
            // exchange of the 4 x 256 logits costs less than the half sweep (search alone 5.5 -> 4.45 ms for the headline batch).  The
            // slabs wait for each other (bounded; *overflow = 2 on a timeout): the launch is kept for a repeat with one slab.
            const bool two = !a.rin && !ctx.one_part && tunables().beam_parts != 1 && K <= 4 && (w.Vp >> 2) <= 128 && (w.Vp >> 2) > 64 && 2 * B <= std::max(device_cu_count() / 4, 2);
            unsigned long long* xg = two ? ar.take<unsigned long long>((int64_t)B * 2 * 2 * 4 * 256) : nullptr;
            // (hypotheses in device memory: every workgroup keeps its own copy, so two slabs need twice the space)
            int* ys_g = hyp_in_lds ? nullptr : ar.take<int>((int64_t)(two ? 2 : 1) * 2 * M * cap);
            int* ts_g = hyp_in_lds ? nullptr : ar.take<int>((int64_t)(two ? 2 : 1) * 2 * M * cap);
            float* yp_g = (hyp_in_lds || !yp) ? nullptr : ar.take<float>((int64_t)(two ? 2 : 1) * 2 * M * cap);
            if (ctx.dry) return;
            BeamLoopArgs la;
            la.enc = a.enc; la.Tp = a.Tp; la.K = K; la.cap = cap;
            la.tokens = a.tokens; la.timestamps = a.timestamps; la.n_tokens = a.n_tokens; la.scores = a.scores;
            la.max_tokens = a.max_tokens; la.overflow = a.overflow;
            la.ys_g = ys_g; la.ts_g = ts_g;
            la.want_yp = yp; la.yp_g = yp_g; la.nb = a.nb; la.yp_out = a.yp_out;
            la.xg = xg;
            la.trace = a.trace;
            la.rin = a.rin; la.rout = a.rout;
            la.hw_next = a.hw_next; la.hw_bonus = a.hw_bonus; la.hw_pending = a.hw_pending;
            la.hw_streams = a.hw_streams; la.st_in = a.st_in; la.st_out = a.st_out;
            la.lm = a.lm; la.lst_in = a.lst_in; la.lst_out = a.lst_out;
            K2_HIP(hipMemsetAsync(a.overflow, 0, sizeof(int), ctx.stream));
            static LdsAttrOnce lds_attr, lds_attr1, lds_attr_hw, lds_attr1_hw;
            if (hw) {
                lds_attr_hw.ensure(k_beam_loop<2, true>, 150 * 1024);
                lds_attr1_hw.ensure(k_beam_loop<1, true>, 150 * 1024);
            } else {
                lds_attr.ensure(k_beam_loop<2, false>, 150 * 1024);
                lds_attr1.ensure(k_beam_loop<1, false>, 150 * 1024);
            }
            if (two) K2_HIP(hipMemsetAsync(xg, 0, sizeof(unsigned long long) * (size_t)B * 2 * 2 * 4 * 256, ctx.stream));
            const dim3 grid1(two ? 2 * B : B);
            if (K <= 4 && hw) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_beam_loop<1, true>), grid1, dim3(GT), lds, ctx.stream, w, la);
            else if (K <= 4) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_beam_loop<1, false>), grid1, dim3(GT), lds, ctx.stream, w, la);
            else if (hw) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_beam_loop<2, true>), dim3(B), dim3(GT), lds, ctx.stream, w, la);
            else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_beam_loop<2, false>), dim3(B), dim3(GT), lds, ctx.stream, w, la);
            K2_HIP(hipGetLastError());
            if (ctx.greedy_rec) {
                ctx.greedy_rec->valid = two;
                ctx.greedy_rec->beam = true;
                ctx.greedy_rec->w = w;
                ctx.greedy_rec->a.B = B;
                ctx.greedy_rec->a.overflow = a.overflow;
                ctx.greedy_rec->ba = la;
                ctx.greedy_rec->beam_lds = lds;
            }
            if (two && tunables().test_greedy_timeout) K2_HIP(hipMemsetD32Async((hipDeviceptr_t)a.overflow, 2, 1, ctx.stream));
            return;
        }
    }
    if (ctx.greedy_rec) ctx.greedy_rec->valid = false;
    BeamState s;
    s.K = K;
    s.cap = cap;
    s.ys = ar.take<int>((int64_t)2 * M * cap);
    s.ts = ar.take<int>((int64_t)2 * M * cap);
    if (yp) {
        s.yp = ar.take<float>((int64_t)2 * M * cap);
        s.yp_out = a.yp_out;
    }
    s.n = ar.take<int>((int64_t)2 * M);
    s.lp = ar.take<float>(M);
    s.lp_next = s.lp;  // in place: within k_beam_step every read of a stream's lp / nhyp precedes (barrier-separated) tid 0's write
    s.ctx = ar.take<long long>((int64_t)2 * M);
    s.ctx_next = s.ctx;
    s.nhyp = ar.take<int>(B);
    s.nhyp_next = s.nhyp;
    if (a.rin) {
        s.org = ar.take<int>((int64_t)2 * M);
        s.rin = a.rin;
        s.Tp = a.Tp;
    }
    if (hw) {
        s.st = ar.take<int>((int64_t)2 * M);
        s.hw_next = a.hw_next; s.hw_bonus = a.hw_bonus; s.hw_pending = a.hw_pending;
        s.hw_streams = a.hw_streams; s.st_in = a.st_in; s.st_out = a.st_out;
        if (a.lm.states) {
            s.lst = ar.take<int>((int64_t)2 * M);
            s.lm = a.lm; s.lst_in = a.lst_in; s.lst_out = a.lst_out;
        }
    }
    // neural LM: the slots' LSTM states [2][L][M][H] and rows [2][M][V] by frame parity, the step's notes for the LM launches
    const RnnLmDev& nd = a.nlm.dev;
    float *nh = nullptr, *nc = nullptr, *nq = nullptr;
    const int64_t nst = nlm ? (int64_t)nd.L * M * nd.H : 0;
    if (nlm) {
        nh = ar.take<float>(2 * nst);
        nc = ar.take<float>(2 * nst);
        nq = ar.take<float>((int64_t)2 * M * nd.V);
        s.nq = nq;
        s.npar = ar.take<int>(M);
        s.ntok = ar.take<int>(M);
        s.nflag = ar.take<int>(a.Tp);
        s.nscale = a.nlm.scale;
        if (a.lodr.states) {
            s.dst = ar.take<int>((int64_t)2 * M);
            s.lodr = a.lodr; s.dst_in = a.dst_in; s.dst_out = a.dst_out;
        }
        if (!ctx.dry) K2_HIP(hipMemsetAsync(s.nflag, 0, sizeof(int) * (size_t)a.Tp, ctx.stream));
        // (the resumed form: the streams' carried blocks, the in blocks' first int naming the live slots)
        if (a.rin) nlm_load_streams(ctx, nd, a.nlm_io, a.rin, BeamResumeLayout{K, a.Tp}.in_ints(), nh, nc, nq, B, K);
        else nlm_broadcast(ctx, nd, nh, nc, nq, M);
    }
    float* hbuf = ar.take<float>((int64_t)M * w.DD);
    float* act = ar.take<float>((int64_t)M * w.J);
    float* logits = ar.take<float>((int64_t)M * w.V);
    if (!ctx.dry) {
        K2_HIP(hipMemsetAsync(a.overflow, 0, sizeof(int), ctx.stream));
        if (a.rin) hipLaunchKernelGGL(k_beam_resume_init, dim3(cdiv(M, 256)), dim3(256), 0, ctx.stream, s, B);
        else hipLaunchKernelGGL(k_beam_init, dim3(cdiv(M, 256)), dim3(256), 0, ctx.stream, s, B);
        K2_HIP(hipGetLastError());
    }
    for (int t = 0; t < a.Tp; t++) {
        // four launches per frame: the decoder front end (embedding + conv + ReLU, elementwise); act = tanh(enc_t + decoder_proj(h)) as
        // ONE small-problem GEMM whose epilogue adds the stream's encoder frame (row / K) before the tanh; the joiner GEMM; the
        // per-stream step.  (Folding the front end into the step's tail only moved its time into the 32-workgroup step kernel.)
        if (!ctx.dry) hipLaunchKernelGGL(k_beam_embconv, dim3(cdiv((long long)M * w.DD, 256)), dim3(256), 0, ctx.stream, w, s.ctx, hbuf, M);
        {
            GemmArgs g;
            g.A = hbuf; g.lda = w.DD; g.W = a.dproj_w; g.ldw = w.DD; g.bias = w.dproj_b;
            g.C = act; g.ldc = w.J; g.M = M; g.N = w.J; g.K = w.DD;
            g.act = ACT_TANH; g.act_after_res = 1; g.res = a.enc + (long long)t * w.J; g.ldr = a.Tp * w.J; g.res_div = K;
            gemm(ctx, g);
        }
        linear(ctx, act, w.J, a.out_w, w.out_b, logits, w.V, M, w.J, w.V);
        if (!ctx.dry) {
            if (nlm) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_beam_step<true, true>), dim3(B), dim3(BT), 0, ctx.stream, s, logits, w.V, t, t & 1, B, a.trace, a.Tp);
            else if (hw) hipLaunchKernelGGL(k_beam_step<true>, dim3(B), dim3(BT), 0, ctx.stream, s, logits, w.V, t, t & 1, B, a.trace, a.Tp);
            else hipLaunchKernelGGL(k_beam_step<false>, dim3(B), dim3(BT), 0, ctx.stream, s, logits, w.V, t, t & 1, B, a.trace, a.Tp);
            K2_HIP(hipGetLastError());
        }
        if (nlm && (a.rin || t + 1 < a.Tp)) {   // (resumed: behind the last frame too -- the next chunk needs the survivors' state)
            // the LM behind the step: one launch per layer over all slots (state of parity t & 1 gathered through npar into the other
            // parity), then the rows; on a frame in which no slot appended a token they only move state and rows
            const int cur = t & 1, nxt = cur ^ 1;
            for (int k = 0; k < nd.L; k++) {
                NlmAdvance v;
                v.wcat = nd.wcat[k]; v.bias = nd.bias[k];
                v.emb = k == 0 ? nd.emb : nullptr;
                v.x_rows = k == 0 ? nullptr : nh + nxt * nst + (int64_t)(k - 1) * M * nd.H;
                v.h_par = nh + cur * nst + (int64_t)k * M * nd.H; v.c_par = nc + cur * nst + (int64_t)k * M * nd.H;
                v.h_out = nh + nxt * nst + (int64_t)k * M * nd.H; v.c_out = nc + nxt * nst + (int64_t)k * M * nd.H;
                v.par = s.npar; v.tok = s.ntok; v.live = s.nflag + t; v.work = a.rin ? nullptr : nd.work;   // (the counters are the offline search's)
                v.M = M; v.in = k == 0 ? nd.E : nd.H; v.H = nd.H;
                nlm_advance(ctx, v);
            }
            nlm_rows(ctx, nh + nxt * nst + (int64_t)(nd.L - 1) * M * nd.H, nd.w_out, nd.out_b, nq + (int64_t)cur * M * nd.V, nq + (int64_t)nxt * M * nd.V,
                     s.npar, s.ntok, s.nflag + t, M, nd.H, nd.V);
        }
    }
    if (nlm && a.rin) {   // slot k of the final parity into slot k of the stream's other half (beam_resume_write keeps the slots' order)
        const int fin = a.Tp & 1;
        nlm_store_streams(ctx, nd, a.nlm_io, nh + fin * nst, nc + fin * nst, nq + (int64_t)fin * M * nd.V, B, K);
    }
    if (!ctx.dry) {
        if (a.rin && hw) hipLaunchKernelGGL(k_beam_resume_final<true>, dim3(B), dim3(256), 0, ctx.stream, s, a.Tp & 1, B, a.rout);
        else if (a.rin) hipLaunchKernelGGL(k_beam_resume_final<false>, dim3(B), dim3(256), 0, ctx.stream, s, a.Tp & 1, B, a.rout);
        else if (hw) hipLaunchKernelGGL(k_beam_final<true>, dim3(B), dim3(256), 0, ctx.stream, s, a.Tp & 1, B, a.tokens, a.timestamps, a.n_tokens,
                                        a.scores, a.max_tokens, a.overflow, a.nb);
        else hipLaunchKernelGGL(k_beam_final<false>, dim3(B), dim3(256), 0, ctx.stream, s, a.Tp & 1, B, a.tokens, a.timestamps, a.n_tokens, a.scores,
                                a.max_tokens, a.overflow, a.nb);
        K2_HIP(hipGetLastError());
    }
}

void beam_launch_counts(long long* plain, long long* hw) {
    *plain = g_launches[0].load();
    *hw = g_launches[1].load();
}

void beam_relaunch_one_slab(hipStream_t stream, const GreedyLaunch& rec) {
    K2_REQUIRE(rec.valid && rec.beam, "beam retry: no repeatable launch on record");
    BeamLoopArgs la = rec.ba;
    la.xg = nullptr;
    K2_HIP(hipMemsetAsync(la.overflow, 0, sizeof(int), stream));
    if (tunables().test_greedy_timeout) {   // (as greedy_relaunch_one_part: the caller must get the REPEAT's output)
        K2_HIP(hipMemsetAsync(la.tokens, 0xEE, sizeof(long long) * (size_t)rec.a.B * la.max_tokens, stream));
        K2_HIP(hipMemsetAsync(la.timestamps, 0xEE, sizeof(int) * (size_t)rec.a.B * la.max_tokens, stream));
        K2_HIP(hipMemsetAsync(la.n_tokens, 0xEE, sizeof(int) * (size_t)rec.a.B, stream));
        if (la.scores) K2_HIP(hipMemsetAsync(la.scores, 0xEE, sizeof(float) * (size_t)rec.a.B, stream));
    }
    // (la carries the hotword and LM tables of the first launch; its LDS size was computed with them)
    if (la.hw_next || la.hw_streams || la.lm.states) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_beam_loop<1, true>), dim3(rec.a.B), dim3(GT), rec.beam_lds, stream, rec.w, la);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_beam_loop<1, false>), dim3(rec.a.B), dim3(GT), rec.beam_lds, stream, rec.w, la);
    K2_HIP(hipGetLastError());
}

}  // namespace k2hip
