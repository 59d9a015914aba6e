// CTC prefix beam search with N-best (semantics: include/k2hip.h, DESIGN.md "CTC prefix beam search"; host reference, THE fold rule
// and THE tie rule: ctc_prefix_ref.h).
//
//   k_ctc_prefix   one workgroup of 256 per row, frames sequential.  The live hypotheses (at most 8 slots: pb, pnb, tot, last token,
//                  length, history node, rolling hashes) ping-pong in LDS.  Per frame:
//                    candidates   the threads stride over the columns v; a thread forms the candidates of its columns for every slot
//                                 from the slots' (pb, tot, e) held in registers and keeps its best `beam` in a sorted register list;
//                                 thread k < n also forms slot k's stay candidate (with the fold it receives).  Columns named by the
//                                 frame's fold table (slot j spells slot k + [e_j]: at most `beam` pairs) are skipped for slot k.
//                    selection    `beam` rounds of wave_best take every wave's winners in rank order (no barrier), one barrier, then
//                                 every wave repeats the rounds over the 4 x beam wave winners -- the workgroup's winners in rank
//                                 order, known to every lane.  The order is (total desc, flat index k V + v asc) throughout.
//                    update       thread r builds slot r of the other parity; an extension appends a node (parent, token, frame,
//                                 lp(t, v)) to the row's pool at t * beam + r.
//                    fold table   for the next frame, 64 threads, one per (j, k): length, rolling hash of the prefix without its last
//                                 token as the filter, then the confirmation: the two parent chains are walked until the node ids
//                                 coincide (zero steps when j was extended from k's node), comparing tokens.  Sequence identity, not
//                                 node identity: a prefix that left the beam and was spelled again has another node.
//                  The first 256 columns of frame t + 1 are requested before frame t's work.  After the last frame every surviving
//                  slot's chain is walked back into its output row from index len - 1 down.
//   k_ctc_prefix<true>  the same frames resumed from the live prefixes of the chunks before (streaming; CtcPrefixResumeLayout).  The
//                  per-frame body is the one above -- one piece of source, the same float32 operations in the same order, so a stream's
//                  prefixes after any chunking are bit for bit those of the search over all its frames.  What differs is outside the
//                  arithmetic: the slots start from the in block (carried slot a is the pool's root -1 - a, its parent kNoParent), the
//                  fold table is also built before the first frame, its confirmation walks through the boundary (both chains in lock
//                  step; where one reaches its root a while the other is d tokens above its root b, the answer is rel[a][b] == d with
//                  relx equal to those tokens; a carried slot with nothing appended is the case S_a = S_b + s_k + [e_a]), and the
//                  survivors go to the out block as (origin, appended tokens / frames / log-probs, pb, pnb, hashes).
//   k_ctc_prefix<false, true>  the offline search with hotword and n-gram LM biasing (semantics: include/k2hip.h "Hotword and n-gram
//                  LM biasing of the CTC prefix beam search"; host reference: ctc_prefix_bias_ref.h).  The same source again; what the
//                  instantiation adds: three more words per slot and parity in LDS (hs, ls, ctx), the slots' hs / ctx in registers
//                  beside pb / tot in the column loop and ONE coalesced bonus[hs_k V + v] load per live slot and column, so that a
//                  candidate's KEY is its acoustic total plus ctx (plus the bonus of the extension); pb / pnb / tot stay acoustic, the
//                  slot-building thread forms them again from the same operands.  Behind the second-level selection every wave knows
//                  all winners: wave w takes the LM walks (lm_walk.h, a wave per walk) of winners 2 w and 2 w + 1, term and next state
//                  go through LDS -- one more barrier per frame -- to the thread that builds the slot, which loads next[hs_k V + v]
//                  itself.  After the last frame final = (tot + ctx) - pending[hs] and the entries' order are formed in LDS before the
//                  chains are written.  Null hotword tables / null LM tables: that half adds nothing (a null check).
//   k_ctc_prefix<true, true>  the resumed search with biasing (include/k2hip.h "Biasing of the streaming CTC prefix beam search").  The
//                  same source a fourth time.  The tables are the row's own: row_hw / row_lm read the row's entry of hw_streams [B] and
//                  the call's LM (null where the row's flag is clear) once, wave-uniformly; the offline form reads its single pair
//                  through the same two accessors.  The slots' (ctx, hs, ls) start from the side in block -- ctx with the pending bonus
//                  of a match under way, the slots in selection order --, a slot that receives a fold through the boundary keeps its
//                  own three values as inside a chunk, and after the chunk's last frame final and the entries' order are formed by the
//                  code the offline form runs there; the survivors' (ctx, hs, ls, fin, ord) go to the side out block beside the
//                  unchanged out block, whose tot stays acoustic (CtcPrefixResumeBiasLayout).
// No workgroup waits for another; every loop is bounded by T, beam, a hypothesis length, K2HIP_NGRAM_MAX_ORDER - 1 levels or the walk's
// 64-ary narrowing; all stores are ordinary vector stores.
#include <climits>

#include "kernels.h"
#include "lm_walk.h"
#include "wave_best.h"

namespace k2hip {
namespace {

constexpr int PT = 256, PW = PT / 64;   // threads / waves of the workgroup
constexpr int KB = kMaxBeam;

__device__ __forceinline__ float ninf() { return -__builtin_inff(); }

// logaddexp(a, b) = m + log1p(exp(min - m)); -inf operands never make a NaN
__device__ __forceinline__ float logaddexp_f(float a, float b) {
    const float m = fmaxf(a, b), n = fminf(a, b);
    if (n == ninf()) return m;
    return m + log1pf(expf(n - m));
}

// the live hypotheses of one frame parity
struct Slots {
    float pb[KB], pnb[KB], tot[KB];
    int e[KB], len[KB], node[KB], pnode[KB];   // last token (-1: the empty prefix), length, history node and its parent (-1: none)
    unsigned long long hash[KB], phash[KB];    // rolling hash of the prefix / of the prefix without its last token
    int n;
};
// what the biased instantiation keeps beside them (empty otherwise: no LDS)
template <bool BIAS>
struct BiasLds {};
template <>
struct BiasLds<true> {
    float ctx[2][KB];               // accumulated context score of the slots, per frame parity
    int hs[2][KB], ls[2][KB];       // hotword graph state, LM state
    float stay_tot[KB];             // the stay candidates' acoustic totals (the selection carries keys)
    float term[KB];                 // the selected candidates' LM terms and next LM states, by rank
    int lnext[KB];
    float fin[KB];                  // after the last frame: final scores by slot, slots by final rank
    int ord[KB];
};
constexpr unsigned long long kHashSeed = kCtcPrefixHashSeed, kHashMul = kCtcPrefixHashMul;

constexpr int kNoParent = INT_MIN;   // resume: the parent of a carried slot's last token lies outside the chunk

// Resume: the confirmation of slot j = slot k + [e_j] once a chain has left the chunk.  p (from j's parent) and q (from k's node) have
// spelled equal tokens so far and differ, and at least one is no in-chunk node.  jn: slot j's node.
__device__ __forceinline__ bool fold_through_boundary(int p, int q, int jn, const int4* nodes, const int* in, CtcPrefixResumeLayout L, int* status) {
    int a, o, skip = 0;   // a: the carried slot a chain ended in; o: where the other chain stands; skip: e_a itself is not walked
    if (p == kNoParent) { a = -1 - jn; o = q; skip = 1; }
    else if (p < 0 && q < 0) return false;   // two different carried slots: different sequences
    else if (p < 0) { a = -1 - p; o = q; }
    else { a = -1 - q; o = p; }
    int d = 0, b = o;
    while (b >= 0 && d < L.Tc) { b = nodes[b].x; d++; }
    if (b >= 0 || b == kNoParent || a < 0 || a >= L.K || -1 - b >= L.K) { *status = 1; return false; }
    const int ab = a * L.K + (-1 - b);
    if (in[L.in_rel() + ab] != d + skip) return false;
    const int* x = in + L.in_relx() + ab * L.Tc;
    for (int i = d - 1; i >= 0; i--) {   // (d + skip <= Tc by the table's cap)
        const int4 nd = nodes[o];
        if (nd.y != x[i]) return false;
        o = nd.x;
    }
    return true;
}

// The tables a row reads (BIAS): the call's single pair offline; resumed, the row's own graph out of hw_streams [B] (all null: none)
// and the call's LM, masked off for a row whose side in block does not set flag bit 0.  Wave-uniform: r = blockIdx.x.
__device__ __forceinline__ BeamHwStream row_hw(const CtcPrefixBiasArgs& a, int) { return a.hw; }
__device__ __forceinline__ BeamLm row_lm(const CtcPrefixBiasArgs& a, int) { return a.lm; }
__device__ __forceinline__ BeamHwStream row_hw(const CtcPrefixResumeBiasArgs& a, int r) { return a.hw_streams[r]; }
__device__ __forceinline__ BeamLm row_lm(const CtcPrefixResumeBiasArgs& a, int r) {
    BeamLm lm = a.lm;
    if (!(a.side_in[(long long)r * CtcPrefixResumeBiasLayout{a.beam}.in_ints()] & 1)) lm.states = nullptr;
    return lm;
}
template <typename Args>
__device__ __forceinline__ BeamHwStream row_hw(const Args&, int) { return {}; }
template <typename Args>
__device__ __forceinline__ BeamLm row_lm(const Args&, int) { return {}; }

template <bool RESUME, bool BIAS, typename Args>
__global__ __launch_bounds__(PT) void k_ctc_prefix(Args a) {
    __shared__ Slots sl[2];
    [[maybe_unused]] __shared__ BiasLds<BIAS> bl;
    __shared__ float stay_pb[KB], stay_pnb[KB];
    __shared__ int fold_par[KB];   // slot j -> the slot k whose extension by e_j spells j, or -1
    __shared__ float wl_v[PW][KB];
    __shared__ int wl_i[PW][KB];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = a.V, beam = a.beam;
    [[maybe_unused]] const BeamHwStream hw = row_hw(a, r);   // (BIAS; wave-uniform, read once)
    [[maybe_unused]] const BeamLm lm = row_lm(a, r);
    int Tp;
    if constexpr (RESUME) Tp = a.Tc;
    else Tp = a.Tp;
    const int T = min(max(a.n_frames ? a.n_frames[r] : Tp, 0), Tp);
    const float* lp = a.log_probs + (long long)r * Tp * V;
    int4* nodes = a.nodes + (long long)r * Tp * beam;
    // the next frame's fold table: does slot j spell slot k + [e_j]?  (live prefixes are distinct: at most one k per j)
    auto fold_table = [&](const Slots& nx) {
        if (tid < KB * KB) {
            const int j = tid / KB, k = tid & (KB - 1), n2 = nx.n;
            if (j < n2 && k < n2 && j != k && nx.len[j] == nx.len[k] + 1 && nx.phash[j] == nx.hash[k]) {
                int p = nx.pnode[j], q = nx.node[k];
                bool same = true;
                while (p != q) {   // equal lengths: both chains end at their roots together; every step shortens both
                    if (p < 0 || q < 0) {
                        if constexpr (RESUME) same = fold_through_boundary(p, q, nx.node[j], nodes, a.in + (long long)r * CtcPrefixResumeLayout{beam, Tp}.in_ints(),
                                                                           CtcPrefixResumeLayout{beam, Tp}, a.status);
                        else same = false;
                        break;
                    }
                    const int4 np = nodes[p], nq = nodes[q];
                    if (np.y != nq.y) { same = false; break; }
                    p = np.x;
                    q = nq.x;
                }
                if (same) fold_par[j] = k;
            }
        }
    };
    if constexpr (RESUME) {
        const CtcPrefixResumeLayout L{beam, Tp};
        const int* in = a.in + (long long)r * L.in_ints();
        if (tid < KB) fold_par[tid] = -1;
        if (tid == 0) sl[0].n = min(max(in[0], 1), beam);
        if (tid < beam) {
            Slots& s = sl[0];
            const int k = tid, e = in[L.in_e() + k];
            s.pb[k] = __int_as_float(in[L.in_pb() + k]);
            s.pnb[k] = __int_as_float(in[L.in_pnb() + k]);
            s.tot[k] = logaddexp_f(s.pb[k], s.pnb[k]);   // (the value the frame before formed from the same two operands)
            s.e[k] = e >= 1 && e < V ? e : -1;
            s.len[k] = in[L.in_len() + k];
            s.node[k] = -1 - k; s.pnode[k] = kNoParent;
            s.hash[k] = (unsigned long long)(unsigned)in[L.in_hash() + 2 * k] | (unsigned long long)(unsigned)in[L.in_hash() + 2 * k + 1] << 32;
            s.phash[k] = (unsigned long long)(unsigned)in[L.in_phash() + 2 * k] | (unsigned long long)(unsigned)in[L.in_phash() + 2 * k + 1] << 32;
            if constexpr (BIAS) {   // the carried (ctx, hs, ls): ctx with the pending bonus still in it
                const CtcPrefixResumeBiasLayout SL{beam};
                const int* sin = a.side_in + (long long)r * SL.in_ints();
                bl.ctx[0][k] = __int_as_float(sin[SL.in_ctx() + k]); bl.hs[0][k] = sin[SL.in_hs() + k]; bl.ls[0][k] = sin[SL.in_ls() + k];
            }
        }
    } else if (tid == 0) {
        Slots& s = sl[0];
        s.pb[0] = 0.f; s.pnb[0] = ninf(); s.tot[0] = 0.f;
        s.e[0] = -1; s.len[0] = 0; s.node[0] = -1; s.pnode[0] = -1;
        s.hash[0] = kHashSeed; s.phash[0] = 0;
        s.n = 1;
        fold_par[0] = -1;
        if constexpr (BIAS) { bl.ctx[0][0] = 0.f; bl.hs[0][0] = 0; bl.ls[0][0] = lm.start; }
    }
    float px = T > 0 && tid < V ? lp[tid] : ninf();
    __syncthreads();
    if constexpr (RESUME) {   // the first frame's fold table: the relations among the carried slots
        fold_table(sl[0]);
        __syncthreads();
    }
    for (int t = 0; t < T; t++) {
        const Slots& c = sl[t & 1];
        Slots& nx = sl[(t + 1) & 1];
        const float* row = lp + (long long)t * V;
        const float cx = px;
        if (t + 1 < T && tid < V) px = row[V + tid];   // the next frame's first chunk, before this frame's barriers
        const int n = c.n;
        float s_pb[KB], s_tot[KB];
        int s_e[KB], s_fp[KB];
        [[maybe_unused]] float s_ctx[KB];
        [[maybe_unused]] int s_hs[KB];
#pragma unroll
        for (int k = 0; k < KB; k++) {
            const bool live = k < n;
            if constexpr (BIAS) {
                s_ctx[k] = live ? bl.ctx[t & 1][k] : 0.f;
                s_hs[k] = live ? bl.hs[t & 1][k] : 0;
            }
            s_pb[k] = live ? c.pb[k] : ninf();
            s_tot[k] = live ? c.tot[k] : ninf();
            s_e[k] = live ? c.e[k] : -1;
            s_fp[k] = live ? fold_par[k] : -1;
        }
        // the thread's best `beam` candidates, sorted by (total desc, flat index asc); index < 0 = none
        float lv[KB];
        int li[KB];
#pragma unroll
        for (int s = 0; s < KB; s++) { lv[s] = ninf(); li[s] = -1; }
        auto insert = [&](float v, int i) {
#pragma unroll
            for (int s = 0; s < KB; s++)
                if (s < beam && i >= 0 && (li[s] < 0 || v > lv[s] || (v == lv[s] && i < li[s]))) {
                    const float tv = lv[s]; const int ti = li[s];
                    lv[s] = v; li[s] = i;
                    v = tv; i = ti;
                }
        };
        if (tid < n) {   // the stay candidate of slot tid, with the fold it receives
            const int k = tid, e = c.e[k];
            const float lpe = e >= 0 ? row[e] : ninf();
            const float spb = c.tot[k] + row[0];
            float spnb = e >= 0 ? c.pnb[k] + lpe : ninf();
            const int p = fold_par[k];
            if (p >= 0) spnb = logaddexp_f(spnb, (e == c.e[p] ? c.pb[p] : c.tot[p]) + lpe);
            const float st = logaddexp_f(spb, spnb);
            stay_pb[k] = spb;
            stay_pnb[k] = spnb;
            if constexpr (BIAS) {
                bl.stay_tot[k] = st;
                if (st > ninf()) insert(st + bl.ctx[t & 1][k], k * V);
            } else if (st > ninf()) insert(st, k * V);
        }
        for (int v0 = 0; v0 < V; v0 += PT) {
            const int v = v0 + tid;
            if (v >= 1 && v < V) {
                const float xl = v0 == 0 ? cx : row[v];
                unsigned kill = 0;   // bit k: slot k + [v] is a live slot, the extension joined that slot's stay candidate
#pragma unroll
                for (int j = 0; j < KB; j++)
                    if (s_fp[j] >= 0 && s_e[j] == v) kill |= 1u << s_fp[j];
#pragma unroll
                for (int k = 0; k < KB; k++) {
                    const float x = (v == s_e[k] ? s_pb[k] : s_tot[k]) + xl;
                    if constexpr (BIAS) {   // the key: acoustic total + (ctx + bonus); dropped on the acoustic total
                        if (k < n && !(kill >> k & 1u) && x > ninf()) {
                            float cb = s_ctx[k];
                            if (hw.bonus) cb += hw.bonus[(long long)s_hs[k] * V + v];
                            insert(x + cb, k * V + v);
                        }
                    } else if (k < n && !(kill >> k & 1u) && x > ninf()) insert(x, k * V + v);
                }
            }
        }
        // every wave's winners in rank order
#pragma unroll
        for (int q = 0; q < KB; q++)
            if (q < beam) {
                float bv = lv[0];
                int bi = li[0];
                wave_best(bv, bi);
                if (bi >= 0 && li[0] == bi) {
#pragma unroll
                    for (int s = 0; s + 1 < KB; s++) { lv[s] = lv[s + 1]; li[s] = li[s + 1]; }
                    li[KB - 1] = -1;
                }
                if (lane == 0) { wl_v[wave][q] = bv; wl_i[wave][q] = bi; }
            }
        __syncthreads();
        // the workgroup's winners in rank order, in every lane of every wave
        float mv = ninf();
        int mi = -1;
        if (lane < PW * KB && (lane & (KB - 1)) < beam) {
            mv = wl_v[lane / KB][lane & (KB - 1)];
            mi = wl_i[lane / KB][lane & (KB - 1)];
        }
        float win_v = ninf();
        int win_i = -1, m = 0;
        [[maybe_unused]] int walk_i[2] = {-1, -1};   // BIAS: the winners 2 wave, 2 wave + 1, whose LM walks this wave takes
#pragma unroll
        for (int q = 0; q < KB; q++)
            if (q < beam) {
                float bv = mv;
                int bi = mi;
                wave_best(bv, bi);
                if (bi >= 0) {
                    if (mi == bi) mi = -1;
                    if (tid == q) { win_v = bv; win_i = bi; }
                    if constexpr (BIAS)
                        if ((q >> 1) == wave) walk_i[q & 1] = bi;
                    m++;
                }
            }
        if constexpr (BIAS) {   // (wave-uniform throughout: every lane holds the same winners)
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int i = walk_i[j];
                if (i >= 0) {
                    const int k = i / V, v = i - k * V;
                    float term = 0.f;
                    int ls = bl.ls[t & 1][k];
                    if (v != 0 && v != K2HIP_UNK_ID && lm.states) beam_lm_walk(lm, ls, v, lane, &term, &ls);
                    if (lane == 0) { bl.term[2 * wave + j] = term; bl.lnext[2 * wave + j] = ls; }
                }
            }
            __syncthreads();
        }
        // thread q builds slot q of the other parity (no finite candidate: slot 0 stays, its scores -inf from then on)
        if (tid < max(m, 1)) {
            int k = 0, v = 0;
            float pb = ninf(), pnb = ninf(), tot = ninf();
            if (m > 0) {
                k = win_i / V;
                v = win_i - k * V;
                tot = win_v;
                pb = v ? ninf() : stay_pb[k];
                pnb = v ? win_v : stay_pnb[k];
                if constexpr (BIAS) {   // win_v is the key: the acoustic values again, from the same operands
                    tot = v ? (v == c.e[k] ? c.pb[k] : c.tot[k]) + row[v] : bl.stay_tot[k];
                    if (v) pnb = tot;
                }
            }
            if constexpr (BIAS) {
                const int par = t & 1;
                float ctx = bl.ctx[par][k];
                int hs = bl.hs[par][k], ls = bl.ls[par][k];
                if (m > 0 && v) {
                    if (hw.bonus) {
                        ctx += hw.bonus[(long long)hs * V + v];
                        hs = hw.next[(long long)hs * V + v];
                    }
                    ctx = ctx + bl.term[tid];
                    ls = bl.lnext[tid];
                }
                bl.ctx[par ^ 1][tid] = ctx; bl.hs[par ^ 1][tid] = hs; bl.ls[par ^ 1][tid] = ls;
            }
            nx.pb[tid] = pb; nx.pnb[tid] = pnb; nx.tot[tid] = tot;
            if (v == 0) {
                nx.e[tid] = c.e[k]; nx.len[tid] = c.len[k]; nx.node[tid] = c.node[k]; nx.pnode[tid] = c.pnode[k];
                nx.hash[tid] = c.hash[k]; nx.phash[tid] = c.phash[k];
            } else {
                const int id = t * beam + tid;   // < T * beam <= Tp * beam: inside the row's pool
                nodes[id] = make_int4(c.node[k], v, t, __float_as_int(row[v]));
                nx.e[tid] = v; nx.len[tid] = c.len[k] + 1; nx.node[tid] = id; nx.pnode[tid] = c.node[k];
                nx.phash[tid] = c.hash[k];
                nx.hash[tid] = c.hash[k] * kHashMul + (unsigned long long)(v + 1);
            }
            fold_par[tid] = -1;
        }
        if (tid == 0) nx.n = max(m, 1);
        __syncthreads();
        fold_table(nx);
        __syncthreads();
    }
    const Slots& f = sl[T & 1];
    const int n = f.n;
    if constexpr (BIAS) {   // final = (tot + ctx) - pending[hs]; the entries by (final desc, slot asc)
        if (tid < n) {
            const float fv = f.tot[tid] + bl.ctx[T & 1][tid];
            bl.fin[tid] = hw.pending ? fv - hw.pending[bl.hs[T & 1][tid]] : fv;
        }
        __syncthreads();
        if (tid < n) {
            int rank = 0;
            for (int j = 0; j < n; j++) rank += bl.fin[j] > bl.fin[tid] || (bl.fin[j] == bl.fin[tid] && j < tid);
            bl.ord[rank] = tid;
        }
        __syncthreads();
    }
    if constexpr (RESUME) {
        const CtcPrefixResumeLayout L{beam, Tp};
        int* out = a.out + (long long)r * L.out_ints();
        if (tid == 0) out[0] = n;
        if (tid < n) {   // survivor tid: back to its root for (origin, appended), then the appended part from its end down
            const int q = tid;
            int napp = 0, root = f.node[q];
            while (root >= 0 && napp < Tp) { root = nodes[root].x; napp++; }
            if (root >= 0 || root == kNoParent || -1 - root >= beam) { *a.status = 1; root = -1; napp = 0; }
            out[L.out_org() + q] = -1 - root;
            out[L.out_napp() + q] = napp;
            out[L.out_pb() + q] = __float_as_int(f.pb[q]);
            out[L.out_pnb() + q] = __float_as_int(f.pnb[q]);
            out[L.out_tot() + q] = __float_as_int(f.tot[q]);
            if constexpr (BIAS) {   // beside the unchanged block: what the slot carries on, its final score, and the q-th slot in final order
                const CtcPrefixResumeBiasLayout SL{beam};
                int* so = a.side_out + (long long)r * SL.out_ints();
                so[SL.out_ctx() + q] = __float_as_int(bl.ctx[T & 1][q]); so[SL.out_hs() + q] = bl.hs[T & 1][q]; so[SL.out_ls() + q] = bl.ls[T & 1][q];
                so[SL.out_fin() + q] = __float_as_int(bl.fin[q]); so[SL.out_ord() + q] = bl.ord[q];
            }
            out[L.out_hash() + 2 * q] = (int)(unsigned)f.hash[q]; out[L.out_hash() + 2 * q + 1] = (int)(unsigned)(f.hash[q] >> 32);
            out[L.out_phash() + 2 * q] = (int)(unsigned)f.phash[q]; out[L.out_phash() + 2 * q + 1] = (int)(unsigned)(f.phash[q] >> 32);
            int node = f.node[q];
            for (int i = napp - 1; i >= 0; i--) {
                const int4 nd = nodes[node];
                out[L.out_ys() + q * Tp + i] = nd.y;
                out[L.out_ts() + q * Tp + i] = nd.z;
                out[L.out_yp() + q * Tp + i] = nd.w;
                node = nd.x;
            }
        }
    } else {
        auto slot_of = [&](int i) {
            if constexpr (BIAS) return bl.ord[i];
            else return i;
        };
        auto score_of = [&](int q) {
            if constexpr (BIAS) return bl.fin[q];
            else return f.tot[q];
        };
        // a slot's chain walked back into a row, from index len - 1 down
        auto write_chain = [&](int q, long long* tok, int* ts, float* yp, long long o) {
            int node = f.node[q];
            for (int i = f.len[q] - 1; i >= 0 && node >= 0; i--) {
                const int4 nd = nodes[node];
                tok[o + i] = nd.y;
                ts[o + i] = nd.z;
                if (yp) yp[o + i] = __int_as_float(nd.w);
                node = nd.x;
            }
        };
        if (tid == 64) {   // the single result: slot 0 (BIAS: the first in final order)
            const int s0 = slot_of(0);
            const int len = f.len[s0];
            if (len > a.max_tokens) {
                *a.overflow = 1;
                a.n_tokens[r] = 0;
            } else {
                write_chain(s0, a.tokens, a.timestamps, nullptr, (long long)r * a.max_tokens);
                a.n_tokens[r] = len;
            }
            if (a.scores) a.scores[r] = score_of(s0);
        }
        if (a.nb.tokens && tid < KB) {
            const int nh = min(n, a.nb.nbest);
            if (tid < nh) {
                const int q = slot_of(tid);
                const long long en = (long long)r * a.nb.nbest + tid;
                const int len = f.len[q];
                if (len > a.max_tokens) {   // (the single result's rule, per entry)
                    *a.overflow = 1;
                    a.nb.n_tokens[en] = 0;
                } else {
                    write_chain(q, a.nb.tokens, a.nb.timestamps, a.nb.token_log_probs, en * a.max_tokens);
                    a.nb.n_tokens[en] = len;
                }
                a.nb.scores[en] = score_of(q);
            }
            if (tid == 0) a.nb.n_hyps[r] = nh;
        }
    }
}

}  // namespace

void ctc_prefix_search(const Ctx& ctx, const CtcPrefixArgs& a) {
    if (ctx.dry) return;
    K2_REQUIRE(a.R >= 1 && a.R <= 65535 && a.Tp >= 1 && a.V >= 1 && (long long)kMaxBeam * a.V <= INT_MAX && a.beam >= 1 && a.beam <= kMaxBeam &&
                   a.max_tokens >= 1 && (!a.nb.tokens || (a.nb.nbest >= 1 && a.nb.nbest <= a.beam)),
               "ctc_prefix_search: bad shape R=%d T'=%d V=%d beam=%d nbest=%d max_tokens=%d", a.R, a.Tp, a.V, a.beam, a.nb.nbest, a.max_tokens);
    hipLaunchKernelGGL((k_ctc_prefix<false, false, CtcPrefixArgs>), dim3(a.R), dim3(PT), 0, ctx.stream, a);
    K2_HIP(hipGetLastError());
}

void ctc_prefix_search_biased(const Ctx& ctx, const CtcPrefixBiasArgs& a) {
    if (ctx.dry) return;
    K2_REQUIRE(a.R >= 1 && a.R <= 65535 && a.Tp >= 1 && a.V >= 1 && (long long)kMaxBeam * a.V <= INT_MAX && a.beam >= 1 && a.beam <= kMaxBeam &&
                   a.max_tokens >= 1 && (!a.nb.tokens || (a.nb.nbest >= 1 && a.nb.nbest <= a.beam)),
               "ctc_prefix_search_biased: bad shape R=%d T'=%d V=%d beam=%d nbest=%d max_tokens=%d", a.R, a.Tp, a.V, a.beam, a.nb.nbest, a.max_tokens);
    K2_REQUIRE(!a.hw.next == !a.hw.bonus && !a.hw.next == !a.hw.pending, "ctc_prefix_search_biased: incomplete hotword tables");
    K2_REQUIRE(!a.lm.states || (a.lm.uni_lp && a.lm.uni_next && a.lm.start >= 0), "ctc_prefix_search_biased: incomplete LM tables");   // (no arcs at all: null arc arrays)
    hipLaunchKernelGGL((k_ctc_prefix<false, true, CtcPrefixBiasArgs>), dim3(a.R), dim3(PT), 0, ctx.stream, a);
    K2_HIP(hipGetLastError());
}

void ctc_prefix_resume_biased(const Ctx& ctx, const CtcPrefixResumeBiasArgs& a) {
    if (ctx.dry) return;
    K2_REQUIRE(a.B >= 1 && a.B <= 65535 && a.Tc >= 1 && a.V >= 1 && (long long)kMaxBeam * a.V <= INT_MAX && a.beam >= 1 && a.beam <= kMaxBeam &&
                   (long long)a.Tc * a.beam <= INT_MAX / 2 && a.in && a.out && a.nodes && a.status && a.hw_streams && a.side_in && a.side_out,
               "ctc_prefix_resume_biased: bad shape B=%d Tc=%d V=%d beam=%d", a.B, a.Tc, a.V, a.beam);
    K2_REQUIRE(!a.lm.states || (a.lm.uni_lp && a.lm.uni_next && a.lm.start >= 0), "ctc_prefix_resume_biased: incomplete LM tables");
    hipLaunchKernelGGL((k_ctc_prefix<true, true, CtcPrefixResumeBiasArgs>), dim3(a.B), dim3(PT), 0, ctx.stream, a);
    K2_HIP(hipGetLastError());
}

void ctc_prefix_resume(const Ctx& ctx, const CtcPrefixResumeArgs& a) {
    if (ctx.dry) return;
    K2_REQUIRE(a.B >= 1 && a.B <= 65535 && a.Tc >= 1 && a.V >= 1 && (long long)kMaxBeam * a.V <= INT_MAX && a.beam >= 1 && a.beam <= kMaxBeam &&
                   (long long)a.Tc * a.beam <= INT_MAX / 2 && a.in && a.out && a.nodes && a.status,
               "ctc_prefix_resume: bad shape B=%d Tc=%d V=%d beam=%d", a.B, a.Tc, a.V, a.beam);
    hipLaunchKernelGGL((k_ctc_prefix<true, false, CtcPrefixResumeArgs>), dim3(a.B), dim3(PT), 0, ctx.stream, a);
    K2_HIP(hipGetLastError());
}

}  // namespace k2hip
