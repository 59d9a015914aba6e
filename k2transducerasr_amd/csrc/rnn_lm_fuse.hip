// Neural LM shallow fusion: the LSTM language model stepped INSIDE the offline modified beam search (semantics: include/k2hip.h and
// DESIGN.md "Neural LM shallow fusion"; the LM itself: rnn_lm_ref.h; the search: beam.hip).
//
// Every hypothesis slot m of the M = B x beam slots carries (h, c) of all layers and the LM's next-token log-probs, double-buffered by
// frame parity.  After frame t's step kernel has written, for every new slot, the slot it continues (par) and the token it appended
// (tok, -1 for none), the search enqueues per layer
//   k_nlm_advance    gates = [x ; h_par] . [W_ih ; W_hh]^T + b for the rows that appended, on v_mfma_f32_32x32x2_f32.  A workgroup owns
//                    8 hidden columns x the four gates (the 32 columns of one tile) and ALL row strips of up to 256 rows, wave w the
//                    strips w and w + 4: every strip's accumulators stay in registers while k runs, so each weight leaves memory once
//                    per launch (the rescoring step of rnn_lm.hip re-reads W_hh once per 32-row strip), and H / 8 workgroups share
//                    the matrix work.  The weights are re-laid at upload in panels [Kc / 4][32][4]
//                    (RnnLmDev::wcat): a lane's B operand of four k is one 16-byte load, a wave's load 1 KiB contiguous, and chunk
//                    c + 1's loads are in flight while chunk c is staged.  The A operand ([x ; h] of the rows, GATHERED through par /
//                    tok) is staged per 32 k in LDS as [k / 4][row][4]: written and read as 16-byte pieces, row-contiguous, so both
//                    sides are conflict-free.  Lane (r, hh) feeds the MFMA of step i with k = 8 g + 4 hh + i on both operands: a
//                    permutation of k inside a group of 8, which a sum does not see.  In the epilogue a lane fetches the other three
//                    gates of its cell from its neighbours (no LDS), applies the cell against the gathered c and stores h and c; gates
//                    never reach memory.  Rows that appended nothing copy their parent's h and c.  Strips without an appended row issue
//                    no matrix work; with *live == 0 no weight is read at all.
//                    MEASURED (DESIGN.md "Neural LM shallow fusion"): per product the kernel is 2.4 to 3.3 times slower than the GEMM
//                    launcher + cell kernel at 128 rows.  At that row count the step is bound by the float32 matrix pipe, not by the
//                    weights' bytes, and this kernel feeds the pipe poorly: one accumulator chain per wave (128 rows give every wave
//                    one strip, so consecutive MFMAs wait for each other), the four waves of a workgroup each load the same B
//                    operand, and the A image is single-buffered behind two barriers per 32 k.
//   nlm_rows         q = log_softmax(h^{L-1} W_out^T + b) for the rows that appended (the GEMM launcher behind the same device flag,
//                    then k_nlm_rows: one workgroup per row), the parent's row copied for the others.
//   k_nlm_load_streams / k_nlm_store_streams   the STREAMING form (the resumed search): the streams' carried blocks
//                    (rnn_lm_stream_pool.h) into the parity-0 slot arrays before the first frame, the final-parity arrays into the
//                    blocks' other halves behind the last frame's LM launches.  One workgroup per slot, 16 bytes per lane where both
//                    sides are aligned.
// No workgroup waits for another; every store is an ordinary vector store.
#include <atomic>

#include "kernels.h"
#include "rnn_lm_stream_pool.h"

namespace k2hip {
namespace {

std::atomic<long long> g_nlm_searches, g_nlm_stream_searches;

constexpr int NT = 256;    // threads per workgroup: four waves, each with its own row strips
constexpr int NKC = 32;    // k staged in LDS at a time
constexpr int NMAXR = 256; // rows a workgroup walks

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

template <int NS>
__global__ __launch_bounds__(NT) void k_nlm_advance(NlmAdvance a) {
    constexpr int Rp = 32 * NS, NSW = (NS + 3) / 4;   // strips of the workgroup, strips per wave (wave w: strips w, w + 4)
    __shared__ float4 aS[(NKC / 4) * Rp];
    __shared__ int has[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int row0 = blockIdx.y * NMAXR, j0 = blockIdx.x * 8;
    const int H = a.H, Ip = (a.in + 31) / 32 * 32, Kc = Ip + H;
    const int live = a.live ? *a.live : 1;
    // this thread's staging row (Rp divides NT: the same row for every piece it stages) and what it gathers
    const int srow = tid % Rp, sm = row0 + srow;
    int spar = 0, stok = -1;
    if (sm < a.M) {
        spar = a.par[sm];
        stok = a.tok[sm];
    }
    {
        const unsigned long long bal = __ballot(live && tid < Rp && stok >= 0);   // (tid < Rp: every strip is seen once)
        if (lane == 0) {
            has[2 * wave] = (bal & 0xffffffffull) != 0;
            has[2 * wave + 1] = (bal >> 32) != 0;
        }
    }
    __syncthreads();
    bool any = false;
#pragma unroll
    for (int s = 0; s < NS; s++) any |= has[s] != 0;
    // debug counters: launches are ordered on their stream and one thread of each writes, so a plain add is enough
    if (a.work && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) a.work[live ? 0 : 1] += 1;
    f32x16 acc[NSW];
#pragma unroll
    for (int s = 0; s < NSW; s++)
#pragma unroll
        for (int g = 0; g < 16; g++) acc[s][g] = 0.f;
    if (any) {   // (uniform over the workgroup: every wave takes part in the staging)
        const float* wp = a.wcat + ((long long)blockIdx.x * Kc) * 32 + (hh * 32 + r) * 4;   // + (k / 4) * 128 floats
        const float* xrow = stok >= 0 ? (a.emb ? a.emb + (long long)stok * a.in : a.x_rows + (long long)sm * a.in) : nullptr;
        const float* hrow = a.h_par + (long long)spar * H;
        float4 b[4];
#pragma unroll
        for (int g = 0; g < 4; g++) b[g] = *reinterpret_cast<const float4*>(wp + (long long)(2 * g) * 128);
        for (int k0 = 0; k0 < Kc; k0 += NKC) {
            if (k0) __syncthreads();
            for (int kq = tid / Rp; kq < NKC / 4; kq += NT / Rp) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (sm < a.M) {
                    const int k = k0 + 4 * kq;
                    if (k0 < Ip) {
                        if (xrow && k < a.in) v = *reinterpret_cast<const float4*>(xrow + k);
                    } else {
                        v = *reinterpret_cast<const float4*>(hrow + (k - Ip));
                    }
                }
                aS[kq * Rp + srow] = v;
            }
            float4 bn[4];
            if (k0 + NKC < Kc) {
#pragma unroll
                for (int g = 0; g < 4; g++) bn[g] = *reinterpret_cast<const float4*>(wp + (long long)((k0 + NKC) / 4 + 2 * g) * 128);
            }
            __syncthreads();
#pragma unroll
            for (int g = 0; g < 4; g++) {
#pragma unroll
                for (int i = 0; i < NSW; i++) {
                    const int s = wave + 4 * i;
                    if (s >= NS || !has[s]) continue;   // (uniform over the wave)
                    const float4 av = aS[(2 * g + hh) * Rp + 32 * s + r];
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b[g].x, acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b[g].y, acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, b[g].z, acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, b[g].w, acc[i], 0, 0, 0);
                }
            }
            if (k0 + NKC < Kc) {
#pragma unroll
                for (int g = 0; g < 4; g++) b[g] = bn[g];
            }
        }
    }
    // epilogue, per wave on its own strips: column c of the tile is gate c >> 3 of hidden column j0 + (c & 7), so lane (row, j < 8)
    // holds i and fetches f, g, o of its cell from the lanes 8, 16 and 24 to its right
    const float bias = a.bias[(long long)(r >> 3) * H + j0 + (r & 7)];
#pragma unroll
    for (int i = 0; i < NSW; i++) {
        const int s = wave + 4 * i;
        if (s >= NS || row0 + 32 * s >= a.M) continue;   // (uniform over the wave)
#pragma unroll
        for (int g = 0; g < 16; g++) {
            const float v = acc[i][g] + bias;
            const float vf = __shfl(v, lane + 8), vg = __shfl(v, lane + 16), vo = __shfl(v, lane + 24);
            const int m = row0 + 32 * s + (g & 3) + 8 * (g >> 2) + 4 * hh;
            if (r >= 8 || m >= a.M) continue;
            const long long src = (long long)a.par[m] * H + j0 + r, dst = (long long)m * H + j0 + r;
            if (live && a.tok[m] >= 0) {
                const float cn = sigmoid_f(vf) * a.c_par[src] + sigmoid_f(v) * tanhf(vg);
                a.c_out[dst] = cn;
                a.h_out[dst] = sigmoid_f(vo) * tanhf(cn);
            } else {
                a.c_out[dst] = a.c_par[src];
                a.h_out[dst] = a.h_par[src];
            }
        }
    }
}

// one workgroup per slot: the log-softmax of the row the GEMM wrote, or the parent's row
__global__ __launch_bounds__(NT) void k_nlm_rows(const float* __restrict__ q_par, float* __restrict__ q_out, const int* __restrict__ par,
                                                 const int* __restrict__ tok, const int* __restrict__ live, int V) {
    __shared__ float red[NT / 64];
    const int m = blockIdx.x, tid = threadIdx.x;
    float* q = q_out + (long long)m * V;
    if (!(live ? *live : 1) || tok[m] < 0) {
        const float* p = q_par + (long long)par[m] * V;
        for (int v = tid; v < V; v += NT) q[v] = p[v];
        return;
    }
    float mx = -INFINITY;
    for (int v = tid; v < V; v += NT) mx = fmaxf(mx, q[v]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sm = 0.f;
    for (int v = tid; v < V; v += NT) sm += expf(q[v] - mx);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sm += __shfl_xor(sm, o);
    if ((tid & 63) == 0) red[tid >> 6] = sm;
    __syncthreads();
    const float lse = mx + logf((red[0] + red[1]) + (red[2] + red[3]));
    for (int v = tid; v < V; v += NT) q[v] = q[v] - lse;
}

// the start hypothesis' state and row into every slot of parity 0
__global__ void k_nlm_broadcast(const float* __restrict__ h0, const float* __restrict__ c0, const float* __restrict__ q0, float* __restrict__ h,
                                float* __restrict__ c, float* __restrict__ q, int L, int M, int H, int V) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long nh = (long long)L * M * H;
    if (i < nh) {
        const int j = (int)(i % H), k = (int)(i / ((long long)M * H));
        h[i] = h0[k * H + j];
        c[i] = c0[k * H + j];
    } else if (i < nh + (long long)M * V) {
        q[i - nh] = q0[(i - nh) % V];
    }
}

// ---- the streaming form's movers: one workgroup per slot m = b K + k ------------------------------------------------------------------
// n floats from src to dst by the whole workgroup: 16 bytes per lane where both start on 16 bytes (every state row; a row of q only
// when V and the slot allow it), the tail and the unaligned rows float by float
__device__ __forceinline__ void nlm_move(float* __restrict__ dst, const float* __restrict__ src, int n) {
    const int tid = threadIdx.x, nt = blockDim.x;
    if ((((unsigned long long)dst | (unsigned long long)src) & 15ull) == 0) {
        const int n4 = n >> 2;
        for (int i = tid; i < n4; i += nt) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
        for (int i = 4 * n4 + tid; i < n; i += nt) dst[i] = src[i];
    } else {
        for (int i = tid; i < n; i += nt) dst[i] = src[i];
    }
}
__global__ __launch_bounds__(NT) void k_nlm_load_streams(const NlmStreamIO* __restrict__ io, const int* __restrict__ nh, int nh_stride,
                                                         const float* __restrict__ h0, const float* __restrict__ c0, const float* __restrict__ q0,
                                                         float* __restrict__ h, float* __restrict__ c, float* __restrict__ q, NlmStreamLayout lay, int M) {
    const int m = blockIdx.x, b = m / lay.K, k = m - b * lay.K;
    const float* half = io[b].rd;
    const bool start = half == nullptr || k >= nh[(long long)b * nh_stride];
    for (int l = 0; l < lay.L; l++) {
        const long long dst = ((long long)l * M + m) * lay.H;
        nlm_move(h + dst, start ? h0 + (long long)l * lay.H : half + lay.state_off(k, l, 0), lay.H);
        nlm_move(c + dst, start ? c0 + (long long)l * lay.H : half + lay.state_off(k, l, 1), lay.H);
    }
    nlm_move(q + (long long)m * lay.V, start ? q0 : half + lay.row_off(k), lay.V);
}
__global__ __launch_bounds__(NT) void k_nlm_store_streams(const NlmStreamIO* __restrict__ io, const float* __restrict__ h, const float* __restrict__ c,
                                                          const float* __restrict__ q, NlmStreamLayout lay, int M) {
    const int m = blockIdx.x, b = m / lay.K, k = m - b * lay.K;
    float* half = io[b].wr;
    for (int l = 0; l < lay.L; l++) {
        const long long src = ((long long)l * M + m) * lay.H;
        nlm_move(half + lay.state_off(k, l, 0), h + src, lay.H);
        nlm_move(half + lay.state_off(k, l, 1), c + src, lay.H);
    }
    nlm_move(half + lay.row_off(k), q + (long long)m * lay.V, lay.V);
}

}  // namespace

void nlm_load_streams(const Ctx& ctx, const RnnLmDev& d, const NlmStreamIO* io, const int* nh, int nh_stride, float* h, float* c, float* q, int B, int K) {
    K2_REQUIRE(B > 0 && K >= 1 && K <= kMaxBeam && d.L >= 1 && d.H > 0 && d.H % 4 == 0 && d.V > 0, "nlm_load_streams: %d streams, beam %d, %d layers of %d, V = %d", B,
               K, d.L, d.H, d.V);
    if (ctx.dry) return;
    K2_REQUIRE(io && nh && h && c && q && d.h0 && d.c0 && d.q0, "nlm_load_streams: null argument");
    hipLaunchKernelGGL(k_nlm_load_streams, dim3(B * K), dim3(NT), 0, ctx.stream, io, nh, nh_stride, d.h0, d.c0, d.q0, h, c, q, NlmStreamLayout{K, d.L, d.H, d.V}, B * K);
    K2_HIP(hipGetLastError());
}
void nlm_store_streams(const Ctx& ctx, const RnnLmDev& d, const NlmStreamIO* io, const float* h, const float* c, const float* q, int B, int K) {
    K2_REQUIRE(B > 0 && K >= 1 && K <= kMaxBeam && d.L >= 1 && d.H > 0 && d.H % 4 == 0 && d.V > 0, "nlm_store_streams: %d streams, beam %d, %d layers of %d, V = %d", B,
               K, d.L, d.H, d.V);
    if (ctx.dry) return;
    K2_REQUIRE(io && h && c && q, "nlm_store_streams: null argument");
    hipLaunchKernelGGL(k_nlm_store_streams, dim3(B * K), dim3(NT), 0, ctx.stream, io, h, c, q, NlmStreamLayout{K, d.L, d.H, d.V}, B * K);
    K2_HIP(hipGetLastError());
}

void nlm_advance(const Ctx& ctx, const NlmAdvance& a) {
    K2_REQUIRE(a.M > 0 && a.H > 0 && a.H % 32 == 0 && a.in > 0 && a.in % 4 == 0, "nlm_advance: %d rows, input %d (a multiple of 4), hidden_dim %d (a multiple of 32)",
               a.M, a.in, a.H);
    K2_REQUIRE(ctx.dry || (a.wcat && a.bias && (a.emb || a.x_rows) && a.h_par && a.c_par && a.h_out && a.c_out && a.par && a.tok), "nlm_advance: null argument");
    K2_REQUIRE(a.h_out != a.h_par && a.c_out != a.c_par, "nlm_advance: the new state must not overwrite the state it is gathered from");
    if (ctx.dry) return;
    const int rows = std::min(a.M, NMAXR), strips = cdiv(rows, 32);
    const dim3 grid(a.H / 8, cdiv(a.M, NMAXR)), block(NT);
    if (strips <= 1) hipLaunchKernelGGL(k_nlm_advance<1>, grid, block, 0, ctx.stream, a);
    else if (strips <= 2) hipLaunchKernelGGL(k_nlm_advance<2>, grid, block, 0, ctx.stream, a);
    else if (strips <= 4) hipLaunchKernelGGL(k_nlm_advance<4>, grid, block, 0, ctx.stream, a);
    else hipLaunchKernelGGL(k_nlm_advance<8>, grid, block, 0, ctx.stream, a);
    K2_HIP(hipGetLastError());
}

void nlm_rows(const Ctx& ctx, const float* h, const float* w_out, const float* out_b, const float* q_par, float* q_out, const int* par,
              const int* tok, const int* live, int M, int H, int V) {
    K2_REQUIRE(M > 0 && H > 0 && H % 4 == 0 && V > 0, "nlm_rows: %d rows, hidden_dim %d, V = %d", M, H, V);
    K2_REQUIRE(q_out != q_par, "nlm_rows: the new rows must not overwrite the rows they are copied from");
    GemmArgs g;
    g.A = h; g.lda = H; g.W = w_out; g.ldw = H; g.bias = out_b; g.C = q_out; g.ldc = V; g.M = M; g.N = V; g.K = H;
    g.skip_if_zero = live;
    gemm(ctx, g);
    if (ctx.dry) return;
    hipLaunchKernelGGL(k_nlm_rows, dim3(M), dim3(NT), 0, ctx.stream, q_par, q_out, par, tok, live, V);
    K2_HIP(hipGetLastError());
}

void nlm_broadcast(const Ctx& ctx, const RnnLmDev& d, float* h, float* c, float* q, int M) {
    if (ctx.dry) return;
    const long long n = (long long)d.L * M * d.H + (long long)M * d.V;
    hipLaunchKernelGGL(k_nlm_broadcast, dim3(cdiv(n, 256)), dim3(256), 0, ctx.stream, d.h0, d.c0, d.q0, h, c, q, d.L, M, d.H, d.V);
    K2_HIP(hipGetLastError());
}

void nlm_start_state(const Ctx& ctx, const RnnLmDev& d) {
    // one row that appends sos to the zero state: layers through scratch (parity 0 = zeros, parity 1 = the result), then its row
    Arena& ar = *ctx.arena;
    const int H = d.H, L = d.L;
    float* zero = ar.take<float>(H);
    float* qz = ar.take<float>(d.V);
    int* ids = ar.take<int>(4);   // par = 0 | tok = sos
    if (!ctx.dry) {
        K2_HIP(hipMemsetAsync(zero, 0, sizeof(float) * (size_t)H, ctx.stream));
        K2_HIP(hipMemsetAsync(qz, 0, sizeof(float) * (size_t)d.V, ctx.stream));
        K2_HIP(hipMemsetD32Async((hipDeviceptr_t)ids, 0, 1, ctx.stream));
        K2_HIP(hipMemsetD32Async((hipDeviceptr_t)(ids + 1), d.sos, 1, ctx.stream));
    }
    for (int k = 0; k < L; k++) {
        NlmAdvance a;
        a.wcat = d.wcat[k]; a.bias = d.bias[k];
        a.emb = k == 0 ? d.emb : nullptr;
        a.x_rows = k == 0 ? nullptr : d.h0 + (long long)(k - 1) * H;
        a.h_par = zero; a.c_par = zero;
        a.h_out = d.h0 + (long long)k * H; a.c_out = d.c0 + (long long)k * H;
        a.par = ids; a.tok = ids + 1;
        a.M = 1; a.in = k == 0 ? d.E : H; a.H = H;
        nlm_advance(ctx, a);
    }
    nlm_rows(ctx, d.h0 + (long long)(L - 1) * H, d.w_out, d.out_b, qz, d.q0, ids, ids + 1, nullptr, 1, H, d.V);
}

void nlm_note_search() { g_nlm_searches++; }
long long beam_nlm_launch_count() { return g_nlm_searches.load(); }
void nlm_note_stream_search() { g_nlm_stream_searches++; }
long long beam_nlm_stream_launch_count() { return g_nlm_stream_searches.load(); }

}  // namespace k2hip
