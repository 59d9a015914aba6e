// Neural LM shallow fusion with half-precision weights (k2hip_set_rnn_lm_fusion_precision; DESIGN.md "Half-precision LM weights in the
// fused search"): k_nlm_advance_f16, the launch behind nlm_advance when the upload holds f16 panels.  The contract is nlm_advance's
// (kernels.h NlmAdvance): gates = f16([x ; h_par[par]]) . f16(W)^T + bias summed in float32 for the rows that appended, the cell and the
// state in float32, the other rows copied bit for bit, no weight read with *live == 0, no matrix work for a strip nobody appended to.
//
// The split.  A workgroup owns 8 hidden columns x the four gates -- one tile of 32 columns -- and up to 256 rows, as the float32 kernel
// does, so the cell is applied from registers.  Inside it the work is split along k, not along the rows: k runs in chunks of 32, wave w
// takes the chunks w, w + 4, .. and holds accumulator tiles for EVERY row strip (NS strips of 32 rows; two chains per strip up to four
// strips, so a wave always has at least two and usually eight independent v_mfma_f32_32x32x16_f16 chains in flight).  So
//   - a weight leaves memory once per launch and once per workgroup: no two waves load the same B operand.  A lane's B operand of one
//     instruction is one 16-byte load, a wave's 1 KiB contiguous (RnnLmDev::wcat_h), and the loads run two chunks ahead of the MFMAs;
//   - an element of the gathered A image [x ; h_par[par]] is needed by exactly ONE lane of ONE wave (row r of a strip, lane half hh, the
//     wave that owns the chunk), so it is gathered straight into that lane's registers -- 16 consecutive floats, a 128-byte line per
//     row and chunk between the two lane halves -- and rounded to f16 there.  An LDS image would add a round trip and share nothing.
//     The registers are double-buffered: chunk c + 4's floats are in flight while chunk c's MFMAs issue, and there is no barrier in
//     the k loop at all;
//   - the four waves' partial tiles meet in LDS once, after the k loop: strip s is finished by wave s % 4, which adds the other three
//     waves' tiles to its own in a fixed order (its own, then the others by wave number), applies bias and cell and stores h and c.
//     Gates never reach memory.
// Instruction j (0, 1) of chunk q feeds lane half hh with k = 32 q + 16 hh + 8 j + e on both operands: a permutation of k inside a chunk,
// which a sum does not see.  No workgroup waits for another; every load and store is an ordinary vector access.
#include "kernels.h"

namespace k2hip {
namespace {

constexpr int NT = 256;    // four waves: the k split
constexpr int NMAXR = 256; // rows a workgroup walks (8 strips x 16 accumulator registers per wave)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

template <int NS>
__global__ __launch_bounds__(NT) void k_nlm_advance_f16(NlmAdvance a) {
    constexpr int NA = NS <= 4 ? 2 : 1;   // accumulator chains per strip
    constexpr int OW = NS < 4 ? NS : 4;   // strips finished per round, one per wave
    __shared__ float red[OW * 3 * 1024];  // [finishing wave][the other three][16 registers][64 lanes]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int row0 = blockIdx.y * NMAXR, j0 = blockIdx.x * 8;
    const int H = a.H, Ip = (a.in + 31) / 32 * 32, Kc = Ip + H, NC = Kc / 32;
    const int live = a.live ? *a.live : 1;
    // lane (r, hh) gathers row r of every strip; has: the strips somebody appended to (the same in every wave of the workgroup)
    int par[NS], tok[NS];
    unsigned has = 0;
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const int m = row0 + 32 * s + r;
        par[s] = 0;
        tok[s] = -1;
        if (live && m < a.M) {
            par[s] = a.par[m];
            tok[s] = a.tok[m];
        }
        if (__ballot(tok[s] >= 0)) has |= 1u << s;
    }
    // debug counters: launches are ordered on their stream and one thread of each writes, so a plain add is enough
    if (a.work && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) a.work[live ? 0 : 1] += 1;
    f32x16 acc[NS][NA];
#pragma unroll
    for (int s = 0; s < NS; s++)
#pragma unroll
        for (int n = 0; n < NA; n++)
#pragma unroll
            for (int g = 0; g < 16; g++) acc[s][n][g] = 0.f;
    if (has) {
        const f16x8* wp = reinterpret_cast<const f16x8*>(a.wcat_h) + ((long long)blockIdx.x * Kc) * 4 + (hh * 32 + r);   // + (2 q + j) 64
        auto load_b = [&](int q, f16x8 (&b)[2]) {
            b[0] = wp[(long long)(2 * q) * 64];
            b[1] = wp[(long long)(2 * q + 1) * 64];
        };
        // the lane's 16 floats of chunk q for every live strip: k = 32 q + 16 hh .. + 15 (a chunk lies in x or in h: Ip % 32 == 0)
        auto load_a = [&](int q, float4 (&raw)[NS][4]) {
            const int k = 32 * q + 16 * hh;
#pragma unroll
            for (int s = 0; s < NS; s++) {
                if (!((has >> s) & 1u)) continue;   // (uniform over the workgroup)
#pragma unroll
                for (int p = 0; p < 4; p++) raw[s][p] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (tok[s] < 0) continue;           // (rows that appended nothing and rows >= M feed zeros; their tiles are not used)
                if (k < Ip) {
                    const float* x = a.emb ? a.emb + (long long)tok[s] * a.in : a.x_rows + (long long)(row0 + 32 * s + r) * a.in;
#pragma unroll
                    for (int p = 0; p < 4; p++)
                        if (k + 4 * p < a.in) raw[s][p] = *reinterpret_cast<const float4*>(x + k + 4 * p);
                } else {
                    const float* h = a.h_par + (long long)par[s] * H + (k - Ip);
#pragma unroll
                    for (int p = 0; p < 4; p++) raw[s][p] = *reinterpret_cast<const float4*>(h + 4 * p);
                }
            }
        };
        f16x8 b0[2], b1[2], b2[2];
        float4 raw[NS][4];
#pragma unroll
        for (int j = 0; j < 2; j++) b0[j] = b1[j] = b2[j] = f16x8{};
#pragma unroll
        for (int s = 0; s < NS; s++)
#pragma unroll
            for (int p = 0; p < 4; p++) raw[s][p] = make_float4(0.f, 0.f, 0.f, 0.f);
        int q = wave;
        if (q < NC) {
            load_b(q, b0);
            load_a(q, raw);
        }
        if (q + 4 < NC) load_b(q + 4, b1);
        for (; q < NC; q += 4) {
            f16x8 ah[NS][2];   // this chunk's A operands, rounded to nearest even (v_cvt_f16_f32; f16 subnormals kept)
#pragma unroll
            for (int s = 0; s < NS; s++)
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const float4 lo = raw[s][2 * j], hi = raw[s][2 * j + 1];
                    ah[s][j] = f16x8{(_Float16)lo.x, (_Float16)lo.y, (_Float16)lo.z, (_Float16)lo.w,
                                     (_Float16)hi.x, (_Float16)hi.y, (_Float16)hi.z, (_Float16)hi.w};
                }
            if (q + 8 < NC) load_b(q + 8, b2);
            if (q + 4 < NC) load_a(q + 4, raw);   // (in flight while this chunk's MFMAs issue)
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    if (!((has >> s) & 1u)) continue;
                    acc[s][j % NA] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[s][j], b0[j], acc[s][j % NA], 0, 0, 0);
                }
#pragma unroll
            for (int j = 0; j < 2; j++) {
                b0[j] = b1[j];
                b1[j] = b2[j];
            }
        }
    }
    // column c of the tile is gate c >> 3 of hidden column j0 + (c & 7), so lane (row, j < 8) holds i and fetches f, g, o of its cell
    // from the lanes 8, 16 and 24 to its right
    const float bias = a.bias[(long long)(r >> 3) * H + j0 + (r & 7)];
    auto finish = [&](int s, const f32x16& t) {
        if (row0 + 32 * s >= a.M) return;   // (uniform over the wave)
#pragma unroll
        for (int g = 0; g < 16; g++) {
            const float v = t[g] + bias;
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
    };
#pragma unroll
    for (int i = 0; i < (NS + 3) / 4; i++) {
        f32x16 mine;
#pragma unroll
        for (int g = 0; g < 16; g++) mine[g] = 0.f;
        if (has) {   // (uniform over the workgroup: the barriers are met by every wave)
            if (i) __syncthreads();
#pragma unroll
            for (int o = 0; o < OW; o++) {
                const int s = 4 * i + o;
                if (s >= NS || !((has >> s) & 1u)) continue;
                f32x16 t = acc[s][0];
                if (NA == 2) t += acc[s][NA - 1];
                if (o == wave) {
                    mine = t;
                } else {
                    float* dst = red + (o * 3 + (wave < o ? wave : wave - 1)) * 1024 + lane;
#pragma unroll
                    for (int g = 0; g < 16; g++) dst[g * 64] = t[g];
                }
            }
            __syncthreads();
            if (wave < OW && 4 * i + wave < NS && ((has >> (4 * i + wave)) & 1u)) {
#pragma unroll
                for (int w = 0; w < 3; w++)
#pragma unroll
                    for (int g = 0; g < 16; g++) mine[g] += red[(wave * 3 + w) * 1024 + g * 64 + lane];
            }
        }
        if (wave < OW && 4 * i + wave < NS) finish(4 * i + wave, mine);
    }
}

}  // namespace

void nlm_advance_f16(const Ctx& ctx, const NlmAdvance& a) {
    if (ctx.dry) return;
    const int rows = std::min(a.M, NMAXR), strips = cdiv(rows, 32);
    const dim3 grid(a.H / 8, cdiv(a.M, NMAXR)), block(NT);
    if (strips <= 1) hipLaunchKernelGGL(k_nlm_advance_f16<1>, grid, block, 0, ctx.stream, a);
    else if (strips <= 2) hipLaunchKernelGGL(k_nlm_advance_f16<2>, grid, block, 0, ctx.stream, a);
    else if (strips <= 4) hipLaunchKernelGGL(k_nlm_advance_f16<4>, grid, block, 0, ctx.stream, a);
    else hipLaunchKernelGGL(k_nlm_advance_f16<8>, grid, block, 0, ctx.stream, a);
    K2_HIP(hipGetLastError());
}

}  // namespace k2hip
