// Neural LM rescoring with a half-precision recurrent product (k2hip_set_rnn_lm_rescoring_precision; DESIGN.md "Half-precision LSTM step
// in the rescoring"): k_lm_lstm_step_f16, the launch behind one (layer, position) of the scoring call while the switch is on.  The
// contract is rnn_lm_step's (kernels.h) with gates = gx[row] + f16(h_prev[row]) . f16(W_hh)^T: both operands of the product in f16,
// products exact in and summed in float32, gx, the cell, c and the stored h in float32.
//
// The split.  A workgroup owns 8 hidden columns x the four gates -- one tile of 32 columns, panel blockIdx.x of RnnLmDev::whh_h -- and
// the row block blockIdx.y of up to 256 active rows, so the cell is applied from registers.  k runs in chunks of 32; wave w takes the
// chunks w, w + 4, .. and holds accumulator tiles for EVERY live strip of 32 rows (two chains per strip up to four strips), so
//   - a weight leaves memory once per launch and row block: no two waves load the same B operand, a lane's B operand of one
//     v_mfma_f32_32x32x16_f16 is one 16-byte load, a wave's 1 KiB contiguous, and the loads run two chunks ahead of the MFMAs;
//   - the A operand is ALREADY f16: step t - 1's epilogue stored every h twice, the float32 row into the layer's output and the same
//     value rounded to nearest even into a mirror of halves.  Lane (r, hh) reads row r's 16 halves k = 32 q + 16 hh .. + 15 of the mirror
//     -- two 16-byte loads, one per instruction -- one chunk ahead of the MFMAs.  No float32 read of A, no conversion, no LDS image
//     and no barrier in the k loop;
//   - the four waves' partial tiles meet in LDS once, after the loop: strip s is finished by wave s % 4, which adds the other three
//     waves' tiles to its own in a fixed order (its own, then the others by wave number), so a sum depends on a and H alone.
// The kernel is instantiated on the strips of the launch's largest row block (1, 2, 4, 8): most positions of a call have fewer than 32
// active rows and carry one strip's accumulators.  Strips at or beyond row a (the tail of the last row block) issue no matrix work.
// Instruction j (0, 1) of chunk q feeds lane half hh with k = 32 q + 16 hh + 8 j + e on both operands: a permutation of k inside a chunk,
// which a sum does not see.  No workgroup waits for another; every load and store is an ordinary vector access; every loop is bounded
// by H / 32 or the strip count.
#include "kernels.h"

namespace k2hip {
namespace {

constexpr int HT = 256;     // four waves: the k split
constexpr int HMAXR = 256;  // rows of a row block (8 strips x 16 accumulator registers per wave)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

template <int NS>
__global__ __launch_bounds__(HT) void k_lm_lstm_step_f16(const uint16_t* __restrict__ h_prev16, const uint16_t* __restrict__ whh_h,
                                                         const float* __restrict__ gx, float* __restrict__ c, float* __restrict__ h_out,
                                                         uint16_t* __restrict__ h_out16, int a, int H) {
    constexpr int NA = NS <= 4 ? 2 : 1;   // accumulator chains per strip
    constexpr int OW = NS < 4 ? NS : 4;   // strips finished per round, one per wave
    __shared__ float red[OW * 3 * 1024];  // [finishing wave][the other three][16 registers][64 lanes]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int row0 = blockIdx.y * HMAXR, j0 = blockIdx.x * 8;
    const int NC = H / 32;
    // the strips of this row block that hold an active row (the same in every wave); none at the first position: h = 0, no product
    unsigned has = 0;
    if (h_prev16) {
#pragma unroll
        for (int s = 0; s < NS; s++)
            if (row0 + 32 * s < a) has |= 1u << s;
    }
    f32x16 acc[NS][NA];
#pragma unroll
    for (int s = 0; s < NS; s++)
#pragma unroll
        for (int n = 0; n < NA; n++)
#pragma unroll
            for (int g = 0; g < 16; g++) acc[s][n][g] = 0.f;
    if (has) {
        const f16x8* wp = reinterpret_cast<const f16x8*>(whh_h) + ((long long)blockIdx.x * H) * 4 + (hh * 32 + r);   // + (2 q + j) 64
        auto load_b = [&](int q, f16x8 (&b)[2]) {
            b[0] = wp[(long long)(2 * q) * 64];
            b[1] = wp[(long long)(2 * q + 1) * 64];
        };
        // the lane's 16 halves of chunk q for every live strip; rows >= a feed zeros (their tiles are not used) and are never read
        auto load_a = [&](int q, f16x8 (&av)[NS][2]) {
#pragma unroll
            for (int s = 0; s < NS; s++) {
                if (!((has >> s) & 1u)) continue;   // (uniform over the workgroup)
                const int m = row0 + 32 * s + r;
                av[s][0] = av[s][1] = f16x8{};
                if (m >= a) continue;
                const f16x8* ap = reinterpret_cast<const f16x8*>(h_prev16 + (long long)m * H) + (4 * q + 2 * hh);
                av[s][0] = ap[0];
                av[s][1] = ap[1];
            }
        };
        f16x8 b0[2], b1[2], b2[2], a0[NS][2], a1[NS][2];
#pragma unroll
        for (int j = 0; j < 2; j++) b0[j] = b1[j] = b2[j] = f16x8{};
#pragma unroll
        for (int s = 0; s < NS; s++)
#pragma unroll
            for (int j = 0; j < 2; j++) a0[s][j] = a1[s][j] = f16x8{};
        int q = wave;
        if (q < NC) {
            load_b(q, b0);
            load_a(q, a0);
        }
        if (q + 4 < NC) load_b(q + 4, b1);
        for (; q < NC; q += 4) {
            if (q + 8 < NC) load_b(q + 8, b2);
            if (q + 4 < NC) load_a(q + 4, a1);   // (in flight while this chunk's MFMAs issue)
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    if (!((has >> s) & 1u)) continue;
                    acc[s][j % NA] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[s][j], b0[j], acc[s][j % NA], 0, 0, 0);
                }
#pragma unroll
            for (int j = 0; j < 2; j++) {
                b0[j] = b1[j];
                b1[j] = b2[j];
#pragma unroll
                for (int s = 0; s < NS; s++) a0[s][j] = a1[s][j];
            }
        }
    }
    // column r of the tile is gate r >> 3 of hidden column j0 + (r & 7), so lane (row, j < 8) holds i and fetches f, g, o of its cell
    // from the lanes 8, 16 and 24 to its right
    const long long G = 4LL * H;
    const float* gcol = gx + (long long)(r >> 3) * H + j0 + (r & 7);
    auto finish = [&](int s, const f32x16& t) {
        if (row0 + 32 * s >= a) return;   // (uniform over the wave)
#pragma unroll
        for (int g = 0; g < 16; g++) {
            const int m = row0 + 32 * s + (g & 3) + 8 * (g >> 2) + 4 * hh;
            const float v = m < a ? t[g] + gcol[(long long)m * G] : 0.f;
            const float vf = __shfl(v, lane + 8), vg = __shfl(v, lane + 16), vo = __shfl(v, lane + 24);
            if (r >= 8 || m >= a) continue;
            const long long o = (long long)m * H + j0 + r;
            const float cn = sigmoid_f(vf) * c[o] + sigmoid_f(v) * tanhf(vg);
            float hn = sigmoid_f(vo) * tanhf(cn);
            // the mirror is f16 of the STORED float32 value: without this fence the compiler folds the product and the conversion into
            // one v_fma_mixlo_f16, which rounds the exact product once and differs from f16(h_out) where the two roundings do not commute
            asm volatile("" : "+v"(hn));
            c[o] = cn;
            h_out[o] = hn;
            const _Float16 h16 = (_Float16)hn;   // nearest even, f16 subnormals kept: the next position's A operand
            h_out16[o] = __builtin_bit_cast(uint16_t, h16);
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

void rnn_lm_step_f16(const Ctx& ctx, const uint16_t* h_prev16, const uint16_t* whh_h, const float* gx, float* c, float* h_out, uint16_t* h_out16,
                     int a, int H) {
    K2_REQUIRE(a > 0 && H > 0 && H % 32 == 0, "rnn_lm_step_f16: %d rows, hidden_dim %d (a multiple of 32)", a, H);
    if (ctx.dry) return;
    K2_REQUIRE(whh_h && gx && c && h_out && h_out16, "rnn_lm_step_f16: a buffer is missing");
    const int strips = cdiv(std::min(a, HMAXR), 32);
    const dim3 grid(H / 8, cdiv(a, HMAXR)), block(HT);
    if (strips <= 1) hipLaunchKernelGGL(k_lm_lstm_step_f16<1>, grid, block, 0, ctx.stream, h_prev16, whh_h, gx, c, h_out, h_out16, a, H);
    else if (strips <= 2) hipLaunchKernelGGL(k_lm_lstm_step_f16<2>, grid, block, 0, ctx.stream, h_prev16, whh_h, gx, c, h_out, h_out16, a, H);
    else if (strips <= 4) hipLaunchKernelGGL(k_lm_lstm_step_f16<4>, grid, block, 0, ctx.stream, h_prev16, whh_h, gx, c, h_out, h_out16, a, H);
    else hipLaunchKernelGGL(k_lm_lstm_step_f16<8>, grid, block, 0, ctx.stream, h_prev16, whh_h, gx, c, h_out, h_out16, a, H);
    K2_HIP(hipGetLastError());
}

}  // namespace k2hip
