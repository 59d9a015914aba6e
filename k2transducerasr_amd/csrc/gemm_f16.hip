// Half-precision-operand GEMM for gfx950:  C = epilogue(f16(A) . f16(W)^T), float32 sums (Engine::set_encoder_precision).
//
// Why a kernel of its own: v_mfma_f32_32x32x16_f16 does eight times the multiply-adds of v_mfma_f32_32x32x2_f32 per instruction, so at
// the encoder's shapes (K = 192 .. 2048) the matrix pipe is no longer what a launch waits for -- the float32 A tile that has to be read
// and rounded, and the float32 C tile that has to be written, are.  The float32 kernels' K loop is built around keeping every VALU
// instruction out of it; this one spends VALU work (the rounding of A) inside it on purpose and keeps the LDS image in the order the
// MFMA operands are read, so that every operand is ONE ds_read_b128.
//
// Operands
//   A  float32 [M, K] as the producers leave it in HBM (lda % 4 == 0).  Rounded to f16 TO NEAREST EVEN (v_cvt_f16_f32; f16 subnormals
//      kept) on its way into LDS: values beyond the f16 range become infinities, NaNs stay NaNs.
//   W  the f16 panels of gemm_f16_layout.h, built once per model: blocks of 32 columns x chunks of 32 k, a (block, chunk) being 2 KiB
//      in operand order [j: 2][hh: 2][32 columns][e: 8].  The float32 matrix is never read.
// k order: instruction j (0, 1) of chunk q takes from lane half hh the eight k = 32 q + 16 hh + 8 j + e on both operands -- a permutation
// of k inside a chunk, which a sum does not see.  A lane's A side of both instructions is one run of 16 consecutive floats of its row.
//
// Work split: 256 threads, four waves as 2 x 2, each wave a (BM / 2) x (BN / 2) block of 32 x 32 accumulator tiles; workgroup tiles
// 128 x 128, 128 x 64, 64 x 64 (K2_F16_TABLE; plan_gemm_f16 picks one by workgroup count), walked in xcd_tile's order.
//
// Data movement: a stage is BK = 64, two chunks.  While a stage's MFMAs issue, every thread holds the NEXT stage in registers:
//   A  BM / 64 runs of 16 consecutive floats (four float4 loads each; four neighbouring lanes cover 256 contiguous bytes of a row; rows
//      >= M clamped to M - 1, their results never stored).  After the MFMAs the runs are rounded and written as two 16-byte LDS stores
//      each, in operand order [32-row block][q][j][hh][32 rows][e: 8] with the row slot rotated by 4 (2 q + hh) so that the four lanes
//      of a row -- whose groups are 512 bytes apart -- fall on different banks.
//   W  BN / 32 16-byte loads: the stage of a column block is 4 KiB contiguous in the panels and is copied as it lies, thread t moving
//      bytes 16 t .. 16 t + 15 of each block (a wave's load and its LDS store are 1 KiB contiguous).  The two waves of a column share it.
//      Through registers rather than by LDS-DMA: the A side needs the register round trip anyway (the rounding), so both operands of a
//      stage then ride on ONE wait and ONE barrier that the compiler places, with no hand-written M0 / vmcnt bookkeeping beside
//      compiler-scheduled loads.
// Two stages of (BM + BN) x 64 halves: 64 KiB for 128 x 128 (two workgroups per CU in 160 KiB), 48 / 32 KiB for the smaller tiles.  One
// barrier per stage.  K % 32 == 0: an odd chunk count ends in a half stage whose second chunk is neither loaded nor multiplied.
//
// Epilogue: the C/D layout of 32x32x16_f16 is that of 32x32x2_f32, so it is gemm_epilogue.h's epilogue_rows<16, Rows32> -- bias, every
// act, act_cols, res (in place too), act_after_res and, at level 2 of the switch, glu / glu_cols and the bypass mix.  Everything else
// stays on the float32 kernels (gemm_plan.cpp gemm_f16_form).
//
// GATHER (level 3; every tile): the conv-gather form of gemm.hip's MODE_CONV -- A is an NHWC tensor, row r's window starts at the
// base GemmArgs cv_* name and k sits at (k / seg_len) seg_stride + k % seg_len.  Only the ADDRESS of a thread's run of 16 consecutive
// floats changes (seg_len % 16 == 0: a run never straddles a segment; cv_C, seg_stride % 4 == 0: its float4 loads stay aligned): the
// row base once, the segment of the run's k stage by stage.  Everything behind the LDS store is the loop and the epilogue below.
// encoder_embed.conv.7: K = 288 = three segments of 96, nine chunks (a half-stage tail).
//
// DWK > 0 (15 or 31; BN = 64 only): the offline conv module's form at level 2 -- in_proj + GLU + depthwise Conv1d over time + bias +
// SwooshR in one launch, the f16 counterpart of gemm_f32_mfma_pipe<..., DWK>.  One M tile per STREAM: the tile of stream b starts at row
// b dw_T (dw_T <= BM; rows >= dw_T of the tile are staged like any rows -- clamped to M - 1 -- and never used).  A workgroup owns the 32
// channels of its 64 GEMM columns.  After the K loop, in the stage memory (every wave has passed the loop's last barrier):
//   xs   [BM + DWK - 1][32] floats: bias + GLU formed operation for operation as epilogue_rows forms them, the value lanes writing frame
//        t to row DWK / 2 + t; the DWK / 2 rows in front of and behind the stream are zeroed -- the conv's padding.  Rows past
//        dw_T + DWK - 1 keep whatever the stages left: they feed only frames >= dw_T, which are not stored.
//   taps [DWK][32] floats behind it.  The float32 form keeps a thread's DWK taps in registers from in front of the K loop; here that
//        would put 31 more registers on a loop that runs at 142 (128 x 64) -- past the 168 that three waves per SIMD allow.  Instead
//        every thread requests <= 4 elements of the workgroup's tap tile and its channel's conv bias in front of the K loop (5 registers
//        across it) and drops the taps into LDS behind the loop.
//   Thread (channel = tid % 32, frame group = tid / 32) forms FT = BM / 8 consecutive frames (16 / 8) of its channel.  Taps ascending:
//   tap q is one LDS read (32 lanes, 32 consecutive floats), the input window slides by one row -- one more LDS read -- and every output
//   takes one fmaf: each sum starts from the conv bias and takes its taps in ascending order, the order and the operations of
//   k_glu_dwconv1d.  2 LDS reads per FT fmas; live registers FT outputs + FT window.  Then SwooshR and the store to C = y [M, N / 2]
//   (a 32-lane half writes 128 contiguous bytes).  Frame groups that start at or past dw_T do nothing.
#include "gemm_epilogue.h"
#include "kernels.h"

namespace k2hip {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

namespace {

__device__ __forceinline__ f16x8 round8(const float4& lo, const float4& hi) {   // plain conversions: v_cvt_f16_f32, nearest even
    return f16x8{(_Float16)lo.x, (_Float16)lo.y, (_Float16)lo.z, (_Float16)lo.w, (_Float16)hi.x, (_Float16)hi.y, (_Float16)hi.z, (_Float16)hi.w};
}

template <int BM, int BN, int DWK = 0, bool GATHER = false>
__global__ __launch_bounds__(256) void gemm_f16_mfma(GemmArgs g, const uint16_t* __restrict__ panels) {
    constexpr int MT = BM / 64, NT = BN / 64;        // 32 x 32 accumulator tiles of a wave
    constexpr int NU = BM / 64;                      // A runs of 16 floats per thread and stage
    constexpr int NWL = BN / 32;                     // W 16-byte pieces per thread and stage: one per column block
    constexpr int A_HALVES = BM * 64, STAGE = (BM + BN) * 64;
    static_assert(BM % 64 == 0 && BN % 64 == 0, "f16 gemm: four waves of whole 32 x 32 tiles");
    constexpr int DW_CH = 32, DW_FT = BM / 8, DW_HALF = DWK / 2, DW_XS = (BM + DWK - 1) * DW_CH;   // the conv tail's LDS image, in floats
    constexpr int DW_NTAP = (DWK * DW_CH + 255) / 256;                                            // tap elements a thread stages
    static_assert(!GATHER || DWK == 0, "f16 gemm: the conv-gather form has the plain epilogue");
    static_assert(DWK == 0 || (BN == 64 && DWK % 2 == 1 && (DW_XS + DWK * DW_CH) * 4 <= 2 * STAGE * 2), "f16 gemm: conv tail's tile form");
    extern __shared__ __attribute__((aligned(16))) _Float16 smem_h[];   // [2][STAGE]: the A image, then the W image

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int li = lane & 31, lh = lane >> 5;
    int mb_, nb_;
    xcd_tile(mb_, nb_, g.xcd_panels == 1 ? 0 : g.M, g.N);
    const int m0 = DWK > 0 ? mb_ * g.dw_T : mb_ * BM, n0 = nb_ * BN;
    const int K = g.K, nk = K / 32, ns = (nk + 1) / 2;
    const int NB = (g.N + 31) / 32;                  // column blocks the panels hold

    // ---- this thread's loads and LDS stores of a stage: addresses, once ----
    const float* ap[NU];
    int a_dst[NU];      // halves from the stage's start, instruction j = 0 (j = 1: + 2 * 32 * 8)
    int a_q[NU];
    const int a_k0 = 16 * (tid & 3);   // GATHER: k of this thread's runs in stage 0 (seg = tid & 3 for every i)
#pragma unroll
    for (int i = 0; i < NU; i++) {
        const int u = tid + 256 * i, row = u >> 2, seg = u & 3, q = seg >> 1, hh = seg & 1;
        if constexpr (GATHER) {   // the row's window in the NHWC input (kernels.h GemmArgs cv_*); the k offset is added stage by stage
            const int r = min(m0 + row, g.M - 1), f = r % g.cv_Fout, bt = r / g.cv_Fout, t = bt % g.cv_Tout, b = bt / g.cv_Tout;
            ap[i] = g.A + (((long long)b * g.cv_Tin + (long long)t * g.cv_st) * g.cv_Fin + (long long)f * g.cv_sf) * g.cv_C;
        } else
            ap[i] = g.A + (long long)min(m0 + row, g.M - 1) * g.lda + 32 * q + 16 * hh;
        a_dst[i] = ((((row >> 5) * 2 + q) * 4 + hh) * 32 + (((row & 31) + 4 * seg) & 31)) * 8;
        a_q[i] = q;
    }
    const _Float16* wp[NWL];
#pragma unroll
    for (int i = 0; i < NWL; i++)
        wp[i] = reinterpret_cast<const _Float16*>(panels) + (long long)min(n0 / 32 + i, NB - 1) * 32 * K + tid * 8;
    const int w_q = tid >> 7;   // the chunk of the stage this thread's W pieces belong to

    float4 araw[NU][4];
    f16x8 wraw[NWL];
    auto load_stage = [&](int s) {
        const int left = nk - 2 * s;   // chunks of stage s: 1 or >= 2
        // GATHER: k -> (k / seg_len) seg_stride + k % seg_len; seg_len % 16 == 0, so the run of 16 stays inside its segment
        const int gk = a_k0 + 64 * s, gseg = GATHER ? gk / g.seg_len : 0;
        const long long koff = GATHER ? (long long)gseg * g.seg_stride + (gk - gseg * g.seg_len) : 64 * s;
#pragma unroll
        for (int i = 0; i < NU; i++) {
            if (a_q[i] < left) {
                const float4* p = reinterpret_cast<const float4*>(ap[i] + koff);
#pragma unroll
                for (int v = 0; v < 4; v++) araw[i][v] = p[v];
            } else {
#pragma unroll
                for (int v = 0; v < 4; v++) araw[i][v] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int i = 0; i < NWL; i++) {
            if (w_q < left) wraw[i] = *reinterpret_cast<const f16x8*>(wp[i] + 2048 * s);
            else wraw[i] = f16x8{};
        }
    };
    auto store_stage = [&](int buf) {
        _Float16* st = smem_h + buf * STAGE;
#pragma unroll
        for (int i = 0; i < NU; i++) {
            *reinterpret_cast<f16x8*>(st + a_dst[i]) = round8(araw[i][0], araw[i][1]);
            *reinterpret_cast<f16x8*>(st + a_dst[i] + 2 * 32 * 8) = round8(araw[i][2], araw[i][3]);
        }
#pragma unroll
        for (int i = 0; i < NWL; i++) *reinterpret_cast<f16x8*>(st + A_HALVES + i * 2048 + tid * 8) = wraw[i];
    };

    load_stage(0);
    float bias_pre[NT];
#pragma unroll
    for (int j = 0; j < NT; j++) bias_pre[j] = g.bias ? g.bias[min(n0 + (wc * NT + j) * 32 + li, g.N - 1)] : 0.f;

    // (DWK: this thread's share of the workgroup's tap tile [DWK][32] and its channel's conv bias, in flight under the K loop)
    float dw_stage[DWK > 0 ? DW_NTAP : 1], dw_bias = 0.f;
    if constexpr (DWK > 0) {
        const int ch0 = n0 >> 1, D = g.N >> 1;   // (N % BN == 0: every channel of the tile exists)
        dw_bias = g.dw_b[ch0 + (tid & (DW_CH - 1))];
#pragma unroll
        for (int i = 0; i < DW_NTAP; i++) {
            const int e = tid + 256 * i;
            dw_stage[i] = e < DWK * DW_CH ? g.dw_w[(long long)(e >> 5) * D + ch0 + (e & (DW_CH - 1))] : 0.f;
        }
    }

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; i++)
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

    // operand read offsets (halves from the stage's start) of chunk 0, instruction 0; chunk q: the A slot rotates by 8 q, + q * 4 * 256
    // (A) / + q * 1024 (W); instruction j: + j * 2 * 256 on both
    int a_src[2];
#pragma unroll
    for (int q = 0; q < 2; q++) a_src[q] = ((((wr * MT) * 2 + q) * 4 + lh) * 32 + ((li + 4 * (2 * q + lh)) & 31)) * 8;
    const int b_src = A_HALVES + (wc * NT) * 2048 + (lh * 32 + li) * 8;

    store_stage(0);
    __syncthreads();
    for (int s = 0; s < ns; s++) {
        const bool more = s + 1 < ns;
        if (more) load_stage(s + 1);
        const _Float16* st = smem_h + (s & 1) * STAGE;
        const int left = nk - 2 * s;
#pragma unroll
        for (int q = 0; q < 2; q++) {
            if (q < left) {   // wave-uniform: the half stage at the end of an odd chunk count
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    f16x8 fa[MT], fb[NT];
#pragma unroll
                    for (int i = 0; i < MT; i++) fa[i] = *reinterpret_cast<const f16x8*>(st + a_src[q] + i * 2 * 4 * 256 + j * 2 * 256);
#pragma unroll
                    for (int n = 0; n < NT; n++) fb[n] = *reinterpret_cast<const f16x8*>(st + b_src + n * 2048 + q * 1024 + j * 2 * 256);
#pragma unroll
                    for (int i = 0; i < MT; i++)
#pragma unroll
                        for (int n = 0; n < NT; n++) acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i], fb[n], acc[i][n], 0, 0, 0);
                }
            }
        }
        if (more) store_stage((s + 1) & 1);
        __syncthreads();   // stage s + 1 is whole; everyone has left stage s, which the next iteration's stores overwrite
    }

    if constexpr (DWK > 0) {
        const int T = g.dw_T;
        float* xs = reinterpret_cast<float*>(smem_h);   // behind the loop's last barrier nobody reads the stages any more
        float* taps = xs + DW_XS;
#pragma unroll
        for (int i = 0; i < DW_NTAP; i++)
            if (tid + 256 * i < DWK * DW_CH) taps[tid + 256 * i] = dw_stage[i];
        for (int e = tid; e < 2 * DW_HALF * DW_CH; e += 256) {   // the time halo
            const int r = e >> 5;
            xs[((r < DW_HALF ? r : T + r) << 5) + (e & (DW_CH - 1))] = 0.f;
        }
#pragma unroll
        for (int n = 0; n < NT; n++)
#pragma unroll
            for (int i = 0; i < MT; i++) {
                // (value | gate) blocks of 32 columns: the value lanes (li & 16) == 0 hold channel 16 (column / 32) + (li & 15)
                const int ch = (wc * NT + n) * 16 + (li & 15), lrow0 = (wr * MT + i) * 32 + 4 * lh;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const float v = acc[i][n][r] + bias_pre[n];
                    const float other = __shfl_xor(v, 16, 64);
                    const float gated = v * (1.0f / (1.0f + __expf(-other)));   // epilogue_rows' GLU, operation for operation
                    const int lrow = lrow0 + Rows32::off(r);
                    if ((li & 16) == 0 && lrow < T) xs[((DW_HALF + lrow) << 5) + ch] = gated;
                }
            }
        __syncthreads();
        const int ch = tid & (DW_CH - 1), t0 = (tid >> 5) * DW_FT;
        if (t0 >= T) return;
        const float* xp = xs + (t0 << 5) + ch;   // rows t0 .. t0 + DW_FT + DWK - 2 <= BM + DWK - 2: inside xs
        float o[DW_FT], win[DW_FT];
#pragma unroll
        for (int i = 0; i < DW_FT; i++) {
            o[i] = dw_bias;
            win[i] = xp[i << 5];
        }
#pragma unroll
        for (int q = 0; q < DWK; q++) {   // window slot (q + i) % DW_FT holds input row t0 + q + i
            const float tq = taps[(q << 5) + ch];
#pragma unroll
            for (int i = 0; i < DW_FT; i++) o[i] = __builtin_fmaf(tq, win[(q + i) % DW_FT], o[i]);
            if (q + 1 < DWK) win[q % DW_FT] = xp[(q + DW_FT) << 5];
        }
        float* yp = g.C + (long long)(m0 + t0) * g.ldc + (n0 >> 1) + ch;
#pragma unroll
        for (int i = 0; i < DW_FT; i++)
            if (t0 + i < T) yp[(long long)i * g.ldc] = swoosh_r(o[i]);
        return;
    }

#pragma unroll
    for (int n = 0; n < NT; n++)
#pragma unroll
        for (int i = 0; i < MT; i++) {
            float vals[16];
#pragma unroll
            for (int r = 0; r < 16; r++) vals[r] = acc[i][n][r];
            epilogue_rows<16, Rows32>(g, vals, m0 + (wr * MT + i) * 32 + 4 * lh, n0 + (wc * NT + n) * 32 + li, g.C, g.res, vals, false, nullptr,
                                      g.bias, true, bias_pre[n]);
        }
}

template <int BM, int BN, bool GATHER = false>
void launch_f16(const Ctx& ctx, const GemmArgs& a, const uint16_t* panels) {
    dim3 grid(cdiv(a.N, BN), cdiv(a.M, BM), 1);
    const size_t lds = sizeof(uint16_t) * 2 * (BM + BN) * 64;
    static LdsAttrOnce lds_attr;
    lds_attr.ensure(gemm_f16_mfma<BM, BN, 0, GATHER>, (int)lds);
    hipLaunchKernelGGL((gemm_f16_mfma<BM, BN, 0, GATHER>), grid, dim3(256), lds, ctx.stream, a, panels);
}

// the conv-tail form: one M tile per stream
template <int BM, int DWK>
void launch_f16_dwconv(const Ctx& ctx, const GemmArgs& a, const uint16_t* panels) {
    K2_REQUIRE(a.dw_K == DWK && a.dw_T >= 1 && a.dw_T <= BM && a.M % a.dw_T == 0 && a.N % 64 == 0 && a.ldc >= a.N / 2 && a.dw_w && a.dw_b && a.bias,
               "gemm_f16: conv tail needs whole streams of <= %d frames and whole column tiles (T %d, M %d, N %d)", BM, a.dw_T, a.M, a.N);
    dim3 grid(a.N / 64, a.M / a.dw_T, 1);
    const size_t lds = sizeof(uint16_t) * 2 * (BM + 64) * 64;
    static LdsAttrOnce lds_attr;
    lds_attr.ensure(gemm_f16_mfma<BM, 64, DWK>, (int)lds);
    hipLaunchKernelGGL((gemm_f16_mfma<BM, 64, DWK>), grid, dim3(256), lds, ctx.stream, a, panels);
}

}  // namespace

void gemm_f16_launch(const Ctx& ctx, const GemmArgs& a, const uint16_t* panels, const GemmF16Plan& p) {
    K2_REQUIRE(panels && gemm_f16_fits(a, 3), "gemm_f16: %d x %d x %d (lda %d) is not a form the half-precision kernel takes", a.M, a.N, a.K, a.lda);
    if (a.cv_Fout > 0) {
        K2_REQUIRE(gemm_f16_fits(a, 3), "gemm_f16: not a conv gather the half-precision kernel takes (seg_len %d, seg_stride %d, C %d)", a.seg_len, a.seg_stride, a.cv_C);
        switch (p.idx) {
#define X(i, bm, bn) case i: launch_f16<bm, bn, true>(ctx, a, panels); break;
            K2_F16_TABLE(X)
#undef X
            default: failf(K2HIP_ERR_INVALID, "gemm_f16: no tile %d", p.idx);
        }
        return;
    }
    if (a.dw_w) {
        K2_REQUIRE((p.idx == 1 || p.idx == 2) && a.dw_T <= p.BM, "gemm_f16: tile %d does not hold a stream of %d frames", p.idx, a.dw_T);
        if (p.idx == 1) a.dw_K == 15 ? launch_f16_dwconv<128, 15>(ctx, a, panels) : launch_f16_dwconv<128, 31>(ctx, a, panels);
        else a.dw_K == 15 ? launch_f16_dwconv<64, 15>(ctx, a, panels) : launch_f16_dwconv<64, 31>(ctx, a, panels);
        return;
    }
    switch (p.idx) {
#define X(i, bm, bn) case i: launch_f16<bm, bn>(ctx, a, panels); break;
        K2_F16_TABLE(X)
#undef X
        default: failf(K2HIP_ERR_INVALID, "gemm_f16: no tile %d", p.idx);
    }
}

}  // namespace k2hip
