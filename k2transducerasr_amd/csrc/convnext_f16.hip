// The embed's ConvNeXt pointwise pair in ONE launch for gfx950 (level 3 of Engine::set_encoder_precision):
//   C[m, :] = R[m, :] + W2 . f16(SwooshL(W1 . f16(X[m, :]) + b1)) + b2        X [M, 128] float32, hidden 384, C / R [M, 128] float32
//
// Why a kernel of its own: as two gemm_f16_mfma launches the [M, 384] float32 hidden tensor is written to HBM and read back (0.9 GB at
// the headline batch) only to be rounded to f16 on its way into the second product.  Here the rounded hidden values go straight into
// LDS, already in the order the second product reads its A operand, and never leave the CU.
//
// Contract: both products on v_mfma_f32_32x32x16_f16 with float32 sums; an accumulator takes its k in ascending chunks of 32, inside a
// chunk instruction j = 0 then 1 in gemm_f16_layout.h's k permutation; bias, SwooshL, residual are gemm_epilogue.h's, operation for
// operation; every rounding is v_cvt_f16_f32 (nearest even).  So the output is BIT FOR BIT that of gemm_f16_mfma(W1, SwooshL) into a
// float32 hidden tensor followed by gemm_f16_mfma(W2, res in place), whatever tiles those launches take.
//
// Work split: 256 threads = four waves, a tile of 128 pixels per workgroup (grid: one workgroup per tile, walked in xcd_tile's order --
// a band of pixels per XCD).  The 384 hidden columns are taken in three groups of 128.  Per group
//   product 1  wave w forms hidden columns 128 g + 32 w .. + 31 of all 128 pixels: four 32 x 32 accumulators (one per 32-pixel block),
//              K = 128 in four chunks.  The product is formed TRANSPOSED -- W1's panel fragment as the A operand, the pixels as B -- so
//              that in the C/D layout a lane holds, for ONE pixel, four runs of 4 consecutive hidden columns: after bias + SwooshL +
//              rounding a run is 8 bytes that lie together in the second product's operand order, and the wave's store of a run is
//              512 contiguous bytes of LDS (the plain orientation would scatter 2-byte stores 4-way onto the same banks).  A and B have
//              the same register layout and a product does not know which factor came from which, so each sum is the plain one's.
//   hidden     the group's 128 x 128 f16 image: the wave's 32 columns are chunk w of the group.
//   product 2  wave w adds the group's four chunks into output columns 32 w .. + 31 of all 128 pixels: four accumulators that stay in
//              registers across the three groups (chunks 4 g .. 4 g + 3 of K = 384: ascending).
// So every wave reads each of its W fragments once per tile and the workgroup fetches each panel exactly once; W is never staged: the
// panels are in MFMA operand order, a fragment is ONE 16-byte global load per lane (1 KiB contiguous per wave) out of 196 KB that stay
// in L2.  A group's eight W1 fragments are requested in front of its first MFMA, its eight W2 fragments
// behind product 1's last, under the hidden epilogue.
//
// LDS: two operand images of 128 rows x 128 k halves, 32 KiB each, in gemm_f16_mfma's A order [32-row block][q: 4][j: 2][hh: 2][32 row
// slots][e: 8] with the row slot rotated by 4 (2 q + hh): the X tile (staged once: a thread's four runs of 16 consecutive floats ->
// two 16-byte stores each) and the hidden group.  64 KiB: two workgroups per CU, whose barriers (two per group) hide behind each other.
// Registers: 64 + 64 accumulators, 64 of W fragments, 16 of A fragments.
// Rows >= M: X rows are clamped to M - 1 on the way in, their results are never stored.
#include "gemm_epilogue.h"
#include "kernels.h"

namespace k2hip {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int TM = 128;              // pixels of a tile
constexpr int IMG = TM * 128;        // halves of an operand image

__device__ __forceinline__ f16x8 round8(const float4& lo, const float4& hi) {   // plain conversions: v_cvt_f16_f32, nearest even
    return f16x8{(_Float16)lo.x, (_Float16)lo.y, (_Float16)lo.z, (_Float16)lo.w, (_Float16)hi.x, (_Float16)hi.y, (_Float16)hi.z, (_Float16)hi.w};
}
// halves from an image's start of row `row`'s eight k = 32 q + 16 hh + 8 j + (0 .. 7)
__device__ __forceinline__ int img_at(int row, int q, int j, int hh) {
    return ((((row >> 5) * 4 + q) * 4 + 2 * j + hh) * 32 + (((row & 31) + 4 * (2 * q + hh)) & 31)) * 8;
}

__global__ __launch_bounds__(256, 2) void convnext_f16_mfma(ConvnextF16Args a) {
    static_assert(kConvnextC == 128 && kConvnextH == 384, "convnext_f16: three groups of four chunks over four chunks of input");
    extern __shared__ __attribute__((aligned(16))) _Float16 smem_h[];
    _Float16* const xs = smem_h;         // f16(X) of the tile
    _Float16* const hs = smem_h + IMG;   // f16(SwooshL(..)) of the current group

    const int tid = threadIdx.x;
    const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    int mb_, nb_;
    xcd_tile(mb_, nb_);
    const int m0 = mb_ * TM, M = a.M;

    // ---- the X tile: 128 rows x 8 runs of 16 floats, four runs per thread (eight neighbouring lanes cover 512 contiguous bytes) ----
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int u = tid + 256 * i, row = u >> 3, seg = u & 7, q = seg >> 1, hh = seg & 1;
        const float4* p = reinterpret_cast<const float4*>(a.X + (long long)min(m0 + row, M - 1) * a.ldx + 16 * seg);
        const float4 v0 = p[0], v1 = p[1], v2 = p[2], v3 = p[3];
        *reinterpret_cast<f16x8*>(xs + img_at(row, q, 0, hh)) = round8(v0, v1);
        *reinterpret_cast<f16x8*>(xs + img_at(row, q, 1, hh)) = round8(v2, v3);
    }
    const float b2_pre = a.b2[w * 32 + li];

    f32x16 acc_o[4];
#pragma unroll
    for (int pb = 0; pb < 4; pb++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc_o[pb][r] = 0.f;

    // a lane's operand read of pixel block pb, chunk q, instruction j: row li of the block, lane half lh
    int src[4];
#pragma unroll
    for (int q = 0; q < 4; q++) src[q] = img_at(li, q, 0, lh);
    constexpr int PB = 4 * 4 * 256, JJ = 2 * 256;   // halves between pixel blocks / between the two instructions of a chunk

    const f16x8* p1 = reinterpret_cast<const f16x8*>(a.p1) + lane;
    const f16x8* p2 = reinterpret_cast<const f16x8*>(a.p2) + (long long)w * 32 * kConvnextH / 8 + lane;
    __syncthreads();

    for (int g = 0; g < 3; g++) {
        // the group's W fragments: W1 column block 4 g + w (its four chunks), W2 column block w, chunks 4 g .. 4 g + 3; a (chunk,
        // instruction) fragment is 512 halves = 64 f16x8
        f16x8 f1[4][2], f2[4][2];
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int j = 0; j < 2; j++) f1[q][j] = p1[((4 * g + w) * 4 + q) * 128 + j * 64];

        // ---- product 1, transposed: D[hidden column][pixel] ----
        f32x16 acc_h[4];
#pragma unroll
        for (int pb = 0; pb < 4; pb++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc_h[pb][r] = 0.f;
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int j = 0; j < 2; j++) {
                f16x8 fx[4];
#pragma unroll
                for (int pb = 0; pb < 4; pb++) fx[pb] = *reinterpret_cast<const f16x8*>(xs + src[q] + pb * PB + j * JJ);
#pragma unroll
                for (int pb = 0; pb < 4; pb++) acc_h[pb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f1[q][j], fx[pb], acc_h[pb], 0, 0, 0);
            }
        // (W2's fragments travel under the hidden epilogue: requested here, they keep 32 registers off product 1's loop)
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int j = 0; j < 2; j++) f2[q][j] = p2[(4 * g + q) * 128 + j * 64];
        float4 bv[4];   // b1 of this lane's hidden columns: 8 g4 + 4 lh + (0 .. 3) of the wave's 32
#pragma unroll
        for (int g4 = 0; g4 < 4; g4++) bv[g4] = *reinterpret_cast<const float4*>(a.b1 + 128 * g + 32 * w + 8 * g4 + 4 * lh);
        if (g > 0) __syncthreads();   // every wave has read the previous group's image to the end
        // register r of lane (li, lh): hidden column (r & 3) + 8 (r >> 2) + 4 lh of the wave's chunk, pixel 32 pb + li.  Run g4 = r >> 2 is
        // k = 8 g4 + 4 lh + (0 .. 3) of chunk w: instruction j = g4 & 1, lane half hh = g4 >> 1, elements 4 lh ..
#pragma unroll
        for (int pb = 0; pb < 4; pb++)
#pragma unroll
            for (int g4 = 0; g4 < 4; g4++) {
                const float b[4] = {bv[g4].x, bv[g4].y, bv[g4].z, bv[g4].w};
                f16x4 h;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    float v = acc_h[pb][4 * g4 + e];
                    v += b[e];                                   // epilogue_rows: v += bias, then the activation
                    h[e] = (_Float16)apply_act(v, ACT_SWOOSH_L);
                }
                *reinterpret_cast<f16x4*>(hs + img_at(32 * pb + li, w, g4 & 1, g4 >> 1) + 4 * lh) = h;
            }
        __syncthreads();
        // ---- product 2: the group's four chunks into the output accumulators ----
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int j = 0; j < 2; j++) {
                f16x8 fh[4];
#pragma unroll
                for (int pb = 0; pb < 4; pb++) fh[pb] = *reinterpret_cast<const f16x8*>(hs + src[q] + pb * PB + j * JJ);
#pragma unroll
                for (int pb = 0; pb < 4; pb++) acc_o[pb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fh[pb], f2[q][j], acc_o[pb], 0, 0, 0);
            }
    }

    // ---- epilogue: + b2, + R (in place: a lane reads exactly the elements it then writes), rows >= M not stored ----
    GemmArgs e;
    e.M = M; e.N = kConvnextC; e.ldc = a.ldc; e.ldr = a.ldr;
#pragma unroll
    for (int pb = 0; pb < 4; pb++) {
        float vals[16];
#pragma unroll
        for (int r = 0; r < 16; r++) vals[r] = acc_o[pb][r];
        epilogue_rows<16, Rows32>(e, vals, m0 + 32 * pb + 4 * lh, 32 * w + li, a.C, a.R, vals, false, nullptr, a.b2, true, b2_pre);
    }
}

}  // namespace

void convnext_f16(const Ctx& ctx, const ConvnextF16Args& a) {
    K2_REQUIRE(a.M >= 1 && a.ldx >= kConvnextC && a.ldx % 4 == 0 && a.ldc >= kConvnextC && a.ldr >= kConvnextC,
               "convnext_f16: shape (M %d, ldx %d, ldr %d, ldc %d)", a.M, a.ldx, a.ldr, a.ldc);
    K2_REQUIRE((long long)a.M * a.ldx < (1ll << 29) && (long long)a.M * a.ldc < (1ll << 29) && (long long)a.M * a.ldr < (1ll << 29),
               "convnext_f16: %d pixels are too many for 32-bit lane offsets", a.M);
    const double fl = 2.0 * a.M * (double)kConvnextC * kConvnextH;
    ctx.add_flops(2.0 * fl, 0.0, 1);   // the two GEMMs it replaces, as one launch
    if (ctx.dry) return;   // (the sizing pass: the arena hands out no memory yet)
    K2_REQUIRE(a.X && a.p1 && a.p2 && a.b1 && a.b2 && a.R && a.C, "convnext_f16: a null operand");
    if (ctx.instrument) K2_HIP(hipEventRecord(ctx.next_event(), ctx.stream));
    if (ctx.instrument && ctx.gemm_log) ctx.gemm_log->push_back({a.M, kConvnextC, kConvnextC + kConvnextH, 1, ACT_SWOOSH_L, 1, gemm_kind_convnext_f16(), 0.f});
    constexpr size_t lds = sizeof(uint16_t) * 2 * IMG;
    static LdsAttrOnce lds_attr;
    lds_attr.ensure(convnext_f16_mfma, (int)lds);
    hipLaunchKernelGGL(convnext_f16_mfma, dim3(1, cdiv(a.M, TM), 1), dim3(256), lds, ctx.stream, a);
    K2_HIP(hipGetLastError());
    if (ctx.f16) ctx.f16->launches++;
    if (ctx.instrument) K2_HIP(hipEventRecord(ctx.next_event(), ctx.stream));
}

}  // namespace k2hip
