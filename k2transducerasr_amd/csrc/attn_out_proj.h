// Phase C of attn_f16.hip's k_attn_av_out_f16: a workgroup's 16 context rows in LDS times out_proj, plus bias and residual, on the f32
// 16x16x4 MFMA.  It is k_attn_av_out's phase C (attn.hip), operation for operation, as a function.  attn.hip keeps its own inline
// copy: calling this function from there moved the float32 kernel's instruction schedule (same instructions, another order; the
// resource report and the bits of that kernel are held fixed), so the body exists twice on purpose.
#pragma once
#include "kernels.h"

namespace k2hip {

typedef float attn_f32x4 __attribute__((ext_vector_type(4)));

// out[16, D] = avs[16, HV] . wout^T + bias + xres, rows i0 .. i0 + 15 of stream b (rows >= T not stored); avs [16][AS] floats in LDS,
// complete (the caller has passed its barrier).  lane = (column n, k group kq); the four waves take the column tiles of this
// blockIdx.z slice in turn.
__device__ __forceinline__ void attn_out_proj_tiles(const float* avs, int AS, int HV, const float* __restrict__ wout,
                                                    const float* __restrict__ bias, const float* xres, float* x, int b, int T, int D,
                                                    int i0, int n, int kq, int wave, int tiles_per_z) {
    // the A operand (this lane's context values) is the same for every column tile.
    // blockIdx.z splits the column tiles when there are too few row strips to fill the chip (phase A is then repeated per slice).
    constexpr int MAXC = 8;  // HV <= 128
    const int nch = (HV + 15) >> 4;
    float4 av4[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; c++) {
        const int kb = 16 * c + 4 * kq;
        const float* ar = avs + n * AS + kb;
        av4[c] = (c < nch && kb < HV) ? make_float4(ar[0], ar[1], ar[2], ar[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const int ct0 = blockIdx.z * tiles_per_z, ct1 = min(D >> 4, ct0 + tiles_per_z);
    float4 wc[MAXC], wn[MAXC];
    auto load_w = [&](float4* dst, int ct) {
        const float* wr = wout + (long long)(ct * 16 + n) * HV + 4 * kq;
#pragma unroll
        for (int c = 0; c < MAXC; c++)
            dst[c] = (c < nch && 16 * c + 4 * kq < HV) ? *reinterpret_cast<const float4*>(wr + 16 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    // Two register sets, no copies: a tile's weights, residual and bias are loaded one tile ahead, i.e. IN FRONT of the previous
    // tile's stores (vmcnt retires in issue order: a load issued behind those stores would make its wait drain them too, and the
    // tiles of a wave would run a store round trip apart).
    float xa[4], xb[4], ba = 0.f, bb = 0.f;
    auto load_x = [&](float* dst, float& bdst, int ct) {
        const int col = ct * 16 + n;
        bdst = bias[col];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int i = i0 + 4 * kq + e;
            dst[e] = i < T ? xres[((long long)b * T + i) * D + col] : 0.f;
        }
    };
    auto tile = [&](const float4* w, const float* xr, float bv, int ct) {
        const int col = ct * 16 + n;
        attn_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < MAXC; c++) {
            if (c < nch) {
                if (c & 1) {
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av4[c].x, w[c].x, acc1, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av4[c].y, w[c].y, acc1, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av4[c].z, w[c].z, acc1, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av4[c].w, w[c].w, acc1, 0, 0, 0);
                } else {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av4[c].x, w[c].x, acc0, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av4[c].y, w[c].y, acc0, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av4[c].z, w[c].z, acc0, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av4[c].w, w[c].w, acc0, 0, 0, 0);
                }
            }
        }
        float o[4];  // all four values first, then four stores with nothing loaded in between (else: a vmcnt(0) per store)
#pragma unroll
        for (int e = 0; e < 4; e++) o[e] = acc0[e] + acc1[e] + bv + xr[e];
        asm volatile("" : "+v"(o[0]), "+v"(o[1]), "+v"(o[2]), "+v"(o[3]));  // (keeps the sums out of the conditional store blocks)
        float* xp = x + ((long long)b * T + i0 + 4 * kq) * D + col;
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (i0 + 4 * kq + e < T) xp[(long long)e * D] = o[e];
    };
    int ct = ct0 + wave;
    if (ct < ct1) {
        load_w(wc, ct);
        load_x(xa, ba, ct);
    }
    while (ct < ct1) {
        if (ct + 4 < ct1) {
            load_w(wn, ct + 4);
            load_x(xb, bb, ct + 4);
        }
        tile(wc, xa, ba, ct);
        ct += 4;
        if (ct >= ct1) break;
        if (ct + 4 < ct1) {
            load_w(wc, ct + 4);
            load_x(xa, ba, ct + 4);
        }
        tile(wn, xb, bb, ct);
        ct += 4;
    }
}

}  // namespace k2hip
