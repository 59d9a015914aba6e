// The attention core of the offline Conformer layer with half-precision operands, for gfx950 (level 2 of
// Engine::set_conformer_precision): both score products and the weights . values product run on the f16 matrix pipe with float32 sums,
// the attention weights live in memory as f16.  The softmax stays float32; in_proj in front and out_proj behind are linear() launches.
//
//   k_conformer_scores_softmax_f16   q (+ u, v), k, projected table -> aw16 [B*H][T][Tp16] halves (Tp16 = T rounded up to 8: rows
//                                    16-byte aligned, pad columns +0)
//   k_conformer_av_f16               ctx[b, :, h] = aw16[b, h] . f16(v[b, :, h]) into the [M, D] float32 context
//
// Rounding is the plain conversion (nearest even, subnormals kept): an operand beyond the f16 range becomes an infinity and poisons
// its row, as level 1's operands do; nothing is clamped.
#include "kernels.h"

namespace k2hip {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

namespace {

__device__ __forceinline__ f16x8 round8(const float4& lo, const float4& hi) {   // nearest even
    return f16x8{(_Float16)lo.x, (_Float16)lo.y, (_Float16)lo.z, (_Float16)lo.w, (_Float16)hi.x, (_Float16)hi.y, (_Float16)hi.z, (_Float16)hi.w};
}
__device__ __forceinline__ f16x4 round4(const float4& a) { return f16x4{(_Float16)a.x, (_Float16)a.y, (_Float16)a.z, (_Float16)a.w}; }

// ---------------------------------------------------------------------------------------
// Scores + softmax.  The decomposition is k_conformer_scores_softmax16s's (conformer.hip): one workgroup of four waves owns a strip of
// 16 query rows of a (stream, head) and all T keys, the float32 strip is the only LDS (three workgroups per CU at T = 750), a wave takes
// a run of 16-key tiles, the positional tile G = (q+v) . p[base ..]^T is WRITTEN skewed into the strip and the content tile added on top,
// keys and table rows are requested two tiles ahead into the register set just consumed.
//
// What changes is the arithmetic of a tile: the head's dk = 16 NG columns are cut into NG / 2 groups of 32 and, NG odd, one last group of
// 16.  A group of 32 is ONE v_mfma_f32_16x16x32_f16: lane (row / key li, quarter kq) supplies columns 32 m + 8 kq + (0 .. 7) of its row,
// two adjacent float4 loads rounded to eight halves.  The odd group of 16 (dk = 16, 48) is one v_mfma_f32_16x16x16_f16 over columns
// 32 (NG / 2) + 4 kq + (0 .. 3) -- no zero-filled upper half, no wasted pass of the pipe.  dk = 64: 2 + 2 MFMAs per key tile against
// 16 + 16 of 16x16x4 f32.  The C layout of all three instructions is the same (column = lane & 15, row = 4 (lane >> 4) + e), so the
// scatter is the float32 kernel's.  The (q scaling + u) and (q scaling + v) fragments are formed in float32 as there and rounded ONCE in
// front of the tile loop; key and table fragments are rounded as they arrive.
//
// Then the float32 row softmax over the strip, and a lane's four consecutive weights leave as one 8-byte store of halves.
// ---------------------------------------------------------------------------------------
template <int NG>
__global__ __launch_bounds__(256) void k_conformer_scores_softmax_f16(const float* __restrict__ qu, const float* __restrict__ qv,
                                                                      const float* __restrict__ kmat, int ldk, const float* __restrict__ pp,
                                                                      _Float16* __restrict__ aw16, int B, int H, int T, int Tp16, int D,
                                                                      int lds_stride, int ldq, const float* __restrict__ bu,
                                                                      const float* __restrict__ bv, float scaling) {
    constexpr int DK = 16 * NG, NP2 = NG / 2, NW = 4;
    constexpr bool ODD = (NG & 1) != 0;
    extern __shared__ __attribute__((aligned(16))) float csm[];
    float* S = csm;                                   // [16][lds_stride] | 64 dump slots
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int i0 = blockIdx.x * 16, b = blockIdx.y, h = blockIdx.z, NP = 2 * T - 1;
    const long long rowbase = (long long)b * T;
    const int dump = 16 * lds_stride + lane;
    // float4 g of a lane's fragment: groups of 32 hold the pairs (2 m, 2 m + 1), the odd group of 16 is the last one
    auto frag_off = [&](int g) { return g < 2 * NP2 ? 32 * (g >> 1) + 8 * kq + 4 * (g & 1) : 32 * NP2 + 4 * kq; };

    f16x8 hu[NP2 + 1], hv[NP2 + 1];   // (one spare element: NP2 may be 0)
    f16x4 hu4 = {0, 0, 0, 0}, hv4 = {0, 0, 0, 0};
    {
        const int row = i0 + li;
        float4 fu[NG], fv[NG];
#pragma unroll
        for (int g = 0; g < NG; g++) {
            fu[g] = fv[g] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < T) {
                const int col = h * DK + frag_off(g);
                if (bu) {   // q * scaling + pos_bias_u / pos_bias_v in float32, as k_conformer_qprep forms them
                    float4 q = *reinterpret_cast<const float4*>(qu + (rowbase + row) * ldq + col);
                    const float4 u = *reinterpret_cast<const float4*>(bu + col);
                    const float4 v = *reinterpret_cast<const float4*>(bv + col);
                    q.x *= scaling; q.y *= scaling; q.z *= scaling; q.w *= scaling;
                    fu[g] = make_float4(q.x + u.x, q.y + u.y, q.z + u.z, q.w + u.w);
                    fv[g] = make_float4(q.x + v.x, q.y + v.y, q.z + v.z, q.w + v.w);
                } else {
                    fu[g] = *reinterpret_cast<const float4*>(qu + (rowbase + row) * D + col);
                    fv[g] = *reinterpret_cast<const float4*>(qv + (rowbase + row) * D + col);
                }
            }
        }
#pragma unroll
        for (int m = 0; m < NP2; m++) {
            hu[m] = round8(fu[2 * m], fu[2 * m + 1]);
            hv[m] = round8(fv[2 * m], fv[2 * m + 1]);
        }
        if (ODD) {
            hu4 = round4(fu[NG - 1]);
            hv4 = round4(fv[NG - 1]);
        }
    }
    const int njt = (T + 15) / 16;
    auto load_k = [&](int jt, float4* k_) {
        const int jr = min(jt * 16 + li, T - 1);
#pragma unroll
        for (int g = 0; g < NG; g++) k_[g] = *reinterpret_cast<const float4*>(kmat + (rowbase + jr) * ldk + h * DK + frag_off(g));
    };
    auto load_p = [&](int nrow, float4* p_) {   // table row nrow (out-of-table rows only meet masked entries)
        const int nr = min(max(nrow, 0), NP - 1);
#pragma unroll
        for (int g = 0; g < NG; g++) p_[g] = *reinterpret_cast<const float4*>(pp + (long long)nr * D + h * DK + frag_off(g));
    };
    auto mma = [&](const f16x8* a8, const f16x4& a4, const float4* bq, f32x4 acc) {
#pragma unroll
        for (int m = 0; m < NP2; m++) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a8[m], round8(bq[2 * m], bq[2 * m + 1]), acc, 0, 0, 0);
        if (ODD) acc = __builtin_amdgcn_mfma_f32_16x16x16f16(a4, round4(bq[NG - 1]), acc, 0, 0, 0);
        return acc;
    };
    const int tpw = (njt + NW - 1) / NW, jt_beg = wave * tpw, jt_end = min(njt, jt_beg + tpw);
    if (jt_beg < jt_end) {
        const int col_lo = 16 * jt_beg, col_hi = min(16 * jt_end, T);   // the strip columns this wave owns
        // positional tile m = jt_beg .. jt_end: table rows base0 + 16 (m - jt_beg) + li
        const int base0 = T - 1 - i0 - 15 + jt_beg * 16;
        auto put_pos = [&](const f32x4& g, int m) {   // element (rl, li) belongs to column 16 (m - 1) + 1 + li + rl of row rl
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int rl = 4 * kq + e, col = 16 * (m - 1) + 1 + li + rl;
                S[(col >= col_lo && col < col_hi) ? rl * lds_stride + col : dump] = g[e];
            }
        };
        auto step = [&](int jt, float4* K_, float4* P_) {   // key tile jt (operands in K_) and positional tile jt + 1 (in P_)
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            const f32x4 acc = mma(hu, hu4, K_, zero), g = mma(hv, hv4, P_, zero);
            if (jt + 2 < jt_end) {   // (wave-uniform) two tiles ahead, into the registers just consumed
                load_k(jt + 2, K_);
                load_p(base0 + (jt + 3 - jt_beg) * 16 + li, P_);
            }
            put_pos(g, jt + 1);
            const int j = jt * 16 + li;
            int idx[4];
            float sv[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                idx[e] = j < T ? (4 * kq + e) * lds_stride + j : dump;
                sv[e] = S[idx[e]];
            }
#pragma unroll
            for (int e = 0; e < 4; e++) S[idx[e]] = sv[e] + acc[e];
        };
        float4 k0[NG], k1[NG], p0[NG], p1[NG];
        load_p(base0 + li, p1);
        load_k(jt_beg, k0);
        load_p(base0 + 16 + li, p0);
        put_pos(mma(hv, hv4, p1, f32x4{0.f, 0.f, 0.f, 0.f}), jt_beg);
        if (jt_beg + 1 < jt_end) {
            load_k(jt_beg + 1, k1);
            load_p(base0 + 32 + li, p1);
        }
        for (int jt = jt_beg; jt < jt_end; jt += 2) {
            step(jt, k0, p0);
            if (jt + 1 < jt_end) step(jt + 1, k1, p1);
        }
    }
    __syncthreads();
    // row softmax in float32: wave w owns rows 4 w .. 4 w + 3; a row's scores are read ONCE into registers (Tp16 <= 64 * 20), four
    // consecutive columns per lane and instruction.  Rows are lds_stride = Tp16 + 4 floats, 16-byte aligned.
    _Float16* out = aw16 + (((long long)b * H + h) * T) * Tp16;
    const int nu = (Tp16 + 255) >> 8;   // groups of 256 columns (<= 5)
    for (int rr = 0; rr < 16 / NW; rr++) {
        const int rl = wave * (16 / NW) + rr, i = i0 + rl;
        if (i >= T) break;
        const float* srow = S + rl * lds_stride;
        float4 v[5];
        float mx = -INFINITY;
#pragma unroll
        for (int u = 0; u < 5; u++) {
            if (u < nu) {
                const int jj = 4 * lane + 256 * u;
                const float4 x = *reinterpret_cast<const float4*>(srow + min(jj, lds_stride - 4));
                v[u].x = jj < T ? x.x : -INFINITY;
                v[u].y = jj + 1 < T ? x.y : -INFINITY;
                v[u].z = jj + 2 < T ? x.z : -INFINITY;
                v[u].w = jj + 3 < T ? x.w : -INFINITY;
                mx = fmaxf(fmaxf(mx, fmaxf(v[u].x, v[u].y)), fmaxf(v[u].z, v[u].w));
            }
        }
        mx = wave_max_dpp(mx);
        float sum = 0.f;
#pragma unroll
        for (int u = 0; u < 5; u++) {
            if (u < nu) {   // exp(-inf) = 0 for the masked columns
                v[u].x = __expf(v[u].x - mx);
                v[u].y = __expf(v[u].y - mx);
                v[u].z = __expf(v[u].z - mx);
                v[u].w = __expf(v[u].w - mx);
                sum += (v[u].x + v[u].y) + (v[u].z + v[u].w);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        const float inv = 1.0f / sum;
        _Float16* orow = out + (long long)i * Tp16;
#pragma unroll
        for (int u = 0; u < 5; u++) {
            const int jj = 4 * lane + 256 * u;
            if (u < nu && jj < Tp16)   // (Tp16 % 8 == 0: whole groups of four; the pad columns [T, Tp16) get +0)
                *reinterpret_cast<f16x4*>(orow + jj) = round4(make_float4(v[u].x * inv, v[u].y * inv, v[u].z * inv, v[u].w * inv));
        }
    }
}

// ---------------------------------------------------------------------------------------
// ctx[b, i, h dk + n] = sum_j aw16[b H + h][i][j] f16(v[b T + j, h dk + n]) on v_mfma_f32_16x16x32_f16, 64 keys per step.
//
// The split: a workgroup of four waves owns 64 query rows of ONE (stream, head) -- wave w the 16-row strip i0 + 16 w -- and all dk
// value columns, so a step's values are staged once for 64 rows (T = 750, dk = 64, 64 pairs: 12 x 64 = 768 workgroups, three per CU
// and all resident; a pair's values, 192 KB, are re-read twelve times from the L2, the weights, 72 MB, once from memory).
// A operand: lane (row n, quarter kq) holds keys k0 + 32 j + 8 kq + (0 .. 7) of its aw16 row, ONE 16-byte load per MFMA.
// B operand: 8 consecutive keys of one value column, which is strided in the float32 [T][ldv] values -- the workgroup stages the step
// as k_attn_av_out_f16 (attn_f16.hip) does: coalesced float4 rows of two neighbouring keys per thread, rounded, written transposed as
// half2 into LDS [dk][64 + 8] halves (rows 144 bytes apart: 16-byte aligned, and 16 lanes' ds_read_b128 spread over the banks).  Two
// buffers, one barrier per step: a step's buffer is written while the previous one is read, and the barrier that publishes it also
// retires every read of the buffer the next step overwrites.  Every B operand is then one ds_read_b128, shared by the four waves.
// Keys >= T are staged as zeros (a pad weight times garbage must not reach a sum); weight columns >= Tp16 are not read.
// The C tile (column = lane & 15, row = 4 (lane >> 4) + e) goes straight to the context: 64 contiguous bytes per row and instruction.
// ---------------------------------------------------------------------------------------
constexpr int VS = 64 + 8;    // halves per staged value column

template <int NT>             // dk = 16 NT
__global__ __launch_bounds__(256) void k_conformer_av_f16(const _Float16* __restrict__ aw16, const float* __restrict__ v, int ldv,
                                                          float* __restrict__ out, int ldc, int H, int T, int Tp16) {
    constexpr int DK = 16 * NT, C4 = DK / 4, ITEMS = 32 * C4, NQ = (ITEMS + 255) / 256;   // staging items: (key pair, column group)
    __shared__ __attribute__((aligned(16))) _Float16 vst[2 * DK * VS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, kq = lane >> 4;
    const int z = blockIdx.y, b = z / H, h = z - b * H;
    const int i0 = blockIdx.x * 64 + 16 * wave;
    const bool live = i0 < T;                        // (wave-uniform) a strip past the last row only helps staging
    v += (long long)b * T * ldv + h * DK;
    const int Tk = (T + 63) & ~63;

    float4 sv[NQ][2];
    auto stage_load = [&](int k0) {
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const int e = tid + 256 * q;
            sv[q][0] = sv[q][1] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (e < ITEMS) {
                const int kp = e / C4, c = (e - kp * C4) * 4, k = k0 + 2 * kp;
                if (k < T) sv[q][0] = *reinterpret_cast<const float4*>(v + (long long)k * ldv + c);
                if (k + 1 < T) sv[q][1] = *reinterpret_cast<const float4*>(v + (long long)(k + 1) * ldv + c);
            }
        }
    };
    auto stage_store = [&](_Float16* buf) {
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const int e = tid + 256 * q;
            if (e < ITEMS) {
                const int kp = e / C4, c = (e - kp * C4) * 4;
                _Float16* d = buf + c * VS + 2 * kp;
                *reinterpret_cast<f16x2*>(d) = f16x2{(_Float16)sv[q][0].x, (_Float16)sv[q][1].x};
                *reinterpret_cast<f16x2*>(d + VS) = f16x2{(_Float16)sv[q][0].y, (_Float16)sv[q][1].y};
                *reinterpret_cast<f16x2*>(d + 2 * VS) = f16x2{(_Float16)sv[q][0].z, (_Float16)sv[q][1].z};
                *reinterpret_cast<f16x2*>(d + 3 * VS) = f16x2{(_Float16)sv[q][0].w, (_Float16)sv[q][1].w};
            }
        }
    };

    const _Float16* arow = aw16 + ((long long)z * T + min(i0 + n, T - 1)) * Tp16;   // clamped rows are computed and dropped
    const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    f16x8 a[2] = {zero8, zero8}, an[2] = {zero8, zero8};
    auto load_a = [&](f16x8* ad, int k0) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int kb = k0 + 32 * j + 8 * kq;
            ad[j] = live && kb < Tp16 ? *reinterpret_cast<const f16x8*>(arow + kb) : zero8;
        }
    };
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    load_a(a, 0);
    stage_load(0);
    stage_store(vst);
    __syncthreads();
    for (int k0 = 0, s = 0; k0 < Tk; k0 += 64, s++) {
        const bool more = k0 + 64 < Tk;
        if (more) {   // in flight under this step's MFMAs
            load_a(an, k0 + 64);
            stage_load(k0 + 64);
        }
        if (live) {
            const _Float16* bp = vst + (s & 1) * DK * VS + n * VS + 8 * kq;
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const f16x8 b0 = *reinterpret_cast<const f16x8*>(bp + 16 * t * VS), b1 = *reinterpret_cast<const f16x8*>(bp + 16 * t * VS + 32);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[0], b0, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[1], b1, acc[t], 0, 0, 0);
            }
        }
        if (more) {
            stage_store(vst + ((s + 1) & 1) * DK * VS);
            a[0] = an[0];
            a[1] = an[1];
        }
        __syncthreads();
    }
    if (!live) return;
    float* orow = out + (long long)b * T * ldc + h * DK + n;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int i = i0 + 4 * kq + e;
        if (i < T) {
#pragma unroll
            for (int t = 0; t < NT; t++) orow[(long long)i * ldc + 16 * t] = acc[t][e];
        }
    }
}

template <int NG>
void scores_launch(const Ctx& ctx, const float* qu, const float* qv, const float* kmat, int ldk, const float* pp, _Float16* aw16, int B, int H,
                   int T, int Tp16, int D, int ldq, const float* bu, const float* bv, float scaling) {
    const int lds_stride = Tp16 + 4;
    const size_t lds = sizeof(float) * ((size_t)16 * lds_stride + 64);   // + a dump slot per lane (masked positional writes)
    static LdsAttrOnce lds_attr;
    lds_attr.ensure((k_conformer_scores_softmax_f16<NG>), 96 * 1024);
    hipLaunchKernelGGL((k_conformer_scores_softmax_f16<NG>), dim3(cdiv(T, 16), B, H), dim3(256), lds, ctx.stream, qu, qv, kmat, ldk, pp, aw16, B, H,
                       T, Tp16, D, lds_stride, ldq, bu, bv, scaling);
}

}  // namespace

bool conformer_scores_softmax_f16(const Ctx& ctx, const float* qu, const float* qv, const float* kmat, int ldk, const float* pp, uint16_t* aw16,
                                  int B, int H, int T, int D, int ldq, const float* bias_u, const float* bias_v, float scaling) {
    if (B < 1 || H < 1 || T < 1 || D < 1 || D % H != 0 || B > 65535 || H > 65535) return false;
    const int dk = D / H, Tp16 = attn_f16_tp16(T);
    if (dk % 16 != 0 || dk > 64 || ldk % 4 != 0 || ldk < D) return false;
    if (bias_u && (ldq % 4 != 0 || ldq < D || !bias_v)) return false;
    if (Tp16 > 64 * 20) return false;   // a row's scores in a wave's registers: 5 groups of 256 columns (the strip then takes 82 KB)
    ctx.add_flops(0.0, 2.0 * dk * (double)T * (3.0 * T) * B * H, 0);
    if (ctx.dry) return true;
    _Float16* aw = reinterpret_cast<_Float16*>(aw16);
    switch (dk / 16) {
        case 1: scores_launch<1>(ctx, qu, qv, kmat, ldk, pp, aw, B, H, T, Tp16, D, ldq, bias_u, bias_v, scaling); break;
        case 2: scores_launch<2>(ctx, qu, qv, kmat, ldk, pp, aw, B, H, T, Tp16, D, ldq, bias_u, bias_v, scaling); break;
        case 3: scores_launch<3>(ctx, qu, qv, kmat, ldk, pp, aw, B, H, T, Tp16, D, ldq, bias_u, bias_v, scaling); break;
        default: scores_launch<4>(ctx, qu, qv, kmat, ldk, pp, aw, B, H, T, Tp16, D, ldq, bias_u, bias_v, scaling); break;
    }
    K2_HIP(hipGetLastError());
    if (ctx.f16) ctx.f16->launches++;
    return true;
}

bool conformer_av_f16(const Ctx& ctx, const uint16_t* aw16, const float* v, int ldv, float* out, int ldc, int B, int H, int T, int dk) {
    if (B < 1 || H < 1 || T < 1 || dk < 16 || dk > 64 || dk % 16 != 0 || ldv % 4 != 0 || ldv < H * dk || ldc < H * dk) return false;
    if ((long long)B * H > 65535) return false;
    ctx.add_flops(0.0, 2.0 * B * H * (double)T * T * dk, 0);
    if (ctx.dry) return true;
    const _Float16* aw = reinterpret_cast<const _Float16*>(aw16);
    const int Tp16 = attn_f16_tp16(T);
    const dim3 grid(cdiv(T, 64), B * H);
    switch (dk / 16) {
        case 1: hipLaunchKernelGGL(k_conformer_av_f16<1>, grid, dim3(256), 0, ctx.stream, aw, v, ldv, out, ldc, H, T, Tp16); break;
        case 2: hipLaunchKernelGGL(k_conformer_av_f16<2>, grid, dim3(256), 0, ctx.stream, aw, v, ldv, out, ldc, H, T, Tp16); break;
        case 3: hipLaunchKernelGGL(k_conformer_av_f16<3>, grid, dim3(256), 0, ctx.stream, aw, v, ldv, out, ldc, H, T, Tp16); break;
        default: hipLaunchKernelGGL(k_conformer_av_f16<4>, grid, dim3(256), 0, ctx.stream, aw, v, ldv, out, ldc, H, T, Tp16); break;
    }
    K2_HIP(hipGetLastError());
    if (ctx.f16) ctx.f16->launches++;
    return true;
}

}  // namespace k2hip
