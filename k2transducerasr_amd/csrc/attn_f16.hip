// The self-attention core of the offline Zipformer2 layer with half-precision operands, for gfx950 (level 4 of
// Engine::set_encoder_precision): the attention weights live in memory as f16, the q.k product and the weights . values product run on
// the f16 matrix pipe with float32 sums.  The softmax, the positional term and out_proj stay float32.
//
//   k_attn_scores_softmax_f16   qkp -> aw16 [H][B][T][Tp16] halves (Tp16 = T rounded up to 8: rows 16-byte aligned, pad columns +0)
//                               and head 0 again in float32, aw0 [B][T][Tp], for NonlinAttention's batched product
//   k_attn_av_out_f16           x += out_proj(concat_h(aw16_h . f16(v_h))) + bias
//
// Rounding is the plain conversion (nearest even, subnormals kept): |q| or |k| >= 65520 becomes an infinity and poisons its row, as
// level 1's operands do; nothing is clamped.
#include "attn_out_proj.h"
#include "kernels.h"

namespace k2hip {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int PH = 4;   // pos head dim
constexpr int R = 32;   // query rows per workgroup
constexpr int QH = 32;  // query / key head dim

__device__ __forceinline__ f16x8 round8(const float4& lo, const float4& hi) {   // nearest even
    return f16x8{(_Float16)lo.x, (_Float16)lo.y, (_Float16)lo.z, (_Float16)lo.w, (_Float16)hi.x, (_Float16)hi.y, (_Float16)hi.z, (_Float16)hi.w};
}
__device__ __forceinline__ f16x4 round4(float a, float b, float c, float d) {
    return f16x4{(_Float16)a, (_Float16)b, (_Float16)c, (_Float16)d};
}

// The decomposition of k_attn_scores_softmax<4> (attn.hip): one workgroup of 8 waves owns 32 query rows of a (head, stream) and all T
// keys, the 32 x T strip lives in LDS, the positional term (K = 4) seeds it from the float32 MFMA.  q.k is two v_mfma_f32_32x32x16_f16
// per key tile instead of sixteen 32x32x2 f32: MFMA m takes the float4 groups 2m and 2m + 1 of a lane's fragment of both operands, so
// lane half lh supplies k = 16 m + 4 lh + (0 .. 3) and 16 m + 8 + 4 lh + (0 .. 3) -- every k once, the same permutation on both sides.
// The query fragments are rounded once in front of the key loop, a key tile's as they arrive.  C/D layout: that of 32x32x2 f32.
__global__ __launch_bounds__(512, 4) void k_attn_scores_softmax_f16(const float* __restrict__ qkp, int ld, const float* __restrict__ pp,
                                                                    _Float16* __restrict__ aw16, float* __restrict__ aw0, int B, int T,
                                                                    int Tp, int Tp16, int H, int lds_stride, int koff0, int poff0) {
    extern __shared__ __attribute__((aligned(16))) float S[];  // [R][lds_stride]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int i0 = blockIdx.x * R, b = blockIdx.y, h = blockIdx.z;
    const float* base = qkp + (long long)b * T * ld;
    const int qoff = h * QH, koff = koff0 + h * QH, poff = poff0 + h * PH;
    const int ppld = H * PH;

    f16x8 fq[2];
    {
        const int row = i0 + li;
        float4 f[4];
#pragma unroll
        for (int g = 0; g < 4; g++) {
            f[g] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < T) f[g] = *reinterpret_cast<const float4*>(base + (long long)row * ld + qoff + 8 * g + 4 * lh);
        }
        fq[0] = round8(f[0], f[1]);
        fq[1] = round8(f[2], f[3]);
    }
    const int njt = (T + 31) / 32;
    float4 fkn[4];   // the next key tile's fragments, requested before this tile's strip reads and MFMAs
    auto load_keys = [&](int jt) {
        if (jt >= njt) return;                    // (wave-uniform)
        const int j = min(jt * 32 + li, T - 1);   // (a key past T reads key T-1: its column is never written)
#pragma unroll
        for (int g = 0; g < 4; g++) fkn[g] = *reinterpret_cast<const float4*>(base + (long long)j * ld + koff + 8 * g + 4 * lh);
    };
    load_keys(wave);

    // the positional term, as in k_attn_scores_softmax: P [32 x 4] . pos[window]^T on the float32 MFMA, scattered into the strip
    {
        const int nlo = T - 1 - min(i0 + R - 1, T - 1), nwin = (2 * T - 2 - i0) - nlo + 1;
        float2 fp = make_float2(0.f, 0.f);
        if (i0 + li < T) fp = *reinterpret_cast<const float2*>(base + (long long)(i0 + li) * ld + poff + 2 * lh);
        const float* pw = pp + h * PH + 2 * lh;
        auto load_window = [&](int t) {   // (always in bounds: the row is clamped)
            return *reinterpret_cast<const float2*>(pw + (long long)min(nlo + t * 32 + li, 2 * T - 2) * ppld);
        };
        float2 fw = load_window(wave);
        for (int t = wave; t * 32 < nwin; t += 8) {
            const float2 fwn = load_window(t + 8);
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fp.x, fw.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fp.y, fw.y, acc, 0, 0, 0);
            fw = fwn;
            const int j00 = nlo + t * 32 + i0 - (T - 1);
            const int j0 = j00 + li + 4 * lh;
            float* sp = S + 4 * lh * lds_stride + j0;
            if (j00 >= 0 && j00 + 62 < T) {       // (wave-uniform) an inner tile: every element has its key
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int ro = (r & 3) + 8 * (r >> 2);
                    sp[ro * lds_stride + ro] = acc[r];
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int ro = (r & 3) + 8 * (r >> 2);
                    if ((unsigned)(j0 + ro) < (unsigned)T) sp[ro * lds_stride + ro] = acc[r];
                }
            }
        }
    }
    __syncthreads();

    for (int jt = wave; jt < njt; jt += 8) {
        const int j = jt * 32 + li;
        const f16x8 fk0 = round8(fkn[0], fkn[1]), fk1 = round8(fkn[2], fkn[3]);
        load_keys(jt + 8);
        float* sp = S + 4 * lh * lds_stride + min(j, T - 1);   // (a key past T reads column T-1 and is never written)
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = sp[((r & 3) + 8 * (r >> 2)) * lds_stride];
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fq[0], fk0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fq[1], fk1, acc, 0, 0, 0);
        if (j < T) {
#pragma unroll
            for (int r = 0; r < 16; r++) sp[((r & 3) + 8 * (r >> 2)) * lds_stride] = acc[r];
        }
    }
    __syncthreads();

    // row softmax in float32: wave w (of 8) owns rows 4w .. 4w+3.  A lane's four consecutive weights leave as one 8-byte store of
    // halves; head 0's also as the float4 they were.
    _Float16* out = aw16 + (((long long)h * B + b) * T) * Tp16;
    float* out0 = h == 0 ? aw0 + (long long)b * T * Tp : nullptr;
    if (Tp <= 1024) {
        float4 v[4][4];
        const int nk = (Tp16 + 255) >> 8;  // 256-column chunks in use (wave-uniform)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            const float* srow = S + (wave * 4 + rr) * lds_stride;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int j4 = lane * 4 + 256 * k;
                v[rr][k] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
                if (k < nk && j4 < T) {  // (the strip is padded to a multiple of 4 columns; columns >= T are masked here)
                    const float4 t = *reinterpret_cast<const float4*>(srow + j4);
                    v[rr][k].x = t.x;
                    if (j4 + 1 < T) v[rr][k].y = t.y;
                    if (j4 + 2 < T) v[rr][k].z = t.z;
                    if (j4 + 3 < T) v[rr][k].w = t.w;
                }
            }
        }
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            const int i = i0 + wave * 4 + rr;
            if (i >= T) break;
            float mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < nk) mx = fmaxf(fmaxf(fmaxf(mx, v[rr][k].x), fmaxf(v[rr][k].y, v[rr][k].z)), v[rr][k].w);
            mx = wave_max_dpp(mx);
            float sum = 0.f;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (k >= nk) break;
                v[rr][k].x = __expf(v[rr][k].x - mx); v[rr][k].y = __expf(v[rr][k].y - mx);
                v[rr][k].z = __expf(v[rr][k].z - mx); v[rr][k].w = __expf(v[rr][k].w - mx);
                sum += (v[rr][k].x + v[rr][k].y) + (v[rr][k].z + v[rr][k].w);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
            const float inv = 1.0f / sum;
            _Float16* orow = out + (long long)i * Tp16;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int j4 = lane * 4 + 256 * k;
                if (k < nk && j4 < Tp16) {   // (exp(-inf) = 0: the pad columns are +0)
                    const float4 wv = make_float4(v[rr][k].x * inv, v[rr][k].y * inv, v[rr][k].z * inv, v[rr][k].w * inv);
                    *reinterpret_cast<f16x4*>(orow + j4) = round4(wv.x, wv.y, wv.z, wv.w);
                    if (out0 && j4 < Tp) *reinterpret_cast<float4*>(out0 + (long long)i * Tp + j4) = wv;
                }
            }
        }
        return;
    }
    for (int rr = 0; rr < 4; rr++) {
        const int rl = wave * 4 + rr, i = i0 + rl;
        if (i >= T) break;
        float* srow = S + rl * lds_stride;
        float mx = -INFINITY;
        for (int j = lane; j < T; j += 64) mx = fmaxf(mx, srow[j]);
        mx = wave_max_dpp(mx);
        float sum = 0.f;
        for (int j = lane; j < T; j += 64) {
            const float e = __expf(srow[j] - mx);
            srow[j] = e;
            sum += e;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        const float inv = 1.0f / sum;
        _Float16* orow = out + (long long)i * Tp16;
        for (int j4 = lane * 4; j4 < Tp16; j4 += 256) {
            float4 wv;
            wv.x = (j4 + 0 < T) ? srow[j4 + 0] * inv : 0.f;
            wv.y = (j4 + 1 < T) ? srow[j4 + 1] * inv : 0.f;
            wv.z = (j4 + 2 < T) ? srow[j4 + 2] * inv : 0.f;
            wv.w = (j4 + 3 < T) ? srow[j4 + 3] * inv : 0.f;
            *reinterpret_cast<f16x4*>(orow + j4) = round4(wv.x, wv.y, wv.z, wv.w);
            if (out0 && j4 < Tp) *reinterpret_cast<float4*>(out0 + (long long)i * Tp + j4) = wv;
        }
    }
}

// ---------------------------------------------------------------------------------------
// x += out_proj(concat_h(aw16_h . f16(v_h))) + bias: the offline form of k_attn_av_out (attn.hip) over f16 weights.  Grid, the 16-row
// strip per workgroup, the blockIdx.z column split and phases B / C (attn_out_proj.h) are that kernel's.
//
// Phase A on v_mfma_f32_16x16x32_f16, 64 keys per step.  A operand: lane (row n, kq) holds keys k0 + 32 j + 8 kq + (0 .. 7) of its
// aw16 row, ONE 16-byte load per MFMA (the float32 kernel: a float4 per 4 keys; this read bounds the launch, and it is halved).
// B operand: 8 consecutive keys of one value column, which is strided in the float32 [KL][HV] values -- so the workgroup stages the
// step's values: coalesced float4 rows of two neighbouring keys per thread, rounded, written transposed as half2 into LDS [HV][64 + 8]
// halves (rows 144 bytes apart: 16-byte aligned, and 16 lanes' ds_read_b128 spread over the banks).  Two buffers, one barrier per step:
// a step's buffer is written while the previous one is read, and the barrier that publishes it also retires every read of the buffer
// the next step overwrites.  Every wave's B operand is then one ds_read_b128.  The four waves walk the steps together, wave w keeps
// an accumulator pair for each of its heads w, w + 4, .. (at most 4).  Keys >= KL are staged as zeros (a pad weight times garbage
// must not reach a sum); weight columns >= Tp16 are not read.
// ---------------------------------------------------------------------------------------
constexpr int VS = 64 + 8;    // halves per staged value column
constexpr int MAXHW = 4;      // heads per wave

__global__ __launch_bounds__(256) void k_attn_av_out_f16(const _Float16* __restrict__ aw16, const float* __restrict__ v,
                                                         const float* __restrict__ wout, const float* __restrict__ bias,
                                                         float* __restrict__ x, int B, int T, int KL, int Tp16, int Tk, int H, int vh,
                                                         int D, int tiles_per_z) {
    extern __shared__ __attribute__((aligned(16))) _Float16 vst[];   // [2][HV][VS] halves | avs [16][HV + 1] floats
    const int HV = H * vh, AS = HV + 1, h4 = HV >> 2;
    float* avs = reinterpret_cast<float*>(vst + 2 * HV * VS);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, i0 = blockIdx.x * 16;
    const int n = lane & 15, kq = lane >> 4;
    v += (long long)b * KL * HV;

    // staging: item e = (key pair kp, column group c4), 32 h4 <= 1024 items, four per thread
    const int items = 32 * h4;
    float4 sv[4][2];
    auto stage_load = [&](int k0) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int e = tid + 256 * q;
            sv[q][0] = sv[q][1] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (e < items) {
                const int kp = e / h4, c = (e - kp * h4) * 4, k = k0 + 2 * kp;
                if (k < KL) sv[q][0] = *reinterpret_cast<const float4*>(v + (long long)k * HV + c);
                if (k + 1 < KL) sv[q][1] = *reinterpret_cast<const float4*>(v + (long long)(k + 1) * HV + c);
            }
        }
    };
    auto stage_store = [&](_Float16* buf) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int e = tid + 256 * q;
            if (e < items) {
                const int kp = e / h4, c = (e - kp * h4) * 4;
                _Float16* d = buf + c * VS + 2 * kp;
                *reinterpret_cast<f16x2*>(d) = f16x2{(_Float16)sv[q][0].x, (_Float16)sv[q][1].x};
                *reinterpret_cast<f16x2*>(d + VS) = f16x2{(_Float16)sv[q][0].y, (_Float16)sv[q][1].y};
                *reinterpret_cast<f16x2*>(d + 2 * VS) = f16x2{(_Float16)sv[q][0].z, (_Float16)sv[q][1].z};
                *reinterpret_cast<f16x2*>(d + 3 * VS) = f16x2{(_Float16)sv[q][0].w, (_Float16)sv[q][1].w};
            }
        }
    };

    const int row_a = min(i0 + n, T - 1);  // clamped rows are computed and dropped
    const bool ncol = n < vh;
    const int nh = wave < H ? (H - wave + 3) >> 2 : 0;   // this wave's heads: wave, wave + 4, ..
    const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    f16x8 a[MAXHW][2], an[MAXHW][2];
    auto load_a = [&](f16x8 (*ad)[2], int k0) {
#pragma unroll
        for (int hh = 0; hh < MAXHW; hh++) {
            if (hh >= nh) break;
            const _Float16* arow = aw16 + (((long long)(wave + 4 * hh) * B + b) * T + row_a) * Tp16;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int kb = k0 + 32 * j + 8 * kq;
                ad[hh][j] = kb < Tp16 ? *reinterpret_cast<const f16x8*>(arow + kb) : zero8;
            }
        }
    };
    f32x4 acc[MAXHW][2];
#pragma unroll
    for (int hh = 0; hh < MAXHW; hh++) acc[hh][0] = acc[hh][1] = f32x4{0.f, 0.f, 0.f, 0.f};

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
        const _Float16* buf = vst + (s & 1) * HV * VS;
#pragma unroll
        for (int hh = 0; hh < MAXHW; hh++) {
            if (hh >= nh) break;
            const _Float16* bp = buf + ((wave + 4 * hh) * vh + (ncol ? n : 0)) * VS + 8 * kq;
            const f16x8 b0 = *reinterpret_cast<const f16x8*>(bp), b1 = *reinterpret_cast<const f16x8*>(bp + 32);
            acc[hh][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[hh][0], b0, acc[hh][0], 0, 0, 0);
            acc[hh][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[hh][1], b1, acc[hh][1], 0, 0, 0);
        }
        if (more) {
            stage_store(vst + ((s + 1) & 1) * HV * VS);
#pragma unroll
            for (int hh = 0; hh < MAXHW; hh++) {
                a[hh][0] = an[hh][0];
                a[hh][1] = an[hh][1];
            }
        }
        __syncthreads();
    }
    // ---- phase B: the 16 x HV context rows through LDS (C layout: col = lane & 15, row = 4 * (lane >> 4) + e)
#pragma unroll
    for (int hh = 0; hh < MAXHW; hh++) {
        if (hh >= nh || !ncol) break;
#pragma unroll
        for (int e = 0; e < 4; e++) avs[(4 * kq + e) * AS + (wave + 4 * hh) * vh + n] = acc[hh][0][e] + acc[hh][1][e];
    }
    __syncthreads();
    // ---- phase C: out_proj + bias + residual in float32
    attn_out_proj_tiles(avs, AS, HV, wout, bias, x, x, b, T, D, i0, n, kq, wave, tiles_per_z);
}

}  // namespace

void attn_scores_softmax_f16(const Ctx& ctx, const float* qkp, int ld, const float* pp, uint16_t* aw16, float* aw0, int B, int T, int Tp,
                             int H, int koff0, int poff0) {
    K2_REQUIRE(T >= 1 && Tp == ((T + 3) & ~3), "attn f16: Tp=%d must be T=%d rounded up to 4", Tp, T);
    if (koff0 < 0) koff0 = H * QH;       // Zipformer2 row: q [H*32] | k [H*32] | p [H*4]
    if (poff0 < 0) poff0 = 2 * H * QH;
    K2_REQUIRE(koff0 % 4 == 0 && poff0 % 4 == 0 && ld % 4 == 0, "attn f16: operand offsets must be multiples of 4 floats");
    const int lds_stride = Tp + 4;
    const size_t lds = sizeof(float) * R * lds_stride;
    K2_REQUIRE(lds <= 160 * 1024, "attn f16: %d frames do not fit the score strip", T);
    ctx.add_flops(0.0, 2.0 * (QH + PH) * (double)T * T * B * H, 0);
    if (ctx.dry) return;
    static LdsAttrOnce lds_attr;
    lds_attr.ensure(k_attn_scores_softmax_f16, 160 * 1024);
    hipLaunchKernelGGL(k_attn_scores_softmax_f16, dim3(cdiv(T, R), B, H), dim3(512), lds, ctx.stream, qkp, ld, pp,
                       reinterpret_cast<_Float16*>(aw16), aw0, B, T, Tp, attn_f16_tp16(T), H, lds_stride, koff0, poff0);
    K2_HIP(hipGetLastError());
    if (ctx.f16) ctx.f16->launches++;
}

bool attn_av_out_f16(const Ctx& ctx, const uint16_t* aw16, const float* v, const float* wout, const float* bias, float* x, int B, int T,
                     int KL, int Tp16, int H, int vh, int D) {
    const int HV = H * vh, Tk = (KL + 63) & ~63;
    if (tunables().no_fused_av || T < 1 || KL < 1 || H < 1 || H > 4 * MAXHW || vh < 1 || vh > 16 || HV % 4 != 0 || HV > 128 || D % 16 != 0 ||
        Tp16 % 8 != 0 || Tp16 < KL)
        return false;
    ctx.add_flops(0.0, 2.0 * B * (double)T * HV * (KL + D), 0);
    if (ctx.dry) return true;
    // few row strips (short sequences): split out_proj's column tiles over blockIdx.z, as attn_av_out does
    const int strips = cdiv(T, 16) * B, ntile = D / 16;
    int cs = std::max(1, std::min(4, 512 / std::max(1, strips)));
    cs = std::min(cs, ntile);
    const int tiles_per_z = cdiv(ntile, cs);
    cs = cdiv(ntile, tiles_per_z);
    const size_t lds = sizeof(uint16_t) * 2 * HV * VS + sizeof(float) * 16 * (HV + 1);   // <= 36 KiB + 8 KiB
    hipLaunchKernelGGL(k_attn_av_out_f16, dim3(cdiv(T, 16), B, cs), dim3(256), lds, ctx.stream, reinterpret_cast<const _Float16*>(aw16), v, wout,
                       bias, x, B, T, KL, Tp16, Tk, H, vh, D, tiles_per_z);
    K2_HIP(hipGetLastError());
    if (ctx.f16) ctx.f16->launches++;
    return true;
}

}  // namespace k2hip
