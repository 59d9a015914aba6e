// Voice activity detection on gfx950: the detector of vad_ref.h (the normative text) over the log-mel features of B streams in one
// batched call, each stream with its own frame count and its own carried state.  Three launches, no atomics, nothing shared between
// workgroups, control flow decided by the bounds alone:
//
//   k_vad_score    one wave per frame (4 per workgroup, striding): lane l reads x[t][lo + l], x[t][lo + 64 + l], ... -- consecutive
//                  lanes, consecutive floats, so a row is one or two coalesced reads -- and the six butterfly steps of vad_ref_score
//                  give every lane the sum in the reference's order.
//   k_vad_floor    one workgroup per (stream, tile of kVadTile frames): m over [tile - W + 1, tile end) is staged in LDS (at W = 1024
//                  that is 1279 floats, 5116 bytes) from the two pieces of one logical array -- the carried history in front of frame
//                  t0, the smoothed scores of this call behind it --, then one thread per frame walks its window, u ascending.
//                  Neighbouring threads read neighbouring LDS words in every step: no bank conflicts.
//   k_vad_segment  one wave per stream: 64 decisions per step through a ballot, the machine advanced run by run (a run of equal
//                  decisions holds at most one event: the silence timeout or the forced cut), the forced cut's argmin as a wave-wide
//                  reduction over m with wave_best.h's order (score -m: the smallest m, the LOWER frame on ties).  It also writes the
//                  stream's new carried block.
//
// Where the reference rounds twice the kernels say so (__fmul_rn / __fadd_rn / __fsub_rn) -- and this file is compiled with
// -ffp-contract=off (the Makefile's rule for vad.o): hipcc contracts a * b + c by default, and in this toolchain's headers the _rn
// functions are the plain operators, which contract like any other (the bit comparison of n in tests/test_vad_gpu.py shows it).
#include <algorithm>
#include <cstdint>

#include "kernels.h"
#include "wave_best.h"

namespace k2hip {
namespace {

// s of call-relative frame j (j < 0: the carried four, or s_0 at the start of a stream)
__device__ __forceinline__ float vad_s_at(const VadRow& r, const float* __restrict__ shist, const float* __restrict__ s_new, int j) {
    return j >= 0 ? s_new[j] : r.t0 == 0 ? s_new[0] : shist[4 + j];
}
// m of call-relative frame j >= 0 from the scores
__device__ __forceinline__ float vad_smooth(const VadRow& r, const float* __restrict__ shist, const float* __restrict__ s_new, int j) {
    float a = __fadd_rn(vad_s_at(r, shist, s_new, j - 4), vad_s_at(r, shist, s_new, j - 3));
    a = __fadd_rn(a, vad_s_at(r, shist, s_new, j - 2));
    a = __fadd_rn(a, vad_s_at(r, shist, s_new, j - 1));
    a = __fadd_rn(a, s_new[j]);
    return __fmul_rn(a, 0.2f);
}

__global__ __launch_bounds__(256) void k_vad_score(const VadRow* __restrict__ rows, float* __restrict__ s_all) {
    const VadRow r = rows[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* __restrict__ s_new = s_all + r.work_off;
    for (int i = blockIdx.x * 4 + wave; i < r.n; i += gridDim.x * 4) {   // (the same for the whole wave)
        const float* __restrict__ row = r.feats + (long long)i * r.stride;
        float acc = 0.0f;
        for (int j = r.lo + lane; j < r.hi; j += 64) acc = __fadd_rn(acc, row[j]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, off));
        if (lane == 0) s_new[i] = __fmul_rn(acc, r.inv_band);
    }
}

__global__ __launch_bounds__(kVadTile) void k_vad_floor(const VadRow* __restrict__ rows, const float* __restrict__ st_in, const float* __restrict__ s_all,
                                                        float* __restrict__ m_all, float* __restrict__ n_all, unsigned char* __restrict__ d_all) {
    __shared__ float ms[kVadMaxW - 1 + kVadTile];
    const VadRow r = rows[blockIdx.y];
    const int base = blockIdx.x * kVadTile;
    if (base >= r.n) return;   // (the whole workgroup)
    const int tid = threadIdx.x, W = r.W;
    const int cnt = r.n - base < kVadTile ? r.n - base : kVadTile;
    const float* __restrict__ hist = st_in + r.state_off;
    const float* __restrict__ shist = hist + (W - 1);
    const float* __restrict__ s_new = s_all + r.work_off;
    float* __restrict__ m_new = m_all + r.work_off;
    for (int idx = tid; idx < W - 1 + cnt; idx += kVadTile) {
        const int j = base - (W - 1) + idx;   // call-relative frame
        float v = 0.0f;
        if (j >= 0) {
            v = vad_smooth(r, shist, s_new, j);
            if (j >= base) m_new[j] = v;
        } else if (-j <= r.n_hist) {
            v = hist[W - 1 + j];
        }
        ms[idx] = v;
    }
    __syncthreads();
    if (tid >= cnt) return;
    const int i = base + tid, t = r.t0 + i;
    const float* __restrict__ mine = ms + (W - 1) + tid;   // mine[-k] = m_{t - k}
    int k = t < W - 1 ? t : W - 1;
    float nf = __fadd_rn(mine[-k], __fmul_rn(r.rise, (float)k));
    for (k = k - 1; k >= 0; k--) {
        const float v = __fadd_rn(mine[-k], __fmul_rn(r.rise, (float)k));
        if (v < nf) nf = v;
    }
    const float m = mine[0];
    n_all[r.work_off + i] = nf;
    d_all[r.work_off + i] = (__fsub_rn(m, nf) > r.margin) && (m > r.abs_floor);
}

__global__ __launch_bounds__(64) void k_vad_segment(const VadRow* __restrict__ rows, const float* __restrict__ st_in, float* __restrict__ st_out,
                                                    const float* __restrict__ s_all, const float* __restrict__ m_all,
                                                    const unsigned char* __restrict__ d_all, int* __restrict__ segs) {
    const VadRow r = rows[blockIdx.x];
    const int lane = threadIdx.x, W = r.W;
    const float* __restrict__ hist = st_in + r.state_off;
    const float* __restrict__ shist = hist + (W - 1);
    const float* __restrict__ s_new = s_all + r.work_off;
    const float* __restrict__ m_new = m_all + r.work_off;
    const unsigned char* __restrict__ dd = d_all + r.work_off;
    int* __restrict__ sg = segs + 3 * r.seg_off;
    int trig = r.trig, start = r.start, te = r.te, nseg = 0;
    const int half = r.max_speech / 2;
    auto m_at = [&](int j) { return j >= 0 ? m_new[j] : hist[W - 1 + j]; };   // (j >= -n_hist: checked by the launcher's rules)
    auto emit = [&](int a, int b, int forced) {
        if (lane == 0 && nseg < r.seg_cap) {
            sg[3 * nseg] = a;
            sg[3 * nseg + 1] = b;
            sg[3 * nseg + 2] = forced;
        }
        nseg++;
    };
    // the forced cut at frame tf (whose decision is `speech`): every lane takes part
    auto forced_cut = [&](int tf, bool speech) {
        float bv = 0.f;
        int bi = -1;
        for (int u = tf + 1 - half + lane; u <= tf; u += 64) best_merge(bv, bi, -m_at(u - r.t0), u);
        wave_best(bv, bi);
        emit(start, bi, 1);
        start = bi;
        te = speech ? -1 : (te > bi ? te : bi);
    };
    for (int base = 0; base < r.n; base += 64) {
        const int cnt = r.n - base < 64 ? r.n - base : 64;
        const unsigned long long mask = __ballot(lane < cnt && dd[base + lane] != 0);
        int p = 0;
        while (p < cnt) {   // (every value that steers this loop is the same in all lanes)
            const int t = r.t0 + base + p;
            const unsigned long long rest = mask >> p;
            if (!trig) {
                if (rest == 0) break;
                p += __builtin_ctzll(rest);
                trig = 1;
                start = r.t0 + base + p;
                te = -1;
                p += 1;   // (max_speech >= 2: no forced cut on the frame that triggers)
                continue;
            }
            const int tf = start + r.max_speech - 1 > t ? start + r.max_speech - 1 : t;   // the frame of the next forced cut
            if (rest & 1) {   // a run of speech: nothing but the forced cut can happen in it
                int len = ~rest ? __builtin_ctzll(~rest) : 64;
                len = len < cnt - p ? len : cnt - p;
                te = -1;
                if (tf < t + len) {
                    forced_cut(tf, true);
                    p = tf - (r.t0 + base) + 1;
                } else {
                    p += len;
                }
            } else {          // a run of silence: the timeout or the forced cut, whichever frame comes first (the timeout on a tie)
                int len = rest ? __builtin_ctzll(rest) : 64;
                len = len < cnt - p ? len : cnt - p;
                if (te < 0) te = t;
                const int ts = te + r.min_silence - 1 > t ? te + r.min_silence - 1 : t;
                if (ts <= tf && ts < t + len) {
                    if (te - start >= r.min_speech) emit(start, te, 0);
                    trig = 0;
                    te = -1;
                    p = ts - (r.t0 + base) + 1;
                } else if (tf < ts && tf < t + len) {
                    forced_cut(tf, false);
                    p = tf - (r.t0 + base) + 1;
                } else {
                    p += len;
                }
            }
        }
    }
    // the new carried block: the last W - 1 of [history ; this call's m], the last 4 of s, the machine
    float* __restrict__ oh = st_out + r.state_off;
    for (int q = lane; q < W - 1; q += 64) {
        const int j = r.n - (W - 1) + q;
        oh[q] = j >= 0 ? m_new[j] : -j <= r.n_hist ? hist[W - 1 + j] : 0.0f;
    }
    if (lane < 4) oh[W - 1 + lane] = vad_s_at(r, shist, s_new, r.n - 4 + lane);
    if (lane == 0) {
        int* oi = reinterpret_cast<int*>(oh + W + 3);
        oi[0] = trig;
        oi[1] = start;
        oi[2] = te;
        oi[3] = nseg;
    }
}

}  // namespace

void vad_run(const Ctx& ctx, const VadRow* rows, const VadRow* d_rows, int B, const VadBuffers& buf) {
    K2_REQUIRE(B > 0 && B <= 65535 && rows, "vad: B = %d", B);
    int max_n = 0;
    for (int b = 0; b < B; b++) {
        const VadRow& r = rows[b];
        K2_REQUIRE(r.n > 0 && r.t0 >= 0 && (long long)r.t0 + r.n < (1ll << 30), "vad: stream %d: %d frames at frame %d", b, r.n, r.t0);
        K2_REQUIRE(r.lo >= 0 && r.lo < r.hi && r.hi <= r.stride && (ctx.dry || r.feats), "vad: stream %d: bins [%d, %d) of rows of %lld floats", b, r.lo,
                   r.hi, r.stride);
        K2_REQUIRE(r.W >= 8 && r.W <= kVadMaxW && r.min_silence > 0 && r.min_speech > 0 && r.max_speech >= 2 && r.max_speech / 2 <= r.W,
                   "vad: stream %d: floor_window = %d, max_speech = %d", b, r.W, r.max_speech);
        K2_REQUIRE(r.n_hist == std::min(r.t0, r.W - 1), "vad: stream %d carries %d values of m at frame %d", b, r.n_hist, r.t0);
        K2_REQUIRE(r.trig == 0 || (r.start >= 0 && r.start < r.t0 && r.te < r.t0 && (r.te < 0 || r.te >= r.start) && r.t0 - r.start < r.max_speech),
                   "vad: stream %d: open segment from %d, pause from %d, at frame %d", b, r.start, r.te, r.t0);
        K2_REQUIRE(r.work_off >= 0 && r.work_off + r.n <= buf.n_work && r.state_off >= 0 && r.state_off + vad_state_words(r.W) <= buf.n_state &&
                       r.seg_off >= 0 && r.seg_cap >= 0 && r.seg_off + r.seg_cap <= buf.n_segs,
                   "vad: stream %d: work [%lld, +%d) of %lld, state %lld of %lld, segments [%lld, +%d) of %lld", b, r.work_off, r.n, buf.n_work,
                   r.state_off, buf.n_state, r.seg_off, r.seg_cap, buf.n_segs);
        max_n = std::max(max_n, r.n);
    }
    if (ctx.dry) return;
    hipLaunchKernelGGL(k_vad_score, dim3(std::min(cdiv(max_n, 4), 1024), B), dim3(256), 0, ctx.stream, d_rows, buf.s);
    hipLaunchKernelGGL(k_vad_floor, dim3(cdiv(max_n, kVadTile), B), dim3(kVadTile), 0, ctx.stream, d_rows, buf.st_in, buf.s, buf.m, buf.n, buf.d);
    hipLaunchKernelGGL(k_vad_segment, dim3(B), dim3(64), 0, ctx.stream, d_rows, buf.st_in, buf.st_out, buf.s, buf.m, buf.d, buf.segs);
    K2_HIP(hipGetLastError());
}

}  // namespace k2hip
