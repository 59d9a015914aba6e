// Sample-rate conversion on gfx950: the windowed-sinc plan of resample_plan.h applied to B rows in one launch, each row given as two
// pieces [carried tail ; new samples] that may lie in pinned host memory (read in place over PCIe, as k_gather_samples reads them).
// Rows carry their own plan, so one launch mixes rates, and a row without a plan is copied as the gather copies it.
//
// One workgroup of 256 threads walks tiles of up to kResampleTile consecutive outputs of its row, one thread per output.  The
// tile's input span (tile * iu / ou + taps floats) is staged into LDS first with coalesced reads -- 16 bytes per lane where the source
// allows, scalar at the ragged ends -- because neighbouring outputs share all but iu / ou of their taps and host memory must be read
// once.  The phase weights come from the plan table: a table of up to kWLds floats (every integer ratio: 8, 32, 48 kHz -> 16 kHz) is
// copied to LDS once per workgroup, a larger one (441:160 has 160 x 34) is read through L1 / L2, where it stays.  LDS reads of the
// span are iu / ou floats apart between lanes: free of conflicts at 3:1 and 1:2, two-way at 2:1.  The kernel is bound by the link for
// host sources and has no other state: no atomics, nothing shared between workgroups, control flow decided by the bounds alone.
//
// The dot product is resample_ref.h's: acc = +0.0f, acc = fmaf(w[p][j], x, acc) for j ascending.
#include <algorithm>
#include <cstdint>

#include "kernels.h"

namespace k2hip {
namespace {

constexpr int kSpan = 8192;   // floats of LDS for a tile's input span
constexpr int kWLds = 2048;   // floats: a weight table up to this size is kept in LDS

// outputs per tile of a row: the span of T consecutive outputs is at most (T - 1) * iu / ou + 2 + max_taps floats
__host__ __device__ inline int tile_outputs(int iu, int ou, int max_taps) {
    long long t = (long long)(kSpan - max_taps - 2) * ou / iu;
    if (t > kResampleTile) t = kResampleTile;
    return (int)(t / 256 * 256);
}

__device__ inline bool al16(const void* p) { return (reinterpret_cast<unsigned long long>(p) & 15) == 0; }

// xs[0 .. n) = src[0 .. n): scalar up to the source's next 16-byte boundary, float4 reads from there, scalar for the rest
__device__ inline void stage_piece(float* xs, const float* __restrict__ src, int n, int tid) {
    if (n <= 0) return;
    int pre = (int)((4 - ((reinterpret_cast<unsigned long long>(src) >> 2) & 3)) & 3);
    pre = pre < n ? pre : n;
    const int nv = (n - pre) / 4;
    if (tid < pre) xs[tid] = src[tid];
    for (int v = tid; v < nv; v += 256) {
        const float4 q = *reinterpret_cast<const float4*>(src + pre + 4 * v);
        float* o = xs + pre + 4 * v;
        o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
    }
    for (int i = pre + 4 * nv + tid; i < n; i += 256) xs[i] = src[i];
}

__global__ __launch_bounds__(256) void k_resample_gather(const ResampleRow* __restrict__ rows, float* __restrict__ dst, long long nmax) {
    __shared__ float xs[kSpan];
    __shared__ float ws[kWLds];
    const ResampleRow r = rows[blockIdx.y];
    float* d = dst + (long long)r.dst_row * nmax;
    const int tid = threadIdx.x;
    if (!r.w) {   // pass-through: the two pieces back to back, zeros behind them
        const long long nt = r.n_head + r.n_tail;
        for (long long i4 = (long long)blockIdx.x * 256 + tid; 4 * i4 < nmax; i4 += (long long)gridDim.x * 256) {
            const long long i = 4 * i4;
            const bool dal = i + 3 < nmax && al16(d + i);
            if (dal && i + 3 < r.n_head && al16(r.head + i)) {
                *reinterpret_cast<float4*>(d + i) = *reinterpret_cast<const float4*>(r.head + i);
            } else if (dal && i >= r.n_head && i + 3 < nt && al16(r.tail + (i - r.n_head))) {
                *reinterpret_cast<float4*>(d + i) = *reinterpret_cast<const float4*>(r.tail + (i - r.n_head));
            } else {
                for (int k = 0; k < 4 && i + k < nmax; k++) {
                    const long long a = i + k;
                    d[a] = a < r.n_head ? r.head[a] : a < nt ? r.tail[a - r.n_head] : 0.f;
                }
            }
        }
        return;
    }
    const int iu = r.iu, ou = r.ou, mt = r.max_taps;
    const int T = tile_outputs(iu, ou, mt);
    const bool wl = ou * mt <= kWLds;
    if (wl)
        for (int i = tid; i < ou * mt; i += 256) ws[i] = r.w[i];
    const float* __restrict__ wt = r.w;
    for (long long i0 = (long long)blockIdx.x * T; i0 < nmax; i0 += (long long)gridDim.x * T) {
        const long long i1 = i0 + T < nmax ? i0 + T : nmax;
        const long long o1 = i1 < r.n_out ? i1 : r.n_out;   // the tile's outputs are [i0, o1), zeros from there to i1
        long long lo = 0, uf = 0;
        int pf = 0;
        if (i0 < o1) {   // (the same for the whole workgroup)
            const long long kf = r.k0 + i0, kl = r.k0 + o1 - 1;
            uf = kf / ou;
            pf = (int)(kf % ou);
            const int pl = (int)(kl % ou);
            lo = uf * iu + r.first[pf];
            const long long hi = (kl / ou) * iu + r.first[pl] + r.ntaps[pl];
            const int span = (int)(hi - lo < kSpan ? hi - lo : kSpan);
            const int nz = lo < 0 ? (int)(-lo < span ? -lo : span) : 0;   // in front of the stream's first sample
            for (int i = tid; i < nz; i += 256) xs[i] = 0.f;
            const long long a1 = lo + span, h1 = r.x0 + r.n_head, t1 = h1 + r.n_tail;
            {
                const long long b0 = lo + nz > r.x0 ? lo + nz : r.x0, b1 = a1 < h1 ? a1 : h1;
                if (b0 < b1) stage_piece(xs + (b0 - lo), r.head + (b0 - r.x0), (int)(b1 - b0), tid);
            }
            {
                const long long b0 = lo + nz > h1 ? lo + nz : h1, b1 = a1 < t1 ? a1 : t1;
                if (b0 < b1) stage_piece(xs + (b0 - lo), r.tail + (b0 - h1), (int)(b1 - b0), tid);
            }
        }
        __syncthreads();
        for (long long i = i0 + tid; i < i1; i += 256) {
            float acc = 0.0f;
            if (i < o1) {
                const int off = (int)(i - i0) + pf;
                const int p = off % ou;
                const long long s = (uf + off / ou) * iu + r.first[p];
                const int nt = r.ntaps[p];
                const float* x = xs + (s - lo);
                if (wl) {
                    const float* w = ws + p * mt;
                    for (int j = 0; j < nt; j++) acc = fmaf(w[j], x[j], acc);
                } else {
                    const float* w = wt + (long long)p * mt;
                    for (int j = 0; j < nt; j++) acc = fmaf(w[j], x[j], acc);
                }
            }
            d[i] = acc;
        }
        __syncthreads();   // the next trip stages over xs
    }
}

int64_t floor_div(int64_t a, int64_t b) { return a / b - ((a % b != 0) && ((a < 0) != (b < 0))); }

}  // namespace

void resample_gather(const Ctx& ctx, const ResampleRow* rows, const ResampleRow* d_rows, int B, float* dst, int n_dst_rows, long long nmax) {
    K2_REQUIRE(B > 0 && B <= 65535 && nmax > 0 && n_dst_rows > 0 && rows, "resample_gather: B = %d, nmax = %lld", B, nmax);
    for (int b = 0; b < B; b++) {
        const ResampleRow& r = rows[b];
        K2_REQUIRE(r.dst_row >= 0 && r.dst_row < n_dst_rows && r.n_head >= 0 && r.n_tail >= 0 && (ctx.dry || r.n_head == 0 || r.head) &&
                       (ctx.dry || r.n_tail == 0 || r.tail) && r.n_head + r.n_tail < ((int64_t)1 << 38),
                   "resample_gather: row %d: %lld + %lld samples into row %d of %d", b, r.n_head, r.n_tail, r.dst_row, n_dst_rows);
        if (!r.w) {
            K2_REQUIRE(r.n_head + r.n_tail <= nmax, "resample_gather: row %d passes %lld samples through into %lld", b, r.n_head + r.n_tail, nmax);
            continue;
        }
        K2_REQUIRE(r.first && r.ntaps && r.iu > 0 && r.ou > 0 && r.max_taps > 0 && r.max_taps <= 256 && (int64_t)r.ou * r.max_taps <= 65536 &&
                       r.wmax >= 0 && 2 * r.wmax / r.ou + 1 <= r.max_taps + 1 && tile_outputs(r.iu, r.ou, r.max_taps) >= 256,
                   "resample_gather: row %d: plan %d:%d with %d taps", b, r.iu, r.ou, r.max_taps);
        K2_REQUIRE(r.k0 >= 0 && r.n_out >= 0 && r.n_out <= nmax && r.x0 >= 0 && r.k0 + r.n_out < ((int64_t)1 << 38), "resample_gather: row %d: outputs %lld + %lld into %lld",
                   b, r.k0, r.n_out, nmax);
        if (r.n_out == 0) continue;
        // what the row reads: input samples [start(k0), end(k0 + n_out - 1)) of the stream, those below 0 as zeros
        const int64_t start = -floor_div(-(r.k0 * r.iu - r.wmax), r.ou), end = floor_div((r.k0 + r.n_out - 1) * r.iu + r.wmax, r.ou) + 1;
        K2_REQUIRE(r.x0 <= std::max<int64_t>(start, 0) && end <= r.x0 + r.n_head + r.n_tail,
                   "resample_gather: row %d reads input [%lld, %lld) and holds [%lld, %lld)", b, (long long)start, (long long)end, r.x0,
                   r.x0 + r.n_head + r.n_tail);
    }
    if (ctx.dry) return;
    const int gx = (int)std::min<long long>(cdiv(nmax, kResampleTile), 64);
    hipLaunchKernelGGL(k_resample_gather, dim3(gx, B), dim3(256), 0, ctx.stream, d_rows, dst, nmax);
    K2_HIP(hipGetLastError());
}

}  // namespace k2hip
