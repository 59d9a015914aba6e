// Swoosh's softplus on the hardware transcendental units, shared by the GEMM epilogues (gemm.hip apply_act) and the elementwise
// kernels (elementwise.hip, online.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace k2hip {

// log(1 + e^z) as the library's fast log gives it: `__logf` is the general log, and around v_log_f32 and the extended-precision
// product with ln 2 it carries a denormal pre-scale of the argument (v_cmp, v_cndmask, v_ldexp, v_mov, v_cndmask, v_sub), a
// finiteness select (v_cmp, v_cndmask) and the s_nops between them.  Kept for the comparison op ("act_forms") only.
__device__ __forceinline__ float softplus_libm(float z) { return z > 15.f ? z : __logf(1.0f + __expf(z)); }

// The same value, bit for bit, for an argument that is never below 1: 1 + e^z is no denormal, so the pre-scale never applies, and
// it is infinite only for z > 88, where the z > 15 select discards the logarithm.  What is left is v_log_f32 and the four
// instructions of the compiler's own product y * ln 2 in extended precision (ln 2 = c + c_lo), written out as it emits them.
__device__ __forceinline__ float softplus_ge1(float z) {
    const float y = __builtin_amdgcn_logf(1.0f + __expf(z));
    const float c = __builtin_bit_cast(float, 0x3f317217u), c_lo = __builtin_bit_cast(float, 0x3377d1cfu);
    const float t = c * y;
    float e = __builtin_fmaf(y, c, -t);
    e = __builtin_fmaf(y, c_lo, e);
    const float r = __builtin_fmaf(c, y, e);
    return z > 15.f ? z : r;
}

__device__ __forceinline__ float swoosh_l(float v) { return softplus_ge1(v - 4.0f) - 0.08f * v - 0.035f; }
__device__ __forceinline__ float swoosh_r(float v) { return softplus_ge1(v - 1.0f) - 0.08f * v - 0.313261687f; }

}  // namespace k2hip
