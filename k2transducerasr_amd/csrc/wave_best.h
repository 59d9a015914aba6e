// Wave-wide best (score, index) on data-parallel-primitive lane moves: the candidate order of the searches (beam.hip, ctc_prefix.hip) in
// one place -- higher score first, then the LOWER flat index.  Device code only; every lane of the wave must be active at a call.
#pragma once
#include <hip/hip_runtime.h>

namespace k2hip {

// ---- wave-wide reductions on data-parallel-primitive lane moves (no LDS crossbar: a ds_bpermute butterfly of 6 steps x 2 values is a
// chain of ~900 cycles, and the step runs ~10 of them per frame) ------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false);
}
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141, kDppMirror = 0x140;  // quad_perm [1,0,3,2] / [2,3,0,1], row_half_mirror, row_mirror
// candidate order of the search: higher score first, then the LOWER flat index; index < 0 = no candidate
__device__ __forceinline__ void best_merge(float& bv, int& bi, float ov, int oi) {
    if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
}
// the best (score, index) of the wave, in every lane (a total order: the sequence of merges does not matter)
__device__ __forceinline__ void wave_best(float& bv, int& bi) {
    best_merge(bv, bi, dpp_f<kDppXor1>(bv), dpp_i<kDppXor1>(bi));
    best_merge(bv, bi, dpp_f<kDppXor2>(bv), dpp_i<kDppXor2>(bi));
    best_merge(bv, bi, dpp_f<kDppHalfMirror>(bv), dpp_i<kDppHalfMirror>(bi));
    best_merge(bv, bi, dpp_f<kDppMirror>(bv), dpp_i<kDppMirror>(bi));   // every lane: its row of 16
    float rv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, bv), 0));
    int ri = __builtin_amdgcn_readlane(bi, 0);
#pragma unroll
    for (int row = 1; row < 4; row++)
        best_merge(rv, ri, __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, bv), 16 * row)), __builtin_amdgcn_readlane(bi, 16 * row));
    bv = rv;
    bi = ri;
}

}  // namespace k2hip
