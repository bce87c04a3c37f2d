// Device helpers shared by the training-side units (wn_teacher*.hip, wn_deconv_bwd.hip): the channel order of the G4
// activation layout (wn_mfma_h.h), its hi / lo row pair, the wave maximum, and the power-of-two operand scale of a cotangent.
#pragma once
#include "wn_codec.h"

__device__ inline float wn_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// ---- G4 channel order: word i of a column of group g holds the halves of channels wn_g4_channel(g, i) + {0, 1} ----
__device__ inline int wn_g4_channel(int g, int i) { return 32 * (g >> 2) + 16 * (i >> 1) + 4 * (g & 3) + 2 * (i & 1); }
// ... and its inverse: channel c lives in word `slot` of group g, in the half at bit `sh`
__device__ inline void wn_g4_slot(int c, int& g, int& slot, int& sh) {
    const int cc = c & 31;
    g = (c >> 5) * 4 + ((cc & 15) >> 2);
    slot = ((cc >> 4) << 1) | ((cc >> 1) & 1);
    sh = 16 * (cc & 1);
}
// column `col` of group g in rows of `rowlen` columns: the hi word at group row g, the lo word at group row NG + g
__device__ inline void wn_g4_store(unsigned* base, int NG, long long rowlen, int g, long long col, wn_u4 hw, wn_u4 lw) {
    *reinterpret_cast<wn_u4*>(base + ((size_t)g * rowlen + col) * 4) = hw;
    *reinterpret_cast<wn_u4*>(base + ((size_t)(NG + g) * rowlen + col) * 4) = lw;
}
__device__ inline void wn_g4_load(const unsigned* base, int NG, long long rowlen, int g, long long col, wn_u4& hw, wn_u4& lw) {
    hw = *reinterpret_cast<const wn_u4*>(base + ((size_t)g * rowlen + col) * 4);
    lw = *reinterpret_cast<const wn_u4*>(base + ((size_t)(NG + g) * rowlen + col) * 4);
}

// ---- scale of a cotangent x[n]: the power of two that brings its largest magnitude to [1, 2) (wn_scale.hip) ----
// scal[0] = 2^k with max |x| 2^k in [1, 2) (1 for an all-zero x), scal[1] = what undoes every scale applied so far: 2^-k times
// prev[1], the scale pair of the stage above (null: none).  part: WN_NPART floats of scratch.
constexpr int WN_NPART = 1024;          // workgroups of the max-magnitude pass
void wn_pow2_scale(const float* x, long long n, float* part, float* scal, const float* prev, hipStream_t st);
