// Operand scale of a cotangent for the split-fp16 reverse passes, found on the device (wn_g4.h: wn_pow2_scale).
#include <algorithm>

#include "wn_internal.h"
#include "wn_g4.h"

namespace {
// largest |x| per workgroup ...
__global__ __launch_bounds__(256) void wn_absmax_kernel(const float* __restrict__ x, long long n, float* __restrict__ part) {
    __shared__ float sh[4];
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) m = fmaxf(m, fabsf(x[i]));
    m = wn_wave_max(m);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}
// ... then one workgroup: the scale pair
__global__ __launch_bounds__(256) void wn_scale_kernel(const float* __restrict__ part, int np, float* __restrict__ scal,
                                                       const float* __restrict__ prev) {
    __shared__ float sh[4];
    float m = 0.f;
    for (int i = threadIdx.x; i < np; i += 256) m = fmaxf(m, part[i]);
    m = wn_wave_max(m);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
        int k = 0;
        if (m > 0.f && m < __builtin_inff()) k = min(max(-ilogbf(m), -100), 100);
        scal[0] = ldexpf(1.f, k);
        scal[1] = (prev ? prev[1] : 1.f) * ldexpf(1.f, -k);
    }
}
}  // namespace
void wn_pow2_scale(const float* x, long long n, float* part, float* scal, const float* prev, hipStream_t st) {
    const int nb = (int)std::min<long long>(WN_NPART, (n + 255) / 256);
    hipLaunchKernelGGL(wn_absmax_kernel, dim3(nb), dim3(256), 0, st, x, n, part);
    hipLaunchKernelGGL(wn_scale_kernel, dim3(1), dim3(256), 0, st, part, nb, scal, prev);
}
