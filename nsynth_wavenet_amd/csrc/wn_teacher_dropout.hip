// Dropout of the teacher's training path: the mask kernels the training-tape forward (wn_teacher.hip) and the
// reverse pass (wn_teacher_bwd.hip) launch between their GEMMs, and the kernel that writes the keep bits themselves for tests.
// Every kernel calls the one hash of wn_dropout.h.  A kept element is fp32(v / keep), keep = fp32(1 - rate), as TF1's
// nn.dropout divides; a dropped one is +0 in both words.  At rate 0 a kept G4 element keeps its two halves, at rate 0.5 both are
// doubled in integer arithmetic on their bits -- the exact value, in the split the forward's store gave it; at any other rate
// the element is joined, divided and split again like every G4 store (wn_split_pair).
#include <cmath>

#include "wn_teacher.h"
#include "wn_g4.h"
#include "wn_dropout.h"

namespace {
struct DropArgs {
    uint64_t seed;
    uint32_t site, thr;
    float keep;
    int exact;          // 1: keep == 1, the halves pass;  2: keep == 0.5, the halves are doubled;  0: join, divide, split
};

// 2 h of one fp16 value given by its 16 bits: exact (a subnormal shifts into the exponent field), inf beyond the range
__device__ inline unsigned td_double_half(unsigned h) {
    const unsigned e = (h >> 10) & 31u, sign = h & 0x8000u;
    if (e == 0) return sign | ((h & 0x3ffu) << 1);
    if (e >= 30) return e == 31 ? h : (sign | 0x7c00u);
    return h + 0x400u;
}
__device__ inline unsigned td_double_word(unsigned w) { return td_double_half(w & 0xffffu) | (td_double_half(w >> 16) << 16); }

// one thread: four consecutive columns of one group (8 channels) of one batch element
__global__ __launch_bounds__(256) void td_g4_kernel(const unsigned* __restrict__ src, unsigned* __restrict__ dst, int NG,
                                                    long long rowlen, long long col0, long long T, DropArgs a) {
    const int b = blockIdx.z, g = blockIdx.y;
    const long long col = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (col >= rowlen) return;
    const size_t boff = (size_t)b * NG * 8 * rowlen;
    const long long t0 = col - col0;                      // col0 % 4 == 0: the four columns share one counter
    if (t0 < 0) {                                         // the zero left pad, as the source holds it
        if (src != dst)
            for (int j = 0; j < 4 && col + j < rowlen; ++j) {
                wn_u4 hw, lw;
                wn_g4_load(src + boff, NG, rowlen, g, col + j, hw, lw);
                wn_g4_store(dst + boff, NG, rowlen, g, col + j, hw, lw);
            }
        return;
    }
    const wn_u4 zero = (wn_u4){0u, 0u, 0u, 0u};
    if (t0 >= T) {
        for (int j = 0; j < 4 && col + j < rowlen; ++j) wn_g4_store(dst + boff, NG, rowlen, g, col + j, zero, zero);
        return;
    }
    unsigned km[8];                                       // km[2 i + p]: keep bits of channel wn_g4_channel(g, i) + p
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int p = 0; p < 2; ++p)
            km[2 * i + p] = wn_dropout_keep4(a.seed, a.site, (uint32_t)b, (uint32_t)(wn_g4_channel(g, i) + p), (uint32_t)(t0 >> 2), a.thr);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (col + j >= rowlen) break;
        wn_u4 hw = zero, lw = zero;
        if (t0 + j < T) {
            wn_g4_load(src + boff, NG, rowlen, g, col + j, hw, lw);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool k0 = (km[2 * i] >> j) & 1u, k1 = (km[2 * i + 1] >> j) & 1u;
                if (a.exact) {
                    const unsigned m = (k0 ? 0xffffu : 0u) | (k1 ? 0xffff0000u : 0u);
                    hw[i] = (a.exact == 2 ? td_double_word(hw[i]) : hw[i]) & m;
                    lw[i] = (a.exact == 2 ? td_double_word(lw[i]) : lw[i]) & m;
                } else {
                    float v0, v1;
                    wn_join_pair(hw[i], lw[i], v0, v1);
                    v0 = k0 ? __fdiv_rn(v0, a.keep) : 0.f;
                    v1 = k1 ? __fdiv_rn(v1, a.keep) : 0.f;
                    unsigned h2, l2;
                    wn_split_pair(v0, v1, h2, l2);
                    hw[i] = h2;
                    lw[i] = l2;
                }
            }
        }
        wn_g4_store(dst + boff, NG, rowlen, g, col + j, hw, lw);
    }
}

// accumulator layout: element (t, c) of a batch element is word c % 4 of the float4 at
// ((t / 16) (C / 16) + c / 16) 64 + 16 ((c % 16) / 4) + t % 16.  One thread: four consecutive t of four consecutive channels
__global__ __launch_bounds__(256) void td_acc_kernel(float* __restrict__ s, int nmb, long long Tp, long long T, DropArgs a) {
    const int b = blockIdx.y;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;          // ((t / 16) nmb + mb) 16 + 4 q + tq
    if (idx >= Tp / 16 * nmb * 16) return;
    const int tq = (int)(idx & 3), q = (int)((idx >> 2) & 3);
    const long long blk = idx >> 4;
    const int mb = (int)(blk % nmb);
    const long long t0 = (blk / nmb) * 16 + 4 * tq;
    if (t0 >= T) return;
    f4* p = reinterpret_cast<f4*>(s + (size_t)b * nmb * 16 * Tp) + (size_t)blk * 64 + 16 * q + 4 * tq;
    unsigned km[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
        km[r] = wn_dropout_keep4(a.seed, a.site, (uint32_t)b, (uint32_t)(16 * mb + 4 * q + r), (uint32_t)(t0 >> 2), a.thr);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (t0 + j >= T) break;
        f4 v = p[j];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = (km[r] >> j) & 1u ? __fdiv_rn(v[r], a.keep) : 0.f;
        p[j] = v;
    }
}

__global__ __launch_bounds__(256) void td_keep_kernel(unsigned char* __restrict__ out, long long n, int C, long long T, DropArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;            // [b][t][c]
    if (i >= n) return;
    const int c = (int)(i % C);
    const long long t = i / C % T, b = i / C / T;
    out[i] = wn_dropout_keep(a.seed, a.site, (uint32_t)b, (uint32_t)c, t, a.thr) ? 1 : 0;
}

DropArgs drop_args(const TgDropout& dr, int site) {
    DropArgs a;
    a.seed = dr.seed; a.site = (uint32_t)site; a.thr = dr.thr; a.keep = dr.keep;
    a.exact = dr.keep == 1.0f ? 1 : dr.keep == 0.5f ? 2 : 0;
    return a;
}
}  // namespace

void wn_dropout_g4(const unsigned* src, unsigned* dst, int B, int C, long long rowlen, long long col0, long long T,
                   const TgDropout& dr, int site, hipStream_t st) {
    const dim3 grid((unsigned)((rowlen + 1023) / 1024), C / 8, B);
    hipLaunchKernelGGL(td_g4_kernel, grid, dim3(256), 0, st, src, dst, C / 8, rowlen, col0, T, drop_args(dr, site));
}

void wn_dropout_acc(float* s, int B, int C, long long Tp, long long T, const TgDropout& dr, int site, hipStream_t st) {
    const long long n = Tp / 16 * (C / 16) * 16;
    hipLaunchKernelGGL(td_acc_kernel, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, st, s, C / 16, Tp, T, drop_args(dr, site));
}

uint32_t wn_dropout_threshold(double rate) {
    const double v = std::floor(rate * 4294967296.0 + 0.5);
    return v >= 4294967295.0 ? 0xffffffffu : (uint32_t)v;
}

extern "C" int wn_teacher_dropout_keep(uint64_t seed, int site, int B, int C, int64_t T, double rate, unsigned char* keep,
                                       void* stream) {
    const char* fn = "wn_teacher_dropout_keep";
    if (site < 0 || B < 1 || C < 1 || T < 1 || !keep) return wn_fail(nullptr, WN_EINVAL, "%s: bad argument", fn);
    if (!(rate >= 0.0 && rate < 1.0)) return wn_fail(nullptr, WN_EINVAL, "%s: rate %g is outside [0, 1)", fn, rate);
    TgDropout dr;
    dr.seed = seed; dr.thr = wn_dropout_threshold(rate); dr.keep = (float)(1.0 - rate);
    const long long n = (long long)B * C * T;
    if ((n + 255) / 256 > 0x7fffffffll) return wn_fail(nullptr, WN_EINVAL, "%s: too many elements", fn);
    hipLaunchKernelGGL(td_keep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), keep,
                       n, C, (long long)T, drop_args(dr, site));
    if (hipGetLastError() != hipSuccess) return wn_fail(nullptr, WN_EIO, "%s: launch failed", fn);
    return WN_OK;
}
