// What the log-mel featuriser (wn_mel.hip) shares with the training-batch kernel (wn_batch.hip): its constants, its
// tables and the body of one workgroup.  Both kernels call wn_mel_block, so a frame featurised from a [B][L] buffer and
// the same frame featurised straight from a crop of the dataset pool go through the same operations in the same order
// (tests/test_gpu_train_batch.py holds the two to bit equality).
#pragma once
#include "wn_internal.h"

constexpr int MEL_SR = 16000;
constexpr int MEL_NFFT = 2048;
constexpr int MEL_NBIN = MEL_NFFT / 2 + 1;     // 1025
constexpr int MEL_HOP = 200;                   // 12.5 ms
constexpr int MEL_WIN = 800;                   // 50 ms
constexpr int MEL_NB = 80;
constexpr int MEL_FR = 8;                      // frames per workgroup
constexpr float MEL_MIN_AMP = 1e-5f;
constexpr float MEL_MIN_DB = -140.f;
constexpr int MEL_LDS_FLOATS = 2 * MEL_NFFT + MEL_FR * MEL_WIN + MEL_FR * (MEL_NBIN + 3);

struct MelTables {
    float* twiddle = nullptr;    // [2048][2] cos, sin of 2 pi i / 2048
    float* window = nullptr;     // [800] periodic Hann
    int* band = nullptr;         // [80][2] first bin, bin count
    float* weight = nullptr;     // [80][MEL_WMAX] triangle weights
    int wmax = 0;
};

// The tables of device `dev`, built and uploaded on first use (wn_mel.hip); `fn` names the caller in the message.
int wn_mel_tables(int dev, const char* fn, MelTables** out);

// Frames f0 .. f0 + MEL_FR - 1 of the signal y[0 .. L) (F frames in all) -> mel_row[(f0 + fr) * 80 + m], by one workgroup of
// 256 threads with MEL_LDS_FLOATS floats of LDS.  Reflect padding is applied at y's own edges: every load is y[j] with
// 0 <= j < L (L > MEL_NFFT / 2, checked by the callers).
__device__ __forceinline__ void wn_mel_block(float* lds, const float* __restrict__ y, int64_t L, int F, int f0,
                                             const float* __restrict__ twiddle, const float* __restrict__ window,
                                             const int* __restrict__ band, const float* __restrict__ weight, int wmax,
                                             float* __restrict__ mel_row) {
    float* tw = lds;                                  // [2048][2]
    float* xs = tw + 2 * MEL_NFFT;                    // [MEL_FR][800]
    float* mag = xs + MEL_FR * MEL_WIN;               // [MEL_FR][1028]
    constexpr int MS = MEL_NBIN + 3;
    for (int i = threadIdx.x; i < 2 * MEL_NFFT; i += 256) tw[i] = twiddle[i];
    for (int i = threadIdx.x; i < MEL_FR * MEL_WIN; i += 256) {
        const int fr = i / MEL_WIN, n = i - fr * MEL_WIN;
        // sample of the reflect-padded signal (numpy 'reflect': the edge sample is not repeated)
        int64_t j = (int64_t)(f0 + fr) * MEL_HOP - MEL_WIN / 2 + n;
        if (j < 0) j = -j;
        if (j >= L) j = 2 * (L - 1) - j;
        xs[i] = (f0 + fr < F) ? y[j] * window[n] : 0.f;
    }
    __syncthreads();

    // bins k0 + 256 r, r = 0..3
    float re[4][MEL_FR], im[4][MEL_FR];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int fr = 0; fr < MEL_FR; ++fr) re[r][fr] = im[r][fr] = 0.f;
    int idx[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) idx[r] = 0;
    for (int n = 0; n < MEL_WIN; ++n) {
        float x[MEL_FR];
#pragma unroll
        for (int fr = 0; fr < MEL_FR; ++fr) x[fr] = xs[fr * MEL_WIN + n];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float c = tw[2 * idx[r]], s = tw[2 * idx[r] + 1];
#pragma unroll
            for (int fr = 0; fr < MEL_FR; ++fr) {
                re[r][fr] = fmaf(x[fr], c, re[r][fr]);
                im[r][fr] = fmaf(x[fr], s, im[r][fr]);
            }
            idx[r] = (idx[r] + (int)threadIdx.x + 256 * r) & (MEL_NFFT - 1);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int fr = 0; fr < MEL_FR; ++fr)
            mag[fr * MS + threadIdx.x + 256 * r] = sqrtf(re[r][fr] * re[r][fr] + im[r][fr] * im[r][fr]);
    // bin 1024: sum x[n] (-1)^n, one wave per two frames
    {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        for (int fr = wave; fr < MEL_FR; fr += 4) {
            float a = 0.f;
            for (int n = lane; n < MEL_WIN; n += 64) a += (n & 1) ? -xs[fr * MEL_WIN + n] : xs[fr * MEL_WIN + n];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
            if (lane == 0) mag[fr * MS + MEL_NFFT / 2] = fabsf(a);
        }
    }
    __syncthreads();

    for (int o = threadIdx.x; o < MEL_FR * MEL_NB; o += 256) {
        const int fr = o / MEL_NB, m = o - fr * MEL_NB;
        if (f0 + fr >= F) continue;
        const int k0 = band[2 * m], cnt = band[2 * m + 1];
        const float* wm = weight + (size_t)m * wmax;
        float s = 0.f;
        for (int i = 0; i < cnt; ++i) s = fmaf(wm[i], mag[fr * MS + k0 + i], s);
        const float db = 20.f * log10f(fmaxf(MEL_MIN_AMP, s));
        const float ns = fminf(fmaxf((db - MEL_MIN_DB) / -MEL_MIN_DB, 0.f), 1.f);
        mel_row[(size_t)(f0 + fr) * MEL_NB + m] = ns;
    }
}
