// The batch of one training step, cut from a device-resident pool of utterances and featurised in one launch
// (DESIGN.md 23).  Replaces the reference's input pipeline (auxilaries/reader.py:61-108: a TFRecord queue, tf.random_crop
// of wave_length samples, melspectrogram of the crop through py_func, shuffle_batch) by a pure function of
// (seed, step): row b of stream s takes the Philox4x32-10 words under key = seed, counter = (step lo, step hi, b, s),
//   u     = eligible[(r0 * n_eligible) >> 32]              an utterance of at least L samples, with replacement
//   start = (r1 * (utt_len[u] - L + 1)) >> 32              one of the starts tf.random_crop can return
// Stream 0 is the batch (wav and its mel), stream 1 an unrelated second draw of which only the mel is kept (the
// reference's mel_rand of the contrastive term).  train.batch_picks is the numpy twin.
//
// One workgroup = MEL_FR consecutive frames of one row of one stream, exactly mel_kernel's (wn_mel.h: wn_mel_block is
// the body of both, so the mel equals wn_mel_spectrogram of the materialised crop bit for bit).  It reads its samples
// from pool + utt_off[u] + start with the crop as the signal: reflect padding is applied at the CROP's edges (the
// reference featurises the crop, reader.py:88-90), and no load falls outside [start, start + L) of utterance u.
// Stream-0 workgroups also copy the MEL_HOP * MEL_FR samples they cover into wav (the last one of a row what is left up
// to L), and one thread of each row's first workgroup stores the pick.
#include <mutex>

#include "wn_codec.h"
#include "wn_mel.h"

namespace {

__global__ __launch_bounds__(256) void batch_kernel(const float* __restrict__ pool, const int64_t* __restrict__ utt_off,
                                                    const int64_t* __restrict__ utt_len, const int32_t* __restrict__ eligible,
                                                    int n_eligible, int B, int64_t L, int F, uint32_t seed_lo, uint32_t seed_hi,
                                                    uint32_t step_lo, uint32_t step_hi,
                                                    const float* __restrict__ twiddle, const float* __restrict__ window,
                                                    const int* __restrict__ band, const float* __restrict__ weight, int wmax,
                                                    float* __restrict__ wav, float* __restrict__ mel, int64_t* __restrict__ picks) {
    extern __shared__ float lds[];
    const int b = blockIdx.y, s = blockIdx.z;
    const int f0 = blockIdx.x * MEL_FR;
    uint32_t r[4] = {step_lo, step_hi, (uint32_t)b, (uint32_t)s};
    wn_philox4x32_10(r, seed_lo, seed_hi);
    const int u = eligible[(int)(((uint64_t)r[0] * (uint64_t)(uint32_t)n_eligible) >> 32)];
    const int64_t span = utt_len[u] - L + 1;                                   // >= 1: u is eligible
    const int64_t start = (int64_t)(((uint64_t)r[1] * (uint64_t)span) >> 32);
    const float* y = pool + utt_off[u] + start;
    const size_t row = (size_t)s * B + b;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        picks[2 * row] = u;
        picks[2 * row + 1] = start;
    }
    if (s == 0) {
        const int64_t t0 = (int64_t)f0 * MEL_HOP;                              // <= L: f0 <= F - 1 = L / MEL_HOP
        const int64_t t1 = t0 + MEL_HOP * MEL_FR < L ? t0 + MEL_HOP * MEL_FR : L;
        for (int64_t t = t0 + threadIdx.x; t < t1; t += 256) wav[(size_t)b * L + t] = y[t];
    }
    wn_mel_block(lds, y, L, F, f0, twiddle, window, band, weight, wmax, mel + row * F * MEL_NB);
}

std::mutex g_batch_mu;
bool g_batch_lds[16];

}  // namespace

extern "C" int wn_train_batch(const float* pool, const int64_t* utt_off, const int64_t* utt_len, const int32_t* eligible,
                              int n_eligible, int B, int64_t L, uint64_t seed, uint64_t step, int n_streams, float* wav,
                              float* mel, int64_t* picks, void* stream) {
    if (!pool || !utt_off || !utt_len || !eligible || !wav || !mel || !picks)
        return wn_fail(nullptr, WN_EINVAL, "wn_train_batch: null pointer");
    if (B < 1) return wn_fail(nullptr, WN_EINVAL, "wn_train_batch: B must be >= 1");
    if (B > 65535) return wn_fail(nullptr, WN_EINVAL, "wn_train_batch: B must be <= 65535");
    // as wn_mel_spectrogram: the reflect padding of the crop's centred frames
    if (L <= MEL_NFFT / 2)
        return wn_fail(nullptr, WN_EINVAL, "wn_train_batch: L = %lld samples, need more than %d (reflect padding of the "
                       "centred 2048-point frames)", (long long)L, MEL_NFFT / 2);
    if (L > 0x7fffffff / 2) return wn_fail(nullptr, WN_EINVAL, "wn_train_batch: L too long");
    if (n_eligible < 1) return wn_fail(nullptr, WN_EINVAL, "wn_train_batch: n_eligible must be >= 1 (no utterance of L samples)");
    if (n_streams != 1 && n_streams != 2)
        return wn_fail(nullptr, WN_EINVAL, "wn_train_batch: n_streams must be 1 or 2, got %d", n_streams);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return wn_fail(nullptr, WN_EIO, "wn_train_batch: no HIP device");
    MelTables* t = nullptr;
    if (int rc = wn_mel_tables(dev, "wn_train_batch", &t)) return rc;
    {
        std::lock_guard<std::mutex> lk(g_batch_mu);
        if (!g_batch_lds[dev]) {
            const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(batch_kernel),
                                                      hipFuncAttributeMaxDynamicSharedMemorySize, MEL_LDS_FLOATS * (int)sizeof(float));
            if (ea != hipSuccess)
                return wn_fail(nullptr, WN_EIO, "wn_train_batch: this device does not grant the %d bytes of LDS the kernel "
                               "needs (%s)", MEL_LDS_FLOATS * (int)sizeof(float), hipGetErrorString(ea));
            g_batch_lds[dev] = true;
        }
    }
    const int F = (int)(1 + L / MEL_HOP);
    dim3 grid((F + MEL_FR - 1) / MEL_FR, B, n_streams);
    hipLaunchKernelGGL(batch_kernel, grid, dim3(256), MEL_LDS_FLOATS * sizeof(float), reinterpret_cast<hipStream_t>(stream),
                       pool, utt_off, utt_len, eligible, n_eligible, B, L, F, (uint32_t)seed, (uint32_t)(seed >> 32),
                       (uint32_t)step, (uint32_t)(step >> 32), t->twiddle, t->window, t->band, t->weight, t->wmax, wav, mel,
                       picks);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return wn_fail(nullptr, WN_EIO, "wn_train_batch: launch failed: %s", hipGetErrorString(e));
    return WN_OK;
}
