// Distillation losses of the parallel-WaveNet student against its teacher: ParallelWavenet.kl_loss_logistic,
// kl_loss_gauss and power_loss (wavenet/parallel_wavenet.py:361-479), scored on the teacher's out_params (wn_teacher_forward).
//
// dx_mol_kernel -- the Monte-Carlo cross entropy H(P_s, P_t) of kl_loss_logistic (:361-402).  The reference repeats the
// teacher's [B,T,3M] parameters and the student's mean / scale num_samples times (utils.tf_repeat) and evaluates
// mol_log_probs on the [B*S,T,3M] copy.  Here one LANE owns one row (b, t): it reads the row once, forms the row constants
// (log-softmax of the logits, inv_s = e^-max(log_s,-7), the bin factor 1 - e^-(2 inv_s/Q) of every component) in
// registers, and evaluates its draws x = rl * scale_tot + mean_tot against them; nothing of size [B,S,T,.] exists.  A
// workgroup is 64 consecutive rows x 4 waves; wave w takes the blocks of four draws s = 4q..4q+3 with q = w mod 4, and the
// four partial sums of a row meet in LDS in a fixed order.  Per draw and component: two exp + two divides (the sigmoids),
// the log of the mass, and the exp of the mixture's log-sum-exp -- about 6 M + 3 transcendental-class instructions per
// draw against a few loads per row, so the kernel is bound by the SIMDs' transcendental issue, not by HBM.
// Draws: injected [B,S,T] (row b*S + s of the reference's [B*S,T] draw), or Philox4x32-10 keyed by (seed; t, s/4, b) with
// lane s%4 of the result -- a function of (seed, b, s, t) alone -- through log u - log(1 - u), u ~ U(1e-5, 1 - 1e-5), the
// transform of iaf_noise_draw (wn_iaf_call.hip).
//
// dx_gauss_kernel -- kl_loss_gauss (:404-429): the closed-form KL(q || p) of two Gaussians per sample and the squared
// log-scale difference, elementwise.
//
// pw_kernel -- power_loss (:459-479) with the module constants as the reference freezes them (SPEC_ENHANCE_FACTOR = 1,
// USE_L1_LOSS = False, USE_PRIORITY_FREQ = True, NORM_FEAT = False, USE_MEL = False): tf.contrib.signal.stft(frame_length
// 800, frame_step 200, fft_length 2048, pad_end=True) of both signals (mel_extractor.py:111-121) -- not centred, frames at
// 200 f, the signal zero-padded at its end to ceil(L/200) frames, each frame windowed by a periodic Hann of 800 and
// zero-padded to 2048 at its end -- then (|P| - |O|)^2 over the 1025 bins.  Like mel_kernel (wn_mel.hip) it is a direct
// DFT over the 800 live samples with the twiddle table in LDS; the table and the window are formed in the kernel, so the
// call needs no device tables.
//
// Every sum the losses need is reduced in a fixed order: per-workgroup partials in double (a wave butterfly, then the
// waves in order) into the caller's workspace, and one workgroup of dx_reduce_kernel over the partials in order.  Repeated
// calls are bit-identical.
#include <algorithm>
#include <cmath>

#include "wn_internal.h"
#include "wn_codec.h"
#include "wn_mol.h"

namespace {

constexpr int DX_ROWS = 64;          // rows per workgroup of dx_mol_kernel (one per lane)
constexpr int DX_WAVES = 4;          // waves per workgroup, each on every fourth block of four draws
constexpr int DX_MAX_MIX = 32;       // mixture components held in registers
constexpr int DG_ROWS = 256;         // rows per workgroup of dx_gauss_kernel
constexpr int PW_HOP = 200, PW_WIN = 800, PW_NFFT = 2048;     // 1025 bins
constexpr int PW_PRIO = 384;         // mel_extractor.PRIORITY_FREQ = int(3000 / 8000 * 1025)
constexpr int PW_FR = 4;             // frames per workgroup of pw_kernel
constexpr uint32_t DX_PHILOX_TAG = 0x44534c4cu;

__device__ inline double dx_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Partials are two planes, partial[blk] and partial[nblk + blk]: two 8-byte stores instead of one 16-byte store whose data
// registers the code behind it may overwrite too soon (the gfx950 wide-store hazard, hazard_audit.py).
// Sum of (a, b) over the workgroup (blockDim.x = 256), in a fixed order, into partial[blk], partial[nblk + blk].
__device__ inline void dx_block_sum2(double a, double b, double* __restrict__ partial, size_t blk, size_t nblk) {
    __shared__ double sh[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    a = dx_wave_sum(a);
    b = dx_wave_sum(b);
    if (lane == 0) { sh[0][wave] = a; sh[1][wave] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[blk] = ((sh[0][0] + sh[0][1]) + sh[0][2]) + sh[0][3];
        partial[nblk + blk] = ((sh[1][0] + sh[1][1]) + sh[1][2]) + sh[1][3];
    }
}

// one workgroup: out[0..1] = sums of partial[i], partial[n + i] over i < n
__global__ __launch_bounds__(256) void dx_reduce_kernel(const double* __restrict__ partial, long long n,
                                                        double* __restrict__ out) {
    double a = 0.0, b = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) {
        a += partial[i];
        b += partial[n + i];
    }
    __shared__ double sh[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    a = dx_wave_sum(a);
    b = dx_wave_sum(b);
    if (lane == 0) { sh[0][wave] = a; sh[1][wave] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = ((sh[0][0] + sh[0][1]) + sh[0][2]) + sh[0][3];
        out[1] = ((sh[1][0] + sh[1][1]) + sh[1][2]) + sh[1][3];
    }
}

// H_bl[b,t] = -mean_s log p_teacher(rl[b,s,t] * scale[b,t] + mean[b,t]); partial sums of H_bl and of log scale
template <int MM>
__global__ __launch_bounds__(256) void dx_mol_kernel(const float* __restrict__ te, const float* __restrict__ mean_st,
                                                     const float* __restrict__ scale_st, long long T, int S, int M, int ow,
                                                     int Q, const float* __restrict__ noise, uint64_t seed,
                                                     float* __restrict__ h_bl, float* __restrict__ noise_out,
                                                     double* __restrict__ partial) {
    __shared__ float red[DX_WAVES][DX_ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const long long t = (long long)blockIdx.x * DX_ROWS + lane;
    const bool live = t < T;
    float acc = 0.f, lsc = 0.f;
    if (live) {
        const size_t row = (size_t)b * T + t;
        const float* o = te + row * ow;
        const float iq = 1.0f / (float)Q;
        float min_thres, max_thres;
        wn_mol_thresholds(Q, min_thres, max_thres);
        // row constants (loss_func.py:30-33,62): log-softmax of the logits, inv_s, bin factor
        float lsm[MM], mu[MM], inv[MM], dd[MM];
        float lmax = -__builtin_inff();
#pragma unroll
        for (int k = 0; k < MM; ++k)
            if (k < M) { lsm[k] = o[k]; lmax = fmaxf(lmax, lsm[k]); }
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < MM; ++k)
            if (k < M) se += expf(lsm[k] - lmax);
        const float lse = lmax + logf(se);
#pragma unroll
        for (int k = 0; k < MM; ++k)
            if (k < M) {
                lsm[k] -= lse;
                mu[k] = o[M + k];
                inv[k] = expf(-fmaxf(o[2 * M + k], -7.0f));
                dd[k] = wn_mol_bin_factor(inv[k], iq);
            }
        const float ms = mean_st[row], ss = scale_st[row];
        lsc = logf(ss);
        const int nq = (S + 3) / 4;
        for (int q = wave; q < nq; q += DX_WAVES) {
            float rl[4];
            if (noise) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int s = 4 * q + e;
                    rl[e] = s < S ? noise[((size_t)b * S + s) * T + t] : 0.f;
                }
            } else {
                uint32_t c[4] = {(uint32_t)t, (uint32_t)q, (uint32_t)b, DX_PHILOX_TAG};
                wn_philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float u = wn_u01(c[e]) * (1.f - 2e-5f) + 1e-5f;
                    rl[e] = logf(u) - logf(1.f - u);
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int s = 4 * q + e;
                if (s >= S) break;
                if (noise_out) noise_out[((size_t)b * S + s) * T + t] = rl[e];
                const float x = rl[e] * ss + ms;                       // x_xp (parallel_wavenet.py:379), not quantised
                float v[MM];
                float vmax = -__builtin_inff();
#pragma unroll
                for (int k = 0; k < MM; ++k)
                    if (k < M) {
                        v[k] = wn_mol_component_lp(x, x - mu[k], inv[k], iq, dd[k], min_thres, max_thres) + lsm[k];
                        vmax = fmaxf(vmax, v[k]);
                    }
                float sv = 0.f;
#pragma unroll
                for (int k = 0; k < MM; ++k)
                    if (k < M) sv += expf(v[k] - vmax);
                acc += vmax + logf(sv);
            }
        }
    }
    red[wave][lane] = acc;
    __syncthreads();
    if (wave == 0) {
        float hb = 0.f;
        if (live) {
            hb = -(((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]) / (float)S;
            h_bl[(size_t)b * T + t] = hb;
        }
        const double a = dx_wave_sum((double)hb), c = dx_wave_sum((double)lsc);
        if (lane == 0) {
            const size_t blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
            partial[blk] = a;
            partial[(size_t)gridDim.x * gridDim.y + blk] = c;
        }
    }
}

// kl_bl = log s_p - log s_q + (s_q^2 - s_p^2 + (m_p - m_q)^2) / (2 s_p^2); partial sums of kl_bl and (log s_p - log s_q)^2
__global__ __launch_bounds__(256) void dx_gauss_kernel(const float* __restrict__ te, const float* __restrict__ mean_st,
                                                       const float* __restrict__ scale_st, long long n,
                                                       float* __restrict__ kl_bl, double* __restrict__ partial) {
    const long long i = (long long)blockIdx.x * DG_ROWS + threadIdx.x;
    float kl = 0.f, reg = 0.f;
    if (i < n) {
        const float mp = te[2 * i], lsp = fmaxf(te[2 * i + 1], -7.0f);     // mean_std_from_out_params (loss_func.py:66-75)
        const float sp = expf(lsp);
        const float mq = mean_st[i], sq = scale_st[i], lsq = logf(sq);
        const float vq = sq * sq, vp = sp * sp, dm = mp - mq, dl = lsp - lsq;
        kl = dl + (vq - vp + dm * dm) / (2.0f * vp);
        reg = dl * dl;
        kl_bl[i] = kl;
    }
    dx_block_sum2((double)kl, (double)reg, partial, blockIdx.x, gridDim.x);
}

// sums over (b, frame, bin) of (|P| - |O|)^2 and over the bins below PW_PRIO; PW_FR frames of one utterance per workgroup
__global__ __launch_bounds__(256) void pw_kernel(const float* __restrict__ pred, long long ps, const float* __restrict__ orig,
                                                 long long os, long long L, int NF, double* __restrict__ partial) {
    __shared__ float tw[2 * PW_NFFT];                  // cos, sin of 2 pi i / 2048
    __shared__ float xs[2][PW_FR][PW_WIN];             // windowed frames of pred, orig
    const int b = blockIdx.y, f0 = blockIdx.x * PW_FR;
    for (int i = threadIdx.x; i < PW_NFFT; i += 256) {
        float s, c;
        sincospif((float)i / (float)(PW_NFFT / 2), &s, &c);
        tw[2 * i] = c;
        tw[2 * i + 1] = s;
    }
    for (int i = threadIdx.x; i < PW_FR * PW_WIN; i += 256) {
        const int fr = i / PW_WIN, n = i - fr * PW_WIN;
        const long long j = (long long)(f0 + fr) * PW_HOP + n;
        const float w = 0.5f - 0.5f * cospif((float)n / (float)(PW_WIN / 2));    // periodic Hann of 800
        const bool in = f0 + fr < NF && j < L;
        xs[0][fr][n] = in ? pred[b * ps + j] * w : 0.f;
        xs[1][fr][n] = in ? orig[b * os + j] * w : 0.f;
    }
    __syncthreads();

    // bins k0 + 256 r, r = 0..3 (bin 1024 below)
    float re[2][4][PW_FR], im[2][4][PW_FR];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int fr = 0; fr < PW_FR; ++fr) re[p][r][fr] = im[p][r][fr] = 0.f;
    int idx[4] = {0, 0, 0, 0};
    for (int n = 0; n < PW_WIN; ++n) {
        float x[2][PW_FR];
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int fr = 0; fr < PW_FR; ++fr) x[p][fr] = xs[p][fr][n];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float c = tw[2 * idx[r]], s = tw[2 * idx[r] + 1];
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int fr = 0; fr < PW_FR; ++fr) {
                    re[p][r][fr] = fmaf(x[p][fr], c, re[p][r][fr]);
                    im[p][r][fr] = fmaf(x[p][fr], s, im[p][r][fr]);
                }
            idx[r] = (idx[r] + (int)threadIdx.x + 256 * r) & (PW_NFFT - 1);
        }
    }
    float all = 0.f, prio = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = threadIdx.x + 256 * r;
#pragma unroll
        for (int fr = 0; fr < PW_FR; ++fr) {
            const float mp = sqrtf(re[0][r][fr] * re[0][r][fr] + im[0][r][fr] * im[0][r][fr]);
            const float mo = sqrtf(re[1][r][fr] * re[1][r][fr] + im[1][r][fr] * im[1][r][fr]);
            const float d = (mp - mo) * (mp - mo);
            all += d;
            if (k < PW_PRIO) prio += d;
        }
    }
    // bin 1024: sum x[n] (-1)^n, wave w on frame w
    {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        float a0 = 0.f, a1 = 0.f;
        for (int n = lane; n < PW_WIN; n += 64) {
            a0 += (n & 1) ? -xs[0][wave][n] : xs[0][wave][n];
            a1 += (n & 1) ? -xs[1][wave][n] : xs[1][wave][n];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a0 += __shfl_xor(a0, o);
            a1 += __shfl_xor(a1, o);
        }
        if (lane == 0) {
            const float d = fabsf(a0) - fabsf(a1);
            all += d * d;
        }
    }
    dx_block_sum2((double)all, (double)prio, partial, (size_t)blockIdx.y * gridDim.x + blockIdx.x, (size_t)gridDim.x * gridDim.y);
}

size_t dx_mol_blocks(int B, long long T) { return (size_t)B * ((T + DX_ROWS - 1) / DX_ROWS); }
size_t dx_gauss_blocks(int B, long long T) { return ((size_t)B * T + DG_ROWS - 1) / DG_ROWS; }
long long pw_frames(long long L) { return (L + PW_HOP - 1) / PW_HOP; }
size_t pw_blocks(int B, long long L) { return (size_t)B * ((pw_frames(L) + PW_FR - 1) / PW_FR); }

// the checks both teacher-side calls share (include/wnhip.h, "Distillation losses")
int dx_check(wn_handle* h, const char* fn, int want_loss, const float* out_params, int out_width, const float* mean_tot,
             const float* scale_tot, int B, long long T, const void* sums, const void* ws, size_t ws_bytes, size_t need) {
    if (!h) return wn_fail(nullptr, WN_EINVAL, "%s: null handle", fn);
    const wn_config& c = h->cfg;
    if (c.kind != WN_KIND_TEACHER)
        return wn_fail(h, WN_EINVAL, "%s: this is a ParallelWavenet student handle; the distillation losses are scored "
                       "under the TEACHER's handle", fn);
    if (want_loss == WN_LOSS_MOL && c.loss_type == WN_LOSS_CE)
        return wn_fail(h, WN_EINVAL, "%s: cross-entropy (ce) teacher: kl_loss_logistic needs a mixture-of-logistics "
                       "teacher (parallel_wavenet.py:133-135)", fn);
    if (c.loss_type != want_loss)
        return wn_fail(h, WN_EINVAL, "%s: the teacher's loss_type is not %s (parallel_wavenet.py:133-135 pairs a logistic "
                       "student with a mol teacher, a gauss student with a gauss teacher)", fn,
                       want_loss == WN_LOSS_MOL ? "mol" : "gauss");
    if (c.use_mu_law)
        return wn_fail(h, WN_EINVAL, "%s: mu-law teacher: the reference would score the student's audio unencoded "
                       "(CLIP = False); mu-law students and teachers are not supported by the distillation losses", fn);
    if (out_width != c.out_width)
        return wn_fail(h, WN_EINVAL, "%s: out_params [..., %d] do not match the teacher's out_width %d", fn, out_width,
                       c.out_width);
    if (B < 1 || T < 1 || !out_params || !mean_tot || !scale_tot || !sums || !ws)
        return wn_fail(h, WN_EINVAL, "%s: bad argument", fn);
    if (T > 0x7fffffffll) return wn_fail(h, WN_EINVAL, "%s: %lld samples per utterance exceed 32-bit counters", fn, T);
    if (ws_bytes < need) return wn_fail(h, WN_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, need);
    return WN_OK;
}

}  // namespace

extern "C" size_t wn_distill_workspace_bytes(const wn_handle* h, int B, int64_t T) {
    if (!h || B < 1 || T < 1) return 0;
    const size_t nb = std::max(dx_mol_blocks(B, T), dx_gauss_blocks(B, T));
    return align_up(nb * 2 * sizeof(double), 256);
}

extern "C" int wn_distill_mol_xent(wn_handle* h, const float* out_params, int out_width, const float* mean_tot,
                                   const float* scale_tot, int B, int64_t T, int S, const float* noise, uint64_t seed,
                                   float* h_bl, float* noise_out, double* sums, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "wn_distill_mol_xent";
    if (int rc = dx_check(h, fn, WN_LOSS_MOL, out_params, out_width, mean_tot, scale_tot, B, T, sums, ws, ws_bytes,
                          wn_distill_workspace_bytes(h, B, T)))
        return rc;
    if (S < 1)
        return wn_fail(h, WN_EINVAL, "%s: num_samples = %d; the Monte-Carlo estimate needs at least one draw (the "
                       "reference's default num_samples = 0 averages over nothing)", fn, S);
    if (!h_bl) return wn_fail(h, WN_EINVAL, "%s: bad argument (h_bl)", fn);
    const int M = h->cfg.mol_mix;
    if (M < 1 || M > DX_MAX_MIX || out_width != 3 * M)
        return wn_fail(h, WN_EINVAL, "%s: %d mixture components (1..%d supported)", fn, M, DX_MAX_MIX);
    const WnWork work(h);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double* partial = reinterpret_cast<double*>(ws);
    const long long nbt = (T + DX_ROWS - 1) / DX_ROWS;
    const dim3 grid((unsigned)nbt, (unsigned)B);
    const int Q = 65536;                                 // quant_chann of a student without mu-law (parallel_wavenet.py:137-140)
    if (M <= 10)
        hipLaunchKernelGGL(dx_mol_kernel<10>, grid, dim3(256), 0, st, out_params, mean_tot, scale_tot, (long long)T, S, M,
                           out_width, Q, noise, seed, h_bl, noise_out, partial);
    else
        hipLaunchKernelGGL(dx_mol_kernel<DX_MAX_MIX>, grid, dim3(256), 0, st, out_params, mean_tot, scale_tot, (long long)T, S,
                           M, out_width, Q, noise, seed, h_bl, noise_out, partial);
    hipLaunchKernelGGL(dx_reduce_kernel, dim3(1), dim3(256), 0, st, partial, (long long)(nbt * B), sums);
    WN_HIP(h, hipGetLastError());
    return WN_OK;
}

extern "C" int wn_distill_gauss_kl(wn_handle* h, const float* out_params, int out_width, const float* mean_tot,
                                   const float* scale_tot, int B, int64_t T, float* kl_bl, double* sums, void* ws,
                                   size_t ws_bytes, void* stream) {
    const char* fn = "wn_distill_gauss_kl";
    if (int rc = dx_check(h, fn, WN_LOSS_GAUSS, out_params, out_width, mean_tot, scale_tot, B, T, sums, ws, ws_bytes,
                          wn_distill_workspace_bytes(h, B, T)))
        return rc;
    if (!kl_bl) return wn_fail(h, WN_EINVAL, "%s: bad argument (kl_bl)", fn);
    const WnWork work(h);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double* partial = reinterpret_cast<double*>(ws);
    const long long n = (long long)B * T;
    const size_t nb = dx_gauss_blocks(B, T);
    hipLaunchKernelGGL(dx_gauss_kernel, dim3((unsigned)nb), dim3(256), 0, st, out_params, mean_tot, scale_tot, n, kl_bl,
                       partial);
    hipLaunchKernelGGL(dx_reduce_kernel, dim3(1), dim3(256), 0, st, partial, (long long)nb, sums);
    WN_HIP(h, hipGetLastError());
    return WN_OK;
}

extern "C" size_t wn_power_loss_workspace_bytes(int B, int64_t L) {
    if (B < 1 || L < 1) return 0;
    return align_up(pw_blocks(B, L) * 2 * sizeof(double), 256);
}

extern "C" int wn_power_loss(const float* pred, int64_t pred_stride, const float* orig, int64_t orig_stride, int B, int64_t L,
                             double* out2, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "wn_power_loss";
    if (!pred || !orig || !out2 || !ws) return wn_fail(nullptr, WN_EINVAL, "%s: null pointer", fn);
    if (B < 1 || L < 1) return wn_fail(nullptr, WN_EINVAL, "%s: B = %d, L = %lld", fn, B, (long long)L);
    if (pred_stride < L || orig_stride < L)
        return wn_fail(nullptr, WN_EINVAL, "%s: row strides %lld / %lld below the length %lld", fn, (long long)pred_stride,
                       (long long)orig_stride, (long long)L);
    if (L > 0x7fffffffll) return wn_fail(nullptr, WN_EINVAL, "%s: utterance too long", fn);
    const size_t need = wn_power_loss_workspace_bytes(B, L);
    if (ws_bytes < need) return wn_fail(nullptr, WN_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, need);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double* partial = reinterpret_cast<double*>(ws);
    const long long NF = pw_frames(L);
    const dim3 grid((unsigned)((NF + PW_FR - 1) / PW_FR), (unsigned)B);
    hipLaunchKernelGGL(pw_kernel, grid, dim3(256), 0, st, pred, (long long)pred_stride, orig, (long long)orig_stride,
                       (long long)L, (int)NF, partial);
    hipLaunchKernelGGL(dx_reduce_kernel, dim3(1), dim3(256), 0, st, partial, (long long)pw_blocks(B, L), out2);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return wn_fail(nullptr, WN_EIO, "%s: launch failed: %s", fn, hipGetErrorString(e));
    return WN_OK;
}

// ---- gradients of the three losses.  Each takes `fac`, two float64 values on the device: the loss's
// derivative with respect to the two sums the forward call returns (sums / out2), so a backward pass needs no host read.
// Tie conventions are TensorFlow's (include/wnhip.h).  No atomics: every value is written by exactly one lane. ----
namespace {

// H_bl rows as dx_mol_kernel evaluates them, differentiated: per draw the mixture weights w_k = softmax_k(v) of the
// component log-probabilities; d/d logit_k = sum_s (w_k - p_k), d/d mean_k and d/d log_scale_k through the component,
// d/d x_s -> d mean_tot, rl_s d/d x_s -> d scale_tot.  Same tile, row constants and draws as dx_mol_kernel; the four
// waves' partial sums meet in LDS in a fixed order.
template <int MM>
__global__ __launch_bounds__(256) void dx_mol_grad_kernel(const float* __restrict__ te, const float* __restrict__ mean_st,
                                                          const float* __restrict__ scale_st, long long T, int S, int M,
                                                          int ow, int Q, const float* __restrict__ noise, uint64_t seed,
                                                          const double* __restrict__ fac, float* __restrict__ d_te,
                                                          float* __restrict__ d_mean, float* __restrict__ d_scale) {
    __shared__ float red[DX_WAVES][DX_ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const long long t = (long long)blockIdx.x * DX_ROWS + lane;
    const bool live = t < T;
    float gw[MM], gmu[MM], gin[MM], inv[MM], lsm[MM], raw_ls[MM];
#pragma unroll
    for (int k = 0; k < MM; ++k) gw[k] = gmu[k] = gin[k] = inv[k] = lsm[k] = raw_ls[k] = 0.f;
    float gx = 0.f, gxr = 0.f, ss = 1.f;
    const size_t row = live ? (size_t)b * T + t : 0;
    if (live) {
        const float* o = te + row * ow;
        const float iq = 1.0f / (float)Q;
        float min_thres, max_thres;
        wn_mol_thresholds(Q, min_thres, max_thres);
        float mu[MM], dd[MM];
        float lmax = -__builtin_inff();
#pragma unroll
        for (int k = 0; k < MM; ++k)
            if (k < M) { lsm[k] = o[k]; lmax = fmaxf(lmax, lsm[k]); }
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < MM; ++k)
            if (k < M) se += expf(lsm[k] - lmax);
        const float lse = lmax + logf(se);
#pragma unroll
        for (int k = 0; k < MM; ++k)
            if (k < M) {
                lsm[k] -= lse;
                mu[k] = o[M + k];
                raw_ls[k] = o[2 * M + k];
                inv[k] = expf(-fmaxf(raw_ls[k], -7.0f));
                dd[k] = wn_mol_bin_factor(inv[k], iq);
            }
        const float ms = mean_st[row];
        ss = scale_st[row];
        const int nq = (S + 3) / 4;
        for (int q = wave; q < nq; q += DX_WAVES) {
            float rl[4];
            if (noise) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int s = 4 * q + e;
                    rl[e] = s < S ? noise[((size_t)b * S + s) * T + t] : 0.f;
                }
            } else {
                uint32_t c[4] = {(uint32_t)t, (uint32_t)q, (uint32_t)b, DX_PHILOX_TAG};
                wn_philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float u = wn_u01(c[e]) * (1.f - 2e-5f) + 1e-5f;
                    rl[e] = logf(u) - logf(1.f - u);
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int s = 4 * q + e;
                if (s >= S) break;
                const float x = rl[e] * ss + ms;
                float v[MM], dxk[MM], dik[MM];
                float vmax = -__builtin_inff();
#pragma unroll
                for (int k = 0; k < MM; ++k)
                    if (k < M) {
                        const float cc = x - mu[k];
                        v[k] = wn_mol_component_lp(x, cc, inv[k], iq, dd[k], min_thres, max_thres) + lsm[k];
                        vmax = fmaxf(vmax, v[k]);
                        wn_mol_component_grad(x, cc, inv[k], iq, dd[k], min_thres, max_thres, dxk[k], dik[k]);
                    }
                float sv = 0.f;
#pragma unroll
                for (int k = 0; k < MM; ++k)
                    if (k < M) { v[k] = expf(v[k] - vmax); sv += v[k]; }
                const float isv = 1.f / sv;
                float gxs = 0.f;
#pragma unroll
                for (int k = 0; k < MM; ++k)
                    if (k < M) {
                        const float w = v[k] * isv;
                        gw[k] += w;
                        gmu[k] -= w * dxk[k];
                        gin[k] += w * dik[k];
                        gxs += w * dxk[k];
                    }
                gx += gxs;
                gxr += rl[e] * gxs;
            }
        }
    }
    // fixed-order sum of the four waves' partials; wave 0 writes the row
    auto meet = [&](float v) {
        red[wave][lane] = v;
        __syncthreads();
        const float r = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
        __syncthreads();
        return r;
    };
    const float c = (float)(-fac[0] / (double)S);          // d loss / d log p of one draw of the row
    float* dt = d_te + row * ow;
#pragma unroll
    for (int k = 0; k < MM; ++k)
        if (k < M) {
            const float w = meet(gw[k]), m = meet(gmu[k]), in = meet(gin[k]);
            if (wave == 0 && live) {
                dt[k] = c * (w - (float)S * expf(lsm[k]));
                dt[M + k] = c * m;
                dt[2 * M + k] = raw_ls[k] >= -7.0f ? -c * in * inv[k] : 0.f;     // tf.maximum(log_s, -7)
            }
        }
    const float x1 = meet(gx), x2 = meet(gxr);
    if (wave == 0 && live) {
        d_mean[row] = c * x1;
        d_scale[row] = c * x2 + (float)fac[1] / ss;         // H_Ps = mean(log scale_tot) + 2
    }
}

// kl_bl = dl + (s_q^2 - s_p^2 + dm^2) / (2 s_p^2), reg = dl^2 with dl = log s_p - log s_q, dm = m_p - m_q
__global__ __launch_bounds__(256) void dx_gauss_grad_kernel(const float* __restrict__ te, const float* __restrict__ mean_st,
                                                            const float* __restrict__ scale_st, long long n,
                                                            const double* __restrict__ fac, float* __restrict__ d_te,
                                                            float* __restrict__ d_mean, float* __restrict__ d_scale) {
    const long long i = (long long)blockIdx.x * DG_ROWS + threadIdx.x;
    if (i >= n) return;
    const float f0 = (float)fac[0], f1 = (float)fac[1];
    const float raw = te[2 * i + 1], mp = te[2 * i];
    const float lsp = fmaxf(raw, -7.0f), sp = expf(lsp);
    const float mq = mean_st[i], sq = scale_st[i], lsq = logf(sq);
    const float vp = sp * sp, dm = mp - mq, dl = lsp - lsq;
    const float g_mp = f0 * dm / vp;
    const float g_lsp = f0 * (1.f - (sq * sq + dm * dm) / vp) + f1 * 2.f * dl;
    d_te[2 * i] = g_mp;
    d_te[2 * i + 1] = raw >= -7.0f ? g_lsp : 0.f;
    d_mean[i] = -g_mp;
    d_scale[i] = f0 * (sq / vp - 1.f / sq) - f1 * 2.f * dl / sq;
}

// power loss transposed, per frame: c_k = 2 (|P_k| - |O_k|) (fac0 + [k < 384] fac1), then
// d y_n = w_n sum_k c_k (re_k cos + im_k sin)(2 pi k n / 2048) / |P_k| (0 where |P_k| = 0) -> gframe[b][f][800]
__global__ __launch_bounds__(256) void pw_grad_kernel(const float* __restrict__ pred, long long ps, const float* __restrict__ orig,
                                                      long long os, long long L, int NF, const double* __restrict__ fac,
                                                      float* __restrict__ gframe) {
    __shared__ float tw[2 * PW_NFFT];
    __shared__ float buf[2 * PW_FR * 1025];            // windowed frames [2][PW_FR][800], then coefficients [PW_FR][1025][2]
    const int b = blockIdx.y, f0 = blockIdx.x * PW_FR;
    const float fa = (float)fac[0], fp = (float)fac[1];
    for (int i = threadIdx.x; i < PW_NFFT; i += 256) {
        float s, c;
        sincospif((float)i / (float)(PW_NFFT / 2), &s, &c);
        tw[2 * i] = c;
        tw[2 * i + 1] = s;
    }
    auto xs = [&](int p, int fr, int n) -> float& { return buf[(p * PW_FR + fr) * PW_WIN + n]; };
    for (int i = threadIdx.x; i < PW_FR * PW_WIN; i += 256) {
        const int fr = i / PW_WIN, n = i - fr * PW_WIN;
        const long long j = (long long)(f0 + fr) * PW_HOP + n;
        const float w = 0.5f - 0.5f * cospif((float)n / (float)(PW_WIN / 2));
        const bool in = f0 + fr < NF && j < L;
        xs(0, fr, n) = in ? pred[b * ps + j] * w : 0.f;
        xs(1, fr, n) = in ? orig[b * os + j] * w : 0.f;
    }
    __syncthreads();
    float re[2][4][PW_FR], im[2][4][PW_FR];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int fr = 0; fr < PW_FR; ++fr) re[p][r][fr] = im[p][r][fr] = 0.f;
    int idx[4] = {0, 0, 0, 0};
    for (int n = 0; n < PW_WIN; ++n) {
        float x[2][PW_FR];
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int fr = 0; fr < PW_FR; ++fr) x[p][fr] = xs(p, fr, n);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float c = tw[2 * idx[r]], s = tw[2 * idx[r] + 1];
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int fr = 0; fr < PW_FR; ++fr) {
                    re[p][r][fr] = fmaf(x[p][fr], c, re[p][r][fr]);
                    im[p][r][fr] = fmaf(x[p][fr], s, im[p][r][fr]);
                }
            idx[r] = (idx[r] + (int)threadIdx.x + 256 * r) & (PW_NFFT - 1);
        }
    }
    // bin 1024 (cos = (-1)^n, sin = 0): wave w on frame w
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float a0 = 0.f, a1 = 0.f;
    for (int n = lane; n < PW_WIN; n += 64) {
        a0 += (n & 1) ? -xs(0, wave, n) : xs(0, wave, n);
        a1 += (n & 1) ? -xs(1, wave, n) : xs(1, wave, n);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a0 += __shfl_xor(a0, o);
        a1 += __shfl_xor(a1, o);
    }
    __syncthreads();                                   // the frames are read; buf becomes the coefficients
    auto cf = [&](int fr, int k, int c) -> float& { return buf[(fr * 1025 + k) * 2 + c]; };
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = threadIdx.x + 256 * r;
#pragma unroll
        for (int fr = 0; fr < PW_FR; ++fr) {
            const float rp = re[0][r][fr], ip = im[0][r][fr];
            const float mp = sqrtf(rp * rp + ip * ip);
            const float mo = sqrtf(re[1][r][fr] * re[1][r][fr] + im[1][r][fr] * im[1][r][fr]);
            const float g = mp > 0.f ? 2.f * (mp - mo) * (k < PW_PRIO ? fa + fp : fa) / mp : 0.f;   // |z|' = 0 at 0
            cf(fr, k, 0) = g * rp;
            cf(fr, k, 1) = g * ip;
        }
    }
    if (lane == 0) {
        const float mp = fabsf(a0);
        cf(wave, 1024, 0) = mp > 0.f ? 2.f * (mp - fabsf(a1)) * fa * (a0 > 0.f ? 1.f : -1.f) : 0.f;
        cf(wave, 1024, 1) = 0.f;
    }
    __syncthreads();
    for (int n = threadIdx.x; n < PW_WIN; n += 256) {
        float acc[PW_FR];
#pragma unroll
        for (int fr = 0; fr < PW_FR; ++fr) acc[fr] = 0.f;
        int id = 0;
        for (int k = 0; k <= 1024; ++k) {
            const float c = tw[2 * id], s = tw[2 * id + 1];
#pragma unroll
            for (int fr = 0; fr < PW_FR; ++fr) acc[fr] = fmaf(cf(fr, k, 0), c, fmaf(cf(fr, k, 1), s, acc[fr]));
            id = (id + n) & (PW_NFFT - 1);
        }
        const float w = 0.5f - 0.5f * cospif((float)n / (float)(PW_WIN / 2));
#pragma unroll
        for (int fr = 0; fr < PW_FR; ++fr)
            if (f0 + fr < NF) gframe[((size_t)b * NF + f0 + fr) * PW_WIN + n] = acc[fr] * w;
    }
}

// overlap-add of the frames' gradients, frames in increasing order: d pred[b][j] = sum_f gframe[b][f][j - 200 f]
__global__ __launch_bounds__(256) void pw_ola_kernel(const float* __restrict__ gframe, long long L, int NF,
                                                     float* __restrict__ dp, long long ds) {
    const int b = blockIdx.y;
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= L) return;
    const long long fhi = std::min<long long>(NF - 1, j / PW_HOP);
    const long long flo = j >= PW_WIN ? (j - PW_WIN) / PW_HOP + 1 : 0;
    float acc = 0.f;
    for (long long f = flo; f <= fhi; ++f) acc += gframe[((size_t)b * NF + f) * PW_WIN + (j - f * PW_HOP)];
    dp[b * ds + j] = acc;
}

}  // namespace

extern "C" int wn_distill_mol_xent_grad(wn_handle* h, const float* out_params, int out_width, const float* mean_tot,
                                        const float* scale_tot, int B, int64_t T, int S, const float* noise, uint64_t seed,
                                        const double* fac, float* d_out_params, float* d_mean_tot, float* d_scale_tot,
                                        void* stream) {
    const char* fn = "wn_distill_mol_xent_grad";
    int dummy = 0;
    if (int rc = dx_check(h, fn, WN_LOSS_MOL, out_params, out_width, mean_tot, scale_tot, B, T, &dummy, &dummy, 0, 0))
        return rc;
    if (S < 1) return wn_fail(h, WN_EINVAL, "%s: num_samples = %d; the Monte-Carlo estimate needs at least one draw", fn, S);
    if (!fac || !d_out_params || !d_mean_tot || !d_scale_tot) return wn_fail(h, WN_EINVAL, "%s: bad argument", fn);
    const int M = h->cfg.mol_mix;
    if (M < 1 || M > DX_MAX_MIX || out_width != 3 * M)
        return wn_fail(h, WN_EINVAL, "%s: %d mixture components (1..%d supported)", fn, M, DX_MAX_MIX);
    const WnWork work(h);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((T + DX_ROWS - 1) / DX_ROWS), (unsigned)B);
    const int Q = 65536;
    if (M <= 10)
        hipLaunchKernelGGL(dx_mol_grad_kernel<10>, grid, dim3(256), 0, st, out_params, mean_tot, scale_tot, (long long)T, S, M,
                           out_width, Q, noise, seed, fac, d_out_params, d_mean_tot, d_scale_tot);
    else
        hipLaunchKernelGGL(dx_mol_grad_kernel<DX_MAX_MIX>, grid, dim3(256), 0, st, out_params, mean_tot, scale_tot,
                           (long long)T, S, M, out_width, Q, noise, seed, fac, d_out_params, d_mean_tot, d_scale_tot);
    WN_HIP(h, hipGetLastError());
    return WN_OK;
}

extern "C" int wn_distill_gauss_kl_grad(wn_handle* h, const float* out_params, int out_width, const float* mean_tot,
                                        const float* scale_tot, int B, int64_t T, const double* fac, float* d_out_params,
                                        float* d_mean_tot, float* d_scale_tot, void* stream) {
    const char* fn = "wn_distill_gauss_kl_grad";
    int dummy = 0;
    if (int rc = dx_check(h, fn, WN_LOSS_GAUSS, out_params, out_width, mean_tot, scale_tot, B, T, &dummy, &dummy, 0, 0))
        return rc;
    if (!fac || !d_out_params || !d_mean_tot || !d_scale_tot) return wn_fail(h, WN_EINVAL, "%s: bad argument", fn);
    const WnWork work(h);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long n = (long long)B * T;
    hipLaunchKernelGGL(dx_gauss_grad_kernel, dim3((unsigned)dx_gauss_blocks(B, T)), dim3(256), 0, st, out_params, mean_tot,
                       scale_tot, n, fac, d_out_params, d_mean_tot, d_scale_tot);
    WN_HIP(h, hipGetLastError());
    return WN_OK;
}

extern "C" size_t wn_power_loss_grad_workspace_bytes(int B, int64_t L) {
    if (B < 1 || L < 1) return 0;
    return align_up((size_t)B * pw_frames(L) * PW_WIN * sizeof(float), 256);
}

extern "C" int wn_power_loss_grad(const float* pred, int64_t pred_stride, const float* orig, int64_t orig_stride, int B,
                                  int64_t L, const double* fac, float* d_pred, int64_t d_pred_stride, void* ws, size_t ws_bytes,
                                  void* stream) {
    const char* fn = "wn_power_loss_grad";
    if (!pred || !orig || !fac || !d_pred || !ws) return wn_fail(nullptr, WN_EINVAL, "%s: null pointer", fn);
    if (B < 1 || L < 1) return wn_fail(nullptr, WN_EINVAL, "%s: B = %d, L = %lld", fn, B, (long long)L);
    if (pred_stride < L || orig_stride < L || d_pred_stride < L)
        return wn_fail(nullptr, WN_EINVAL, "%s: row strides below the length %lld", fn, (long long)L);
    if (L > 0x7fffffffll) return wn_fail(nullptr, WN_EINVAL, "%s: utterance too long", fn);
    const size_t need = wn_power_loss_grad_workspace_bytes(B, L);
    if (ws_bytes < need) return wn_fail(nullptr, WN_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, need);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float* gframe = reinterpret_cast<float*>(ws);
    const long long NF = pw_frames(L);
    hipLaunchKernelGGL(pw_grad_kernel, dim3((unsigned)((NF + PW_FR - 1) / PW_FR), (unsigned)B), dim3(256), 0, st, pred,
                       (long long)pred_stride, orig, (long long)orig_stride, (long long)L, (int)NF, fac, gframe);
    hipLaunchKernelGGL(pw_ola_kernel, dim3((unsigned)((L + 255) / 256), (unsigned)B), dim3(256), 0, st, gframe, (long long)L,
                       (int)NF, d_pred, (long long)d_pred_stride);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return wn_fail(nullptr, WN_EIO, "%s: launch failed: %s", fn, hipGetErrorString(e));
    return WN_OK;
}
