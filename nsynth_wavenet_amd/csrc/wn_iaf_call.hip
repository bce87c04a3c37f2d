// Parallel-WaveNet (IAF) student generation, the call: workspace layout, the element-wise kernels of a call's front and
// back (pads + noise, final affine + _clip_quant_scale, their windowed forms), the call skeleton with one flow runner per
// launch form, the launch-form policy, the range-status calls and the profiler.  The kernels of the residual stack live with
// their launch functions in wn_iaf.hip (fp32 MFMA), wn_iaf_h/c/g.hip (split-fp16) and wn_iaf_x.hip (generic widths).
#include <cstdlib>

#include "wn_internal.h"
#include "wn_codec.h"

namespace {

constexpr float EXP_7 = 1096.6331584284585f;

// ---------------- noise (parallel_wavenet.py:172-184) ----------------
// The four draws of Philox counter (i4, b): samples 4 i4 .. 4 i4 + 3 of utterance b.  logistic: log u - log(1-u),
// u ~ U(1e-5, 1-1e-5); gauss: Box-Muller.
__device__ inline void iaf_noise_draw(int64_t i4, int b, uint64_t seed, int gauss, float (&v)[4]) {
    uint32_t c[4] = {(uint32_t)i4, (uint32_t)(i4 >> 32), (uint32_t)b, 0x49414630u};
    wn_philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    if (!gauss) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float u01 = (float)(c[e] >> 8) * (1.0f / 16777216.0f);
            const float u = u01 * (1.f - 2e-5f) + 1e-5f;
            v[e] = logf(u) - logf(1.f - u);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
            const float u1 = ((float)(c[e] >> 8) + 1.0f) * (1.0f / 16777216.0f);   // (0,1]
            const float u2 = (float)(c[e + 1] >> 8) * (1.0f / 16777216.0f);
            const float rr = sqrtf(-2.f * logf(u1));
            v[e] = rr * cosf(6.283185307179586f * u2);
            v[e + 1] = rr * sinf(6.283185307179586f * u2);
        }
    }
}

// one-shot: 4 samples per thread, the counter is the thread's index in the row
__device__ inline void iaf_noise_body(float* __restrict__ x0, float* __restrict__ x, int64_t T, int XR,
                                      uint64_t seed, int gauss, int bx, int b) {
    const int64_t i4 = (int64_t)bx * blockDim.x + threadIdx.x;
    if (i4 * 4 >= T) return;
    float v[4];
    iaf_noise_draw(i4, b, seed, gauss, v);
    *reinterpret_cast<f4*>(x0 + (size_t)b * T + i4 * 4) = (f4){v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f4*>(x + (size_t)b * XR + IAF_XP + i4 * 4) = (f4){v[0], v[1], v[2], v[3]};
}

__device__ inline void iaf_copy_noise_body(const float* __restrict__ noise, float* __restrict__ x, int64_t T, int XR,
                                           int bx, int b) {
    const int64_t i4 = (int64_t)bx * blockDim.x + threadIdx.x;
    if (i4 * 4 >= T) return;
    *reinterpret_cast<f4*>(x + (size_t)b * XR + IAF_XP + i4 * 4) =
        *reinterpret_cast<const f4*>(noise + (size_t)b * T + i4 * 4);
}

// zero the left pads (pad floats, row stride rs) of both activation buffers and of the flow input, one launch (bz picks)
// dl_rj > 0: lB holds the DL layout of wn_iaf_g.hip (32 residue rows of dl_rj 16-byte words per group row, 64 zero
// words in front of each) instead of one left pad per row
__device__ inline void zero_pads_body(float* __restrict__ lA, float* __restrict__ lB, int64_t rs, int pad, int rows,
                                      float* __restrict__ x, int64_t xrs, int xpad, int xrows, unsigned* __restrict__ status,
                                      int dl_rj, int bx, int by, int bz, int gy) {
    const int c = bx * blockDim.x + threadIdx.x;
    if (by == 0 && c == 0 && bz == 0) *status = 0u;  // range-guard word of this call (wn_codec.h)
    // grid.y is capped (65 535 rows per launch dimension): rows are walked
    for (int row = by; row < max(rows, xrows); row += gy) {
        if (bz < 2) {
            float* p = bz ? lB : lA;
            if (bz == 1 && dl_rj > 0) {
                // 32 x 64 words x 4 floats = pad floats again: float c -> residue c / 256, float c % 256 of its pad
                if (row < rows && c < pad) p[(size_t)row * rs + (size_t)(c >> 8) * dl_rj * 4 + (c & 255)] = 0.f;
            } else if (row < rows && c < pad) p[(size_t)row * rs + c] = 0.f;
        } else if (row < xrows && c < xpad) {
            x[(size_t)row * xrs + c] = 0.f;
        }
    }
}

// The call's prologue as ONE launch (round 5): the zero pads and the flow input (noise drawn here, or the caller's copied)
// are independent element-wise jobs of a few microseconds each; a 1-D grid holds the blocks of both, pads first.
struct PrologueArgs {
    float *lA, *lB, *x, *x0g;
    const float* noise;
    unsigned* status;
    int64_t rs, xrs, T;
    uint64_t seed;
    int pad, rows, xpad, xrows, dl_rj, pgx, pgy, npad, ngx, XR, gauss;
};
__global__ void iaf_prologue_kernel(const PrologueArgs A) {
    const int bid = blockIdx.x;
    if (bid < A.npad) {
        const int bx = bid % A.pgx, by = (bid / A.pgx) % A.pgy, bz = bid / (A.pgx * A.pgy);
        zero_pads_body(A.lA, A.lB, A.rs, A.pad, A.rows, A.x, A.xrs, A.xpad, A.xrows, A.status, A.dl_rj, bx, by, bz, A.pgy);
    } else {
        const int nb = bid - A.npad, bx = nb % A.ngx, b = nb / A.ngx;
        if (A.noise) iaf_copy_noise_body(A.noise, A.x, A.T, A.XR, bx, b);
        else iaf_noise_body(A.x0g, A.x, A.T, A.XR, A.seed, A.gauss, bx, b);
    }
}

// ---------------- final affine + _clip_quant_scale (parallel_wavenet.py:326-330,347-359) ----------------
__device__ inline void clip_quant_one(float y, int Q, int mu, float& wav, int& qi) {
    qi = wn_clip_quantize(y, Q);
    wav = wn_dequant(qi, Q, mu);
}

// One output element of a call: the scale clamp, y = x0 s + m, _clip_quant_scale; m and s leave as the totals handed out.
// bad: a split-fp16 operand left the fp16 range somewhere in this call (wn_codec.h), so whatever the flows computed after
// that is not the reference's result.  Never hand it out as audio -- every float output becomes NaN, the index 0;
// wn_iaf_range_status() reports WN_ERANGE and the caller re-runs the call with wn_iaf_generate_form(h, WN_FORM_F32, ...).
__device__ inline void iaf_final_one(float x0, float& m, float& s, bool bad, int Q, int mu, float& w, float& y, int& qi) {
    s = fminf(s, EXP_7);                                    // :327
    y = x0 * s + m;                                         // :330
    clip_quant_one(y, Q, mu, w, qi);
    if (bad) { w = y = m = s = __builtin_nanf(""); qi = 0; }
}

__global__ void iaf_final_kernel(const float* __restrict__ x0, const float* __restrict__ Mt,
                                 const float* __restrict__ St, int64_t n, int Q, int mu,
                                 float* __restrict__ wav, int* __restrict__ idx, float* __restrict__ xraw,
                                 float* __restrict__ mean_tot, float* __restrict__ scale_tot,
                                 unsigned* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool bad = *status != 0u;                         // the call's range flag: iaf_final_one
    // status[1] accumulates over the calls made on this workspace (the prologue, zero_pads_body, clears status[0] only): a caller
    // that keeps a run of calls asynchronous asks ONCE at the end (wn_iaf_range_status_since_reset)
    if (bad && i == 0) atomicOr(status + 1, *status);
    float s = St[i], m = Mt[i], w, y;
    int qi;
    iaf_final_one(x0[i], m, s, bad, Q, mu, w, y, qi);
    wav[i] = w;
    if (idx) idx[i] = qi;
    if (xraw) xraw[i] = y;
    if (mean_tot) mean_tot[i] = m;
    if (scale_tot) scale_tot[i] = s;
}

__global__ void clip_quant_kernel(const float* __restrict__ x, int64_t n, int Q, int mu,
                                  float* __restrict__ wav, int* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float w; int qi;
    clip_quant_one(x[i], Q, mu, w, qi);
    if (wav) wav[i] = w;
    if (idx) idx[i] = qi;
}

// ---------------- the back of an encode sweep (wn_iaf_encode) ----------------
// iaf_final_kernel's counterpart for the inverse direction: z' = (x - Mt) / min(St, e^7), non-finite -> 0, clamped to
// +-z_max, written over z.  A thread owns one quad of a row (16-byte accesses where T and the pointers allow, vec), a
// workgroup 1024 samples.  The row's front -- the first sample the sweep changed by more than tol -- is a per-block minimum
// here (a wave butterfly, then the waves in order) into part[0][b][bx], the clamp count likewise into part[1][b][bx];
// iaf_encode_reduce_kernel folds them.  No atomics but the range flag, no initialisation between sweeps.
constexpr int ENC_BLOCK = 1024;      // samples of a row per workgroup of iaf_encode_back_kernel

struct EncBackArgs {
    const float *x, *Mt, *St;                                // [B][T]
    float *z, *mean_tot, *scale_tot;                         // [B][T]; z read and written
    int64_t T;
    float z_max, tol;
    int vec, nblk;
    int* part;                                               // [2][B][nblk]
    const unsigned* status;                                  // the sweep's range word (wn_codec.h)
    int* counts;                                             // counts[1]: OR of the range words of the call's sweeps
};

__global__ __launch_bounds__(256) void iaf_encode_back_kernel(const EncBackArgs A) {
    // an earlier sweep of this call met the stop condition (iaf_encode_reduce_kernel): z, the totals and the partials stay
    // those of that sweep, so what the call hands out belongs to the sweep counts[2] names -- with tol > 0 a later sweep
    // could move a sample by more than tol again
    if (A.counts[2] != 0) return;
    const int b = blockIdx.y;
    const int64_t t0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4, row = (int64_t)b * A.T;
    // a split-fp16 operand left the fp16 range in this sweep: Mt and St are not the reference's.  z stays as it is (the
    // caller goes on from it on the fp32 form), nothing counts as converged, and the totals handed out are NaN
    const bool bad = *A.status != 0u;
    if (bad && b == 0 && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(reinterpret_cast<unsigned*>(A.counts) + 1, *A.status);
    int fr = 0x7fffffff, nc = 0;
    if (t0 < A.T) {
        const int n = (int)(A.T - t0 < 4 ? A.T - t0 : 4);
        float xv[4], mv[4], sv[4], zo[4], zn[4];
        if (A.vec) {
            const f4 a = *reinterpret_cast<const f4*>(A.x + row + t0), m = *reinterpret_cast<const f4*>(A.Mt + row + t0),
                     s = *reinterpret_cast<const f4*>(A.St + row + t0), z = *reinterpret_cast<const f4*>(A.z + row + t0);
#pragma unroll
            for (int e = 0; e < 4; ++e) { xv[e] = a[e]; mv[e] = m[e]; sv[e] = s[e]; zo[e] = z[e]; }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool in = e < n;
                xv[e] = in ? A.x[row + t0 + e] : 0.f;
                mv[e] = in ? A.Mt[row + t0 + e] : 0.f;
                sv[e] = in ? A.St[row + t0 + e] : 1.f;
                zo[e] = in ? A.z[row + t0 + e] : 0.f;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sv[e] = fminf(sv[e], EXP_7);                     // parallel_wavenet.py:327
            float v = (xv[e] - mv[e]) / sv[e];
            if (!(fabsf(v) <= 3.0e38f)) v = 0.f;             // NaN or +-inf
            if (e < n && fabsf(v) > A.z_max) { v = copysignf(A.z_max, v); ++nc; }
            const bool moved = A.tol == 0.f ? __float_as_uint(v) != __float_as_uint(zo[e]) : !(fabsf(v - zo[e]) <= A.tol);
            if (e < n && (moved || bad)) fr = min(fr, (int)(t0 + e));
            zn[e] = v;
            if (bad) mv[e] = sv[e] = __builtin_nanf("");
        }
        if (bad) nc = 0;
        if (A.vec) {
            if (!bad) *reinterpret_cast<f4*>(A.z + row + t0) = (f4){zn[0], zn[1], zn[2], zn[3]};
            if (A.mean_tot) *reinterpret_cast<f4*>(A.mean_tot + row + t0) = (f4){mv[0], mv[1], mv[2], mv[3]};
            if (A.scale_tot) *reinterpret_cast<f4*>(A.scale_tot + row + t0) = (f4){sv[0], sv[1], sv[2], sv[3]};
        } else {
            for (int e = 0; e < n; ++e) {
                if (!bad) A.z[row + t0 + e] = zn[e];
                if (A.mean_tot) A.mean_tot[row + t0 + e] = mv[e];
                if (A.scale_tot) A.scale_tot[row + t0 + e] = sv[e];
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        fr = min(fr, __shfl_xor(fr, o));
        nc += __shfl_xor(nc, o);
    }
    __shared__ int sh[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { sh[0][wave] = fr; sh[1][wave] = nc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const size_t i = (size_t)b * A.nblk + blockIdx.x;
        A.part[i] = min(min(sh[0][0], sh[0][1]), min(sh[0][2], sh[0][3]));
        A.part[(size_t)gridDim.y * A.nblk + i] = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
    }
}

// One workgroup: front[b] = min over the row's block minima (T where nothing moved), counts[0] = the sweep's clamp count,
// counts[2] = the first sweep of the call (from 1) after which every front was T and nothing was clamped.  Wave w takes the
// rows w, w + 4, ...; its lanes stride the row's partials.
__global__ __launch_bounds__(256) void iaf_encode_reduce_kernel(const int* __restrict__ part, int B, int nblk, int T, int sweep,
                                                                int* __restrict__ front, int* __restrict__ counts) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int nc = 0, open = 0;                                    // clamped elements / rows whose front is not T, of this wave's rows
    for (int b = wave; b < B; b += 4) {
        int fr = T;
        for (int i = lane; i < nblk; i += 64) {
            fr = min(fr, part[(size_t)b * nblk + i]);
            nc += part[(size_t)B * nblk + (size_t)b * nblk + i];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) fr = min(fr, __shfl_xor(fr, o));
        if (lane == 0) front[b] = fr;
        open += fr != T;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nc += __shfl_xor(nc, o);
    __shared__ int sh[2][4];
    if (lane == 0) { sh[0][wave] = nc; sh[1][wave] = open; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int c = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
        counts[0] = c;
        if (c == 0 && sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3] == 0 && counts[2] == 0) counts[2] = sweep + 1;
    }
}

// log p(x) = log f(z) - log scale_tot (wn_iaf_latent_log_prob), one workgroup per row.  Evaluated in double and rounded
// once; the row sum is taken as the distillation kernels take theirs (wn_distill.hip): double, each thread its quads in
// order, a wave butterfly, then the waves in order.
__global__ __launch_bounds__(256) void iaf_latent_log_prob_kernel(const float* __restrict__ z, const float* __restrict__ st,
                                                                  int64_t T, int gauss, int vec, float* __restrict__ lp,
                                                                  double* __restrict__ row_sums) {
    const int64_t row = (int64_t)blockIdx.x * T;
    double acc = 0.0;
    for (int64_t t0 = (int64_t)threadIdx.x * 4; t0 < T; t0 += 1024) {
        const int n = (int)(T - t0 < 4 ? T - t0 : 4);
        float zv[4], sv[4], out[4];
        if (vec) {
            const f4 a = *reinterpret_cast<const f4*>(z + row + t0), s = *reinterpret_cast<const f4*>(st + row + t0);
#pragma unroll
            for (int e = 0; e < 4; ++e) { zv[e] = a[e]; sv[e] = s[e]; }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                zv[e] = e < n ? z[row + t0 + e] : 0.f;
                sv[e] = e < n ? st[row + t0 + e] : 1.f;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double zd = (double)zv[e];
            // Logistic(0,1): -z - 2 softplus(-z), softplus(y) = max(y, 0) + log1p(exp(-|y|)); Normal(0,1)
            const double lf = gauss ? -0.5 * zd * zd - 0.9189385332046727 : -zd - 2.0 * (fmax(-zd, 0.0) + log1p(exp(-fabs(zd))));
            out[e] = (float)(lf - log((double)sv[e]));
            if (e < n) acc += (double)out[e];
        }
        if (lp) {
            if (vec) *reinterpret_cast<f4*>(lp + row + t0) = (f4){out[0], out[1], out[2], out[3]};
            else for (int e = 0; e < n; ++e) lp[row + t0 + e] = out[e];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    __shared__ double sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && row_sums) row_sums[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// ---------------- windowed generation (wn_iaf_generate_windows) ----------------
// Row r of a window call is an ordinary row of T samples whose local sample t is sample t_origin + t of utterance b.
// Prologue: iaf_prologue_kernel's two jobs with the noise taken at ABSOLUTE positions -- Philox counter (t_origin / 4 + i4, b),
// the one-shot's counter words (t_origin is a multiple of 4), or the caller's noise_abs [B_out][T_out] at t_origin + t, 0
// outside it.  Both forms also fill the x0 rows, which the final kernel reads.
struct WinPrologueArgs {
    PrologueArgs P;
    const wn_iaf_window_row* rows;
    const float* noise_abs;
    int64_t T_out;
};
__global__ void iaf_window_prologue_kernel(const WinPrologueArgs W) {
    const PrologueArgs& A = W.P;
    const int bid = blockIdx.x;
    if (bid < A.npad) {
        const int bx = bid % A.pgx, by = (bid / A.pgx) % A.pgy, bz = bid / (A.pgx * A.pgy);
        zero_pads_body(A.lA, A.lB, A.rs, A.pad, A.rows, A.x, A.xrs, A.xpad, A.xrows, A.status, A.dl_rj, bx, by, bz, A.pgy);
        return;
    }
    const int nb = bid - A.npad, bx = nb % A.ngx, r = nb / A.ngx;
    const int64_t i4 = (int64_t)bx * blockDim.x + threadIdx.x;
    if (i4 * 4 >= A.T) return;
    const int b = W.rows[r].b;
    const int64_t g = W.rows[r].t_origin + i4 * 4;           // absolute position of the thread's first sample
    float v[4];
    if (!W.noise_abs) {
        iaf_noise_draw(g >> 2, b, A.seed, A.gauss, v);
    } else {
        const float* np = W.noise_abs + (size_t)b * W.T_out;
        if (g >= 0 && g + 4 <= W.T_out && ((W.T_out | g) & 3) == 0) {      // 16-byte aligned and inside
            const f4 w = *reinterpret_cast<const f4*>(np + g);
            v[0] = w[0]; v[1] = w[1]; v[2] = w[2]; v[3] = w[3];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (g + e >= 0 && g + e < W.T_out) ? np[g + e] : 0.f;
        }
    }
    *reinterpret_cast<f4*>(A.x0g + (size_t)r * A.T + i4 * 4) = (f4){v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f4*>(A.x + (size_t)r * A.XR + IAF_XP + i4 * 4) = (f4){v[0], v[1], v[2], v[3]};
}

// Final kernel: iaf_final_kernel's arithmetic over the KEPT columns [keep_from, keep_to) of every row, stored at
// out[b][out_t + (t - keep_from)].  A thread owns one 16-byte-aligned quad of the OUTPUT row: whole quads leave as one
// 16-byte store per output (vec: every output pointer and T_out allow it), the ragged first / last quad element by element;
// the inputs are read 16 bytes at a time where the row's source columns happen to be aligned like its destination.
struct WinFinalArgs {
    const wn_iaf_window_row* rows;
    const float *x0, *Mt, *St;                               // [R][T]
    int64_t T, T_out;
    int Q, mu, vec;
    float *wav, *xraw, *mean_tot, *scale_tot, *rand_out;     // [B_out][T_out]
    int* idx;
    unsigned* status;
};
__global__ void iaf_window_final_kernel(const WinFinalArgs A) {
    const int r = blockIdx.y;
    const wn_iaf_window_row row = A.rows[r];
    const int64_t n = row.keep_to - row.keep_from;
    const int64_t e0 = (int64_t)row.b * A.T_out + row.out_t;                 // output element of the first kept column
    const int64_t k0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4 - (e0 & 3);   // first kept column of this quad
    const bool bad = *A.status != 0u;                                        // as iaf_final_kernel: NaN, never saturated audio
    if (bad && r == 0 && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(A.status + 1, *A.status);
    if (k0 >= n) return;
    const int64_t src = (int64_t)r * A.T + row.keep_from + k0, dst = e0 + k0;
    const bool full = k0 >= 0 && k0 + 4 <= n;
    float x0v[4], mv[4], sv[4];
    if (full && (src & 3) == 0) {
        const f4 a = *reinterpret_cast<const f4*>(A.x0 + src), m = *reinterpret_cast<const f4*>(A.Mt + src),
                 s = *reinterpret_cast<const f4*>(A.St + src);
#pragma unroll
        for (int e = 0; e < 4; ++e) { x0v[e] = a[e]; mv[e] = m[e]; sv[e] = s[e]; }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool in = k0 + e >= 0 && k0 + e < n;
            x0v[e] = in ? A.x0[src + e] : 0.f;
            mv[e] = in ? A.Mt[src + e] : 0.f;
            sv[e] = in ? A.St[src + e] : 0.f;
        }
    }
    f4 w, y, m, s, x0o;
    int q4[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float se = sv[e], me = mv[e], we, ye;
        int qi;
        iaf_final_one(x0v[e], me, se, bad, A.Q, A.mu, we, ye, qi);
        w[e] = we; y[e] = ye; m[e] = me; s[e] = se; q4[e] = qi; x0o[e] = x0v[e];
    }
    if (full && A.vec) {
        *reinterpret_cast<f4*>(A.wav + dst) = w;
        if (A.idx) *reinterpret_cast<int4*>(A.idx + dst) = make_int4(q4[0], q4[1], q4[2], q4[3]);
        if (A.xraw) *reinterpret_cast<f4*>(A.xraw + dst) = y;
        if (A.mean_tot) *reinterpret_cast<f4*>(A.mean_tot + dst) = m;
        if (A.scale_tot) *reinterpret_cast<f4*>(A.scale_tot + dst) = s;
        if (A.rand_out) *reinterpret_cast<f4*>(A.rand_out + dst) = x0o;
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (k0 + e < 0 || k0 + e >= n) continue;
        A.wav[dst + e] = w[e];
        if (A.idx) A.idx[dst + e] = q4[e];
        if (A.xraw) A.xraw[dst + e] = y[e];
        if (A.mean_tot) A.mean_tot[dst + e] = m[e];
        if (A.scale_tot) A.scale_tot[dst + e] = s[e];
        if (A.rand_out) A.rand_out[dst + e] = x0o[e];
    }
}

struct IafLayout {
    int64_t T, TE, RS;
    int XR, c0;
    size_t status, enc, lA, lB, x, x0, M, S, C, scratch, total;   // byte offsets
    int64_t c_bstride;                                    // floats of hoisted conditioning per batch row
    int form;                                             // WN_COND_FUSED / WN_COND_HOISTED for this call
};

IafLayout iaf_layout(const wn_handle* h, int B, int F, int form) {
    IafLayout L;
    L.T = wn_iaf_length(h, F);
    L.TE = (int64_t)F * h->frame_shift;
    L.c0 = (int)((L.TE - L.T) / 2);                        // wavenet.py:76-85
    L.RS = IAF_LP + L.T;
    L.XR = (int)(IAF_XP + L.T);
    size_t o = 0;
    auto carve = [&](size_t floats) { size_t r = o; o += align_up(floats * sizeof(float), 256); return r; };
    L.form = wn_iaf_form(h, B, L.T, form);
    L.status = carve(64);                                  // range-guard word: first bytes of the workspace
    // the generic student (wn_iaf_x.hip) keeps fp32 rows of the model's own widths (wn_iaf_form: never hoisted)
    const size_t W = h->generic_student ? h->cfg.width : IAF_W, Cd = h->generic_student ? h->cfg.deconv_width : IAF_CD;
    L.enc = carve((size_t)B * Cd * L.TE + 64);
    L.lA = carve((size_t)B * W * L.RS);
    L.lB = carve((size_t)B * W * L.RS);
    L.x = carve((size_t)2 * B * L.XR);      // flow input and, for flows that are ONE layer group, a second copy (wn_iaf_g.hip)
    L.x0 = carve((size_t)B * L.T);
    L.M = carve((size_t)B * L.T);
    L.S = carve((size_t)B * L.T);
    const bool hoist = L.form == WN_COND_HOISTED;
    L.c_bstride = hoist ? (int64_t)wn_iaf_c_floats(h->cfg.share_deconv ? h->cond_rows : 0, L.T) : 0;
    if (hoist && !h->cfg.share_deconv) {        // private deconv stacks: one flow's rows at a time
        int mx = 0;
        for (const IafFlowPack& fp : h->flows) mx = std::max(mx, (int)fp.layers.size() + 1);
        L.c_bstride = (int64_t)wn_iaf_c_floats(mx, L.T);
    }
    L.C = carve((size_t)B * L.c_bstride);
    L.scratch = o;
    o += wn_deconv_scratch_bytes(h, B, F);
    L.total = o;
    return L;
}

// ---------------------------------------------------------------------------
// One generate call.  An entry point (wn_iaf_generate_form, wn_iaf_generate_windows) refuses what it refuses and then walks
//   iaf_call_fill   the IafCall, once: workspace pointers, sizes, the switches in force, the flow runner
//   its front       pads + flow input, one launch (iaf_prologue_kernel / iaf_window_prologue_kernel)
//   iaf_call_body   per flow [upsampler + conditioning GEMM where due, the flow runner of the call's launch form]
//   its back        final kernel (iaf_final_kernel / iaf_window_final_kernel)
//   iaf_call_close
// The form is chosen once per call (iaf_runner); no runner tests precision, conditioning placement or group use inside its
// layer loop.

constexpr size_t MAX_PART_EVENTS = 4096;   // a power loop of thousands of calls stops recording, not allocating

struct IafCall;
using IafRunner = int (*)(IafCall&, int, const float*);

struct IafCall {
    wn_handle* h;
    IafLayout L;
    int B, F;
    const float* mel;
    hipStream_t st;
    float *enc, *lA, *lB, *x0g, *Mt, *St, *Cc;
    float *xbuf0, *x;                  // the two copies of the flow input start at xbuf0; x is the one in force (run_groups)
    unsigned* status;
    void* scratch;
    int prec;                          // WN_PREC_* of this call
    bool f16x3, hoist, use_groups;
    size_t rb_floats;                  // C floats of one row block
    IafRunner run_flow;
    // switches, each read ONCE at the call's entry
    bool prof_on, parts_on;
    int pmask;                         // parts the call runs: a restriction exists only inside a parts session (wn_profile_parts_only)
    bool no_pair, no_headfuse;         // WN_NO_PAIR / WN_NO_HEADFUSE (cross-form tests): no two-layer launches / no head in a last layer
    // wn_iaf_encode: the body leaves out the upsampler and the conditioning GEMM of a SHARED deconv stack -- enc and C in the
    // workspace are those of an earlier sweep of the same encode.  Generate calls never set it.
    bool skip_front;
    // measurement state
    int part_now = -2;
    bool prof_open = false;

    int record(std::vector<hipEvent_t>& list, int tag) {
        hipEvent_t ev;
        WN_HIP(h, hipEventCreate(&ev));
        {
            std::lock_guard<std::mutex> g(h->list_mu);
            list.push_back(ev);
            if (&list == &h->part_events) h->part_tags.push_back(tag);
        }
        WN_HIP(h, hipEventRecord(ev, st));
        return WN_OK;
    }
    // measurement aid (wn_profile_parts_begin): an event where a part of the call begins.  Parts: 0 prologue / epilogue
    // (pads, noise, final), 1 upsampler, 2 conditioning GEMM, 3 residual stack (start convs, layers, heads)
    int part(int tag) {
        if (!parts_on || tag == part_now) return WN_OK;
        part_now = tag;
        {
            std::lock_guard<std::mutex> g(h->list_mu);
            if (h->part_events.size() >= MAX_PART_EVENTS) return WN_OK;
        }
        return record(h->part_events, tag);
    }
    // bench.py measurement aid: event pairs around every maximal run of single-layer launches (the dominant kernel);
    // two-layer launches and heads stay outside the brackets
    int prof_mark(bool open, int launches) {
        if (!prof_on) return WN_OK;
        if (open != prof_open) {
            if (int rc = record(h->prof_events, 0)) return rc;
            prof_open = open;
        }
        if (open) {
            std::lock_guard<std::mutex> g(h->list_mu);
            h->prof_launches += launches;
        }
        return WN_OK;
    }
    const unsigned* blob_u(size_t off) const { return reinterpret_cast<const unsigned*>(h->d_blob + off); }
};

// prologue: zero left pads + the flow input (drawn on the device, or the caller's noise), one launch
void iaf_prologue_args(const IafCall& c, const float* noise, uint64_t seed, PrologueArgs& A) {
    const IafLayout& L = c.L;
    // G4 layout (f16x3) and the Q4 rows of the hoisted fp32 form: 16 interleaved group rows per batch element, each
    // 4*(LP+T) words; fused fp32 form and the generic student: planar rows, one per channel
    const bool rows16 = c.f16x3 || c.hoist;
    A.rows = rows16 ? c.B * 16 : c.B * c.h->cfg.width;
    A.rs = rows16 ? 4 * L.RS : L.RS;
    A.pad = rows16 ? 4 * IAF_LP : IAF_LP;
    A.lA = c.lA; A.lB = c.lB; A.x = c.x; A.x0g = c.x0g; A.noise = noise; A.status = c.status;
    A.xrs = (int64_t)L.XR; A.xpad = IAF_XP; A.xrows = 2 * c.B;
    A.dl_rj = c.use_groups ? 64 + (int)(L.T / 32) : 0;
    A.pgx = (A.pad + 255) / 256;
    A.pgy = std::min(std::max(A.rows, 2 * c.B), 32768);
    A.npad = A.pgx * A.pgy * 3;
    A.T = L.T; A.XR = L.XR; A.seed = seed; A.gauss = c.h->cfg.loss_type == WN_LOSS_GAUSS ? 1 : 0;
    A.ngx = (int)((L.T / 4 + 255) / 256);
}
void iaf_prologue(const IafCall& c, const float* noise, uint64_t seed) {
    PrologueArgs A{};
    iaf_prologue_args(c, noise, seed, A);
    hipLaunchKernelGGL(iaf_prologue_kernel, dim3((unsigned)(A.npad + A.ngx * c.B)), dim3(256), 0, c.st, A);
}

// Upsampler of deconv stack si, then (hoisted forms) the conditioning GEMM of its R row blocks, which start at row block
// rb0 of the student's tables; order / n_nat: wn_iaf_c_cond.  Once per call for a shared stack, once per flow otherwise.
int iaf_upsample_cond(IafCall& c, int si, int rb0, int R, const unsigned* order, int n_nat) {
    wn_handle* h = c.h;
    const IafLayout& L = c.L;
    if (int rc = c.part(1)) return rc;
    if (c.pmask & 2)
        if (int rc = wn_run_deconv(h, si, c.mel, c.B, c.F, c.enc, L.TE, c.scratch, c.st, c.f16x3, c.status, c.prec)) return rc;
    if (!c.hoist) return WN_OK;
    if (int rc = c.part(2)) return rc;
    if (!(c.pmask & 4)) return WN_OK;
    if (c.f16x3)
        wn_iaf_c_cond(c.enc, h->d_blob, c.blob_u(h->cond_tab_off) + rb0, order, n_nat, c.Cc, L.c_bstride, L.TE, L.c0, R, c.B,
                      L.T, h->num_cu, c.st);
    else
        wn_iaf_f_cond(h, c.enc, c.blob_u(h->cond_tab_f_off) + 2 * rb0, R, c.Cc, L.c_bstride, L.TE, L.c0, c.B, L.T, c.st);
    return WN_OK;
}

// ---- flow runners: flow k from the start conv to the head, one per launch form.  Cf: the flow's row blocks inside C ----

// Layer groups (wn_iaf_g.hip): natural / decimated layer groups in LDS: lA natural, lB DL; the first group computes the
// start conv from x, the last one runs the flow head
int run_groups(IafCall& c, int k, const float* Cf) {
    wn_handle* h = c.h;
    const IafLayout& L = c.L;
    const IafFlowPack& fp = h->flows[k];
    float* gin = c.lA;
    float* gout = c.lB;
    if (c.prof_on) if (int rc = c.record(h->prof_events, 0)) return rc;
    for (size_t gi = 0; gi < fp.groups.size(); ++gi) {
        const WnGroup& g = fp.groups[gi];
        const bool lastg = gi + 1 == fp.groups.size();
        // a flow that is ONE group reads x (start conv, with its halo) and writes x (head) in the same launch:
        // the new x goes to the other copy, which becomes the flow input from then on
        float* xnew = (gi == 0 && lastg) ? (c.x == c.xbuf0 ? c.xbuf0 + (size_t)c.B * L.XR : c.xbuf0) : c.x;
        wn_iaf_g_run(h, g, fp.layers.data(), Cf + (size_t)g.begin * c.rb_floats, c.rb_floats, L.c_bstride, gin, gout, L.RS,
                     lastg ? 0 : fp.groups[gi + 1].kind, c.B, L.T, gi == 0 ? c.x : nullptr, L.XR, h->d_blob + fp.start_off,
                     lastg, h->d_blob + fp.head_off_h, c.x, xnew, c.Mt, c.St, k == 0 ? 1 : 0, c.status, c.st);
        c.x = xnew;
        std::swap(gin, gout);
    }
    if (c.prof_on) {
        if (int rc = c.record(h->prof_events, 0)) return rc;
        std::lock_guard<std::mutex> g(h->list_mu);
        h->prof_launches += (int64_t)fp.groups.size();
    }
    return WN_OK;
}

// Split-fp16, hoisted conditioning, per-layer launches (wn_iaf_c.hip): layer pairs with small dilations run as one launch,
// and when the flow starts with such a pair the start conv runs inside it; the last layer, unless a pair took it, carries
// the head.  Pairs never overlap (the second layer of one has dilation 2 or 8, the first 1 or 4), so pair_at is exact.
int run_f16x3_hoisted(IafCall& c, int k, const float* Cf) {
    const wn_handle* h = c.h;
    const IafLayout& L = c.L;
    const IafFlowPack& fp = h->flows[k];
    const size_t n = fp.layers.size();
    const int first = k == 0 ? 1 : 0;
    auto pair_at = [&](size_t i) {
        return !c.no_pair && i + 1 < n && wn_iaf_c_pair_ok(fp.layers[i].dilation, fp.layers[i + 1].dilation);
    };
    const bool pair_start = pair_at(0) && fp.layers[0].dilation == 1;
    const bool head_in_last = n > 0 && !c.no_headfuse && !(n >= 2 && pair_at(n - 2));
    const size_t n_plain = head_in_last ? n - 1 : n;      // layers launched without the head
    if (!pair_start) wn_iaf_h_start(c.x, h->d_blob + fp.start_off, c.lA, L.T, L.XR, L.RS, c.B, c.st, c.status);
    float* lin = c.lA;
    float* lout = c.lB;
    for (size_t i = 0; i < n_plain;) {
        const IafLayerPack& lp = fp.layers[i];
        const float* Ci = Cf + i * c.rb_floats;
        if (pair_at(i)) {
            const IafLayerPack& lq = fp.layers[i + 1];
            if (int rc = c.prof_mark(false, 0)) return rc;
            wn_iaf_c_pair(lin, lout, Ci, Ci + c.rb_floats, L.c_bstride, h->d_blob + lp.off_h, h->d_blob + lq.off_h, L.RS,
                          lp.dilation, lq.dilation, c.B, L.T, h->num_cu, c.st, (i == 0 && pair_start) ? c.x : nullptr, L.XR,
                          h->d_blob + fp.start_off, c.status);
            i += 2;
        } else {
            if (int rc = c.prof_mark(true, 1)) return rc;
            wn_iaf_c_layer(lin, lout, Ci, L.c_bstride, h->d_blob + lp.off_h, L.RS, lp.dilation, c.B, L.T, h->num_cu, c.st,
                           c.status);
            ++i;
        }
        std::swap(lin, lout);
    }
    if (int rc = c.prof_mark(false, 0)) return rc;
    const float* Ch = Cf + n * c.rb_floats;
    if (head_in_last)
        wn_iaf_c_layer_head(lin, Ch - c.rb_floats, Ch, L.c_bstride, h->d_blob + fp.layers[n - 1].off_h,
                            h->d_blob + fp.head_off_h, c.x, c.Mt, c.St, L.RS, L.XR, fp.layers[n - 1].dilation, first, c.B, L.T,
                            h->num_cu, c.st, c.status);
    else
        wn_iaf_c_head(lin, Ch, L.c_bstride, h->d_blob + fp.head_off_h, c.x, c.Mt, c.St, L.RS, L.XR, L.T, first, c.B,
                      h->num_cu, c.st);
    return WN_OK;
}

// Split-fp16, conditioning fused into every layer (wn_iaf_h.hip): the start conv runs inside the first layer kernel of the
// flow when its dilation is 1
int run_f16x3_fused(IafCall& c, int k, const float*) {
    const wn_handle* h = c.h;
    const IafLayout& L = c.L;
    const IafFlowPack& fp = h->flows[k];
    const bool fuse_start = !fp.layers.empty() && fp.layers[0].dilation == 1;
    if (!fuse_start) wn_iaf_h_start(c.x, h->d_blob + fp.start_off, c.lA, L.T, L.XR, L.RS, c.B, c.st, c.status);
    float* lin = c.lA;
    float* lout = c.lB;
    for (size_t i = 0; i < fp.layers.size(); ++i) {
        const IafLayerPack& lp = fp.layers[i];
        if (int rc = c.prof_mark(true, 1)) return rc;
        wn_iaf_h_layer(lin, lout, c.enc, h->d_blob + lp.off_h, L.RS, L.TE, L.c0, lp.dilation, c.B, L.T, h->num_cu, c.st,
                       c.status, (i == 0 && fuse_start) ? c.x : nullptr, L.XR, h->d_blob + fp.start_off);
        std::swap(lin, lout);
    }
    if (int rc = c.prof_mark(false, 0)) return rc;
    wn_iaf_h_head(lin, c.enc, h->d_blob + fp.head_off_h, c.x, c.Mt, c.St, L.RS, L.TE, L.c0, L.XR, L.T, k == 0 ? 1 : 0, c.B,
                  h->num_cu, c.st);
    return WN_OK;
}

// fp32, hoisted conditioning: the last layer of the flow carries the head in its epilogue (iaf_layer_kernel<true, true>);
// with at least two layers and a first dilation of 1 the start conv runs in front of the first one (<true, false, true>)
int run_f32_hoisted(IafCall& c, int k, const float* Cf) {
    const wn_handle* h = c.h;
    const IafLayout& L = c.L;
    const IafFlowPack& fp = h->flows[k];
    const size_t n = fp.layers.size();
    const int first = k == 0 ? 1 : 0;
    const bool start_in_layer = n >= 2 && fp.layers[0].dilation == 1;
    if (!start_in_layer) wn_iaf_f32_start(c.x, h->d_blob + fp.start_off, c.lA, L.T, L.XR, L.RS, c.B, true, c.st);
    float* lin = c.lA;
    float* lout = c.lB;
    for (size_t i = 0; i + 1 < n; ++i) {
        if (int rc = c.prof_mark(true, 1)) return rc;
        wn_iaf_f32_layer_c(lin, lout, Cf + i * c.rb_floats, L.c_bstride, h->d_blob + fp.layers[i].off, L.RS,
                           fp.layers[i].dilation, c.B, L.T, h->num_cu, c.st, (i == 0 && start_in_layer) ? c.x : nullptr, L.XR,
                           h->d_blob + fp.start_off);
        std::swap(lin, lout);
    }
    const float* Ch = Cf + n * c.rb_floats;
    if (n == 0) {
        wn_iaf_f32_head_c(lin, Ch, L.c_bstride, h->d_blob + fp.head_off, c.x, c.Mt, c.St, L.RS, L.XR, L.T, first, c.B,
                          h->num_cu, c.st);
        return WN_OK;
    }
    // the last layer counts as a single-layer launch and runs outside the brackets, like every launch with a head in it
    if (int rc = c.prof_mark(true, 1)) return rc;
    if (int rc = c.prof_mark(false, 0)) return rc;
    wn_iaf_f32_layer_head(lin, Ch - c.rb_floats, Ch, L.c_bstride, h->d_blob + fp.layers[n - 1].off, h->d_blob + fp.head_off,
                          c.x, c.Mt, c.St, L.RS, L.XR, fp.layers[n - 1].dilation, first, c.B, L.T, h->num_cu, c.st);
    return WN_OK;
}

// fp32, conditioning fused into every layer: start conv, layers and head are one launch each
int run_f32_fused(IafCall& c, int k, const float*) {
    const wn_handle* h = c.h;
    const IafLayout& L = c.L;
    const IafFlowPack& fp = h->flows[k];
    wn_iaf_f32_start(c.x, h->d_blob + fp.start_off, c.lA, L.T, L.XR, L.RS, c.B, false, c.st);
    float* lin = c.lA;
    float* lout = c.lB;
    for (const IafLayerPack& lp : fp.layers) {
        if (int rc = c.prof_mark(true, 1)) return rc;
        wn_iaf_f32_layer(lin, lout, c.enc, h->d_blob + lp.off, L.RS, L.TE, L.c0, lp.dilation, c.B, L.T, h->num_cu, c.st);
        std::swap(lin, lout);
    }
    if (int rc = c.prof_mark(false, 0)) return rc;
    wn_iaf_f32_head(lin, c.enc, h->d_blob + fp.head_off, c.x, c.Mt, c.St, L.RS, L.TE, L.c0, L.XR, L.T, k == 0 ? 1 : 0, c.B,
                    h->num_cu, c.st);
    return WN_OK;
}

// A student whose widths the MFMA kernels are not specialised for: the generic fp32 kernels of wn_iaf_x.hip (fp32 upsampler
// GEMM, one launch per start conv / layer / head, fp32 rows of the model's own widths, no fp16 anywhere)
int run_generic(IafCall& c, int k, const float*) {
    const wn_handle* h = c.h;
    const IafLayout& L = c.L;
    const IafFlowX& fx = h->flows_x[k];
    wn_iaf_x_start(h, fx, c.x, c.lA, L.T, L.XR, L.RS, c.B, c.st);
    float* lin = c.lA;
    float* lout = c.lB;
    for (const IafLayerX& lx : fx.layers) {
        wn_iaf_x_layer(h, lx, lin, lout, c.enc, L.RS, L.TE, L.c0, c.B, L.T, c.st);
        std::swap(lin, lout);
    }
    wn_iaf_x_head(h, fx, lin, c.enc, c.x, c.Mt, c.St, L.RS, L.TE, L.c0, L.XR, L.T, k == 0 ? 1 : 0, c.B, c.st);
    return WN_OK;
}

IafRunner iaf_runner(const IafCall& c) {
    if (c.h->generic_student) return run_generic;
    if (c.use_groups) return run_groups;
    if (c.f16x3) return c.hoist ? run_f16x3_hoisted : run_f16x3_fused;
    return c.hoist ? run_f32_hoisted : run_f32_fused;
}

// The IafCall of `rows` rows of `frames` frames, filled once: the only place that reads the switches and the two environment
// variables, carves the workspace and picks the runner.  form_rows: the row count the group / per-layer size policy is
// evaluated for.  Nothing is dereferenced here: the entry points refuse a null or short workspace afterwards, from c.L.
IafCall iaf_call_fill(wn_handle* h, int form, int rows, int frames, int form_rows, const float* mel, void* ws, void* stream) {
    IafCall c{};
    c.h = h;
    c.prof_on = h->prof_on;
    c.parts_on = h->parts_on;
    c.pmask = c.parts_on ? h->parts_mask : 0xf;
    c.no_pair = getenv("WN_NO_PAIR") != nullptr;
    c.no_headfuse = getenv("WN_NO_HEADFUSE") != nullptr;
    c.L = iaf_layout(h, rows, frames, form);
    const IafLayout& L = c.L;
    const uintptr_t base = reinterpret_cast<uintptr_t>(ws);
    auto at = [base](size_t off) { return reinterpret_cast<float*>(base + off); };
    c.B = rows; c.F = frames; c.mel = mel;
    c.st = reinterpret_cast<hipStream_t>(stream);
    c.enc = at(L.enc); c.lA = at(L.lA); c.lB = at(L.lB); c.x0g = at(L.x0); c.Mt = at(L.M); c.St = at(L.S); c.Cc = at(L.C);
    c.xbuf0 = c.x = at(L.x);
    c.status = reinterpret_cast<unsigned*>(at(L.status));
    c.scratch = at(L.scratch);
    c.prec = h->generic_student ? WN_PREC_F32 : wn_form_precision(h, form);
    c.f16x3 = c.prec == WN_PREC_F16X3;
    c.hoist = L.form == WN_COND_HOISTED;
    c.use_groups = c.f16x3 && wn_iaf_use_groups(h, form_rows, L.T, L.form);
    c.rb_floats = (size_t)(L.T / 16) * 1024;
    c.run_flow = iaf_runner(c);
    return c;
}

// Between a call's front and its back: the upsampler and conditioning GEMM of a shared stack, then per flow those of its
// private stack and the flow runner.  Ends where part 0 (prologue / epilogue) resumes.
int iaf_call_body(IafCall& c) {
    wn_handle* h = c.h;
    const wn_config& cfg = h->cfg;
    if (cfg.share_deconv && !c.skip_front)
        if (int rc = iaf_upsample_cond(c, 0, 0, h->cond_rows, c.blob_u(c.use_groups ? h->order_all_off : h->order_id_off),
                                       c.use_groups ? h->n_nat_all : h->cond_rows))
            return rc;
    for (int k = 0; k < cfg.n_flows; ++k) {
        // the flow's row blocks in the conditioning tables (the generic student has none: it is never hoisted)
        const IafFlowPack* fp = h->generic_student ? nullptr : &h->flows[k];
        const int rb0 = fp ? fp->rb_base : 0, R = fp ? (int)fp->layers.size() + 1 : 0;
        if (!cfg.share_deconv)
            if (int rc = iaf_upsample_cond(c, fp ? fp->deconv_stack : h->flows_x[k].deconv_stack, rb0, R,
                                           c.use_groups ? c.blob_u(h->order_flow_off) + rb0 : c.blob_u(h->order_id_off),
                                           c.use_groups ? h->n_nat_flow[k] : R))
                return rc;
        if (int rc = c.part(3)) return rc;
        if (!(c.pmask & 8)) continue;
        // row blocks of this flow inside C (all flows when the deconv stack is shared)
        if (int rc = c.run_flow(c, k, c.Cc + (cfg.share_deconv ? (size_t)rb0 * c.rb_floats : 0))) return rc;
    }
    return c.part(0);
}

int iaf_call_close(IafCall& c) {
    wn_handle* h = c.h;
    if (int rc = c.part(-1)) return rc;
    if (c.parts_on) {
        std::lock_guard<std::mutex> g(h->list_mu);
        ++h->part_calls;
    }
    WN_HIP(h, hipGetLastError());
    return WN_OK;
}

}  // namespace

extern "C" int wn_iaf_generate(wn_handle* h, const float* mel, int B, int F, const float* noise,
                               uint64_t seed, float* wav, int32_t* idx, float* x_raw, float* mean_tot,
                               float* scale_tot, float* rand_out, void* ws, size_t ws_bytes, void* stream) {
    return wn_iaf_generate_form(h, WN_FORM_DEFAULT, mel, B, F, noise, seed, wav, idx, x_raw, mean_tot, scale_tot, rand_out,
                                ws, ws_bytes, stream);
}

extern "C" int wn_iaf_generate_form(wn_handle* h, int form, const float* mel, int B, int F, const float* noise,
                                    uint64_t seed, float* wav, int32_t* idx, float* x_raw, float* mean_tot,
                                    float* scale_tot, float* rand_out, void* ws, size_t ws_bytes, void* stream) {
    if (!h) return wn_fail(nullptr, WN_EINVAL, "wn_iaf_generate: null handle");
    if (form < WN_FORM_DEFAULT || form > WN_FORM_F16X3_FUSED)
        return wn_fail(h, WN_EINVAL, "wn_iaf_generate_form: unknown form %d", form);
    if (!h->finalized) return wn_fail(h, WN_ESTATE, "wn_iaf_generate: call wn_finalize first");
    if (h->cfg.kind != WN_KIND_STUDENT)
        return wn_fail(h, WN_EINVAL, "wn_iaf_generate: handle is not a ParallelWavenet student");
    if (B < 1 || F < 1) return wn_fail(h, WN_EINVAL, "wn_iaf_generate: B and F must be >= 1");
    // inside the library from here on: the switches (wn_iaf_set_groups, wn_profile_*) are refused until the call returns,
    // and each of them -- the two environment switches included -- is read ONCE, in iaf_call_fill
    const WnWork work(h);
    IafCall c = iaf_call_fill(h, form, B, F, B, mel, ws, stream);
    const IafLayout& L = c.L;
    if (L.T == 0) return WN_OK;   // fewer frames than one max-dilation block: empty output
    if (!mel || !wav || !ws) return wn_fail(h, WN_EINVAL, "wn_iaf_generate: null mel/wav/workspace");
    if (ws_bytes < L.total)
        return wn_fail(h, WN_ENOMEM, "wn_iaf_generate: workspace %zu < %zu bytes", ws_bytes, L.total);
    if ((int64_t)B * L.T / 64 > 0x7fffffff) return wn_fail(h, WN_EINVAL, "wn_iaf_generate: batch too large");
    if (L.TE > WN_MAX_ROW_SAMPLES)   // 32-bit buffer offsets inside one batch element (960 * TE bytes)
        return wn_fail(h, WN_EINVAL, "wn_iaf_generate: %lld samples per utterance exceeds the 2,000,000 "
                       "(125 s) limit of the 32-bit row offsets; split the utterance", (long long)L.TE);

    if (int rc = c.part(0)) return rc;
    iaf_prologue(c, noise, seed);
    if (int rc = iaf_call_body(c)) return rc;
    {
        const wn_config& cfg = h->cfg;
        const float* x0 = noise ? noise : c.x0g;
        const int64_t nn = (int64_t)B * L.T;
        const int Q = cfg.use_mu_law ? 256 : 65536;
        hipLaunchKernelGGL(iaf_final_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, c.st, x0, c.Mt, c.St, nn,
                           Q, cfg.use_mu_law, wav, idx, x_raw, mean_tot, scale_tot, c.status);
        if (rand_out && rand_out != x0)
            WN_HIP(h, hipMemcpyAsync(rand_out, x0, nn * sizeof(float), hipMemcpyDeviceToDevice, c.st));
    }
    return iaf_call_close(c);
}

// ---------------------------------------------------------------------------
// The inverse by fixed-point sweeps: a sweep is a generate call's prologue with noise = z and its body,
// with iaf_encode_back_kernel as the back.  Behind the generate workspace of the call's form: the back kernel's partials.
static int enc_blocks(int64_t T) { return (int)((T + ENC_BLOCK - 1) / ENC_BLOCK); }

static const char* const ENC_NOT_FINALIZED = "call wn_finalize first";

static const char* iaf_encode_refusal(const wn_handle* h, int form, int B, int F) {
    if (!h) return "null handle";
    if (form < WN_FORM_DEFAULT || form > WN_FORM_F16X3_FUSED) return "unknown form";
    if (h->cfg.kind != WN_KIND_STUDENT) return "handle is not a ParallelWavenet student (a teacher has no latent to encode to)";
    if (h->cfg.use_mu_law) return "mu-law students are not supported (their audio is not the flow's output x)";
    if (!h->finalized) return ENC_NOT_FINALIZED;
    if (B < 1 || F < 1) return "B and F must be >= 1";
    if (B > 65535) return "at most 65535 rows per call";
    if (wn_iaf_length(h, F) == 0) return "fewer frames than one max-dilation block";
    if ((int64_t)F * h->frame_shift > WN_MAX_ROW_SAMPLES)
        return "more than 2,000,000 samples (125 s) per row: the limit of the 32-bit row offsets";
    if ((int64_t)B * wn_iaf_length(h, F) / 64 > 0x7fffffff) return "batch too large";
    return nullptr;
}

extern "C" size_t wn_iaf_encode_workspace_bytes(const wn_handle* h, int form, int B, int F) {
    if (iaf_encode_refusal(h, form, B, F)) return 0;
    return align_up(wn_iaf_workspace_bytes(h, B, F, form), 256) +
           align_up((size_t)2 * B * enc_blocks(wn_iaf_length(h, F)) * sizeof(int), 256);
}

extern "C" int wn_iaf_encode(wn_handle* h, int form, const float* mel, int B, int F, const float* x, float* z, int n_sweeps,
                             float z_max, float tol, int first, float* mean_tot, float* scale_tot, int32_t* front,
                             int32_t* counts, void* ws, size_t ws_bytes, void* stream) {
    if (const char* why = iaf_encode_refusal(h, form, B, F))
        return wn_fail(h, why == ENC_NOT_FINALIZED ? WN_ESTATE : WN_EINVAL, "wn_iaf_encode: %s", why);
    if (n_sweeps < 1) return wn_fail(h, WN_EINVAL, "wn_iaf_encode: n_sweeps must be >= 1, got %d", n_sweeps);
    if (!(z_max > 0.f)) return wn_fail(h, WN_EINVAL, "wn_iaf_encode: z_max must be > 0, got %g", (double)z_max);
    if (!(tol >= 0.f)) return wn_fail(h, WN_EINVAL, "wn_iaf_encode: tol must be >= 0, got %g", (double)tol);
    if (!mel || !x || !z || !front || !counts || !ws)
        return wn_fail(h, WN_EINVAL, "wn_iaf_encode: null mel/x/z/front/counts/workspace");
    const size_t need = wn_iaf_encode_workspace_bytes(h, form, B, F);
    if (ws_bytes < need) return wn_fail(h, WN_ENOMEM, "wn_iaf_encode: workspace %zu < %zu bytes", ws_bytes, need);
    const WnWork work(h);
    IafCall c = iaf_call_fill(h, form, B, F, B, mel, ws, stream);
    const IafLayout& L = c.L;
    EncBackArgs A{};
    A.x = x; A.Mt = c.Mt; A.St = c.St; A.z = z; A.mean_tot = mean_tot; A.scale_tot = scale_tot;
    A.T = L.T; A.z_max = z_max; A.tol = tol; A.nblk = enc_blocks(L.T);
    A.part = reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + align_up(wn_iaf_workspace_bytes(h, B, F, form), 256));
    A.status = c.status; A.counts = counts;
    uintptr_t bits = (uintptr_t)(L.T & 3);
    for (const void* p : {(const void*)x, (const void*)z, (const void*)mean_tot, (const void*)scale_tot})
        bits |= reinterpret_cast<uintptr_t>(p) & 15;
    A.vec = bits == 0;
    WN_HIP(h, hipMemsetAsync(counts, 0, 4 * sizeof(int32_t), c.st));
    for (int s = 0; s < n_sweeps; ++s) {
        c.skip_front = h->cfg.share_deconv && (s > 0 || !first);
        c.x = c.xbuf0;                                      // run_groups may have left the other copy in force
        if (int rc = c.part(0)) return rc;
        iaf_prologue(c, z, 0);
        if (int rc = iaf_call_body(c)) return rc;
        hipLaunchKernelGGL(iaf_encode_back_kernel, dim3((unsigned)A.nblk, (unsigned)B), dim3(256), 0, c.st, A);
        hipLaunchKernelGGL(iaf_encode_reduce_kernel, dim3(1), dim3(256), 0, c.st, A.part, B, A.nblk, (int)L.T, s, front, counts);
    }
    return iaf_call_close(c);
}

extern "C" int wn_iaf_latent_log_prob(wn_handle* h, const float* z, const float* scale_tot, int B, int64_t T, float* log_prob,
                                      double* row_sums, void* stream) {
    if (!h) return wn_fail(nullptr, WN_EINVAL, "wn_iaf_latent_log_prob: null handle");
    if (h->cfg.kind != WN_KIND_STUDENT)
        return wn_fail(h, WN_EINVAL, "wn_iaf_latent_log_prob: handle is not a ParallelWavenet student");
    if (B < 1 || T < 1) return wn_fail(h, WN_EINVAL, "wn_iaf_latent_log_prob: B and T must be >= 1");
    if (!z || !scale_tot) return wn_fail(h, WN_EINVAL, "wn_iaf_latent_log_prob: null z/scale_tot");
    uintptr_t bits = (uintptr_t)(T & 3);
    for (const void* p : {(const void*)z, (const void*)scale_tot, (const void*)log_prob}) bits |= reinterpret_cast<uintptr_t>(p) & 15;
    hipLaunchKernelGGL(iaf_latent_log_prob_kernel, dim3((unsigned)B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), z,
                       scale_tot, T, h->cfg.loss_type == WN_LOSS_GAUSS ? 1 : 0, bits == 0 ? 1 : 0, log_prob, row_sums);
    WN_HIP(h, hipGetLastError());
    return WN_OK;
}

// ---------------------------------------------------------------------------
// Windowed generation: R rows of Fw frames run through iaf_call_fill / _body / _close as a batch of R
// utterances; what differs is the call's front (noise at absolute positions) and back (only the kept columns leave, at their
// place in the utterance).  nsynth_wavenet_amd/config.py: iaf_window_geometry is the twin of wn_iaf_window_geometry.
extern "C" int wn_iaf_window_geometry(const wn_handle* h, int64_t* reach, int* frames_before, int* frames_after, int* period) {
    if (!h) return wn_fail(nullptr, WN_EINVAL, "wn_iaf_window_geometry: null handle");
    const wn_config& c = h->cfg;
    if (c.kind != WN_KIND_STUDENT)
        return wn_fail(h, WN_EINVAL, "wn_iaf_window_geometry: handle is not a ParallelWavenet student");
    // a flow's mean and scale at t read x[t - r .. t - 1], r = fl + (fl - 1) sum of its dilations; the flows chain on x
    int64_t rc = 0;
    for (int k = 0; k < c.n_flows; ++k) {
        rc += c.filter_length;
        for (int i = 0; i < c.iaf_layers[k]; ++i) rc += (int64_t)(c.filter_length - 1) << (i % c.num_stages);
    }
    // the input interval one upsampler layer reads for an output interval, last layer first, from one frame far from the edges
    auto fdiv = [](int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };
    const int64_t f = 1 << 20;
    int64_t a = f * h->frame_shift, b = (f + 1) * h->frame_shift - 1;
    for (int j = c.n_deconv - 1; j >= 0; --j) {
        const int64_t K = c.deconv_filter[j], s = c.deconv_stride[j];
        if (c.use_resize_conv) {
            const int64_t pl = (K - 1) / 2;
            a = fdiv(a - pl, s);
            b = fdiv(b - pl + K - 1, s);
        } else {
            const int64_t pL = std::max<int64_t>(K - s, 0) / 2;
            a = -fdiv(-(a + pL - K + 1), s);
            b = fdiv(b + pL, s);
        }
    }
    const int64_t md = (int64_t)1 << (c.num_stages - 1);
    int64_t x = h->frame_shift, y = md;
    while (y) { const int64_t t = x % y; x = y; y = t; }     // x = gcd(frame_shift, max dilation)
    if (reach) *reach = rc;
    if (frames_before) *frames_before = (int)(f - a);
    if (frames_after) *frames_after = (int)(b - f);
    if (period) *period = (int)(md / x);
    return WN_OK;
}

static size_t wn_iaf_windows_table_bytes(int R) { return align_up((size_t)R * sizeof(wn_iaf_window_row), 256); }

extern "C" size_t wn_iaf_windows_workspace_bytes(const wn_handle* h, int R, int Fw, int form) {
    if (!h || h->cfg.kind != WN_KIND_STUDENT || R < 1 || Fw < 1 || form < WN_FORM_DEFAULT || form > WN_FORM_F16X3_FUSED) return 0;
    return align_up(wn_iaf_workspace_bytes(h, R, Fw, form), 256) + wn_iaf_windows_table_bytes(R);
}

extern "C" int wn_iaf_generate_windows(wn_handle* h, int form, int form_rows, const float* mel, int R, int Fw,
                                       const wn_iaf_window_row* rows_host, const float* noise_abs, int B_out, int64_t T_out,
                                       uint64_t seed, float* wav, int32_t* idx, float* x_raw, float* mean_tot,
                                       float* scale_tot, float* rand_out, void* ws, size_t ws_bytes, void* stream) {
    if (!h) return wn_fail(nullptr, WN_EINVAL, "wn_iaf_generate_windows: null handle");
    if (form < WN_FORM_DEFAULT || form > WN_FORM_F16X3_FUSED)
        return wn_fail(h, WN_EINVAL, "wn_iaf_generate_windows: unknown form %d", form);
    if (!h->finalized) return wn_fail(h, WN_ESTATE, "wn_iaf_generate_windows: call wn_finalize first");
    if (h->cfg.kind != WN_KIND_STUDENT)
        return wn_fail(h, WN_EINVAL, "wn_iaf_generate_windows: handle is not a ParallelWavenet student");
    if (R < 1 || Fw < 1) return wn_fail(h, WN_EINVAL, "wn_iaf_generate_windows: R and Fw must be >= 1");
    if (R > 65535) return wn_fail(h, WN_EINVAL, "wn_iaf_generate_windows: at most 65535 rows per call, got %d", R);
    if (form_rows < 0) return wn_fail(h, WN_EINVAL, "wn_iaf_generate_windows: form_rows must be >= 0, got %d", form_rows);
    if (B_out < 1 || T_out < 1) return wn_fail(h, WN_EINVAL, "wn_iaf_generate_windows: B_out and T_out must be >= 1");
    const WnWork work(h);
    // groups or per-layer launches: the one-shot's size policy evaluated for form_rows rows (0: the R of this call).  A caller
    // that wants a row's bits not to depend on how many rows share its call names a fixed count (a stream runs windows as
    // they become possible, Engine.iaf_generate_long eight at a time; both must produce the same audio)
    IafCall c = iaf_call_fill(h, form, R, Fw, form_rows ? form_rows : R, mel, ws, stream);
    const IafLayout& L = c.L;
    if (L.T == 0) return wn_fail(h, WN_EINVAL, "wn_iaf_generate_windows: a window of %d frames is shorter than one max-dilation block", Fw);
    if (!mel || !wav || !ws || !rows_host) return wn_fail(h, WN_EINVAL, "wn_iaf_generate_windows: null mel/wav/workspace/rows");
    if (L.TE > WN_MAX_ROW_SAMPLES)   // 32-bit buffer offsets inside one row (960 * TE bytes): the limit is the WINDOW's, not the utterance's
        return wn_fail(h, WN_EINVAL, "wn_iaf_generate_windows: %lld samples per window exceeds the 2,000,000 "
                       "(125 s) limit of the 32-bit row offsets; plan shorter windows", (long long)L.TE);
    const size_t tab_off = align_up(L.total, 256), tab_bytes = (size_t)R * sizeof(wn_iaf_window_row);
    if (ws_bytes < tab_off + tab_bytes)
        return wn_fail(h, WN_ENOMEM, "wn_iaf_generate_windows: workspace %zu < %zu bytes", ws_bytes, tab_off + tab_bytes);
    if ((int64_t)R * L.T / 64 > 0x7fffffff) return wn_fail(h, WN_EINVAL, "wn_iaf_generate_windows: batch too large");
    // the row table: every refusal by name, then one writer per output element
    int64_t max_keep = 0;
    std::vector<std::pair<int64_t, int64_t>> spans((size_t)R);
    for (int r = 0; r < R; ++r) {
        const wn_iaf_window_row& w = rows_host[r];
        if (w.b < 0 || w.b >= B_out)
            return wn_fail(h, WN_EINVAL, "wn_iaf_generate_windows: row %d: b = %d outside [0, B_out = %d)", r, w.b, B_out);
        if (w.t_origin < 0 || (w.t_origin & 3))
            return wn_fail(h, WN_EINVAL, "wn_iaf_generate_windows: row %d: t_origin = %lld is not a non-negative multiple of 4 "
                           "(unaligned t_origin: the noise counter covers four samples)", r, (long long)w.t_origin);
        if (w.keep_from < 0 || w.keep_to < w.keep_from || w.keep_to > L.T)
            return wn_fail(h, WN_EINVAL, "wn_iaf_generate_windows: row %d: kept range [%lld, %lld) outside [0, T_w = %lld)", r,
                           (long long)w.keep_from, (long long)w.keep_to, (long long)L.T);
        const int64_t n = w.keep_to - w.keep_from;
        if (w.out_t < 0 || w.out_t + n > T_out)
            return wn_fail(h, WN_EINVAL, "wn_iaf_generate_windows: row %d: out_t = %lld plus %lld kept samples past T_out = %lld",
                           r, (long long)w.out_t, (long long)n, (long long)T_out);
        spans[r] = {(int64_t)w.b * T_out + w.out_t, n};
        max_keep = std::max(max_keep, n);
    }
    std::sort(spans.begin(), spans.end());
    for (int r = 0; r + 1 < R; ++r)
        if (spans[r].second > 0 && spans[r].first + spans[r].second > spans[r + 1].first && spans[r + 1].second > 0)
            return wn_fail(h, WN_EINVAL, "wn_iaf_generate_windows: overlapping kept ranges: two rows write output element %lld",
                           (long long)spans[r + 1].first);
    // the table goes up from a copy the handle keeps (the upload is asynchronous), as wn_iaf_set_weights keeps its tables
    wn_iaf_window_row* d_rows = reinterpret_cast<wn_iaf_window_row*>(reinterpret_cast<char*>(ws) + tab_off);
    {
        auto keep = std::make_shared<std::vector<wn_iaf_window_row>>(rows_host, rows_host + R);
        WN_HIP(h, hipMemcpyAsync(d_rows, keep->data(), tab_bytes, hipMemcpyHostToDevice, c.st));
        std::lock_guard<std::mutex> g(h->list_mu);
        h->window_tables[h->window_tables_next++ % h->window_tables.size()] = keep;
    }
    if (int rc = c.part(0)) return rc;
    {
        WinPrologueArgs W{};
        iaf_prologue_args(c, nullptr, seed, W.P);
        W.rows = d_rows; W.noise_abs = noise_abs; W.T_out = T_out;
        hipLaunchKernelGGL(iaf_window_prologue_kernel, dim3((unsigned)(W.P.npad + W.P.ngx * R)), dim3(256), 0, c.st, W);
    }
    if (int rc = iaf_call_body(c)) return rc;
    if (max_keep > 0) {
        const wn_config& cfg = h->cfg;
        WinFinalArgs A{};
        A.rows = d_rows; A.x0 = c.x0g; A.Mt = c.Mt; A.St = c.St; A.T = L.T; A.T_out = T_out;
        A.Q = cfg.use_mu_law ? 256 : 65536; A.mu = cfg.use_mu_law;
        A.wav = wav; A.idx = idx; A.xraw = x_raw; A.mean_tot = mean_tot; A.scale_tot = scale_tot; A.rand_out = rand_out;
        A.status = c.status;
        uintptr_t bits = (uintptr_t)(T_out & 3);
        for (const void* p : {(const void*)wav, (const void*)idx, (const void*)x_raw, (const void*)mean_tot,
                              (const void*)scale_tot, (const void*)rand_out})
            bits |= reinterpret_cast<uintptr_t>(p) & 15;
        A.vec = bits == 0;
        // a quad per thread; the first quad of a row may start up to three elements before its first kept column
        const unsigned gx = (unsigned)(((max_keep + 3) / 4 + 1 + 255) / 256);
        hipLaunchKernelGGL(iaf_window_final_kernel, dim3(gx, (unsigned)R), dim3(256), 0, c.st, A);
    }
    return iaf_call_close(c);
}

extern "C" int wn_clip_quant(wn_handle* h, const float* x, int64_t n, float* wav, int32_t* idx, void* stream) {
    if (!h) return wn_fail(nullptr, WN_EINVAL, "wn_clip_quant: null handle");
    if (n < 0 || (n > 0 && !x)) return wn_fail(h, WN_EINVAL, "wn_clip_quant: bad argument");
    if (n == 0) return WN_OK;
    const int Q = h->cfg.use_mu_law ? 256 : 65536;
    hipLaunchKernelGGL(clip_quant_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), x, n, Q, h->cfg.use_mu_law, wav, idx);
    WN_HIP(h, hipGetLastError());
    return WN_OK;
}

// Where the per-layer conditioning 1x1s run (f16x3 only).  Hoisted (default): one GEMM per deconv
// stack writes every layer's projection, the layer kernels stream 768 B/sample (+ 256 B written by
// the GEMM) and the small-dilation layers run two per launch (wn_iaf_c_pair).  Fused
// (cond_mode / WN_COND=fused): every layer kernel streams enc itself (1536 B/sample/layer, no extra
// workspace).  Measured on MI355X (M samples/s, hoisted / fused): 50.7 / 46.8 at one utterance of
// 4.8 s, 56 / 49 at two, 61 / 42 at eight.
int wn_form_precision(const wn_handle* h, int form) {
    return form == WN_FORM_F32 ? WN_PREC_F32 : form == WN_FORM_DEFAULT ? h->cfg.precision : WN_PREC_F16X3;
}

int wn_iaf_set_attrs(wn_handle* h) {
    if (h->generic_student) return wn_iaf_x_set_attrs(h);
    int rc = wn_iaf_h_set_attrs(h);
    if (rc) return rc;
    rc = wn_iaf_c_set_attrs(h);
    if (rc) return rc;
    rc = wn_iaf_g_set_attrs(h);
    if (rc) return rc;
    return wn_iaf_f32_set_attrs(h);
}

int wn_iaf_form(const wn_handle* h, int B, int64_t T, int form) {
    if (h->generic_student) return WN_COND_FUSED;               // fp32 kernels of wn_iaf_x.hip: no projected term
    if (form == WN_FORM_F16X3_FUSED) return WN_COND_FUSED;
    // fp32 form (round 6): the same placement policy; its conditioning GEMM walks 128-column tiles
    if (wn_form_precision(h, form) != WN_PREC_F16X3 && T % 128 != 0) return WN_COND_FUSED;
    int mode = h->cfg.cond_mode;
    if (mode == WN_COND_AUTO) mode = h->cond_env_mode;           // WN_COND, resolved once in wn_create
    if (mode == WN_COND_FUSED) return WN_COND_FUSED;
    if (mode == WN_COND_HOISTED) return WN_COND_HOISTED;
    return wn_iaf_hoisted(h, B, T) ? WN_COND_HOISTED : WN_COND_FUSED;
}

// Default placement (cond_mode 0, no WN_COND): hoisted while the projected term (256 B per sample and row
// block) stays below a third of the device memory, else the fused form, which needs no such workspace.
bool wn_iaf_hoisted(const wn_handle* h, int B, int64_t T) {
    int rows = h->cond_rows;
    if (!h->cfg.share_deconv) {
        rows = 0;
        for (const IafFlowPack& fp : h->flows) rows = std::max(rows, (int)fp.layers.size() + 1);
    }
    return (double)B * (double)T * 256.0 * rows <= h->hoist_limit_bytes;
}

// The layer-group kernel (wn_iaf_g.hip) runs the hoisted form whenever every flow has a group plan and the decimated
// view exists (T a multiple of 32 * 16); lA then keeps the natural layout and lB the DL layout for the whole call.
// Where it pays (round 5, profiles/r05_batch_sweep.txt; configs[1] utterances on one box, ms per call groups | per-layer
// launches): 1.19 | 1.43 at one utterance, 4.71 | 4.74 at four, 6.99 | 6.92 at six, 9.30 | 9.29 at eight, 13.91 | 14.27 at twelve,
// 18.35 | 18.78 at sixteen.  From two utterances on BOTH forms run at the package power cap, so what decides
// is energy per sample: the group form moves the residual stream through the fabric twice per ten layers instead of eight
// times, the per-layer form has no halo recompute; the groups are 2.3-2.5 % ahead from twelve utterances and within +-1 % of
// the per-layer form below (second sweep, same file: the per-layer form 0.6-1.5 % ahead at five to seven utterances, the
// groups 0.5 % ahead at eight, 3.5 % at ten).  Default: groups, except between 4.5 and 7 segments per CU.  wn_iaf_set_groups
// (or WN_GROUPS=1 / WN_NO_GROUPS=1 at wn_create) forces either form (A/B measurements, cross-form tests).
bool wn_iaf_use_groups(const wn_handle* h, int B, int64_t T, int form) {
    if (form != WN_COND_HOISTED || !h->groups_ok || T % 512 != 0) return false;
    if (h->groups_env) return h->groups_env > 0;                // wn_iaf_set_groups; WN_NO_GROUPS / WN_GROUPS set its initial value in wn_create
    // five to seven utterances' worth of segments: the per-layer launches are 0.6-1.5 % ahead there (r05_batch_sweep.txt)
    const int64_t segs = (int64_t)B * ((T / 16 + 19) / 20);
    return segs <= 4 * (int64_t)h->num_cu + h->num_cu / 2 || segs > 7 * (int64_t)h->num_cu;
}

extern "C" int wn_iaf_set_groups(wn_handle* h, int mode) {
    if (!h) return wn_fail(nullptr, WN_EINVAL, "wn_iaf_set_groups: null handle");
    if (mode < -1 || mode > 1) return wn_fail(h, WN_EINVAL, "wn_iaf_set_groups: mode must be -1 (never), 0 (as created) or 1 (always), got %d", mode);
    WN_SWITCH(h, "wn_iaf_set_groups");
    h->groups_env = mode ? mode : h->groups_env0;      // 0: what wn_create resolved (the size policy, or WN_GROUPS / WN_NO_GROUPS)
    return WN_OK;
}

extern "C" int wn_iaf_layer_groups(const wn_handle* h, int B, int F) {
    if (!h || h->cfg.kind != WN_KIND_STUDENT || B < 1 || F < 1 || h->cfg.precision != WN_PREC_F16X3) return 0;
    const int64_t T = wn_iaf_length(h, F);
    return wn_iaf_use_groups(h, B, T, wn_iaf_form(h, B, T, WN_FORM_DEFAULT)) ? 1 : 0;
}

extern "C" int wn_iaf_cond_hoisted(const wn_handle* h, int B, int F) {
    if (!h || h->cfg.kind != WN_KIND_STUDENT || B < 1 || F < 1) return 0;
    return wn_iaf_form(h, B, wn_iaf_length(h, F), WN_FORM_DEFAULT) == WN_COND_HOISTED ? 1 : 0;
}

// default form: room for the fp32 re-run of a call that left the fp16 range as well (it needs less: no projected term)
size_t wn_iaf_workspace_bytes(const wn_handle* h, int B, int F, int form) {
    size_t n = iaf_layout(h, B, F, form).total;
    if (form == WN_FORM_DEFAULT) n = std::max(n, iaf_layout(h, B, F, WN_FORM_F32).total);
    return n;
}

static int range_report(wn_handle* h, unsigned flag) {
    if (flag)
        return wn_fail(h, WN_ERANGE, "wn_iaf_generate: an activation left the fp16 range of the split-fp16 arithmetic "
                       "(|value| >= 65504); the outputs of that call are NaN -- re-run it with "
                       "wn_iaf_generate_form(h, WN_FORM_F32, ...)");
    return WN_OK;
}

extern "C" int wn_iaf_range_status(wn_handle* h, const void* ws, void* stream) {
    if (!h || !ws) return wn_fail(h, WN_EINVAL, "wn_iaf_range_status: null argument");
    unsigned flag = 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WN_HIP(h, hipMemcpyAsync(&flag, ws, sizeof(flag), hipMemcpyDeviceToHost, st));      // the status word leads the workspace
    WN_HIP(h, hipStreamSynchronize(st));
    return range_report(h, flag);
}

extern "C" int wn_iaf_range_reset(wn_handle* h, void* ws, void* stream) {
    if (!h || !ws) return wn_fail(h, WN_EINVAL, "wn_iaf_range_reset: null argument");
    WN_HIP(h, hipMemsetAsync(ws, 0, 64, reinterpret_cast<hipStream_t>(stream)));
    return WN_OK;
}

extern "C" int wn_iaf_range_status_since_reset(wn_handle* h, void* ws, void* stream) {
    if (!h || !ws) return wn_fail(h, WN_EINVAL, "wn_iaf_range_status_since_reset: null argument");
    unsigned flags[2] = {0, 0};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WN_HIP(h, hipMemcpyAsync(flags, ws, sizeof(flags), hipMemcpyDeviceToHost, st));
    WN_HIP(h, hipStreamSynchronize(st));
    if (flags[0] | flags[1]) WN_HIP(h, hipMemsetAsync(ws, 0, 64, st));
    return range_report(h, flags[0] | flags[1]);
}

extern "C" int wn_profile_begin(wn_handle* h) {
    if (!h) return wn_fail(nullptr, WN_EINVAL, "wn_profile_begin: null handle");
    WN_SWITCH(h, "wn_profile_begin");
    for (hipEvent_t e : h->prof_events) (void)hipEventDestroy(e);
    h->prof_events.clear();
    h->prof_launches = 0;
    h->prof_on = true;
    return WN_OK;
}

extern "C" int wn_profile_parts_begin(wn_handle* h) {
    if (!h) return wn_fail(nullptr, WN_EINVAL, "wn_profile_parts_begin: null handle");
    WN_SWITCH(h, "wn_profile_parts_begin");
    for (hipEvent_t e : h->part_events) (void)hipEventDestroy(e);
    h->part_events.clear();
    h->part_tags.clear();
    h->part_calls = 0;
    h->parts_mask = 0xf;
    h->parts_on = true;
    return WN_OK;
}

extern "C" int wn_profile_parts_only(wn_handle* h, int mask) {
    if (!h) return wn_fail(nullptr, WN_EINVAL, "wn_profile_parts_only: null handle");
    if (mask < 1 || mask > 0xf) return wn_fail(h, WN_EINVAL, "wn_profile_parts_only: mask must be in 1..15, got %d", mask);
    WN_SWITCH(h, "wn_profile_parts_only");
    if (!h->parts_on)      // a restricted call skips work: the switch lives and dies with a measurement session
        return wn_fail(h, WN_ESTATE, "wn_profile_parts_only: only between wn_profile_parts_begin and wn_profile_parts_end");
    h->parts_mask = mask;
    return WN_OK;
}

extern "C" int wn_profile_parts_end(wn_handle* h, double* part_ms, int64_t* calls) {
    if (!h) return wn_fail(nullptr, WN_EINVAL, "wn_profile_parts_end: null handle");
    WN_SWITCH(h, "wn_profile_parts_end");
    h->parts_on = false;
    h->parts_mask = 0xf;                                           // never left armed
    double ms[WN_PROFILE_PARTS] = {0.0};
    hipError_t bad = hipSuccess;
    for (size_t i = 0; i + 1 < h->part_events.size() && bad == hipSuccess; ++i) {
        const int tag = h->part_tags[i];
        if (tag < 0 || tag >= WN_PROFILE_PARTS) continue;          // -1: between two calls
        float f = 0.f;
        bad = hipEventSynchronize(h->part_events[i + 1]);
        if (bad == hipSuccess) bad = hipEventElapsedTime(&f, h->part_events[i], h->part_events[i + 1]);
        ms[tag] += f;
    }
    for (hipEvent_t e : h->part_events) (void)hipEventDestroy(e);   // (on the error path as well)
    h->part_events.clear();
    h->part_tags.clear();
    if (bad != hipSuccess) return wn_fail(h, WN_EIO, "wn_profile_parts_end: %s", hipGetErrorString(bad));
    if (part_ms) for (int i = 0; i < WN_PROFILE_PARTS; ++i) part_ms[i] = ms[i];
    if (calls) *calls = h->part_calls;
    return WN_OK;
}

extern "C" int wn_profile_pause(wn_handle* h, int paused) {
    if (!h) return wn_fail(nullptr, WN_EINVAL, "wn_profile_pause: null handle");
    WN_SWITCH(h, "wn_profile_pause");
    h->prof_on = !paused;
    return WN_OK;
}

extern "C" int wn_profile_end(wn_handle* h, double* layer_ms, int64_t* layer_launches) {
    if (!h) return wn_fail(nullptr, WN_EINVAL, "wn_profile_end: null handle");
    WN_SWITCH(h, "wn_profile_end");
    h->prof_on = false;
    double ms = 0.0;
    for (size_t i = 0; i + 1 < h->prof_events.size(); i += 2) {
        float f = 0.f;
        WN_HIP(h, hipEventSynchronize(h->prof_events[i + 1]));
        WN_HIP(h, hipEventElapsedTime(&f, h->prof_events[i], h->prof_events[i + 1]));
        ms += f;
    }
    for (hipEvent_t e : h->prof_events) (void)hipEventDestroy(e);
    h->prof_events.clear();
    if (layer_ms) *layer_ms = ms;
    if (layer_launches) *layer_launches = h->prof_launches;
    return WN_OK;
}
