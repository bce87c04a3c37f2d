// The gradient of the student's log-likelihood.
//
// log p(x) = log f(z) - log scale_tot with z = encode(x).  The tape forward at noise = z gives
// x^ = z S + M, S = scale_tot, M = mean_tot, both functions of z[<t]; z solves x^(z) = x.  For a cotangent c of log p:
//   g_z = c (log f)'(z),  d_S = -c / S                                    wn_iaf_latent_log_prob_grad
//   A^T lam = g_z + (dS/dz)^T d_S,  A = d x^ / d z (lower triangular, diagonal S)      wn_iaf_adjoint
// and d loss / d x = lam; the weights and the encoding get theirs from wn_iaf_backward_weights(d_x = -lam, 0, d_S).
// The solve is a Jacobi iteration on the reverse data path of wn_iaf_train.hip:
//   lam <- lam + (g_z + r) / min(S, e^7),  r = wn_iaf_backward_input(tape, -lam, d_mean_tot, d_S).d_noise
// A^T is upper triangular, so k sweeps make the last k samples of a row exact.  No sequential kernel, no atomics.
#include <cmath>

#include "wn_internal.h"

namespace {
constexpr float EXP_7 = 1096.6331584284585f;
constexpr int ADJ_BLOCK = 1024;      // samples of a row per workgroup of iaf_adjoint_update_kernel

// one thread per quad; c = d_log_prob, or -1 / n where it is null.  Evaluated in double and rounded once.
__global__ __launch_bounds__(256) void iaf_latent_log_prob_grad_kernel(const float* __restrict__ z, const float* __restrict__ st,
                                                                       const float* __restrict__ dlp, size_t n, double c_mean,
                                                                       int gauss, int vec, float* __restrict__ gz,
                                                                       float* __restrict__ ds) {
    const size_t j0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (j0 >= n) return;
    const int m = (int)(n - j0 < 4 ? n - j0 : 4);
    float zv[4], sv[4], cv[4], g[4], d[4];
    if (vec) {
        const f4 a = *reinterpret_cast<const f4*>(z + j0), s = *reinterpret_cast<const f4*>(st + j0);
        const f4 c = dlp ? *reinterpret_cast<const f4*>(dlp + j0) : (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) { zv[e] = a[e]; sv[e] = s[e]; cv[e] = c[e]; }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            zv[e] = e < m ? z[j0 + e] : 0.f;
            sv[e] = e < m ? st[j0 + e] : 1.f;
            cv[e] = e < m && dlp ? dlp[j0 + e] : 0.f;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double c = dlp ? (double)cv[e] : c_mean, zd = (double)zv[e];
        g[e] = (float)(c * (gauss ? -zd : -tanh(0.5 * zd)));      // Normal(0,1): -z; Logistic(0,1): 1 - 2 sigmoid(z)
        d[e] = (float)(-c / (double)sv[e]);
    }
    if (vec) {
        *reinterpret_cast<f4*>(gz + j0) = (f4){g[0], g[1], g[2], g[3]};
        *reinterpret_cast<f4*>(ds + j0) = (f4){d[0], d[1], d[2], d[3]};
    } else {
        for (int e = 0; e < m; ++e) { gz[j0 + e] = g[e]; ds[j0 + e] = d[e]; }
    }
}

// d_x of the first sweep: -lam
__global__ __launch_bounds__(256) void iaf_adjoint_neg_kernel(const float* __restrict__ lam, float* __restrict__ neg, size_t n) {
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j < n) neg[j] = -lam[j];
}

// The back of a sweep: lam' = lam + (g_z + r) / min(S, e^7), a non-finite value replaced by 0 and counted; lam' over lam,
// -lam' over neg (the next sweep's d_x).  A thread owns one quad of a row, a workgroup ADJ_BLOCK samples.  Per block the
// maxima of |lam' - lam| and |lam'| (a wave butterfly, then the waves: a maximum has no order) into part[0 / 1][b][bx], the
// count into cpart[b][bx]; iaf_adjoint_reduce_kernel folds them.  Nothing to initialise between sweeps.
struct AdjArgs {
    const float *gz, *r, *S;          // [B][T]; S: the tape's scale_tot before the clamp
    float *lam, *neg;                 // [B][T]
    int64_t T;
    int vec, nblk;
    float* part;                      // [2][B][nblk]
    int* cpart;                       // [B][nblk]
    const int* counts;
};
__global__ __launch_bounds__(256) void iaf_adjoint_update_kernel(const AdjArgs A) {
    // an earlier sweep of this call met the tolerance: lam, neg and the partials stay that sweep's
    if (A.counts[2] != 0) return;
    const int b = blockIdx.y;
    const int64_t t0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4, row = (int64_t)b * A.T;
    float md = 0.f, ml = 0.f;
    int nc = 0;
    if (t0 < A.T) {
        const int n = (int)(A.T - t0 < 4 ? A.T - t0 : 4);
        float gv[4], rv[4], sv[4], lo[4], ln[4];
        if (A.vec) {
            const f4 g = *reinterpret_cast<const f4*>(A.gz + row + t0), r = *reinterpret_cast<const f4*>(A.r + row + t0),
                     s = *reinterpret_cast<const f4*>(A.S + row + t0), l = *reinterpret_cast<const f4*>(A.lam + row + t0);
#pragma unroll
            for (int e = 0; e < 4; ++e) { gv[e] = g[e]; rv[e] = r[e]; sv[e] = s[e]; lo[e] = l[e]; }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool in = e < n;
                gv[e] = in ? A.gz[row + t0 + e] : 0.f;
                rv[e] = in ? A.r[row + t0 + e] : 0.f;
                sv[e] = in ? A.S[row + t0 + e] : 1.f;
                lo[e] = in ? A.lam[row + t0 + e] : 0.f;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = lo[e] + (gv[e] + rv[e]) / fminf(sv[e], EXP_7);
            if (!(fabsf(v) <= 3.0e38f)) {                    // NaN or +-inf
                v = 0.f;
                if (e < n) ++nc;
            }
            float d = fabsf(v - lo[e]);
            if (!(d <= 3.0e38f)) d = INFINITY;               // a non-finite starting value: this sweep does not converge
            if (e < n) { md = fmaxf(md, d); ml = fmaxf(ml, fabsf(v)); }
            ln[e] = v;
        }
        if (A.vec) {
            *reinterpret_cast<f4*>(A.lam + row + t0) = (f4){ln[0], ln[1], ln[2], ln[3]};
            *reinterpret_cast<f4*>(A.neg + row + t0) = (f4){-ln[0], -ln[1], -ln[2], -ln[3]};
        } else {
            for (int e = 0; e < n; ++e) { A.lam[row + t0 + e] = ln[e]; A.neg[row + t0 + e] = -ln[e]; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        md = fmaxf(md, __shfl_xor(md, o));
        ml = fmaxf(ml, __shfl_xor(ml, o));
        nc += __shfl_xor(nc, o);
    }
    __shared__ float shf[2][4];
    __shared__ int shi[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { shf[0][wave] = md; shf[1][wave] = ml; shi[wave] = nc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const size_t i = (size_t)b * A.nblk + blockIdx.x, BN = (size_t)gridDim.y * A.nblk;
        A.part[i] = fmaxf(fmaxf(shf[0][0], shf[0][1]), fmaxf(shf[0][2], shf[0][3]));
        A.part[BN + i] = fmaxf(fmaxf(shf[1][0], shf[1][1]), fmaxf(shf[1][2], shf[1][3]));
        A.cpart[i] = shi[0] + shi[1] + shi[2] + shi[3];
    }
}

// One workgroup: resid[b] = (max |lam' - lam|, max |lam'|) of the row, counts[0] = the sweep's non-finite count, counts[1] =
// the rows above the tolerance, counts[2] = the first sweep of the call (from 1) after which no row was and nothing was
// replaced.  Wave w takes the rows w, w + 4, ...; its lanes stride the row's partials.
__global__ __launch_bounds__(256) void iaf_adjoint_reduce_kernel(const float* __restrict__ part, const int* __restrict__ cpart,
                                                                 int B, int nblk, int sweep, float tol, float* __restrict__ resid,
                                                                 int* __restrict__ counts) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t BN = (size_t)B * nblk;
    int nc = 0, open = 0;
    for (int b = wave; b < B; b += 4) {
        float md = 0.f, ml = 0.f;
        for (int i = lane; i < nblk; i += 64) {
            md = fmaxf(md, part[(size_t)b * nblk + i]);
            ml = fmaxf(ml, part[BN + (size_t)b * nblk + i]);
            nc += cpart[(size_t)b * nblk + i];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            md = fmaxf(md, __shfl_xor(md, o));
            ml = fmaxf(ml, __shfl_xor(ml, o));
        }
        if (lane == 0) { resid[2 * b] = md; resid[2 * b + 1] = ml; }
        open += !(md <= tol * ml);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nc += __shfl_xor(nc, o);
    __shared__ int sh[2][4];
    if (lane == 0) { sh[0][wave] = nc; sh[1][wave] = open; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int c = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3], op = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
        counts[0] = c;
        counts[1] = op;
        if (c == 0 && op == 0 && counts[2] == 0) counts[2] = sweep + 1;
    }
}

int adj_blocks(int64_t T) { return (int)((T + ADJ_BLOCK - 1) / ADJ_BLOCK); }

// behind the reverse pass's workspace: -lam, r, a zero d_mean_tot, the partials
struct AdjLayout {
    size_t neg, r, zero, part, cpart, total;
};
AdjLayout adj_layout(const wn_handle* h, int B, int F, int64_t T) {
    AdjLayout L;
    size_t o = align_up(wn_iaf_backward_input_workspace_bytes(h, B, F, T), 256);
    auto carve = [&](size_t bytes) { size_t r = o; o += align_up(bytes, 256); return r; };
    const size_t bt = (size_t)B * T * 4, bn = (size_t)B * adj_blocks(T);
    L.neg = carve(bt); L.r = carve(bt); L.zero = carve(bt);
    L.part = carve(2 * bn * 4);
    L.cpart = carve(bn * 4);
    L.total = o;
    return L;
}
template <class T>
T* at(void* base, size_t off) { return reinterpret_cast<T*>(reinterpret_cast<char*>(base) + off); }
}  // namespace

extern "C" int wn_iaf_latent_log_prob_grad(wn_handle* h, const float* z, const float* scale_tot, int B, int64_t T,
                                           const float* d_log_prob, float* g_z, float* d_scale_tot, void* stream) {
    if (!h) return wn_fail(nullptr, WN_EINVAL, "wn_iaf_latent_log_prob_grad: null handle");
    if (h->cfg.kind != WN_KIND_STUDENT)
        return wn_fail(h, WN_EINVAL, "wn_iaf_latent_log_prob_grad: handle is not a ParallelWavenet student");
    if (B < 1 || T < 1) return wn_fail(h, WN_EINVAL, "wn_iaf_latent_log_prob_grad: B and T must be >= 1");
    if (!z || !scale_tot || !g_z || !d_scale_tot)
        return wn_fail(h, WN_EINVAL, "wn_iaf_latent_log_prob_grad: null z/scale_tot/g_z/d_scale_tot");
    const size_t n = (size_t)B * (size_t)T;
    uintptr_t bits = 0;
    for (const void* p : {(const void*)z, (const void*)scale_tot, (const void*)d_log_prob, (const void*)g_z, (const void*)d_scale_tot})
        bits |= reinterpret_cast<uintptr_t>(p) & 15;
    // a ragged last quad takes the scalar path in every thread: one code path per call
    const int vec = bits == 0 && n % 4 == 0;
    hipLaunchKernelGGL(iaf_latent_log_prob_grad_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), z, scale_tot, d_log_prob, n, -1.0 / (double)n,
                       h->cfg.loss_type == WN_LOSS_GAUSS ? 1 : 0, vec, g_z, d_scale_tot);
    WN_HIP(h, hipGetLastError());
    return WN_OK;
}

extern "C" size_t wn_iaf_adjoint_workspace_bytes(const wn_handle* h, int B, int F, int64_t T) {
    if (wn_iaf_backward_input_workspace_bytes(h, B, F, T) == 0) return 0;      // what the reverse pass refuses
    return adj_layout(h, B, F, T).total;
}

extern "C" int wn_iaf_adjoint(wn_handle* h, const void* tape, size_t tape_bytes, const float* g_z, const float* d_mean_tot,
                              const float* d_scale_tot, int B, int F, int64_t T, float* lam, int n_sweeps, float tol, float* resid,
                              int32_t* counts, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "wn_iaf_adjoint";
    if (int rc = wn_iaf_reverse_check(h, fn, B, F, T)) return rc;
    if (n_sweeps < 1) return wn_fail(h, WN_EINVAL, "%s: n_sweeps must be >= 1, got %d", fn, n_sweeps);
    if (!(tol >= 0.f)) return wn_fail(h, WN_EINVAL, "%s: tol must be >= 0, got %g", fn, (double)tol);
    if (!tape || !g_z || !d_scale_tot || !lam || !resid || !counts || !ws)
        return wn_fail(h, WN_EINVAL, "%s: null tape/g_z/d_scale_tot/lam/resid/counts/workspace", fn);
    if (int rc = wn_iaf_reverse_tape_check(h, fn, tape, tape_bytes, B, F, T)) return rc;
    const AdjLayout L = adj_layout(h, B, F, T);
    if (ws_bytes < L.total) return wn_fail(h, WN_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, L.total);
    const WnWork work(h);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t n = (size_t)B * (size_t)T;
    AdjArgs A{};
    A.gz = g_z; A.r = at<float>(ws, L.r); A.S = wn_iaf_tape_scale_prod(h, tape, B, F, T);
    A.lam = lam; A.neg = at<float>(ws, L.neg);
    A.T = T; A.nblk = adj_blocks(T);
    A.part = at<float>(ws, L.part); A.cpart = at<int>(ws, L.cpart); A.counts = counts;
    uintptr_t bits = (uintptr_t)(T & 3);
    for (const void* p : {(const void*)g_z, (const void*)lam, (const void*)A.S, (const void*)A.r, (const void*)A.neg})
        bits |= reinterpret_cast<uintptr_t>(p) & 15;
    A.vec = bits == 0;
    if (!d_mean_tot) {
        WN_HIP(h, hipMemsetAsync(at<float>(ws, L.zero), 0, n * 4, st));
        d_mean_tot = at<float>(ws, L.zero);
    }
    WN_HIP(h, hipMemsetAsync(counts, 0, 4 * sizeof(int32_t), st));
    hipLaunchKernelGGL(iaf_adjoint_neg_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, lam, A.neg, n);
    for (int s = 0; s < n_sweeps; ++s) {
        if (int rc = wn_iaf_reverse_input_run(h, fn, tape, A.neg, d_mean_tot, d_scale_tot, B, F, T, at<float>(ws, L.r), ws, stream))
            return rc;
        hipLaunchKernelGGL(iaf_adjoint_update_kernel, dim3((unsigned)A.nblk, (unsigned)B), dim3(256), 0, st, A);
        hipLaunchKernelGGL(iaf_adjoint_reduce_kernel, dim3(1), dim3(256), 0, st, A.part, A.cpart, B, A.nblk, s, tol, resid, counts);
    }
    WN_HIP(h, hipGetLastError());
    return WN_OK;
}
