// Teacher training step on the device: the optimiser kernels (global gradient norm, Adam with the EMA
// shadow) and wn_teacher_set_weights, which rewrites a finalized handle's packed weights in place from device-resident
// fp32 masters.
//
// The re-pack repeats wn_finalize's host packs (wn_pack_ar, wn_pack_teacher, wn_pack_deconv, wn_pack_deconv_bwd) with the
// same index maps, one thread per packed word: first the plain fp32 matrices and biases of the AR pack, which are also the
// sources of the teacher's GEMM packs, then -- once the absolute maxima of the split packs have come back and pick_scale has
// chosen their scales -- every split-fp16 pack.  The roundings are wn_pack_h.h's integer code on both sides, the composite
// bias accumulates in double in the host's order, the composite matrices come from wn_finalize's own kernels (wn_ar_compose), so every word equals what a fresh handle would have uploaded.
//
// The index maps live in wn_repack.h as __device__ functions, shared with the student's table-driven re-pack
// (wn_iaf_repack.hip); the per-stack code of the upsampler's re-pack (wn_repack_deconv_*) is defined here and
// runs for both calls.
#include <atomic>

#include "wn_repack.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// optimiser
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SS_MAXBLK = 1024;
inline int ss_blocks(size_t n) { return (int)std::min<size_t>(SS_MAXBLK, (n + 8 * TR_NT - 1) / (8 * TR_NT)); }

// fixed tree over the block's 256 partial sums
__device__ inline double ss_block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = TR_NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// stage 1: block b sums g[i]^2 over i = b * 256 + tid + k * gridDim.x * 256, in that order
__global__ __launch_bounds__(TR_NT) void tr_sumsq1_kernel(const float* __restrict__ g, size_t n, double* __restrict__ part) {
    __shared__ double red[TR_NT];
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * TR_NT + threadIdx.x; i < n; i += (size_t)gridDim.x * TR_NT) {
        const double v = (double)g[i];
        acc += v * v;
    }
    const double s = ss_block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}
// stage 2: one block over the partial sums
__global__ __launch_bounds__(TR_NT) void tr_sumsq2_kernel(const double* __restrict__ part, int nb, double* __restrict__ acc,
                                                          int accumulate) {
    __shared__ double red[TR_NT];
    double a = 0.0;
    for (int i = threadIdx.x; i < nb; i += TR_NT) a += part[i];
    const double s = ss_block_sum(a, red);
    if (threadIdx.x == 0) acc[0] = accumulate ? acc[0] + s : s;
}

struct AdamArgs {
    float* p;
    const float* g;
    float *m, *v, *ema;
    size_t n;
    float lr_t, beta1, beta2, eps, ema_decay_t, clip_norm;
    const double* sumsq;
};
// One element: the update is formed in double from the fp32 state and every stored value is rounded once; p and the shadow
// use the STORED m, v and p, as TensorFlow's kernels do.
__device__ inline void adam_one(const AdamArgs& a, double gs, float& p, float g, float& m, float& v, float* ema) {
    const double gh = (double)g * gs;
    const double b1 = (double)a.beta1, b2 = (double)a.beta2;
    m = (float)(b1 * (double)m + (1.0 - b1) * gh);
    v = (float)(b2 * (double)v + (1.0 - b2) * gh * gh);
    p = (float)((double)p - (double)a.lr_t * (double)m / (sqrt((double)v) + (double)a.eps));
    if (ema) *ema = (float)((double)*ema - (1.0 - (double)a.ema_decay_t) * ((double)*ema - (double)p));
}
// VEC: 16-byte accesses over the first n / 4 quads and a scalar tail; otherwise (a pointer off the 16-byte grid) scalar
template <bool VEC>
__global__ __launch_bounds__(TR_NT) void tr_adam_kernel(AdamArgs a) {
    // tf.clip_by_global_norm: g * clip / max(||g||, clip)
    double gs = 1.0;
    if (a.sumsq) gs = (double)a.clip_norm / fmax(sqrt(a.sumsq[0]), (double)a.clip_norm);
    const size_t i = (size_t)blockIdx.x * TR_NT + threadIdx.x;
    const size_t nq = VEC ? a.n / 4 : 0;
    if (VEC && i < nq) {
        f4 p = reinterpret_cast<f4*>(a.p)[i], m = reinterpret_cast<f4*>(a.m)[i], v = reinterpret_cast<f4*>(a.v)[i];
        const f4 g = reinterpret_cast<const f4*>(a.g)[i];
        f4 e = a.ema ? reinterpret_cast<f4*>(a.ema)[i] : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pk = p[k], mk = m[k], vk = v[k], ek = e[k];
            adam_one(a, gs, pk, g[k], mk, vk, a.ema ? &ek : nullptr);
            p[k] = pk; m[k] = mk; v[k] = vk; e[k] = ek;
        }
        reinterpret_cast<f4*>(a.p)[i] = p;
        reinterpret_cast<f4*>(a.m)[i] = m;
        reinterpret_cast<f4*>(a.v)[i] = v;
        if (a.ema) reinterpret_cast<f4*>(a.ema)[i] = e;
    }
    // tail: the first threads of the grid take the elements behind the last quad
    const size_t t = 4 * nq + i;
    if (i < a.n - 4 * nq && (!VEC || i < 4)) adam_one(a, gs, a.p[t], a.g[t], a.m[t], a.v[t], a.ema ? a.ema + t : nullptr);
}

// Shard combine: out[i] = (((r_0[i] + r_1[i]) + ...) + r_{S-1}[i]) * inv, r_j = rows + j * row_stride.  One
// thread per quad (VEC) or per element, strictly left to right with one rounding per add; rows and out carry no
// __restrict__, since out may be row 0: every thread reads its own elements of every row before it writes them.
// The loads of up to GC_BATCH rows are issued together, the adds follow in row order.
constexpr int GC_BATCH = 8;
template <typename V>
__device__ inline V gc_chain(const float* rows, size_t at, size_t row_stride, int S) {
    V acc = *reinterpret_cast<const V*>(rows + at);
    int j = 1;
    for (; j + GC_BATCH <= S; j += GC_BATCH) {
        V r[GC_BATCH];
#pragma unroll
        for (int k = 0; k < GC_BATCH; ++k) r[k] = *reinterpret_cast<const V*>(rows + (size_t)(j + k) * row_stride + at);
#pragma unroll
        for (int k = 0; k < GC_BATCH; ++k) {
            if constexpr (sizeof(V) == sizeof(float)) {
                acc = __fadd_rn(acc, r[k]);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c] = __fadd_rn(acc[c], r[k][c]);
            }
        }
    }
    for (; j < S; ++j) {
        const V r = *reinterpret_cast<const V*>(rows + (size_t)j * row_stride + at);
        if constexpr (sizeof(V) == sizeof(float)) {
            acc = __fadd_rn(acc, r);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = __fadd_rn(acc[c], r[c]);
        }
    }
    return acc;
}
// VEC: 16-byte accesses over the first n / 4 quads and a scalar tail, as tr_adam_kernel; otherwise all scalar
template <bool VEC>
__global__ __launch_bounds__(TR_NT) void tr_combine_kernel(const float* rows, size_t n, size_t row_stride, int S, float inv,
                                                           float* out) {
    const size_t i = (size_t)blockIdx.x * TR_NT + threadIdx.x;
    const size_t nq = VEC ? n / 4 : 0;
    if (VEC && i < nq) {
        f4 acc = gc_chain<f4>(rows, 4 * i, row_stride, S);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = __fmul_rn(acc[c], inv);
        reinterpret_cast<f4*>(out)[i] = acc;
    }
    const size_t t = 4 * nq + i;
    if (i < n - 4 * nq && (!VEC || i < 4)) out[t] = __fmul_rn(gc_chain<float>(rows, t, row_stride, S), inv);
}

// ---------------------------------------------------------------------------------------------------------------------
// re-pack: plain fp32 parts
// ---------------------------------------------------------------------------------------------------------------------
// the index maps are wn_repack.h's; one thread per packed word
__global__ __launch_bounds__(TR_NT) void tr_scatter_kernel(ScatterArgs a) {
    tr_scatter_word(a, (size_t)blockIdx.x * TR_NT + threadIdx.x);
}
// dst = x + y: the summed biases
__global__ __launch_bounds__(TR_NT) void tr_add_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                       float* __restrict__ dst, int n) {
    const int i = blockIdx.x * TR_NT + threadIdx.x;
    if (i < n) dst[i] = __fadd_rn(x[i], y[i]);
}
// composite bias bm = bd + Wd[tap t] . bres_{j-1}, in double in the host's order (a float x float product is exact in double)
__global__ __launch_bounds__(TR_NT) void tr_bm_kernel(const float* __restrict__ wd, const float* __restrict__ bd,
                                                      const float* __restrict__ brs_prev, float* __restrict__ bm, int G, int W,
                                                      int K) {
    const int o = blockIdx.x * TR_NT + threadIdx.x;
    if (o >= G) return;
    double acc = bd[o];
    for (int cc = 0; cc < W; ++cc) acc += (double)wd[(size_t)o * K + 2 * W + cc] * (double)brs_prev[cc];
    bm[o] = (float)acc;
}
__global__ __launch_bounds__(TR_NT) void tr_frag_kernel(const float* __restrict__ a, float* __restrict__ dst, int rows, int KA) {
    tr_frag_word(a, dst, rows, KA, (size_t)blockIdx.x * TR_NT + threadIdx.x);
}
__global__ __launch_bounds__(TR_NT) void tr_deconv_frag_kernel(const float* __restrict__ W, float* __restrict__ P, int S, int taps,
                                                               int cin, int cout) {
    tr_deconv_frag_word(W, P, S, taps, cin, cout, (size_t)blockIdx.x * TR_NT + threadIdx.x);
}
__global__ __launch_bounds__(TR_NT) void tr_absmax_kernel(const float* __restrict__ x, size_t n, unsigned* __restrict__ out) {
    tr_absmax_block(x, n, out, blockIdx.x, gridDim.x);
}

// ---------------------------------------------------------------------------------------------------------------------
// re-pack: split-fp16 packs.  One thread per packed word of pack_afrag's layout [fragment][plane][lane][4].
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TR_NT) void tr_tile_kernel(TileArgs a) { tr_tile_word(a, (size_t)blockIdx.x * TR_NT + threadIdx.x); }
// tile-ordered bias of a TeacherGemmPack
__global__ __launch_bounds__(TR_NT) void tr_tile_bias_kernel(const float* __restrict__ bsrc, float* __restrict__ dst, int n,
                                                             int rowkind, int M, int H) {
    const int i = blockIdx.x * TR_NT + threadIdx.x;
    if (i >= n) return;
    const int row = tr_row(rowkind, M, H, i);
    dst[i] = row < 0 ? 0.f : bsrc[row];
}

// split-fp16 A fragments of one transposed-conv layer, W [K][cout][cin]: the phase pack [S][ks][mb] (nph = 0) or the row
// groups of ONE phase group [sub][input block][tap][mb8] (nph = 4 | 2 phases from p0) of wn_pack_deconv
struct DeconvHArgs {
    const float* W;
    unsigned* dst;
    float sc;
    int S, taps, cin, cout, pL;
    int nph, p0, nsub;
};
__global__ __launch_bounds__(TR_NT) void tr_deconv_h_kernel(DeconvHArgs a) {
    const size_t i = (size_t)blockIdx.x * TR_NT + threadIdx.x;
    const int ii = i & 3, lane = (i >> 2) & 63, plane = (i >> 8) & 1;
    const int i16 = lane & 15, kg = lane >> 4;
    size_t f = i >> 9;
    uint16_t hh[2];
    if (a.nph == 0) {
        const int nb16 = a.cin / 16, nks = a.taps * nb16 / 2, nmb = a.cout / 16;
        if (f >= (size_t)a.S * nks * nmb) return;
        const int mb = (int)(f % nmb);
        f /= nmb;
        const int ks = (int)(f % nks), r = (int)(f / nks);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int e = 2 * ii + p, g = 2 * ks + (e >> 2), tap = g / nb16, blk = g - tap * nb16;
            const int ci = 16 * blk + 4 * kg + (e & 3);
            hh[p] = split_half(__fmul_rn(a.sc, a.W[((size_t)(a.S * tap + r) * a.cout + 16 * mb + i16) * a.cin + ci]), plane);
        }
    } else {
        const int nb32 = a.cin / 32;
        if (f >= (size_t)a.nsub * nb32 * 4 * 8) return;
        const int mb8 = f & 7, m = (f >> 3) & 3;
        f >>= 5;
        const int cb = (int)(f % nb32), sub = (int)(f / nb32);
        const int ph = a.nph == 4 ? mb8 >> 1 : mb8 >> 2;
        const int cb16 = a.nph == 4 ? 2 * sub + (mb8 & 1) : 4 * sub + (mb8 & 3);
        const int r = (a.p0 + ph + a.pL) % a.S;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int e = 2 * ii + p;
            const int ci = 32 * cb + 16 * (e >> 2) + 4 * kg + (e & 3);
            hh[p] = split_half(__fmul_rn(a.sc, a.W[((size_t)(a.S * m + r) * a.cout + 16 * cb16 + i16) * a.cin + ci]), plane);
        }
    }
    a.dst[i] = (uint32_t)hh[0] | ((uint32_t)hh[1] << 16);
}
// W^T as two planes of halves [k][ci][co] (wn_pack_deconv_bwd); one thread per pair of neighbouring co.  rows: ci rows per k
// of the pack -- cin, or cin rounded up to 64 for the first layer's pack, whose rows behind cin are zero
__global__ __launch_bounds__(TR_NT) void tr_deconv_t_kernel(const float* __restrict__ W, unsigned* __restrict__ dst, float sc, int K,
                                                            int cin, int rows, int cout) {
    const size_t n2 = (size_t)K * rows * cout / 2;
    const size_t i = (size_t)blockIdx.x * TR_NT + threadIdx.x;
    if (i >= n2) return;
    const size_t at = 2 * i;
    const int co = (int)(at % cout), ci = (int)((at / cout) % rows), k = (int)(at / cout / rows);
    if (ci >= cin) {
        dst[i] = 0u;
        dst[n2 + i] = 0u;
        return;
    }
    const float v0 = __fmul_rn(sc, W[((size_t)k * cout + co) * cin + ci]);
    const float v1 = __fmul_rn(sc, W[((size_t)k * cout + co + 1) * cin + ci]);
    dst[i] = (uint32_t)split_half(v0, 0) | ((uint32_t)split_half(v1, 0) << 16);
    dst[n2 + i] = (uint32_t)split_half(v0, 1) | ((uint32_t)split_half(v1, 1) << 16);
}

// ---------------------------------------------------------------------------------------------------------------------
// host side of the re-pack
// ---------------------------------------------------------------------------------------------------------------------
// what the weight-gradient calls support (tw_supported of wn_teacher_wgrad.hip): only such a handle has a parameter layout
bool train_supported(const wn_handle* h) {
    const wn_config& c = h->cfg;
    return c.kind == WN_KIND_TEACHER && c.loss_type != WN_LOSS_CE && !c.use_mu_law && !c.use_weight_norm && h->teacher.vjp_ok &&
           wn_teacher_grad_floats(h) > 0;
}

// the absolute maxima the call reduces: three per layer and four for the head, then one per upsampler layer
struct ScaleSlots {
    int n_layers, n_up;
    int wss() const { return 0; }
    int wo1a() const { return 1; }      // out1 columns
    int wo1b() const { return 2; }      // mel_cond_out1 columns
    int wo2() const { return 3; }
    int dil(int i) const { return 4 + 4 * i; }
    int cond(int i) const { return 5 + 4 * i; }
    int res(int i) const { return 6 + 4 * i; }
    int skip(int i) const { return 7 + 4 * i; }
    int up(int j) const { return 4 + 4 * n_layers + j; }
    int total() const { return 4 + 4 * n_layers + n_up; }
};
ScaleSlots scale_slots(const wn_handle* h) {
    return ScaleSlots{(int)h->ar.layers.size(), h->stacks.empty() ? 0 : (int)h->stacks[0].layers.size()};
}

std::atomic<uint64_t> g_repack_serial{1ull << 62};   // tape serials of re-packed handles: apart from wn_finalize's counter

inline void absmax_launch(const float* x, size_t n, unsigned* out, hipStream_t st) {
    const unsigned nb = (unsigned)std::min<size_t>(256, (n + 4 * TR_NT - 1) / (4 * TR_NT));
    hipLaunchKernelGGL(tr_absmax_kernel, dim3(nb), dim3(TR_NT), 0, st, x, n, out);
}

}  // namespace

uint64_t wn_repack_serial_next() { return g_repack_serial++; }

// ---- one upsampler stack (wn_repack.h): kernel, then bias per layer (sp.lay, wn_deconv_build_layout)
void wn_repack_deconv_absmax(const DeconvStackPack& sp, const float* up, unsigned* amax, hipStream_t st) {
    for (size_t j = 0; j < sp.layers.size(); ++j) {
        const DeconvLayerPack& lp = sp.layers[j];
        absmax_launch(up + sp.lay[j].W, (size_t)lp.K * lp.cout * lp.cin, amax + j, st);
    }
}

void wn_repack_deconv_plain(wn_handle* h, const DeconvStackPack& sp, const float* up, hipStream_t st) {
    float* blob = h->d_blob;
    for (size_t j = 0; j < sp.layers.size(); ++j) {
        const DeconvLayerPack& lp = sp.layers[j];
        const size_t total = (size_t)lp.S * lp.taps * (lp.cin / 16) * (lp.cout / 16) * 256;
        hipLaunchKernelGGL(tr_deconv_frag_kernel, dim3(tr_blocks(total)), dim3(TR_NT), 0, st, up + sp.lay[j].W, blob + lp.w_off,
                           lp.S, lp.taps, lp.cin, lp.cout);
        hipLaunchKernelGGL(tr_scatter_kernel, dim3(tr_blocks((size_t)lp.cout)), dim3(TR_NT), 0, st,
                           ScatterArgs{up + sp.lay[j].b, blob + lp.b_off, 1, lp.cout, 1, 0});
    }
}

void wn_repack_deconv_split(wn_handle* h, DeconvStackPack& sp, const float* up, const float* mx, hipStream_t st) {
    float* blob = h->d_blob;
    for (size_t j = 0; j < sp.layers.size(); ++j) {
        DeconvLayerPack& lp = sp.layers[j];
        const float* W = up + sp.lay[j].W;
        const float sc = pick_scale(mx + j, 1);
        if (lp.w_off_h) {
            lp.inv_scale_h = 1.0f / sc;
            const size_t words = (size_t)lp.S * (lp.taps * (lp.cin / 16) / 2) * (lp.cout / 16) * 512;
            hipLaunchKernelGGL(tr_deconv_h_kernel, dim3(tr_blocks(words)), dim3(TR_NT), 0, st,
                               DeconvHArgs{W, reinterpret_cast<unsigned*>(blob + lp.w_off_h), sc, lp.S, lp.taps, lp.cin, lp.cout,
                                           lp.pL, 0, 0, 0});
        }
        if (lp.w_off_pg) {
            const int nb32 = lp.cin / 32;
            for (int g = 0; g < lp.pg_n; ++g) {
                const int nsub = lp.pg_nph[g] == 4 ? lp.cout / 32 : lp.cout / 64;
                const size_t words = (size_t)nsub * nb32 * 4 * 8 * 512;
                unsigned* dst = reinterpret_cast<unsigned*>(blob + lp.w_off_pg) + (size_t)lp.pg_rg0[g] * nb32 * 4 * 8 * 512;
                hipLaunchKernelGGL(tr_deconv_h_kernel, dim3(tr_blocks(words)), dim3(TR_NT), 0, st,
                                   DeconvHArgs{W, dst, sc, lp.S, lp.taps, lp.cin, lp.cout, lp.pL, lp.pg_nph[g], lp.pg_p0[g], nsub});
            }
        }
        if (lp.wt_off) {
            lp.wt_inv_scale = 1.0f / sc;
            const size_t n2 = (size_t)lp.K * lp.cin * lp.cout / 2;
            hipLaunchKernelGGL(tr_deconv_t_kernel, dim3(tr_blocks(n2)), dim3(TR_NT), 0, st, W,
                               reinterpret_cast<unsigned*>(blob + lp.wt_off), sc, lp.K, lp.cin, lp.cin, lp.cout);
        }
        if (lp.wt_in_off) {
            lp.wt_in_inv_scale = 1.0f / sc;
            const int rows = (lp.cin + 63) / 64 * 64;
            const size_t n2 = (size_t)lp.K * rows * lp.cout / 2;
            hipLaunchKernelGGL(tr_deconv_t_kernel, dim3(tr_blocks(n2)), dim3(TR_NT), 0, st, W,
                               reinterpret_cast<unsigned*>(blob + lp.wt_in_off), sc, lp.K, lp.cin, rows, lp.cout);
        }
    }
}

extern "C" size_t wn_grad_sumsq_workspace_bytes(size_t n) { return align_up((size_t)ss_blocks(std::max<size_t>(n, 1)) * sizeof(double), 256); }

extern "C" int wn_grad_sumsq(const float* g, size_t n, double* acc, int accumulate, void* ws, size_t ws_bytes, void* stream) {
    if (!g || !acc || !ws || n < 1) return wn_fail(nullptr, WN_EINVAL, "wn_grad_sumsq: bad argument");
    if (ws_bytes < wn_grad_sumsq_workspace_bytes(n))
        return wn_fail(nullptr, WN_EINVAL, "wn_grad_sumsq: workspace %zu < %zu bytes", ws_bytes, wn_grad_sumsq_workspace_bytes(n));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int nb = ss_blocks(n);
    double* part = reinterpret_cast<double*>(ws);
    hipLaunchKernelGGL(tr_sumsq1_kernel, dim3(nb), dim3(TR_NT), 0, st, g, n, part);
    hipLaunchKernelGGL(tr_sumsq2_kernel, dim3(1), dim3(TR_NT), 0, st, part, nb, acc, accumulate);
    WN_HIP(nullptr, hipGetLastError());
    return WN_OK;
}

extern "C" int wn_grad_combine(const float* rows, size_t n, size_t row_stride, int S, float* out, void* stream) {
    if (!rows || !out || n < 1) return wn_fail(nullptr, WN_EINVAL, "wn_grad_combine: bad argument");
    if (S < 1 || S > 64) return wn_fail(nullptr, WN_EINVAL, "wn_grad_combine: S = %d is outside [1, 64]", S);
    if (row_stride < n) return wn_fail(nullptr, WN_EINVAL, "wn_grad_combine: row_stride %zu < n = %zu", row_stride, n);
    const float inv = 1.0f / (float)S;
    const uintptr_t bits = (uintptr_t)rows | (uintptr_t)out | (uintptr_t)(row_stride * sizeof(float));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (bits & 15) hipLaunchKernelGGL(tr_combine_kernel<false>, dim3(tr_blocks(n)), dim3(TR_NT), 0, st, rows, n, row_stride, S, inv, out);
    else hipLaunchKernelGGL(tr_combine_kernel<true>, dim3(tr_blocks(std::max<size_t>(n / 4, 4))), dim3(TR_NT), 0, st, rows, n, row_stride, S, inv, out);
    WN_HIP(nullptr, hipGetLastError());
    return WN_OK;
}

extern "C" int wn_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, size_t n, float lr_t, float beta1,
                                float beta2, float eps, float ema_decay_t, const double* sumsq, float clip_norm, void* stream) {
    if (!p || !g || !m || !v || n < 1) return wn_fail(nullptr, WN_EINVAL, "wn_adam_ema_step: bad argument");
    if (sumsq && !(clip_norm > 0.f)) return wn_fail(nullptr, WN_EINVAL, "wn_adam_ema_step: clip_norm must be positive");
    const AdamArgs a{p, g, m, v, ema, n, lr_t, beta1, beta2, eps, ema_decay_t, clip_norm, sumsq};
    const uintptr_t bits = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (bits & 15) hipLaunchKernelGGL(tr_adam_kernel<false>, dim3(tr_blocks(n)), dim3(TR_NT), 0, st, a);
    else hipLaunchKernelGGL(tr_adam_kernel<true>, dim3(tr_blocks(std::max<size_t>(n / 4, 4))), dim3(TR_NT), 0, st, a);
    WN_HIP(nullptr, hipGetLastError());
    return WN_OK;
}

extern "C" size_t wn_teacher_set_weights_workspace_bytes(const wn_handle* h) {
    if (!h || !h->finalized || !train_supported(h)) return 0;
    return align_up((size_t)scale_slots(h).total() * sizeof(float), 256);
}

extern "C" int wn_teacher_set_weights(wn_handle* h, const float* params, size_t params_floats, const float* up_params,
                                      size_t up_floats, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "wn_teacher_set_weights";
    if (!h) return wn_fail(nullptr, WN_EINVAL, "%s: null handle", fn);
    const wn_config& c = h->cfg;
    if (c.kind != WN_KIND_TEACHER) return wn_fail(h, WN_EINVAL, "%s: this is a ParallelWavenet student handle; only a teacher is re-packed", fn);
    if (!h->finalized) return wn_fail(h, WN_ESTATE, "%s: call wn_finalize first", fn);
    if (!train_supported(h))
        return wn_fail(h, WN_EINVAL, "%s: the handle has no parameter layout (mu-law, ce and weight-norm teachers have no weight "
                       "gradients)", fn);
    if (!params || !ws) return wn_fail(h, WN_EINVAL, "%s: null argument", fn);
    const TeacherParamLayout& Q = h->teacher.lay;
    if (params_floats != Q.table.floats)
        return wn_fail(h, WN_EINVAL, "%s: params holds %zu floats, the layout of wn_teacher_grad_info has %zu", fn, params_floats,
                       Q.table.floats);
    if (up_params) {
        if (c.use_resize_conv)
            return wn_fail(h, WN_EINVAL, "%s: use_resize_conv: the resize-conv upsampler has no parameter layout; pass no up_params", fn);
        if (wn_deconv_grad_floats(h, "") == 0)
            return wn_fail(h, WN_EINVAL, "%s: the upsampler has no parameter layout (wn_deconv_grad_floats is 0)", fn);
        if (up_floats != h->stacks[0].table.floats)
            return wn_fail(h, WN_EINVAL, "%s: up_params holds %zu floats, the layout of wn_deconv_grad_info has %zu", fn, up_floats,
                           h->stacks[0].table.floats);
    }
    const size_t need = wn_teacher_set_weights_workspace_bytes(h);
    if (ws_bytes < need) return wn_fail(h, WN_EINVAL, "%s: workspace %zu < %zu bytes", fn, ws_bytes, need);
    WN_SWITCH(h, "wn_teacher_set_weights");

    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int W = c.width, S = c.skip_width, G = c.gate_width, H = G / 2, Cd = c.deconv_width, OW = c.out_width, K = 3 * W + Cd;
    float* blob = h->d_blob;
    ArPack& A = h->ar;
    TeacherPack& T = h->teacher;
    const ScaleSlots SL = scale_slots(h);
    unsigned* amax = reinterpret_cast<unsigned*>(ws);
    auto scatter = [&](const float* src, size_t dst_off, int cin, int cout, int ld, int col0) {
        hipLaunchKernelGGL(tr_scatter_kernel, dim3(tr_blocks((size_t)cin * cout)), dim3(TR_NT), 0, st,
                           ScatterArgs{src, blob + dst_off, cin, cout, ld, col0});
    };
    auto copy = [&](const float* src, size_t dst_off, int n) { scatter(src, dst_off, 1, n, 1, 0); };
    auto add = [&](const float* x, const float* y, size_t dst_off, int n) {
        hipLaunchKernelGGL(tr_add_kernel, dim3(tr_blocks(n)), dim3(TR_NT), 0, st, x, y, blob + dst_off, n);
    };
    auto absmax = [&](const float* x, size_t n, int slot) { absmax_launch(x, n, amax + slot, st); };
    auto frag = [&](size_t src_off, size_t dst_off, int rows, int Kc) {
        const size_t total = (size_t)((rows + 15) / 16) * (Kc / 16) * 256;
        hipLaunchKernelGGL(tr_frag_kernel, dim3(tr_blocks(total)), dim3(TR_NT), 0, st, blob + src_off, blob + dst_off, rows,
                           Kc);
    };
    const size_t nl = A.layers.size();
    // From here on the handle changes: tapes written under the old weights are refused, also after a failure below
    T.serial = wn_repack_serial_next();

    // ---- 1. absolute maxima of the sources of every split pack
    WN_HIP(h, hipMemsetAsync(amax, 0, (size_t)SL.total() * sizeof(unsigned), st));
    absmax(params + Q.skip_start.W, (size_t)W * S, SL.wss());
    absmax(params + Q.out1.W, (size_t)S * S, SL.wo1a());
    absmax(params + Q.cond_out1.W, (size_t)Cd * S, SL.wo1b());
    absmax(params + Q.out2.W, (size_t)S * OW, SL.wo2());
    for (size_t i = 0; i < nl; ++i) {
        absmax(params + Q.layers[i].dil.W, (size_t)3 * W * G, SL.dil((int)i));
        absmax(params + Q.layers[i].cond.W, (size_t)Cd * G, SL.cond((int)i));
        absmax(params + Q.layers[i].res.W, (size_t)H * W, SL.res((int)i));
        absmax(params + Q.layers[i].skip.W, (size_t)H * S, SL.skip((int)i));
    }
    DeconvStackPack* sp = up_params ? &h->stacks[0] : nullptr;
    if (sp) wn_repack_deconv_absmax(*sp, up_params, amax + SL.up(0), st);

    // ---- 2. the plain fp32 matrices and biases (wn_pack_ar), the composites, the fp32 fragments
    copy(params + Q.start.W, A.start_off, 3 * W);
    copy(params + Q.start.b, A.start_off + 3 * (size_t)W, W);
    scatter(params + Q.skip_start.W, A.wss_off, W, S, W, 0);
    copy(params + Q.skip_start.b, A.bss_off, S);
    for (size_t i = 0; i < nl; ++i) {
        ArLayerPack& lp = A.layers[i];
        const float* wd = params + Q.layers[i].dil.W;
        for (int tap = 0; tap < 3; ++tap) scatter(wd + (size_t)tap * W * G, lp.wd_off, W, G, K, tap * W);
        scatter(params + Q.layers[i].cond.W, lp.wd_off, Cd, G, K, 3 * W);
        add(params + Q.layers[i].dil.b, params + Q.layers[i].cond.b, lp.bd_off, G);
        copy(params + Q.layers[i].cond.b, lp.bc_off, G);
        scatter(params + Q.layers[i].res.W, lp.wrs_off, H, W, H, 0);
        scatter(params + Q.layers[i].skip.W, lp.wrs_off + (size_t)W * H, H, S, H, 0);
        copy(params + Q.layers[i].res.b, lp.brs_off, W);
        copy(params + Q.layers[i].skip.b, lp.brs_off + W, S);
        if (i > 0) {
            const ArLayerPack& pv = A.layers[i - 1];
            hipLaunchKernelGGL(tr_bm_kernel, dim3(tr_blocks(G)), dim3(TR_NT), 0, st, blob + lp.wd_off, blob + lp.bd_off,
                               blob + pv.brs_off, blob + lp.bm_off, G, W, K);
        }
    }
    wn_ar_compose(h, st);        // composite matrices and the [wd | wcomp] fragments: wn_finalize's own launches, on this stream
    scatter(params + Q.out1.W, A.wo1_off, S, S, S + Cd, 0);
    scatter(params + Q.cond_out1.W, A.wo1_off, Cd, S, S + Cd, S);
    add(params + Q.out1.b, params + Q.cond_out1.b, A.bo1_off, S);
    copy(params + Q.cond_out1.b, A.bco1_off, S);
    scatter(params + Q.out2.W, A.wo2_off, S, OW, S, 0);
    copy(params + Q.out2.b, A.bo2_off, OW);
    if (A.wss_b_off) {           // the batched step's A-fragment copies exist
        frag(A.wss_off, A.wss_b_off, S, W);
        for (size_t i = 0; i < nl; ++i) {
            ArLayerPack& lp = A.layers[i];
            if (i == 0) frag(lp.wd_off, lp.wd_b_off, G, K);
            frag(lp.wrs_off, lp.wrs_b_off, W + S, H);
            copy(blob + lp.brs_off, lp.brs_gate_off, W + S);
            copy(blob + lp.bd_off, lp.brs_gate_off + W + S, G);
        }
        frag(A.wo1_off, A.wo1_b_off, S, S + Cd);
        frag(A.wo2_off, A.wo2_b_off, OW, S);
    }
    if (sp) wn_repack_deconv_plain(h, *sp, up_params, st);

    // ---- 3. the maxima come back (the call's one read-back: it synchronises the stream); pick_scale on the host
    std::vector<float> mx(SL.total());
    WN_HIP(h, hipMemcpyAsync(mx.data(), amax, mx.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    WN_HIP(h, hipStreamSynchronize(st));
    auto scale_of = [&](std::initializer_list<int> slots) {
        float m = 0.f;
        for (int s : slots) m = std::max(m, mx[s]);
        return pick_scale(&m, 1);
    };

    // ---- 4. the split-fp16 packs (wn_pack_teacher, wn_pack_deconv, wn_pack_deconv_bwd)
    auto tile = [&](TeacherGemmPack& g, float sc, size_t src_off, int ld, int rowkind, int M, int srckind, int R, int c0) {
        g.inv_scale = 1.0f / sc;
        TileArgs a{blob + src_off, reinterpret_cast<unsigned*>(blob + g.w_off), sc, ld, g.nks, g.mtiles, rowkind, M, H, srckind, R, c0, G, W};
        hipLaunchKernelGGL(tr_tile_kernel, dim3(tr_blocks((size_t)g.mtiles * g.nks * 4 * 512)), dim3(TR_NT), 0, st, a);
    };
    auto tile_bias = [&](const TeacherGemmPack& g, size_t b_off, int rowkind, int M) {
        hipLaunchKernelGGL(tr_tile_bias_kernel, dim3(tr_blocks((size_t)g.mtiles * 64)), dim3(TR_NT), 0, st, blob + b_off,
                           blob + g.b_off, g.mtiles * 64, rowkind, M, H);
    };
    const float s_wss = scale_of({SL.wss()}), s_wo1 = scale_of({SL.wo1a(), SL.wo1b()}), s_wo2 = scale_of({SL.wo2()});
    tile(T.skip_start, s_wss, A.wss_off, W, ROW_IDENT, S, SRC_DIRECT, 0, 0);
    tile_bias(T.skip_start, A.bss_off, ROW_IDENT, S);
    tile(T.out1, s_wo1, A.wo1_off, S + Cd, ROW_IDENT, S, SRC_DIRECT, 0, 0);
    tile_bias(T.out1, A.bo1_off, ROW_IDENT, S);
    tile(T.out2, s_wo2, A.wo2_off, S, ROW_IDENT, OW, SRC_DIRECT, 0, 0);
    tile_bias(T.out2, A.bo2_off, ROW_IDENT, OW);
    for (size_t i = 0; i < nl; ++i) {
        const ArLayerPack& lp = A.layers[i];
        TeacherLayerPack& tl = T.layers[i];
        const int li = (int)i;
        tile(tl.gate, scale_of({SL.dil(li), SL.cond(li)}), lp.wd_off, K, ROW_GATE, G, SRC_DIRECT, 0, 0);
        tile_bias(tl.gate, lp.bd_off, ROW_GATE, G);
        tile(tl.rs, scale_of({SL.res(li), SL.skip(li)}), lp.wrs_off, H, ROW_IDENT, W + S, SRC_DIRECT, 0, 0);
        tile_bias(tl.rs, lp.brs_off, ROW_IDENT, W + S);
    }
    if (T.vjp_ok) {              // the transposed packs: zero bias, as packed
        tile(T.skip_start_t, s_wss, A.wss_off, W, ROW_IDENT, W, SRC_T, S, 0);
        tile(T.out1_t, scale_of({SL.wo1a()}), A.wo1_off, S + Cd, ROW_IDENT, S, SRC_T, S, 0);
        tile(T.out2_t, s_wo2, A.wo2_off, S, ROW_IDENT, S, SRC_T, OW, 0);
        for (size_t i = 0; i < nl; ++i) {
            const ArLayerPack& lp = A.layers[i];
            TeacherLayerPack& tl = T.layers[i];
            const int li = (int)i;
            tile(tl.rs_t, scale_of({SL.res(li), SL.skip(li)}), lp.wrs_off, H, ROW_IDENT, H, SRC_T, W + S, 0);
            tile(tl.gate_t, scale_of({SL.dil(li)}), lp.wd_off, K, ROW_IDENT, W, SRC_GATE_T, 0, 0);
            if (T.denc_ok) tile(tl.cond_t, scale_of({SL.cond(li)}), lp.wd_off, K, ROW_IDENT, Cd, SRC_T, G, 3 * W);
        }
        if (T.denc_ok) tile(T.cond_out1_t, scale_of({SL.wo1b()}), A.wo1_off, S + Cd, ROW_IDENT, Cd, SRC_T, S, S);
    }
    if (sp) wn_repack_deconv_split(h, *sp, up_params, mx.data() + SL.up(0), st);
    WN_HIP(h, hipGetLastError());
    return WN_OK;
}
