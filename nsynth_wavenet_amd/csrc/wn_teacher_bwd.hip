// Input VJP of the teacher: d out_params [B,T,ow] -> d wav [B,T], weights frozen.
//
// The tape (wn_teacher_forward_tape) holds what the reverse pass reads: a header, the pre-ReLU skip sum s and out1 rows
// (accumulator layout, as the forward keeps them), and sigma / tanh of every gate.  The reverse pass runs the forward's
// GEMM kernel (wn_teacher.hip) on the transposed packs: d out2 and d out1 through the ReLU masks (MASK), then per layer from
// the last one dm = W_res^T dl + W_skip^T ds with the gate derivative in the epilogue (BGATE) and
// dl += sum_k W_dil[k]^T dd(t + (2-k) d) in place (RS, anti-causal taps: dd rows carry a zero right pad of 2 * max dilation),
// then skip_start^T and the start conv transposed.  The operands are split-fp16 like the forward's, so d out_params enter
// scaled by a power of two that brings their largest magnitude to [1, 2) (found on the device) and d wav leaves unscaled: the
// VJP is linear.  The weight gradients (wn_teacher_wgrad.hip) hook into the same pass.
#include <mutex>
#include <unordered_map>

#include "wn_teacher.h"
#include "wn_g4.h"

namespace {
struct TapeRec {
    uint64_t serial;
    int B;
    long long T;
    int F;              // > 0: a training tape (wn_teacher_forward_train_tape) for F mel frames
    TgDropout drop;     // the dropout its forward applied (wn_teacher_forward_train_tape_dropout; mode 0: none)
};
std::mutex g_tape_mu;
std::unordered_map<const void*, TapeRec> g_tapes;   // tape address -> the handle and shape that last wrote it

struct TbHead {
    unsigned w[8];
};
__global__ void tb_header_kernel(TbHead v, unsigned* __restrict__ dst) {
    if (threadIdx.x < 8) dst[threadIdx.x] = v.w[threadIdx.x];
}

// d out_params [B,T,ow] (scaled by scal[0]) -> G4 rows of Kp channels (zero beyond ow and from column T on)
__global__ __launch_bounds__(256) void tb_dout_kernel(const float* __restrict__ dout, const float* __restrict__ scal,
                                                      unsigned* __restrict__ g4, long long T, long long Tp, int ow, int Kp) {
    const int b = blockIdx.z, gr = blockIdx.y, NG = Kp / 8;
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= Tp) return;
    const float sc = scal[0];
    wn_u4 hw, lw;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float o[2];
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const int ch = wn_g4_channel(gr, i) + hh;
            o[hh] = c < T && ch < ow ? dout[((size_t)b * T + c) * ow + ch] * sc : 0.f;
        }
        unsigned a, a2;
        wn_split_pair(o[0], o[1], a, a2);
        hw[i] = a;
        lw[i] = a2;
    }
    wn_g4_store(g4 + (size_t)b * Kp * Tp, NG, Tp, gr, c, hw, lw);
}

// a start conv transposed (tg_start_kernel: l0(t) = b + w0 x(t-3) + w1 x(t-2) + w2 x(t-1)):
// dx(t) = scal[1] sum_c (w0[c] dl0[c](t+3) + w1[c] dl0[c](t+2) + w2[c] dl0[c](t+1)); 64 columns x 4 waves of channels.
// ADD: added to dx (the student's running d x) instead of stored (the teacher's d wav)
template <bool ADD>
__global__ __launch_bounds__(256) void tb_dx_kernel(const unsigned* __restrict__ dl, const float* __restrict__ wb,
                                                    const float* __restrict__ scal, float* __restrict__ dx, int W, long long T,
                                                    long long Tp) {
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y, NG = W / 8;
    const long long t = (long long)blockIdx.x * 64 + lane;
    float acc = 0.f;
    if (t < T) {
        const unsigned* base = dl + (size_t)b * W * Tp;
        for (int gr = wave; gr < NG; gr += 4) {
            for (int k = 0; k < 3; ++k) {
                const long long col = t + 3 - k;
                if (col >= T) continue;
                wn_u4 hw, lw;
                wn_g4_load(base, NG, Tp, gr, col, hw, lw);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float v0, v1;
                    wn_join_pair(hw[i], lw[i], v0, v1);
                    const int ch = wn_g4_channel(gr, i);
                    acc = fmaf(wb[k * W + ch], v0, acc);
                    acc = fmaf(wb[k * W + ch + 1], v1, acc);
                }
            }
        }
    }
    red[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && t < T) {       // both forms as one expression: the sum's product with scal[1] contracts into the add
        if (ADD) dx[(size_t)b * T + t] += (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]) * scal[1];
        else dx[(size_t)b * T + t] = (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]) * scal[1];
    }
}
}  // namespace

void wn_tape_register(const void* tape, uint64_t serial, int B, long long T, int F) {
    std::lock_guard<std::mutex> lk(g_tape_mu);
    g_tapes[tape] = TapeRec{serial, B, T, F, TgDropout{}};
}
bool wn_tape_lookup(const void* tape, uint64_t* serial, int* B, long long* T, int* F) {
    std::lock_guard<std::mutex> lk(g_tape_mu);
    auto it = g_tapes.find(tape);
    if (it == g_tapes.end()) return false;
    *serial = it->second.serial; *B = it->second.B; *T = it->second.T; *F = it->second.F;
    return true;
}
void wn_tb_dout(const float* dout, const float* scal, unsigned* g4, int B, long long T, long long Tp, int ow, int Kp,
                hipStream_t st) {
    hipLaunchKernelGGL(tb_dout_kernel, dim3((unsigned)((Tp + 255) / 256), Kp / 8, B), dim3(256), 0, st, dout, scal, g4, T, Tp,
                       ow, Kp);
}
void wn_tb_dx(const unsigned* dl, const float* wb, const float* scal, float* dx, int B, int W, long long T, long long Tp, bool add,
              hipStream_t st) {
    const dim3 grid((unsigned)((T + 63) / 64), B);
    if (add) hipLaunchKernelGGL(tb_dx_kernel<true>, grid, dim3(256), 0, st, dl, wb, scal, dx, W, T, Tp);
    else hipLaunchKernelGGL(tb_dx_kernel<false>, grid, dim3(256), 0, st, dl, wb, scal, dx, W, T, Tp);
}

BLayout b_layout(const wn_handle* h, int B, long long T) {
    const wn_config& c = h->cfg;
    BLayout L;
    L.Tp = (T + TG_TN - 1) / TG_TN * TG_TN;
    L.RD = L.Tp + 2 * (1ll << (c.num_stages - 1));
    L.Kp = h->teacher.out2_t.nks * 32;
    size_t o = 0;
    auto carve = [&](size_t words) { size_t r = o; o += align_up(words * 4, 256); return r; };
    L.scal = carve(4 + WN_NPART);
    L.dout = carve((size_t)B * L.Kp * L.Tp);
    L.dh1 = carve((size_t)B * c.skip_width * L.Tp);
    L.ds = carve((size_t)B * c.skip_width * L.Tp);
    L.dl = carve((size_t)B * c.width * L.Tp);
    L.dd = carve((size_t)B * c.gate_width * L.RD);
    L.total = o;
    return L;
}

int tb_check(wn_handle* h, const char* fn) {
    if (!h) return wn_fail(nullptr, WN_EINVAL, "%s: null handle", fn);
    const wn_config& c = h->cfg;
    if (c.kind != WN_KIND_TEACHER)
        return wn_fail(h, WN_EINVAL, "%s: this is a ParallelWavenet student handle; the teacher's input VJP runs under the "
                       "TEACHER's handle", fn);
    if (c.loss_type == WN_LOSS_CE)
        return wn_fail(h, WN_EINVAL, "%s: cross-entropy (ce) teacher: the distillation losses need a mol or gauss teacher "
                       "(parallel_wavenet.py:133-135)", fn);
    if (c.use_mu_law)
        return wn_fail(h, WN_EINVAL, "%s: mu-law teacher: mu-law students and teachers are not supported by the "
                       "distillation losses", fn);
    if (!h->finalized) return wn_fail(h, WN_ESTATE, "%s: call wn_finalize first", fn);
    if (!h->teacher.vjp_ok)
        return wn_fail(h, WN_EINVAL, "%s: width %d, skip_width %d, gate_width / 2 = %d must be multiples of 64 and "
                       "out_width <= 64 for the transposed GEMMs", fn, c.width, c.skip_width, c.gate_width / 2);
    return WN_OK;
}

extern "C" size_t wn_teacher_tape_bytes(const wn_handle* h, int B, int64_t T) {
    if (!h || !h->finalized || h->cfg.kind != WN_KIND_TEACHER || B < 1 || T < 1) return 0;
    return tape_layout(h, B, T).total;
}

extern "C" size_t wn_teacher_backward_workspace_bytes(const wn_handle* h, int B, int64_t T) {
    if (!h || !h->finalized || h->cfg.kind != WN_KIND_TEACHER || !h->teacher.vjp_ok || B < 1 || T < 1) return 0;
    return b_layout(h, B, T).total;
}

int tb_tape_forward(wn_handle* h, const char* fn, uint32_t magic, const float* wav, const float* mel, int B, int F, int64_t T,
                    float* out_params, void* tape, const TgTape& regions, void* ws, size_t ws_bytes, void* stream) {
    TbHead hd;
    const uint64_t ser = h->teacher.serial;
    hd.w[0] = magic; hd.w[1] = (unsigned)ser; hd.w[2] = (unsigned)(ser >> 32); hd.w[3] = (unsigned)B;
    hd.w[4] = (unsigned)T; hd.w[5] = (unsigned)((uint64_t)T >> 32); hd.w[6] = (unsigned)h->teacher.layers.size();
    hd.w[7] = (unsigned)F;
    hipLaunchKernelGGL(tb_header_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), hd,
                       reinterpret_cast<unsigned*>(tape));
    if (int rc = tg_forward(h, fn, wav, mel, B, F, T, out_params, ws, ws_bytes, regions, stream)) return rc;
    std::lock_guard<std::mutex> lk(g_tape_mu);
    g_tapes[tape] = TapeRec{ser, B, (long long)T, magic == TB_MAGIC_TRAIN ? F : 0, regions.drop};
    return WN_OK;
}

extern "C" int wn_teacher_forward_tape(wn_handle* h, const float* wav, const float* mel, int B, int F, int64_t T,
                                       float* out_params, void* tape, size_t tape_bytes, void* ws, size_t ws_bytes,
                                       void* stream) {
    const char* fn = "wn_teacher_forward_tape";
    if (int rc = tb_check(h, fn)) return rc;
    if (int rc = tg_forward_check(h, fn, wav, mel, B, F, T, out_params, ws)) return rc;
    if (!tape) return wn_fail(h, WN_EINVAL, "%s: bad argument (tape)", fn);
    const TapeLayout TL = tape_layout(h, B, T);
    if (tape_bytes < TL.total) return wn_fail(h, WN_ENOMEM, "%s: tape %zu < %zu bytes", fn, tape_bytes, TL.total);
    const WnWork work(h);
    return tb_tape_forward(h, fn, TB_MAGIC, wav, mel, B, F, T, out_params, tape, tape_regions(TL, tape), ws, ws_bytes, stream);
}

int tb_tape_check(wn_handle* h, const char* fn, const void* tape, size_t tape_bytes, int B, int64_t T, int* F,
                  TgDropout* drop) {
    const TapeLayout TL = tape_layout(h, B, T);
    if (tape_bytes < TL.total)
        return wn_fail(h, WN_EINVAL, "%s: a tape of %zu bytes cannot hold B = %d, T = %lld (%zu bytes)", fn, tape_bytes, B,
                       (long long)T, TL.total);
    std::lock_guard<std::mutex> lk(g_tape_mu);
    auto it = g_tapes.find(tape);
    if (it == g_tapes.end() || it->second.serial != h->teacher.serial)
        return wn_fail(h, WN_EINVAL, "%s: the tape was not written by wn_teacher_forward_tape of this handle", fn);
    if (it->second.B != B || it->second.T != (long long)T)
        return wn_fail(h, WN_EINVAL, "%s: the tape holds B = %d, T = %lld, not B = %d, T = %lld", fn, it->second.B,
                       it->second.T, B, (long long)T);
    *F = it->second.F;
    if (drop) *drop = it->second.drop;
    return WN_OK;
}

int tb_reverse(wn_handle* h, const void* tape, const float* d_out_params, int B, int64_t T, float* d_wav, void* ws,
               void* stream, const TwCtx* wg, const TgDropout& dr) {
    const BLayout L = b_layout(h, B, T);
    const wn_config& c = h->cfg;
    const int W = c.width, S = c.skip_width, G = c.gate_width, H = G / 2;
    const TeacherPack& P = h->teacher;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const TbWork w = tb_work(L, ws);
    const TgTape tp = tape_regions(tape_layout(h, B, T), const_cast<void*>(tape));
    const long long Tp = L.Tp;

    // operand scale
    wn_pow2_scale(d_out_params, (long long)B * T * c.out_width, w.scal + 4, w.scal, nullptr, st);
    wn_tb_dout(d_out_params, w.scal, w.dout, B, T, Tp, c.out_width, L.Kp, st);
    WN_HIP(h, hipMemsetAsync(w.dl, 0, (size_t)B * W * Tp * 4, st));
    WN_HIP(h, hipMemsetAsync(w.dd, 0, (size_t)B * G * L.RD * 4, st));

    auto args = [&](const TeacherGemmPack& g, unsigned* og4, long long obstride, long long orowlen, int C) {
        TgArgs a = tg_pack_args(h, g, T);
        a.og4 = og4; a.og4_bstride = obstride; a.og4_rowlen = (int)orowlen; a.og4_col0 = 0; a.og4_ng = C / 8;
        return a;
    };
    const TgSeg seg_ds = tg_seg_g4(w.ds, (long long)S * Tp, Tp, 0, S), seg_dl = tg_seg_g4(w.dl, (long long)W * Tp, Tp, 0, W);
    {   // d relu(h1) = W_out2^T d out, masked by h1 > 0  (wavenet.py:290-292)
        TgArgs a = args(P.out2_t, w.dh1, (long long)S * Tp, Tp, S);
        a.seg[0] = tg_seg_g4(w.dout, (long long)L.Kp * Tp, Tp, 0, L.Kp); a.nseg = 1;
        a.tape = tp.h1; a.tape_bstride = (long long)S * Tp; a.tape_nmb = S / 16;
        wn_tg_launch(TG_EPI_MASK, a, P.out2_t.mtiles, B, Tp, st);
    }
    if (wg) {
        if (int rc = tw_aux(h, *wg, st)) return rc;
        if (int rc = tw_head(h, *wg, st, 0)) return rc;
    }
    {   // ds = W_out1^T d h1 (its skip columns), masked by s > 0  (wavenet.py:283-289)
        TgArgs a = args(P.out1_t, w.ds, (long long)S * Tp, Tp, S);
        a.seg[0] = tg_seg_g4(w.dh1, (long long)S * Tp, Tp, 0, S); a.nseg = 1;
        a.tape = tp.s; a.tape_bstride = (long long)S * Tp; a.tape_nmb = S / 16;
        wn_tg_launch(TG_EPI_MASK, a, P.out1_t.mtiles, B, Tp, st);
    }
    if (wg)
        if (int rc = tw_head(h, *wg, st, 1)) return rc;
    const bool drop_in = dr.mode == WN_DROPOUT_INPUTS, drop_all = dr.mode == WN_DROPOUT_ALL;
    for (size_t li = P.layers.size(); li-- > 0;) {
        const TeacherLayerPack& tl = P.layers[li];
        // res_dropout of layer li's output: dl = d l_{li+1} passes the mask before the residual conv and the
        // identity path see it; the last layer's output was neither masked nor read
        if (drop_all && li + 1 < P.layers.size()) wn_dropout_g4(w.dl, w.dl, B, W, Tp, 0, T, dr, (int)li + 1, st);
        {   // dm = W_res^T dl + W_skip^T ds -> dd through the gate derivative  (wavenet.py:264-277 transposed)
            TgArgs a = args(tl.rs_t, w.dd, (long long)G * L.RD, L.RD, G);
            a.seg[0] = seg_dl; a.seg[1] = seg_ds; a.nseg = 2;
            a.tape = tp.g + li * (size_t)B * G * Tp; a.tape_bstride = (long long)G * Tp; a.tape_nmb = G / 16;
            a.tape_hoff = H / 16;
            wn_tg_launch(TG_EPI_BGATE, a, tl.rs_t.mtiles, B, Tp, st);
        }
        if (wg)     // dl = d l_{li+1} and dd_li are complete here, before the dilated step overwrites dl
            if (int rc = tw_layer(h, *wg, li, st)) return rc;
        {   // dl += sum_k W_dil[k]^T dd(t + (2 - k) dilation)  (wavenet.py:243-262 transposed)
            TgArgs a = args(tl.gate_t, w.dl, (long long)W * Tp, Tp, W);
            for (int k = 0; k < 3; ++k) a.seg[k] = tg_seg_g4(w.dd, (long long)G * L.RD, L.RD, (long long)(2 - k) * tl.dilation, G);
            a.nseg = 3;
            a.res_mtiles = W / 64;
            wn_tg_launch(TG_EPI_RS, a, tl.gate_t.mtiles, B, Tp, st);
        }
    }
    if (drop_in) {      // l_0 and s = skip_start(l_0) were masked after skip_start read the raw l_0: ds reaches it masked
        wn_dropout_g4(w.dl, w.dl, B, W, Tp, 0, T, dr, 0, st);
        wn_dropout_g4(w.ds, w.ds, B, S, Tp, 0, T, dr, 1, st);
    }
    {   // dl0 += W_skip_start^T ds  (wavenet.py:231-233)
        TgArgs a = args(P.skip_start_t, w.dl, (long long)W * Tp, Tp, W);
        a.seg[0] = seg_ds; a.nseg = 1;
        a.res_mtiles = W / 64;
        wn_tg_launch(TG_EPI_RS, a, P.skip_start_t.mtiles, B, Tp, st);
    }
    if (drop_all) wn_dropout_g4(w.dl, w.dl, B, W, Tp, 0, T, dr, 0, st);         // skip_start read the masked l_0
    if (wg)
        if (int rc = tw_tail(h, *wg, st)) return rc;
    if (d_wav) wn_tb_dx(w.dl, h->d_blob + h->ar.start_off, w.scal, d_wav, B, W, T, Tp, false, st);
    WN_HIP(h, hipGetLastError());
    return WN_OK;
}

extern "C" int wn_teacher_backward_input(wn_handle* h, const void* tape, size_t tape_bytes, const float* d_out_params,
                                         int B, int64_t T, float* d_wav, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "wn_teacher_backward_input";
    if (int rc = tb_check(h, fn)) return rc;
    if (B < 1 || T < 1 || !tape || !d_out_params || !d_wav || !ws) return wn_fail(h, WN_EINVAL, "%s: bad argument", fn);
    int F = 0;
    TgDropout dr;
    if (int rc = tb_tape_check(h, fn, tape, tape_bytes, B, T, &F, &dr)) return rc;
    const BLayout L = b_layout(h, B, T);
    if (ws_bytes < L.total) return wn_fail(h, WN_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, L.total);
    const WnWork work(h);
    return tb_reverse(h, tape, d_out_params, B, T, d_wav, ws, stream, nullptr, dr);
}
