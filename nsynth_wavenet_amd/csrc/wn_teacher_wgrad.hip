// Weight gradients of the teacher: d out_params -> d of every variable of the residual stack and head.
//
// The reverse pass (wn_teacher_bwd.hip) already holds every cotangent a weight gradient needs as G4 rows (d out, d h1, ds, and per layer dl
// and dd); the training tape adds the activations they multiply (l_i, enc, the scaled audio; m_i, relu(s), relu(h1) are
// re-formed from the gate / pre-ReLU tapes by tw_act_kernel).  Each gradient is dW[in][out] = sum_{b,t} X[in][b,t] dY[out][b,t]:
// a GEMM whose reduction index is TIME, the column index of both operands.  tw_gemm_kernel puts time into the MFMA K slot by
// transposing BOTH operands on their way into LDS: a thread loads eight consecutive columns of one G4 group (128 contiguous
// bytes: 8 channels x 8 columns of fp16), transposes the 8 x 8 halves in registers and writes eight 16-byte rows
// [channel][8 columns]; a lane's A (dY) or B (X) fragment of a 32-column K-step is then one ds_read_b128.  Split-fp16 like the
// forward (dY.hi X.hi + dY.hi X.lo + dY.lo X.hi, fp32 accumulation).
// Pad columns: the kernel walks valid columns only -- a column >= T is never loaded, its operand words are the constant 0 --
// so the tape's undefined (possibly NaN) contents at [T, Tp) and the rows enc lacks past TE never meet a product.  Taps
// t - (2 - k) d < 0 read the zero left pad of the l_i rows (IAF_LP columns, written by tg_start_kernel and copied with them).
// Time is cut into chunks of a fixed number of 256-column tiles, chosen on the host from B and T alone so that about TW_SLABS
// slabs exist (w_layout: one tile per chunk up to TW_SLABS / B tiles, so short clips fill the machine and long ones do not
// drown in slab traffic); workgroup (tile, op, b x chunk) stores its fp32 partial to its own slab with
// plain vector stores and tw_reduce_kernel sums the slabs in increasing (b, chunk) order, times scal[1]: one writer per
// element, no atomics, bit-identical repeats.  Biases are the products with the all-ones row of `aux`, whose rows 0-2 are the
// shifted audio (conv_start/W).
#include <algorithm>

#include "wn_teacher.h"
#include "wn_g4.h"
#include "wn_mfma_h.h"

namespace {
constexpr int TW_KT = 32;           // columns per LDS stage (one K-step)
constexpr int TW_LD = TW_KT + 8;    // halves per LDS row: 80 bytes, 16 lanes of a ds_read_b128 hit 16 distinct bank quads

// eight columns of one G4 group -> eight rows [channel][8 columns] of an LDS operand image.  r[j] = the four words of
// column j: word i holds channels wn_g4_channel(g, i) + {0, 1}
__device__ inline void tw_put(unsigned short (*img)[TW_LD], int g, int cb, const wn_u4 (&r)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            wn_u4 w;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                w[j] = p == 0 ? (r[2 * j][i] & 0xffffu) | (r[2 * j + 1][i] << 16)
                              : (r[2 * j][i] >> 16) | (r[2 * j + 1][i] & 0xffff0000u);
            const int c = wn_g4_channel(g, i) + p;
            *reinterpret_cast<wn_u4*>(&img[c][8 * cb]) = w;
        }
}

// One 128 (dY channels) x 128 (X channels) tile of one op over one chunk of one batch element, one 32-column K-step per LDS
// stage.  Staging: thread -> (operand = tid >> 7, plane = (tid >> 6) & 1, group = (tid >> 2) & 15, column block = tid & 3);
// the next stage's words are in flight while the MFMAs of this one run.  Waves 2 x 2, 4 x 4 MFMA tiles each.
__global__ __launch_bounds__(256) void tw_gemm_kernel(const TwArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned short lds[2][2][128][TW_LD];     // [dY | X][hi | lo][channel][column]
    const TwOp& o = a.op[blockIdx.y];
    const int mtiles = (o.M + 127) / 128, ntiles = (o.N + 127) / 128;
    if ((int)blockIdx.x >= mtiles * ntiles) return;
    const int mt = blockIdx.x % mtiles, nt = blockIdx.x / mtiles;
    const int b = blockIdx.z / a.nchunk, chunk = blockIdx.z % a.nchunk;
    const long long tbeg = (long long)chunk * a.chunk, tend = a.T < tbeg + a.chunk ? a.T : tbeg + a.chunk;
    const int nst = (int)((tend - tbeg + TW_KT - 1) / TW_KT);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, q = lane >> 4;
    const int wm = wave & 1, wn = wave >> 1;
    const int opnd = tid >> 7, plane = (tid >> 6) & 1, g = (tid >> 2) & 15, cb = tid & 3;

    // this thread's row of its operand (null: a group beyond the operand's channels -> zeros)
    const int C = opnd ? o.N : o.M, gg = (opnd ? nt : mt) * 16 + g;
    const wn_u4* src = nullptr;
    if (gg < C / 8)
        src = reinterpret_cast<const wn_u4*>((opnd ? o.x : o.dy) + (size_t)b * (opnd ? o.x_bs : o.dy_bs)) +
              (size_t)(plane * (C / 8) + gg) * (opnd ? o.x_rowlen : o.dy_rowlen) + (opnd ? o.x_col0 : o.dy_col0);
    auto fetch = [&](int stg, wn_u4 (&r)[8]) {
        const long long t = tbeg + (long long)stg * TW_KT + 8 * cb;
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = src && t + j < tend ? src[t + j] : (wn_u4){0u, 0u, 0u, 0u};
    };
    // 16-row blocks of this wave that hold channels at all
    const int na = min(4, max(0, (o.M - 128 * mt - 64 * wm + 15) / 16));
    const int nb = min(4, max(0, (o.N - 128 * nt - 64 * wn + 15) / 16));

    f4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][e] = (f4){0.f, 0.f, 0.f, 0.f};

    wn_u4 rr[8];
    fetch(0, rr);
    for (int stg = 0; stg < nst; ++stg) {
        tw_put(lds[opnd][plane], g, cb, rr);
        __syncthreads();
        if (stg + 1 < nst) fetch(stg + 1, rr);
        wn_u4 ah[4], al[4], bh[4], bl[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ah[i] = *reinterpret_cast<const wn_u4*>(&lds[0][0][64 * wm + 16 * i + n][8 * q]);
            al[i] = *reinterpret_cast<const wn_u4*>(&lds[0][1][64 * wm + 16 * i + n][8 * q]);
            bh[i] = *reinterpret_cast<const wn_u4*>(&lds[1][0][64 * wn + 16 * i + n][8 * q]);
            bl[i] = *reinterpret_cast<const wn_u4*>(&lds[1][1][64 * wn + 16 * i + n][8 * q]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < na)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < nb) acc[i][e] = mfma3(ah[i], al[i], bh[e], bl[e], acc[i][e]);
        __syncthreads();
    }

    // slab element [x channel][dY channel]: lane (q, n) holds dY channels 4 q .. 4 q + 3 of block i, x channel n of block e
    float* out = a.slab + (size_t)blockIdx.z * a.slab_stride + o.out_off;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int m0 = 128 * mt + 64 * wm + 16 * i + 4 * q, nn = 128 * nt + 64 * wn + 16 * e + n;
            if (m0 < o.M && nn < o.N) *reinterpret_cast<f4*>(out + (size_t)nn * o.M + m0) = acc[i][e];
        }
}

// grads[dst] = scal[1] * sum over the slabs, in slab order
__global__ __launch_bounds__(256) void tw_reduce_kernel(const TwRedArgs a) {
    const TwRed& r = a.r[blockIdx.y];
    const long long cnt = (long long)r.rows * r.cols;
    const float sc = a.scal[1];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (long long)gridDim.x * 256) {
        const int row = (int)(i / r.cols), col = (int)(i % r.cols);
        const float* p = a.slab + r.src_off + (size_t)row * r.src_ld + col;
        float acc = 0.f;
        for (int s = 0; s < a.nslab; ++s) acc += p[(size_t)s * a.slab_stride];
        a.grads[r.dst_off + (size_t)row * r.dst_ld + col] = acc * sc;
    }
}

// accumulator-layout tape rows -> G4 activation rows of C channels, zero from column T on:
// mode 0: relu(src) (the pre-ReLU s / out1 rows);  mode 1: sigma * tanh of a gate tape (m_i, the forward's own product)
__global__ __launch_bounds__(256) void tw_act_kernel(const float* __restrict__ src, long long src_bs, int nmb, int hoff,
                                                     unsigned* __restrict__ g4, long long T, long long Tp, int C, int mode) {
    const int b = blockIdx.z, gr = blockIdx.y, NG = C / 8;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= Tp) return;
    const int s4 = gr >> 2, kg = gr & 3;
    wn_u4 hw = (wn_u4){0u, 0u, 0u, 0u}, lw = hw;
    if (t < T) {
        const f4* p = reinterpret_cast<const f4*>(src + (size_t)b * src_bs) + ((size_t)(t >> 4) * nmb + 2 * s4) * 64 + 16 * kg + (t & 15);
#pragma unroll
        for (int mg = 0; mg < 2; ++mg) {
            f4 v = p[(size_t)mg * 64];
            if (mode == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
            } else {
                const f4 th = p[(size_t)(mg + hoff) * 64];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = v[r] * th[r];
            }
#pragma unroll
            for (int rp = 0; rp < 2; ++rp) {
                unsigned a0, a1;
                wn_split_pair(v[2 * rp], v[2 * rp + 1], a0, a1);
                hw[2 * mg + rp] = a0;
                lw[2 * mg + rp] = a1;
            }
        }
    }
    wn_g4_store(g4 + (size_t)b * C * Tp, NG, Tp, gr, t, hw, lw);
}

// aux rows [B][32][Tp] in G4: channel k < 3 = xs(t - 3 + k) (the three taps of tg_start_kernel), channel 3 = 1, the rest 0;
// all zero from column T on
__global__ __launch_bounds__(256) void tw_aux_kernel(const float* __restrict__ xs, unsigned* __restrict__ g4, long long T,
                                                     long long Tp) {
    const int b = blockIdx.z, gr = blockIdx.y, NG = TW_AUXC / 8;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= Tp) return;
    wn_u4 hw = (wn_u4){0u, 0u, 0u, 0u}, lw = hw;
    if (t < T && gr == 0) {
        const float* xp = xs + (size_t)b * (TG_XP + Tp) + TG_XP + t;
        unsigned a0, a1;
        wn_split_pair(xp[-3], xp[-2], a0, a1);       // channels 0, 1 -> slot 0
        hw[0] = a0; lw[0] = a1;
        wn_split_pair(xp[-1], 1.0f, a0, a1);         // channels 2, 3 -> slot 1
        hw[1] = a0; lw[1] = a1;
    }
    wn_g4_store(g4 + (size_t)b * TW_AUXC * Tp, NG, Tp, gr, t, hw, lw);
}

}  // namespace

struct TrainLayout {
    size_t l, enc, xs, lraw, total; // after the plain tape's regions
    long long RS, TE;
};
// raw: a dropout_inputs tape, which keeps the undropped l_0 row behind everything else
static TrainLayout train_layout(const wn_handle* h, int B, int F, long long T, bool raw = false) {
    const wn_config& c = h->cfg;
    const TapeLayout TL = tape_layout(h, B, T);
    TrainLayout L;
    L.RS = IAF_LP + TL.Tp;
    L.TE = (long long)F * h->frame_shift;
    size_t o = align_up(TL.total, 256);
    auto carve = [&](size_t words) { size_t r = o; o += align_up(words * 4, 256); return r; };
    L.l = carve(h->teacher.layers.size() * (size_t)B * c.width * L.RS);
    L.enc = carve((size_t)B * c.deconv_width * (L.TE + TG_TN) + 64);      // the forward's over-read margin (t_layout)
    L.xs = carve((size_t)B * (TG_XP + TL.Tp));
    L.lraw = carve(raw ? (size_t)B * c.width * L.RS : 0);
    L.total = o;
    return L;
}

// the regions of a training tape: the plain tape's, then the layer inputs, the conditioning and the scaled input row
static TgTape train_regions(const wn_handle* h, const TrainLayout& TR, int B, long long T, void* tape) {
    char* tb = reinterpret_cast<char*>(tape);
    TgTape t = tape_regions(tape_layout(h, B, T), tape);
    t.l = reinterpret_cast<unsigned*>(tb + TR.l);
    t.enc = reinterpret_cast<float*>(tb + TR.enc);
    t.xs = reinterpret_cast<float*>(tb + TR.xs);
    if (TR.total > TR.lraw) t.lraw = reinterpret_cast<unsigned*>(tb + TR.lraw);
    return t;
}

struct WLayout {
    long long Tp, TE, RE;
    int c0, nchunk, chunk;
    size_t aux, xa, xb, denc, slab, slab_floats, total;
};
static WLayout w_layout(const wn_handle* h, int B, int F, long long T) {
    const wn_config& c = h->cfg;
    const int W = c.width, S = c.skip_width, G = c.gate_width, H = G / 2, Cd = c.deconv_width;
    const BLayout BL = b_layout(h, B, T);
    WLayout L;
    L.Tp = BL.Tp;
    L.TE = (long long)F * h->frame_shift;
    L.c0 = (int)((L.TE - T) / 2);
    L.RE = std::max<long long>(L.TE, L.c0 + L.Tp);
    tw_chunks(B, L.Tp, T, &L.chunk, &L.nchunk);
    size_t o = align_up(BL.total, 256);
    auto carve = [&](size_t words) { size_t r = o; o += align_up(words * 4, 256); return r; };
    L.aux = carve((size_t)B * TW_AUXC * L.Tp);
    L.xa = carve((size_t)B * std::max(H, S) * L.Tp);
    L.xb = carve((size_t)B * S * L.Tp);
    L.denc = carve(h->teacher.denc_ok ? (size_t)B * Cd * L.RE : 0);
    const size_t layer = (size_t)H * (W + S) + (size_t)TW_AUXC * (W + S + G) + (size_t)G * (3 * W + Cd);
    const size_t head = (size_t)BL.Kp * (S + TW_AUXC) + (size_t)S * (S + Cd + TW_AUXC);
    const size_t tail = (size_t)S * (W + TW_AUXC) + (size_t)TW_AUXC * W;
    L.slab_floats = std::max(layer, std::max(head, tail));
    L.slab = carve((size_t)B * L.nchunk * L.slab_floats);
    L.total = o;
    return L;
}

// the gradients in one flat float32 buffer: the variables of the residual stack and head in the order weights.py lists them
void wn_teacher_build_layout(wn_handle* h) {
    const wn_config& c = h->cfg;
    const int W = c.width, S = c.skip_width, G = c.gate_width, H = G / 2, Cd = c.deconv_width, OW = c.out_width;
    TeacherParamLayout L;
    auto conv = [&](const std::string& scope, int K, int cin, int cout) {
        return L.table.conv(scope, "/W", "/biases", K, cin, cout, cout);
    };
    L.start = conv("conv_start", 3, 1, W);
    L.skip_start = conv("skip_start", 1, W, S);
    for (size_t i = 0; i < h->teacher.layers.size(); ++i) {
        const std::string n = std::to_string(i + 1);
        TeacherLayerOff o;
        o.dil = conv("dilated_conv_" + n, 3, W, G);
        o.cond = conv("mel_cond_" + n, 1, Cd, G);
        o.res = conv("res_" + n, 1, H, W);
        o.skip = conv("skip_" + n, 1, H, S);
        L.layers.push_back(o);
    }
    L.out1 = conv("out1", 1, S, S);
    L.cond_out1 = conv("mel_cond_out1", 1, Cd, S);
    L.out2 = conv("out2", 1, S, OW);
    h->teacher.lay = std::move(L);
}

struct TwCtx {
    int B;
    long long T;
    WLayout L;
    TrainLayout TR;
    TbWork rw;                      // workspace of the reverse pass: the cotangents
    unsigned *aux, *xa, *xb, *denc; // workspace of the weight side
    float* slab;
    TgTape tp;                      // the training tape
    const unsigned* enc() const { return reinterpret_cast<const unsigned*>(tp.enc); }
    float* grads;
    bool want_denc;
    TwRun run() const {
        return TwRun{"wn_teacher_backward_weights", slab, L.slab_floats, B, T, L.nchunk, L.chunk, rw.scal, grads};
    }
};

// one batch of products and the reduction of their slabs
int TwBatch::run(wn_handle* h, const TwRun& w, hipStream_t st) {
    if (bad || used > (long long)w.slab_floats) return wn_fail(h, WN_EIO, "%s: internal product table overflow", w.fn);
    a.slab = w.slab; a.slab_stride = (long long)w.slab_floats; a.T = w.T; a.nchunk = w.nchunk; a.chunk = w.chunk;
    hipLaunchKernelGGL(tw_gemm_kernel, dim3(max_tiles, nop, w.B * w.nchunk), dim3(256), 0, st, a);
    r.slab = w.slab; r.slab_stride = a.slab_stride; r.nslab = w.B * w.nchunk; r.scal = w.scal; r.grads = w.grads;
    int most = 0;
    for (int i = 0; i < nred; ++i) most = std::max(most, r.r[i].rows * r.r[i].cols);
    hipLaunchKernelGGL(tw_reduce_kernel, dim3(std::min(1024, (most + 255) / 256), nred), dim3(256), 0, st, r);
    WN_HIP(h, hipGetLastError());
    return WN_OK;
}
void wn_tw_act(const float* src, long long src_bs, int nmb, int hoff, unsigned* g4, int B, long long T, long long Tp, int C,
               int mode, hipStream_t st) {
    hipLaunchKernelGGL(tw_act_kernel, dim3((unsigned)(Tp / 256), C / 8, B), dim3(256), 0, st, src, src_bs, nmb, hoff, g4, T, Tp,
                       C, mode);
}
void wn_tw_aux(const float* xs, unsigned* g4, int B, long long T, long long Tp, hipStream_t st) {
    hipLaunchKernelGGL(tw_aux_kernel, dim3((unsigned)(Tp / 256), TW_AUXC / 8, B), dim3(256), 0, st, xs, g4, T, Tp);
}

namespace {
// in-place accumulation of W^T dY into the d enc rows (tg_gemm_kernel, RS epilogue with residual rows only)
void tw_denc_gemm(wn_handle* h, const TwCtx& w, const TeacherGemmPack& g, const unsigned* dy, int C, long long rowlen,
                  hipStream_t st) {
    const int Cd = h->cfg.deconv_width;
    TgArgs a = tg_pack_args(h, g, w.T);
    a.og4 = w.denc; a.og4_bstride = (long long)Cd * w.L.RE; a.og4_rowlen = (int)w.L.RE; a.og4_col0 = w.L.c0; a.og4_ng = Cd / 8;
    a.seg[0] = tg_seg_g4(dy, (long long)C * rowlen, rowlen, 0, C); a.nseg = 1;
    a.res_mtiles = g.mtiles;
    wn_tg_launch(TG_EPI_RS, a, g.mtiles, w.B, w.L.Tp, st);
}
}  // namespace

int tw_aux(wn_handle* h, const TwCtx& w, hipStream_t st) {
    const long long Tp = w.L.Tp;
    wn_tw_aux(w.tp.xs, w.aux, w.B, w.T, Tp, st);
    if (w.want_denc) WN_HIP(h, hipMemsetAsync(w.denc, 0, (size_t)w.B * h->cfg.deconv_width * w.L.RE * 4, st));
    return WN_OK;
}

// stage 0 (d h1 is complete): relu(h1) rows;  stage 1 (ds is complete): the head's products
int tw_head(wn_handle* h, const TwCtx& w, hipStream_t st, int stage) {
    const wn_config& c = h->cfg;
    const int S = c.skip_width, Cd = c.deconv_width, OW = c.out_width, Kp = w.rw.Kp;
    const long long Tp = w.L.Tp;
    const dim3 ga((unsigned)(Tp / 256), S / 8, w.B);
    if (stage == 0) {
        hipLaunchKernelGGL(tw_act_kernel, ga, dim3(256), 0, st, w.tp.h1, (long long)S * Tp, S / 16, 0, w.xa, w.T, Tp, S, 0);
        return WN_OK;
    }
    hipLaunchKernelGGL(tw_act_kernel, ga, dim3(256), 0, st, w.tp.s, (long long)S * Tp, S / 16, 0, w.xb, w.T, Tp, S, 0);
    TwBatch k;
    const long long o2w = k.add(w.rw.dout, Kp, Tp, w.xa, S, Tp, 0);
    const long long o2b = k.add(w.rw.dout, Kp, Tp, w.aux, TW_AUXC, Tp, 0);
    const long long o1w = k.add(w.rw.dh1, S, Tp, w.xb, S, Tp, 0);
    const long long c1w = k.add(w.rw.dh1, S, Tp, w.enc(), Cd, w.L.TE, w.L.c0);
    const long long o1b = k.add(w.rw.dh1, S, Tp, w.aux, TW_AUXC, Tp, 0);
    const TeacherParamLayout& lay = h->teacher.lay;
    k.red(o2w, S, OW, Kp, lay.out2.W, OW);
    k.red(o2b + 3 * Kp, 1, OW, Kp, lay.out2.b, OW);
    k.red(o1w, S, S, S, lay.out1.W, S);
    k.red(c1w, Cd, S, S, lay.cond_out1.W, S);
    k.red(o1b + 3 * S, 1, S, S, lay.out1.b, S);
    k.red(o1b + 3 * S, 1, S, S, lay.cond_out1.b, S);
    if (int rc = k.run(h, w.run(), st)) return rc;
    if (w.want_denc) tw_denc_gemm(h, w, h->teacher.cond_out1_t, w.rw.dh1, S, Tp, st);
    return WN_OK;
}

int tw_layer(wn_handle* h, const TwCtx& w, size_t li, hipStream_t st) {
    const wn_config& c = h->cfg;
    const int W = c.width, S = c.skip_width, G = c.gate_width, H = G / 2, Cd = c.deconv_width;
    const long long Tp = w.L.Tp, RS = w.TR.RS;
    const TeacherLayerPack& tl = h->teacher.layers[li];
    const TeacherLayerOff& lo = h->teacher.lay.layers[li];
    // m_i = sigma * tanh of the gate tape
    hipLaunchKernelGGL(tw_act_kernel, dim3((unsigned)(Tp / 256), H / 8, w.B), dim3(256), 0, st,
                       w.tp.g + li * (size_t)w.B * G * Tp, (long long)G * Tp, G / 16, H / 16, w.xa, w.T, Tp, H, 1);
    const unsigned* l = w.tp.l + li * (size_t)w.B * W * RS;
    TwBatch k;
    const long long rw = k.add(w.rw.dl, W, Tp, w.xa, H, Tp, 0);
    const long long sw = k.add(w.rw.ds, S, Tp, w.xa, H, Tp, 0);
    const long long rb = k.add(w.rw.dl, W, Tp, w.aux, TW_AUXC, Tp, 0);
    const long long sb = k.add(w.rw.ds, S, Tp, w.aux, TW_AUXC, Tp, 0);
    long long dw[3];
    for (int tap = 0; tap < 3; ++tap) dw[tap] = k.add(w.rw.dd, G, w.rw.RD, l, W, RS, IAF_LP - (long long)(2 - tap) * tl.dilation);
    const long long cw = k.add(w.rw.dd, G, w.rw.RD, w.enc(), Cd, w.L.TE, w.L.c0);
    const long long db = k.add(w.rw.dd, G, w.rw.RD, w.aux, TW_AUXC, Tp, 0);
    k.red(rw, H, W, W, lo.res.W, W);
    k.red(sw, H, S, S, lo.skip.W, S);
    k.red(rb + 3 * W, 1, W, W, lo.res.b, W);
    k.red(sb + 3 * S, 1, S, S, lo.skip.b, S);
    for (int tap = 0; tap < 3; ++tap) k.red(dw[tap], W, G, G, lo.dil.W + (size_t)tap * W * G, G);
    k.red(cw, Cd, G, G, lo.cond.W, G);
    k.red(db + 3 * G, 1, G, G, lo.dil.b, G);
    k.red(db + 3 * G, 1, G, G, lo.cond.b, G);
    if (int rc = k.run(h, w.run(), st)) return rc;
    if (w.want_denc) tw_denc_gemm(h, w, tl.cond_t, w.rw.dd, G, w.rw.RD, st);
    return WN_OK;
}

// dl = d l_0: skip_start and conv_start
int tw_tail(wn_handle* h, const TwCtx& w, hipStream_t st) {
    const wn_config& c = h->cfg;
    const int W = c.width, S = c.skip_width;
    const long long Tp = w.L.Tp, RS = w.TR.RS;
    TwBatch k;
    // skip_start read the raw l_0 where dropout_inputs put the dropped one into slot 0
    const long long sw = k.add(w.rw.ds, S, Tp, w.tp.lraw ? w.tp.lraw : w.tp.l, W, RS, IAF_LP);
    const long long sb = k.add(w.rw.ds, S, Tp, w.aux, TW_AUXC, Tp, 0);
    const long long cs = k.add(w.rw.dl, W, Tp, w.aux, TW_AUXC, Tp, 0);
    const TeacherParamLayout& lay = h->teacher.lay;
    k.red(sw, W, S, S, lay.skip_start.W, S);
    k.red(sb + 3 * S, 1, S, S, lay.skip_start.b, S);
    k.red(cs, 3, W, W, lay.start.W, W);
    k.red(cs + 3 * W, 1, W, W, lay.start.b, W);
    return k.run(h, w.run(), st);
}

// what the weight-gradient calls refuse beyond tb_check
static int tw_check(wn_handle* h, const char* fn) {
    if (int rc = tb_check(h, fn)) return rc;
    if (h->cfg.use_weight_norm)
        return wn_fail(h, WN_EINVAL, "%s: weight-norm teacher: the gradients of W_V / W_g are not implemented", fn);
    return WN_OK;
}

extern "C" int wn_teacher_grad_count(const wn_handle* h) {
    if (!h || !h->finalized || h->cfg.kind != WN_KIND_TEACHER) return 0;
    return (int)h->teacher.lay.table.entries.size();
}

extern "C" int wn_teacher_grad_info(const wn_handle* h, int i, char* name, size_t name_cap, int64_t* offset, int64_t* shape4,
                                    int* ndim) {
    if (!h || !h->finalized || h->cfg.kind != WN_KIND_TEACHER)
        return wn_fail(h, WN_EINVAL, "wn_teacher_grad_info: needs a finalized teacher handle");
    return wn_grad_info(h, "wn_teacher_grad_info", h->teacher.lay.table.entries, i, name, name_cap, offset, shape4, ndim);
}

extern "C" size_t wn_teacher_grad_floats(const wn_handle* h) {
    if (!h || !h->finalized || h->cfg.kind != WN_KIND_TEACHER) return 0;
    return h->teacher.lay.table.floats;
}

// the work calls' refusals (tw_check) without a message: the size queries return 0 for what they would refuse
static bool tw_supported(const wn_handle* h) {
    return h && h->finalized && h->cfg.kind == WN_KIND_TEACHER && h->cfg.loss_type != WN_LOSS_CE && !h->cfg.use_mu_law &&
           !h->cfg.use_weight_norm && h->teacher.vjp_ok;
}

extern "C" size_t wn_teacher_train_tape_bytes(const wn_handle* h, int B, int F, int64_t T) {
    if (!tw_supported(h) || B < 1 || F < 1 || T < 1) return 0;
    return train_layout(h, B, F, T).total;
}

extern "C" size_t wn_teacher_backward_weights_workspace_bytes(const wn_handle* h, int B, int F, int64_t T) {
    if (!tw_supported(h) || B < 1 || F < 1 || T < 1) return 0;
    return w_layout(h, B, F, T).total;
}

extern "C" int wn_teacher_forward_train_tape(wn_handle* h, const float* wav, const float* mel, int B, int F, int64_t T,
                                             float* out_params, void* tape, size_t tape_bytes, void* ws, size_t ws_bytes,
                                             void* stream) {
    const char* fn = "wn_teacher_forward_train_tape";
    if (int rc = tw_check(h, fn)) return rc;
    if (int rc = tg_forward_check(h, fn, wav, mel, B, F, T, out_params, ws)) return rc;
    if (!tape) return wn_fail(h, WN_EINVAL, "%s: bad argument (tape)", fn);
    const TrainLayout TR = train_layout(h, B, F, T);
    if (tape_bytes < TR.total) return wn_fail(h, WN_ENOMEM, "%s: tape %zu < %zu bytes", fn, tape_bytes, TR.total);
    const WnWork work(h);
    return tb_tape_forward(h, fn, TB_MAGIC_TRAIN, wav, mel, B, F, T, out_params, tape, train_regions(h, TR, B, T, tape), ws,
                           ws_bytes, stream);
}

// the dropout calls' own refusals
static int tw_dropout_check(wn_handle* h, const char* fn, int mode, double rate) {
    if (mode != WN_DROPOUT_INPUTS && mode != WN_DROPOUT_ALL)
        return wn_fail(h, WN_EINVAL, "%s: unknown dropout mode %d (WN_DROPOUT_INPUTS or WN_DROPOUT_ALL)", fn, mode);
    if (!(rate >= 0.0 && rate < 1.0)) return wn_fail(h, WN_EINVAL, "%s: dropout rate %g is outside [0, 1)", fn, rate);
    return WN_OK;
}

extern "C" size_t wn_teacher_train_tape_dropout_bytes(const wn_handle* h, int B, int F, int64_t T, int mode) {
    if (!tw_supported(h) || B < 1 || F < 1 || T < 1 || (mode != WN_DROPOUT_INPUTS && mode != WN_DROPOUT_ALL)) return 0;
    return train_layout(h, B, F, T, mode == WN_DROPOUT_INPUTS).total;
}

extern "C" int wn_teacher_forward_train_tape_dropout(wn_handle* h, const float* wav, const float* mel, int B, int F, int64_t T,
                                                     float* out_params, void* tape, size_t tape_bytes, void* ws,
                                                     size_t ws_bytes, void* stream, int mode, uint64_t seed, double rate) {
    const char* fn = "wn_teacher_forward_train_tape_dropout";
    if (int rc = tw_check(h, fn)) return rc;
    if (int rc = tw_dropout_check(h, fn, mode, rate)) return rc;
    if (int rc = tg_forward_check(h, fn, wav, mel, B, F, T, out_params, ws)) return rc;
    if (!tape) return wn_fail(h, WN_EINVAL, "%s: bad argument (tape)", fn);
    const TrainLayout TR = train_layout(h, B, F, T, mode == WN_DROPOUT_INPUTS);
    if (tape_bytes < TR.total) return wn_fail(h, WN_ENOMEM, "%s: tape %zu < %zu bytes", fn, tape_bytes, TR.total);
    const WnWork work(h);
    TgTape regions = train_regions(h, TR, B, T, tape);
    regions.drop.mode = mode;
    regions.drop.seed = seed;
    regions.drop.thr = wn_dropout_threshold(rate);
    regions.drop.keep = (float)(1.0 - rate);
    return tb_tape_forward(h, fn, TB_MAGIC_TRAIN, wav, mel, B, F, T, out_params, tape, regions, ws, ws_bytes, stream);
}

extern "C" int wn_teacher_backward_weights(wn_handle* h, const void* tape, size_t tape_bytes, const float* d_out_params, int B,
                                           int F, int64_t T, float* grads, size_t grads_floats, float* d_encoding, float* d_wav,
                                           void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "wn_teacher_backward_weights";
    if (int rc = tw_check(h, fn)) return rc;
    if (B < 1 || F < 1 || T < 1 || !tape || !d_out_params || !grads || !ws) return wn_fail(h, WN_EINVAL, "%s: bad argument", fn);
    int tape_F = 0;
    TgDropout dr;
    if (int rc = tb_tape_check(h, fn, tape, tape_bytes, B, T, &tape_F, &dr)) return rc;
    if (tape_F == 0)
        return wn_fail(h, WN_EINVAL, "%s: a plain tape of wn_teacher_forward_tape holds no layer inputs and no conditioning; "
                       "the weight gradients need a tape of wn_teacher_forward_train_tape", fn);
    if (tape_F != F) return wn_fail(h, WN_EINVAL, "%s: the tape holds F = %d mel frames, not %d", fn, tape_F, F);
    TwCtx w;
    w.TR = train_layout(h, B, F, T, dr.mode == WN_DROPOUT_INPUTS);
    if (tape_bytes < w.TR.total)
        return wn_fail(h, WN_EINVAL, "%s: a tape of %zu bytes cannot hold the training tape of B = %d, F = %d, T = %lld "
                       "(%zu bytes)", fn, tape_bytes, B, F, (long long)T, w.TR.total);
    if (grads_floats < h->teacher.lay.table.floats)
        return wn_fail(h, WN_ENOMEM, "%s: grads holds %zu floats, the gradients need %zu", fn, grads_floats,
                       h->teacher.lay.table.floats);
    if (d_encoding && !h->teacher.denc_ok)
        return wn_fail(h, WN_EINVAL, "%s: d_encoding needs deconv_width %d to be a multiple of 64", fn, h->cfg.deconv_width);
    w.L = w_layout(h, B, F, T);
    if ((long long)B * w.L.nchunk > 65535) return wn_fail(h, WN_EINVAL, "%s: B = %d needs more than 65535 slabs", fn, B);
    if (ws_bytes < w.L.total) return wn_fail(h, WN_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, w.L.total);
    const WnWork work(h);
    char* base = reinterpret_cast<char*>(ws);
    w.B = B; w.T = T;
    w.rw = tb_work(b_layout(h, B, T), ws);
    w.aux = reinterpret_cast<unsigned*>(base + w.L.aux);
    w.xa = reinterpret_cast<unsigned*>(base + w.L.xa);
    w.xb = reinterpret_cast<unsigned*>(base + w.L.xb);
    w.denc = reinterpret_cast<unsigned*>(base + w.L.denc);
    w.slab = reinterpret_cast<float*>(base + w.L.slab);
    w.tp = train_regions(h, w.TR, B, T, const_cast<void*>(tape));
    w.grads = grads;
    w.want_denc = d_encoding != nullptr;
    if (int rc = tb_reverse(h, tape, d_out_params, B, T, d_wav, ws, stream, &w, dr)) return rc;
    if (d_encoding) {
        wn_tw_denc(w.denc, w.rw.scal, d_encoding, B, w.L.TE, w.L.RE, h->cfg.deconv_width, 0, reinterpret_cast<hipStream_t>(stream));
        WN_HIP(h, hipGetLastError());
    }
    return WN_OK;
}
