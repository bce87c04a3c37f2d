// Weight gradients of the ParallelWavenet student: the training forward of every IAF flow onto a tape, and the
// reverse pass over it.
//
// An IAF flow (parallel_wavenet.py:200-287) is a dilated stack with a two-row head: start conv, L gated layers with a
// residual 1x1 (no skip path), out1 over relu(l) plus its conditioning, relu, out2_mean / out2_scale.  That is the
// teacher's network shape, so the flow runs on the teacher's GEMM kernel (tg_gemm_kernel, wn_teacher.hip) with flow packs
// (wn_pack_iaf_train), and its weight products on tw_gemm_kernel / tw_reduce_kernel (wn_teacher_wgrad.hip).  The sequencer
// and what the flow structure adds are here:
//   it_relu_kernel    after the last layer: relu(l_final) as G4 rows (out1's operand, later the X operand of out1/W) and
//                     the pre-ReLU values in accumulator layout (the mask of out1^T)
//   it_head_kernel    after out2: scale = clamp(softplus(p)), x <- x scale + mean, mean_tot, scale_tot; tapes x, scale, p
//   it_binit_kernel / it_bhead_kernel   their transposes, flow n -> 1
//   it_denc_kernel    a flow's d enc rows, unscaled, stored or added into its stack's slice
//   it_dnoise_kernel  wn_iaf_backward_input: d x of flow 1's input plus the noise's own factor in x
// The layer inputs l_i live in consecutive slots of the tape: the gate reads slot i, the residual GEMM (RSC epilogue) reads
// slot i and writes slot i + 1 -- two launches per layer and no copy.
// Pad columns as in DESIGN.md 12 / 14: the tape may hold anything at [T, Tp), cotangents are exactly zero there, the time
// reductions walk valid columns only.
#include <algorithm>

#include "wn_teacher.h"
#include "wn_g4.h"
#include "wn_mfma_h.h"

namespace {
constexpr uint32_t IT_MAGIC = 0x31544957u;      // "WIT1"
constexpr size_t IT_HEAD = 256;

// l_final (G4 rows with their left pad) -> relu as G4 rows of Tp columns and the raw values in accumulator layout
// [t / 16][16-row block][lane][4]; both zero from column T on
__global__ __launch_bounds__(256) void it_relu_kernel(const unsigned* __restrict__ l, long long RS, unsigned* __restrict__ rl,
                                                      float* __restrict__ acc, long long T, long long Tp, int W) {
    const int b = blockIdx.z, gr = blockIdx.y, NG = W / 8;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= Tp) return;
    const int s4 = gr >> 2, kg = gr & 3;
    wn_u4 hw = (wn_u4){0u, 0u, 0u, 0u}, lw = hw;
    f4 raw[2] = {(f4){0.f, 0.f, 0.f, 0.f}, (f4){0.f, 0.f, 0.f, 0.f}};
    if (t < T) {
        wn_u4 ih, il;
        wn_g4_load(l + (size_t)b * W * RS, NG, RS, gr, IAF_LP + t, ih, il);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v0, v1;
            wn_join_pair(ih[i], il[i], v0, v1);
            raw[i >> 1][2 * (i & 1)] = v0;
            raw[i >> 1][2 * (i & 1) + 1] = v1;
            unsigned a0, a1;
            wn_split_pair(fmaxf(v0, 0.f), fmaxf(v1, 0.f), a0, a1);
            hw[i] = a0;
            lw[i] = a1;
        }
    }
    wn_g4_store(rl + (size_t)b * W * Tp, NG, Tp, gr, t, hw, lw);
    f4* p = reinterpret_cast<f4*>(acc + (size_t)b * W * Tp) + ((size_t)(t >> 4) * (W / 16) + 2 * s4) * 64 + 16 * kg + (t & 15);
    p[0] = raw[0];
    p[64] = raw[1];
}

// the head of one flow behind out2 (parallel_wavenet.py:105-114, 279-287): op [B][T][2] = (mean, scale parameter)
struct ItHead {
    const float* op;
    const float* xs;            // the flow's input row [B][TG_XP + Tp]
    float* xs_next;             // the next flow's, or null
    const float *Min, *Sin;     // mean_tot / scale_tot before this flow (null: 0 / 1)
    float *sc, *pr, *Mout, *Sout;
    const float* noise;         // last flow: the three outputs
    float *x_out, *mean_out, *scale_out;
    long long T, Tp;
};
__global__ __launch_bounds__(256) void it_head_kernel(const ItHead a) {
    const int b = blockIdx.y;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= TG_XP + a.Tp) return;
    const long long t = i - TG_XP;
    float v = 0.f;
    if (t >= 0 && t < a.T) {
        const size_t j = (size_t)b * a.T + t;
        const float mean = a.op[2 * j], p = a.op[2 * j + 1];
        const float s = fminf(fmaxf(softplus_tf(p), EXP_M9), EXP_7);
        const float x = a.xs[(size_t)b * (TG_XP + a.Tp) + i];
        const float M = a.Min ? a.Min[j] : 0.f, S = a.Sin ? a.Sin[j] : 1.f;
        v = x * s + mean;
        const float nM = mean + M * s, nS = S * s;
        a.sc[j] = s;
        a.pr[j] = p;
        a.Mout[j] = nM;
        a.Sout[j] = nS;
        if (a.x_out) {
            const float so = fminf(nS, EXP_7);                      // parallel_wavenet.py:327
            a.mean_out[j] = nM;
            a.scale_out[j] = so;
            a.x_out[j] = a.noise[j] * so + nM;
        }
    }
    if (a.xs_next) a.xs_next[(size_t)b * (TG_XP + a.Tp) + i] = v;
}

// x = noise scale_tot + mean_tot transposed, and the e^7 clamp of scale_tot (the gradient passes at the tie)
__global__ __launch_bounds__(256) void it_binit_kernel(const float* __restrict__ d_x, const float* __restrict__ d_mean,
                                                       const float* __restrict__ d_scale, const float* __restrict__ xs0,
                                                       const float* __restrict__ Sn, float* __restrict__ dx,
                                                       float* __restrict__ dM, float* __restrict__ dS, long long T,
                                                       long long Tp) {
    const int b = blockIdx.y;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const size_t j = (size_t)b * T + t;
    const float g = d_x[j], noise = xs0[(size_t)b * (TG_XP + Tp) + TG_XP + t];
    dx[j] = 0.f;                            // the last flow's x is read by nothing: the returned x is formed from the totals
    dM[j] = d_mean[j] + g;
    dS[j] = Sn[j] <= EXP_7 ? d_scale[j] + g * noise : 0.f;
}

// it_head_kernel transposed: (d x_k, d mean_tot, d scale_tot) -> the head's cotangent [B][T][2] = (d mean, d p) and the
// cotangents of what the flow read.  softplus' clamp passes the gradient at the ties and none beyond them.
struct ItBHead {
    const float* xs;
    const float *Min, *Sin, *sc, *pr;
    float *dx, *dM, *dS;
    float* dout;
    long long T, Tp;
};
__global__ __launch_bounds__(256) void it_bhead_kernel(const ItBHead a) {
    const int b = blockIdx.y;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.T) return;
    const size_t j = (size_t)b * a.T + t;
    const float s = a.sc[j], p = a.pr[j], x = a.xs[(size_t)b * (TG_XP + a.Tp) + TG_XP + t];
    const float M = a.Min ? a.Min[j] : 0.f, S = a.Sin ? a.Sin[j] : 1.f;
    const float gx = a.dx[j], gM = a.dM[j], gS = a.dS[j];
    const float ds = gx * x + gM * M + gS * S;
    const float sp = softplus_tf(p);
    const float thr = -13.942384719848633f;                          // softplus_tf's branches
    const float dsp = p > -thr ? 1.f : p < thr ? expf(p) : 1.f / (1.f + expf(-p));
    a.dout[2 * j] = gx + gM;
    a.dout[2 * j + 1] = sp >= EXP_M9 && sp <= EXP_7 ? ds * dsp : 0.f;
    a.dx[j] = gx * s;
    a.dM[j] = gM * s;
    a.dS[j] = gS * s;
}

// d noise = d x_0 (the chain through the flows) + d_x scale_tot (x = noise scale_tot + mean_tot read the noise itself)
__global__ __launch_bounds__(256) void it_dnoise_kernel(const float* __restrict__ dx, const float* __restrict__ d_x,
                                                        const float* __restrict__ Sn, float* __restrict__ d_noise, size_t n) {
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j < n) d_noise[j] = fmaf(d_x[j], fminf(Sn[j], EXP_7), dx[j]);
}

// a flow's d enc: G4 rows [B][Cd][RE] (scaled) -> float32 [B][TE][Cd], stored or added
__global__ __launch_bounds__(256) void it_denc_kernel(const unsigned* __restrict__ g4, const float* __restrict__ scal,
                                                      float* __restrict__ out, long long TE, long long RE, int Cd, int add) {
    const int b = blockIdx.z, gr = blockIdx.y, NG = Cd / 8;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= TE) return;
    wn_u4 hw, lw;
    wn_g4_load(g4 + (size_t)b * Cd * RE, NG, RE, gr, t, hw, lw);
    const float sc = scal[1];
    float* o = out + ((size_t)b * TE + t) * Cd;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float v0, v1;
        wn_join_pair(hw[i], lw[i], v0, v1);
        const int ch = wn_g4_channel(gr, i);
        o[ch] = add ? o[ch] + v0 * sc : v0 * sc;
        o[ch + 1] = add ? o[ch + 1] + v1 * sc : v1 * sc;
    }
}

__global__ void it_header_kernel(uint32_t magic, uint32_t s0, uint32_t s1, uint32_t B, uint32_t T, uint32_t F,
                                 unsigned* __restrict__ dst) {
    if (threadIdx.x == 0) {
        dst[0] = magic; dst[1] = s0; dst[2] = s1; dst[3] = B; dst[4] = T; dst[5] = F;
    }
}

// ---- the tape: header | the layer inputs of every flow, slot after slot | per flow the gate tapes, the pre-ReLU l_final and
// out1 rows, relu(l_final), the input row, scale, p, mean_tot, scale_tot | the conditioning of every stack ----
struct ItFlowOff {
    size_t g, lf, rl, h1, xs, sc, pr, M, S;
    int slot0;
};
struct ItLayout {
    long long T, Tp, RS, TE, RE, RD;
    int c0, nstacks, nslots;
    size_t l, slot_bytes, enc, enc_bytes, total;
    std::vector<ItFlowOff> f;
};
ItLayout it_layout(const wn_handle* h, int B, int F, long long T) {
    const wn_config& c = h->cfg;
    const size_t W = c.width, Cd = c.deconv_width;
    ItLayout L;
    L.T = T;
    L.Tp = (T + TG_TN - 1) / TG_TN * TG_TN;
    L.RS = IAF_LP + L.Tp;
    L.TE = (long long)F * h->frame_shift;
    L.c0 = (int)((L.TE - T) / 2);
    L.RE = std::max<long long>(L.TE, L.c0 + L.Tp);
    L.RD = L.Tp + 2 * (1ll << (c.num_stages - 1));
    L.nstacks = c.share_deconv ? 1 : c.n_flows;
    size_t o = IT_HEAD;
    auto carve = [&](size_t bytes) { size_t r = o; o += align_up(bytes, 256); return r; };
    L.nslots = 0;
    for (int k = 0; k < c.n_flows; ++k) L.nslots += c.iaf_layers[k] + 1;
    L.slot_bytes = (size_t)B * W * L.RS * 4;
    L.l = carve(L.nslots * L.slot_bytes);
    const size_t cols = (size_t)B * L.Tp, bt = (size_t)B * T * 4;
    int slot = 0;
    for (int k = 0; k < c.n_flows; ++k) {
        ItFlowOff f;
        f.slot0 = slot;
        slot += c.iaf_layers[k] + 1;
        f.g = carve((size_t)c.iaf_layers[k] * cols * W * 4);
        f.lf = carve(cols * W * 4);
        f.rl = carve(cols * W * 4);
        f.h1 = carve(cols * W * 4);
        f.xs = carve((size_t)B * (TG_XP + L.Tp) * 4);
        f.sc = carve(bt); f.pr = carve(bt); f.M = carve(bt); f.S = carve(bt);
        L.f.push_back(f);
    }
    L.enc_bytes = align_up(((size_t)B * Cd * (L.TE + TG_TN) + 64) * 4, 256);      // the forward's over-read margin (t_layout)
    L.enc = o;
    o += L.nstacks * L.enc_bytes;
    L.total = o;
    return L;
}
struct ItFwdLayout {
    size_t m, op, scratch, total;
};
ItFwdLayout it_fwd_layout(const wn_handle* h, int B, int F, long long T) {
    const long long Tp = (T + TG_TN - 1) / TG_TN * TG_TN;
    ItFwdLayout L;
    size_t o = 0;
    auto carve = [&](size_t bytes) { size_t r = o; o += align_up(bytes, 256); return r; };
    L.m = carve((size_t)B * (h->cfg.width / 2) * Tp * 4);
    L.op = carve((size_t)B * T * 2 * 4);
    L.scratch = o;
    o += wn_deconv_scratch_bytes(h, B, F);
    L.total = o;
    return L;
}
struct ItBwdLayout {
    int nchunk, chunk;
    size_t scal, doutf, dout, dh1, dl, dd, dx, dM, dS, aux, xa, denc, slab, slab_floats, total;
};
// wg: with the operands and slabs of the weight products (wn_iaf_backward_weights); without them, wn_iaf_backward_input's
ItBwdLayout it_bwd_layout(const wn_handle* h, const ItLayout& TL, int B, bool wg) {
    const wn_config& c = h->cfg;
    const size_t W = c.width, H = W / 2, Cd = c.deconv_width, cols = (size_t)B * TL.Tp, bt = (size_t)B * TL.T * 4;
    ItBwdLayout L{};
    tw_chunks(B, TL.Tp, TL.T, &L.chunk, &L.nchunk);
    size_t o = 0;
    auto carve = [&](size_t bytes) { size_t r = o; o += align_up(bytes, 256); return r; };
    L.scal = carve((4 + WN_NPART) * 4);
    L.doutf = carve(2 * bt);
    L.dout = carve(cols * 32 * 4);
    L.dh1 = carve(cols * W * 4);
    L.dl = carve(cols * W * 4);
    L.dd = carve((size_t)B * W * TL.RD * 4);
    L.dx = carve(bt); L.dM = carve(bt); L.dS = carve(bt);
    if (wg) {
        L.aux = carve(cols * TW_AUXC * 4);
        L.xa = carve(cols * W * 4);
    }
    L.denc = carve((size_t)B * Cd * TL.RE * 4);
    if (wg) {
        const size_t layer = W * H + TW_AUXC * W + 3 * W * W + W * Cd + TW_AUXC * W;
        const size_t head = 32 * (W + TW_AUXC) + W * (W + Cd + TW_AUXC);
        L.slab_floats = std::max(layer, std::max(head, (size_t)TW_AUXC * W));
        L.slab = carve((size_t)B * L.nchunk * L.slab_floats * 4);
    }
    L.total = o;
    return L;
}

// what the training calls refuse about the handle; quiet: no message (the size and table queries return 0)
int it_check(const wn_handle* h, const char* fn, bool quiet = false) {
#define IT_REFUSE(code, ...) return quiet ? code : wn_fail(h, code, __VA_ARGS__)
    if (!h) IT_REFUSE(WN_EINVAL, "%s: null handle", fn);
    const wn_config& c = h->cfg;
    if (c.kind != WN_KIND_STUDENT) IT_REFUSE(WN_EINVAL, "%s: handle is not a ParallelWavenet student", fn);
    if (c.use_mu_law)
        IT_REFUSE(WN_EINVAL, "%s: mu-law student: mu-law students and teachers are not supported by the "
                  "distillation losses", fn);
    if (c.use_weight_norm)
        IT_REFUSE(WN_EINVAL, "%s: weight-norm student: the gradients of W_V / W_g are not implemented", fn);
    if (!h->finalized) IT_REFUSE(WN_ESTATE, "%s: call wn_finalize first", fn);
    if (!h->iaf_train.ok)
        IT_REFUSE(WN_EINVAL, "%s: width %d and deconv_width %d must be multiples of 64 for the GEMM kernels", fn,
                  c.width, c.deconv_width);
    return WN_OK;
}
// ... and about the shape
int it_shape_check(const wn_handle* h, const char* fn, int B, int F, int64_t T, bool quiet = false) {
    if (B < 1 || F < 1 || T < 1) IT_REFUSE(WN_EINVAL, "%s: bad argument", fn);
    const long long TE = (long long)F * h->frame_shift, md = 1ll << (h->cfg.num_stages - 1);
    if (T > TE) IT_REFUSE(WN_EINVAL, "%s: %lld samples need more than %d mel frames "
                          "(wavenet.py:79 assert cond_len >= x_len)", fn, (long long)T, F);
    if (T % md) IT_REFUSE(WN_EINVAL, "%s: length %lld is not a multiple of the largest "
                          "dilation %lld (masked.py:188)", fn, (long long)T, md);
    if (TE > WN_MAX_ROW_SAMPLES) IT_REFUSE(WN_EINVAL, "%s: utterance too long (32-bit row offsets)", fn);
    return WN_OK;
#undef IT_REFUSE
}
// both, quietly: what the size queries answer 0 for
bool it_sized(const wn_handle* h, int B, int F, int64_t T) {
    return !it_check(h, "", true) && !it_shape_check(h, "", B, F, T, true);
}
template <class T>
T* at(void* base, size_t off) { return reinterpret_cast<T*>(reinterpret_cast<char*>(base) + off); }
}  // namespace

// ---- the flow packs, from the TF-layout variables (Cin-major [K][Cin][Cout]: a 1x1 kernel IS its transposed matrix) ----
int wn_pack_iaf_train(wn_handle* h, std::vector<float>& blob) {
    const wn_config& c = h->cfg;
    const int W = c.width, H = W / 2, Cd = c.deconv_width;
    IafTrainPack& P = h->iaf_train;
    P.ok = false;
    if (c.use_weight_norm || W % 64 || Cd % 64) return WN_OK;
    auto var = [&](const std::string& n) -> const std::vector<float>& { return h->vars.at(n).data; };
    auto reserve = [&](size_t words) {
        blob.resize(align_up(blob.size(), 64));
        const size_t off = blob.size();
        blob.resize(off + words);
        return off;
    };
    // row-major [M][K] (rows beyond M: zero) -> fragments and the tile-ordered bias (null: zeros)
    auto gemm = [&](const std::vector<float>& src, const std::vector<float>* bias, int K, int mtiles, auto rowfn) {
        TeacherGemmPack g;
        const float sc = pick_scale(src.data(), src.size());
        g.inv_scale = 1.0f / sc;
        g.nks = K / 32;
        g.mtiles = mtiles;
        g.w_off = reserve((size_t)mtiles * g.nks * 4 * 512);
        pack_tiles(blob, g.w_off, src.data(), K, K, mtiles, sc, rowfn);
        g.b_off = reserve((size_t)mtiles * 64);
        for (int i = 0; i < mtiles * 64; ++i) {
            const int row = rowfn(i);
            blob[g.b_off + i] = row < 0 || !bias ? 0.f : (*bias)[row];
        }
        return g;
    };
    auto ident = [](int M) { return [M](int i) { return i < M ? i : -1; }; };
    for (int k = 0; k < c.n_flows; ++k) {
        const std::string p = "iaf_" + std::to_string(k + 1) + "/";
        IafTrainFlow fl;
        fl.deconv_stack = c.share_deconv ? 0 : k;
        {
            const std::vector<float>&w = var(p + "start_conv/W"), &b = var(p + "start_conv/biases");
            fl.start_off = reserve(4 * (size_t)W);
            std::copy(w.begin(), w.end(), blob.begin() + fl.start_off);
            std::copy(b.begin(), b.end(), blob.begin() + fl.start_off + 3 * W);
        }
        for (int i = 0; i < c.iaf_layers[k]; ++i) {
            const std::string n = std::to_string(i + 1);
            const std::vector<float>&Wd = var(p + "dilated_conv_" + n + "/W"), &Wc = var(p + "mel_cond_" + n + "/W"),
                                    &Wr = var(p + "res_" + n + "/W");
            const std::vector<float>&bd = var(p + "dilated_conv_" + n + "/biases"), &bc = var(p + "mel_cond_" + n + "/biases"),
                                    &br = var(p + "res_" + n + "/biases");
            IafTrainLayer tl;
            tl.dilation = 1 << (i % c.num_stages);                      // parallel_wavenet.py:228
            const int Kg = 3 * W + Cd;
            std::vector<float> mg((size_t)W * Kg), bg(W), mr((size_t)W * H), mt((size_t)W * 3 * W);
            for (int g = 0; g < W; ++g) {
                for (int tap = 0; tap < 3; ++tap)
                    for (int w = 0; w < W; ++w) {
                        const float v = Wd[((size_t)tap * W + w) * W + g];
                        mg[(size_t)g * Kg + tap * W + w] = v;
                        mt[(size_t)w * 3 * W + tap * W + g] = v;       // dl(t) += sum_k W_dil[k]^T dd(t + (2 - k) dilation)
                    }
                for (int cc = 0; cc < Cd; ++cc) mg[(size_t)g * Kg + 3 * W + cc] = Wc[(size_t)cc * W + g];
                bg[g] = bd[g] + bc[g];
                for (int hh = 0; hh < H; ++hh) mr[(size_t)g * H + hh] = Wr[(size_t)hh * W + g];
            }
            // m-tile j: sigmoid rows 32 j .. 32 j + 31 then their tanh partners H + 32 j .. (parallel_wavenet.py:246-250)
            tl.gate = gemm(mg, &bg, Kg, H / 32,
                           [H](int r) { const int j = r / 64, lr = r % 64; return lr < 32 ? 32 * j + lr : H + 32 * j + lr - 32; });
            tl.res = gemm(mr, &br, H, W / 64, ident(W));
            tl.gate_t = gemm(mt, nullptr, 3 * W, W / 64, ident(W));
            tl.res_t = gemm(Wr, nullptr, W, (H + 63) / 64, ident(H));    // H = 32: one tile, its upper half zero rows
            tl.cond_t = gemm(Wc, nullptr, W, Cd / 64, ident(Cd));
            fl.layers.push_back(tl);
        }
        const std::vector<float>&Wo = var(p + "out1/W"), &Wco = var(p + "mel_cond_out1/W"), &Wm = var(p + "out2_mean/W"),
                                &Ws = var(p + "out2_scale/W");
        const std::vector<float>&bo = var(p + "out1/biases"), &bco = var(p + "mel_cond_out1/biases");
        const int K1 = W + Cd;
        std::vector<float> m1((size_t)W * K1), b1(W), m2((size_t)2 * W), b2(2), m2t((size_t)W * 32, 0.f);
        for (int o = 0; o < W; ++o) {
            for (int i = 0; i < W; ++i) m1[(size_t)o * K1 + i] = Wo[(size_t)i * W + o];
            for (int cc = 0; cc < Cd; ++cc) m1[(size_t)o * K1 + W + cc] = Wco[(size_t)cc * W + o];
            b1[o] = bo[o] + bco[o];
            m2[o] = Wm[o];
            m2[W + o] = Ws[o];
            m2t[(size_t)o * 32] = Wm[o];
            m2t[(size_t)o * 32 + 1] = Ws[o];
        }
        b2[0] = var(p + "out2_mean/biases")[0];
        b2[1] = var(p + "out2_scale/biases")[0];
        fl.out1 = gemm(m1, &b1, K1, W / 64, ident(W));
        fl.out2 = gemm(m2, &b2, W, 1, ident(2));
        fl.out1_t = gemm(Wo, nullptr, W, W / 64, ident(W));
        fl.out2_t = gemm(m2t, nullptr, 32, W / 64, ident(W));
        fl.cond_out1_t = gemm(Wco, nullptr, W, Cd / 64, ident(Cd));
        P.flows.push_back(fl);
    }
    P.serial = wn_tape_serial_next();
    P.ok = true;
    return WN_OK;
}

// the parameter layout: every variable of every flow in the order weights.py lists them
void wn_iaf_build_layout(wn_handle* h) {
    const wn_config& c = h->cfg;
    const int W = c.width, H = W / 2, Cd = c.deconv_width;
    IafParamLayout L;
    auto conv = [&](const std::string& scope, int K, int cin, int cout) {
        return L.table.conv(scope, "/W", "/biases", K, cin, cout, cout);
    };
    for (int k = 0; k < c.n_flows; ++k) {
        const std::string p = "iaf_" + std::to_string(k + 1) + "/";
        IafFlowLayout f;
        f.start = conv(p + "start_conv", 3, 1, W);
        for (int i = 0; i < c.iaf_layers[k]; ++i) {
            const std::string n = std::to_string(i + 1);
            IafLayerOff o;
            o.dil = conv(p + "dilated_conv_" + n, 3, W, W);
            o.cond = conv(p + "mel_cond_" + n, 1, Cd, W);
            o.res = conv(p + "res_" + n, 1, H, W);
            f.layers.push_back(o);
        }
        f.out1 = conv(p + "out1", 1, W, W);
        f.cond_out1 = conv(p + "mel_cond_out1", 1, Cd, W);
        f.out2_mean = conv(p + "out2_mean", 1, W, 1);
        f.out2_scale = conv(p + "out2_scale", 1, W, 1);
        L.flows.push_back(f);
    }
    h->iaf_train.lay = std::move(L);
}

extern "C" size_t wn_iaf_train_tape_bytes(const wn_handle* h, int B, int F, int64_t T) {
    if (!it_sized(h, B, F, T)) return 0;
    return it_layout(h, B, F, T).total;
}

extern "C" size_t wn_iaf_train_workspace_bytes(const wn_handle* h, int B, int F, int64_t T) {
    if (!it_sized(h, B, F, T)) return 0;
    return it_fwd_layout(h, B, F, T).total;
}

extern "C" size_t wn_iaf_backward_weights_workspace_bytes(const wn_handle* h, int B, int F, int64_t T) {
    if (!it_sized(h, B, F, T)) return 0;
    return it_bwd_layout(h, it_layout(h, B, F, T), B, true).total;
}

extern "C" size_t wn_iaf_backward_input_workspace_bytes(const wn_handle* h, int B, int F, int64_t T) {
    if (!it_sized(h, B, F, T)) return 0;
    return it_bwd_layout(h, it_layout(h, B, F, T), B, false).total;
}

extern "C" int wn_iaf_grad_count(const wn_handle* h) {
    if (it_check(h, "", true)) return 0;
    return (int)h->iaf_train.lay.table.entries.size();
}

extern "C" int wn_iaf_grad_info(const wn_handle* h, int i, char* name, size_t name_cap, int64_t* offset, int64_t* shape4,
                                int* ndim) {
    if (it_check(h, "", true))
        return wn_fail(h, WN_EINVAL, "wn_iaf_grad_info: needs a finalized student handle the training calls accept");
    return wn_grad_info(h, "wn_iaf_grad_info", h->iaf_train.lay.table.entries, i, name, name_cap, offset, shape4, ndim);
}

extern "C" size_t wn_iaf_grad_floats(const wn_handle* h) {
    if (it_check(h, "", true)) return 0;
    return h->iaf_train.lay.table.floats;
}

// for wn_iaf_set_weights (wn_iaf_repack.hip): the refusals by name
int wn_iaf_train_check(wn_handle* h, const char* fn) { return it_check(h, fn); }
// it_denc_kernel for both reverse passes (the teacher's stores: add == 0)
void wn_tw_denc(const unsigned* g4, const float* scal, float* out, int B, long long TE, long long RE, int Cd, int add,
                hipStream_t st) {
    hipLaunchKernelGGL(it_denc_kernel, dim3((unsigned)((TE + 255) / 256), Cd / 8, B), dim3(256), 0, st, g4, scal, out, TE, RE, Cd,
                       add);
}

extern "C" int wn_iaf_forward_train_tape(wn_handle* h, const float* noise, const float* mel, int B, int F, int64_t T, float* x,
                                         float* mean_tot, float* scale_tot, void* tape, size_t tape_bytes, void* ws,
                                         size_t ws_bytes, void* stream) {
    const char* fn = "wn_iaf_forward_train_tape";
    if (int rc = it_check(h, fn)) return rc;
    if (int rc = it_shape_check(h, fn, B, F, T)) return rc;
    if (!noise || !mel || !x || !mean_tot || !scale_tot || !ws) return wn_fail(h, WN_EINVAL, "%s: bad argument", fn);
    if (!tape) return wn_fail(h, WN_EINVAL, "%s: bad argument (tape)", fn);
    const ItLayout TL = it_layout(h, B, F, T);
    if (tape_bytes < TL.total) return wn_fail(h, WN_ENOMEM, "%s: tape %zu < %zu bytes", fn, tape_bytes, TL.total);
    const ItFwdLayout FL = it_fwd_layout(h, B, F, T);
    if (ws_bytes < FL.total) return wn_fail(h, WN_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, FL.total);
    const WnWork work(h);
    const wn_config& c = h->cfg;
    const IafTrainPack& P = h->iaf_train;
    const int W = c.width, H = W / 2, Cd = c.deconv_width, NF = c.n_flows;
    const long long Tp = TL.Tp, RS = TL.RS;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(it_header_kernel, dim3(1), dim3(64), 0, st, IT_MAGIC, (uint32_t)P.serial, (uint32_t)(P.serial >> 32),
                       (uint32_t)B, (uint32_t)T, (uint32_t)F, at<unsigned>(tape, 0));
    // the conditioning of every stack (parallel_wavenet.py:217-220, 311-314), G4 rows of TE columns
    for (int s = 0; s < TL.nstacks; ++s)
        if (int rc = wn_run_deconv(h, s, mel, B, F, at<float>(tape, TL.enc + s * TL.enc_bytes), TL.TE, at<char>(ws, FL.scratch),
                                   st, true))
            return rc;
    // the zero left pad of every slot (slot 0 of a flow gets it from the start conv as well)
    WN_HIP(h, hipMemset2DAsync(at<char>(tape, TL.l), (size_t)RS * 16, 0, (size_t)IAF_LP * 16,
                               (size_t)TL.nslots * B * 2 * (W / 8), st));
    wn_tg_input(noise, at<float>(tape, TL.f[0].xs), B, T, Tp, 0, st);
    unsigned* m = at<unsigned>(ws, FL.m);
    float* op = at<float>(ws, FL.op);
    const TgSeg seg_m = tg_seg_g4(m, (long long)H * Tp, Tp, 0, H);
    for (int k = 0; k < NF; ++k) {
        const IafTrainFlow& fl = P.flows[k];
        const ItFlowOff& fo = TL.f[k];
        const TgSeg seg_enc = tg_seg_g4(at<unsigned>(tape, TL.enc + fl.deconv_stack * TL.enc_bytes), (long long)Cd * TL.TE, TL.TE,
                                        TL.c0, Cd);
        auto slot = [&](size_t i) { return at<unsigned>(tape, TL.l + (fo.slot0 + i) * TL.slot_bytes); };
        // l_0 = start_conv(shift_right(x))  (parallel_wavenet.py:222-225)
        wn_tg_start(at<float>(tape, fo.xs), h->d_blob + fl.start_off, slot(0), B, W, Tp, RS, st);
        for (size_t li = 0; li < fl.layers.size(); ++li) {
            const IafTrainLayer& tl = fl.layers[li];
            const TgSeg seg_l = tg_seg_g4(slot(li), (long long)W * RS, RS, IAF_LP, W);
            {   // d = dilated_conv(l) + mel_cond(enc); m = sigmoid(d[:H]) * tanh(d[H:])  (parallel_wavenet.py:228-250)
                TgArgs a = tg_pack_args(h, tl.gate, T);
                for (int tap = 0; tap < 3; ++tap) {
                    a.seg[tap] = seg_l;
                    a.seg[tap].col0 = IAF_LP - (2 - tap) * tl.dilation;
                }
                a.seg[3] = seg_enc; a.nseg = 4;
                a.og4 = m; a.og4_bstride = (long long)H * Tp; a.og4_rowlen = (int)Tp; a.og4_col0 = 0; a.og4_ng = H / 8;
                a.tape = at<float>(tape, fo.g) + li * (size_t)B * W * Tp;
                a.tape_bstride = (long long)W * Tp; a.tape_nmb = W / 16; a.tape_hoff = H / 16;
                wn_tg_launch(TG_EPI_GATE_TAPE, a, tl.gate.mtiles, B, Tp, st);
            }
            {   // l_{i+1} = l_i + res(m)  (parallel_wavenet.py:252-256): slot i is read, slot i + 1 written
                TgArgs a = tg_pack_args(h, tl.res, T);
                a.seg[0] = seg_m; a.nseg = 1;
                a.ig4 = slot(li);
                a.og4 = slot(li + 1); a.og4_bstride = (long long)W * RS; a.og4_rowlen = (int)RS; a.og4_col0 = IAF_LP;
                a.og4_ng = W / 8;
                a.res_mtiles = W / 64;
                wn_tg_launch(TG_EPI_RSC, a, tl.res.mtiles, B, Tp, st);
            }
        }
        unsigned* rl = at<unsigned>(tape, fo.rl);
        float* h1 = at<float>(tape, fo.h1);
        hipLaunchKernelGGL(it_relu_kernel, dim3((unsigned)(Tp / 256), W / 8, B), dim3(256), 0, st, slot(fl.layers.size()), RS, rl,
                           at<float>(tape, fo.lf), (long long)T, Tp, W);
        {   // out1(relu(l)) + mel_cond_out1(enc)  (parallel_wavenet.py:258-270)
            TgArgs a = tg_pack_args(h, fl.out1, T);
            a.seg[0] = tg_seg_g4(rl, (long long)W * Tp, Tp, 0, W); a.seg[1] = seg_enc; a.nseg = 2;
            a.oacc = h1; a.oacc_bstride = (long long)W * Tp; a.oacc_nmb = W / 16;
            wn_tg_launch(TG_EPI_ACC, a, fl.out1.mtiles, B, Tp, st);
        }
        {   // (out2_mean, out2_scale)(relu(.))  (parallel_wavenet.py:272-277)
            TgArgs a = tg_pack_args(h, fl.out2, T);
            TgSeg sg;
            sg.base = reinterpret_cast<const unsigned*>(h1); sg.bstride = (long long)W * Tp; sg.rowlen = W / 16;
            sg.col0 = 0; sg.nks = W / 32; sg.ng = 0; sg.kind = TG_SRC_ACC_RELU;
            a.seg[0] = sg; a.nseg = 1;
            a.otm = op; a.ow = 2;
            wn_tg_launch(TG_EPI_OUT, a, 1, B, Tp, st);
        }
        ItHead hd{};
        hd.op = op; hd.xs = at<float>(tape, fo.xs);
        hd.xs_next = k + 1 < NF ? at<float>(tape, TL.f[k + 1].xs) : nullptr;
        hd.Min = k ? at<float>(tape, TL.f[k - 1].M) : nullptr;
        hd.Sin = k ? at<float>(tape, TL.f[k - 1].S) : nullptr;
        hd.sc = at<float>(tape, fo.sc); hd.pr = at<float>(tape, fo.pr);
        hd.Mout = at<float>(tape, fo.M); hd.Sout = at<float>(tape, fo.S);
        hd.T = T; hd.Tp = Tp;
        if (k + 1 == NF) { hd.noise = noise; hd.x_out = x; hd.mean_out = mean_tot; hd.scale_out = scale_tot; }
        hipLaunchKernelGGL(it_head_kernel, dim3((unsigned)((TG_XP + Tp + 255) / 256), B), dim3(256), 0, st, hd);
    }
    WN_HIP(h, hipGetLastError());
    wn_tape_register(tape, P.serial, B, T, F);
    return WN_OK;
}

namespace {
// the tape belongs to this handle and this shape
int it_tape_check(wn_handle* h, const char* fn, const void* tape, size_t tape_bytes, const ItLayout& TL, int B, int F, int64_t T) {
    uint64_t ser = 0;
    int tB = 0, tF = 0;
    long long tT = 0;
    if (!wn_tape_lookup(tape, &ser, &tB, &tT, &tF) || ser != h->iaf_train.serial)
        return wn_fail(h, WN_EINVAL, "%s: the tape was not written by wn_iaf_forward_train_tape of this handle", fn);
    if (tB != B || tT != (long long)T)
        return wn_fail(h, WN_EINVAL, "%s: the tape holds B = %d, T = %lld, not B = %d, T = %lld", fn, tB, tT, B, (long long)T);
    if (tF != F) return wn_fail(h, WN_EINVAL, "%s: the tape holds F = %d mel frames, not %d", fn, tF, F);
    if (tape_bytes < TL.total)
        return wn_fail(h, WN_EINVAL, "%s: a tape of %zu bytes cannot hold the training tape of B = %d, F = %d, T = %lld "
                       "(%zu bytes)", fn, tape_bytes, B, F, (long long)T, TL.total);
    return WN_OK;
}

// The reverse pass over a tape, flow n -> 1.  grads: the weight products and their reductions (null: none of them, nor their
// operands -- the data path alone, as tb_reverse without wg); d_noise: null, or the chain is carried through flow 1's start
// conv and the noise's own term added.  What both leave out changes no bit of what remains.
// These are the launches alone: the caller has checked everything (it_reverse, wn_iaf_adjoint) and holds the work lock.
int it_reverse_run(wn_handle* h, const char* fn, const void* tape, const ItLayout& TL, const ItBwdLayout& BL, const float* d_x,
                   const float* d_mean_tot, const float* d_scale_tot, int B, int64_t T, float* grads, float* d_noise,
                   float* d_encoding, void* ws, void* stream) {
    const bool wg = grads != nullptr;
    const IafTrainPack& P = h->iaf_train;
    const wn_config& c = h->cfg;
    const int W = c.width, H = W / 2, Cd = c.deconv_width, NF = c.n_flows, Kp = 32;
    const long long Tp = TL.Tp, RS = TL.RS, RD = TL.RD, RE = TL.RE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    void* tp = const_cast<void*>(tape);
    float* scal = at<float>(ws, BL.scal);
    float* doutf = at<float>(ws, BL.doutf);
    unsigned *dout = at<unsigned>(ws, BL.dout), *dh1 = at<unsigned>(ws, BL.dh1), *dl = at<unsigned>(ws, BL.dl),
             *dd = at<unsigned>(ws, BL.dd), *aux = at<unsigned>(ws, BL.aux), *xa = at<unsigned>(ws, BL.xa),
             *denc = at<unsigned>(ws, BL.denc);
    float *dx = at<float>(ws, BL.dx), *dM = at<float>(ws, BL.dM), *dS = at<float>(ws, BL.dS);
    const TwRun run{fn, at<float>(ws, BL.slab), BL.slab_floats, B, T, BL.nchunk, BL.chunk, scal, grads};
    const dim3 gbt((unsigned)((T + 255) / 256), B);

    hipLaunchKernelGGL(it_binit_kernel, gbt, dim3(256), 0, st, d_x, d_mean_tot, d_scale_tot, at<float>(tp, TL.f[0].xs),
                       at<float>(tp, TL.f[NF - 1].S), dx, dM, dS, (long long)T, Tp);
    WN_HIP(h, hipMemsetAsync(dd, 0, (size_t)B * W * RD * 4, st));      // the zero right pad the anti-causal taps read
    auto args = [&](const TeacherGemmPack& g, unsigned* og4, long long orowlen, long long ocol0, int C) {
        TgArgs a = tg_pack_args(h, g, T);
        a.og4 = og4; a.og4_bstride = (long long)C * orowlen; a.og4_rowlen = (int)orowlen; a.og4_col0 = (int)ocol0; a.og4_ng = C / 8;
        return a;
    };
    // d enc += W^T dY in place (RS epilogue with residual rows only)
    auto denc_gemm = [&](const TeacherGemmPack& g, const unsigned* dy, int C, long long rowlen) {
        TgArgs a = args(g, denc, RE, TL.c0, Cd);
        a.seg[0] = tg_seg_g4(dy, (long long)C * rowlen, rowlen, 0, C); a.nseg = 1;
        a.res_mtiles = g.mtiles;
        wn_tg_launch(TG_EPI_RS, a, g.mtiles, B, Tp, st);
    };
    const TgSeg seg_dl = tg_seg_g4(dl, (long long)W * Tp, Tp, 0, W);
    for (int k = NF; k-- > 0;) {
        const IafTrainFlow& fl = P.flows[k];
        const ItFlowOff& fo = TL.f[k];
        const IafFlowLayout& lay = P.lay.flows[k];
        const unsigned* enc = at<unsigned>(tp, TL.enc + fl.deconv_stack * TL.enc_bytes);
        const float* xs = at<float>(tp, fo.xs);
        auto slot = [&](size_t i) { return at<unsigned>(tp, TL.l + (fo.slot0 + i) * TL.slot_bytes); };
        ItBHead bh{};
        bh.xs = xs;
        bh.Min = k ? at<float>(tp, TL.f[k - 1].M) : nullptr;
        bh.Sin = k ? at<float>(tp, TL.f[k - 1].S) : nullptr;
        bh.sc = at<float>(tp, fo.sc); bh.pr = at<float>(tp, fo.pr);
        bh.dx = dx; bh.dM = dM; bh.dS = dS; bh.dout = doutf; bh.T = T; bh.Tp = Tp;
        hipLaunchKernelGGL(it_bhead_kernel, gbt, dim3(256), 0, st, bh);
        // the operand scale of this flow's cotangents
        wn_pow2_scale(doutf, (long long)B * T * 2, scal + 4, scal, nullptr, st);
        wn_tb_dout(doutf, scal, dout, B, T, Tp, 2, Kp, st);
        if (wg) wn_tw_aux(xs, aux, B, T, Tp, st);
        if (d_encoding) WN_HIP(h, hipMemsetAsync(denc, 0, (size_t)B * Cd * RE * 4, st));
        {   // d relu(h1) = W_out2^T d out, masked by h1 > 0
            TgArgs a = args(fl.out2_t, dh1, Tp, 0, W);
            a.seg[0] = tg_seg_g4(dout, (long long)Kp * Tp, Tp, 0, Kp); a.nseg = 1;
            a.tape = at<float>(tp, fo.h1); a.tape_bstride = (long long)W * Tp; a.tape_nmb = W / 16;
            wn_tg_launch(TG_EPI_MASK, a, fl.out2_t.mtiles, B, Tp, st);
        }
        if (wg) {
            wn_tw_act(at<float>(tp, fo.h1), (long long)W * Tp, W / 16, 0, xa, B, T, Tp, W, 0, st);      // relu(h1)
            TwBatch b;
            const unsigned* rl = at<unsigned>(tp, fo.rl);
            const long long o2w = b.add(dout, Kp, Tp, xa, W, Tp, 0);
            const long long o2b = b.add(dout, Kp, Tp, aux, TW_AUXC, Tp, 0);
            const long long o1w = b.add(dh1, W, Tp, rl, W, Tp, 0);
            const long long c1w = b.add(dh1, W, Tp, enc, Cd, TL.TE, TL.c0);
            const long long o1b = b.add(dh1, W, Tp, aux, TW_AUXC, Tp, 0);
            b.red(o2w, W, 1, Kp, lay.out2_mean.W, 1);
            b.red(o2w + 1, W, 1, Kp, lay.out2_scale.W, 1);
            b.red(o2b + 3 * Kp, 1, 1, Kp, lay.out2_mean.b, 1);
            b.red(o2b + 3 * Kp + 1, 1, 1, Kp, lay.out2_scale.b, 1);
            b.red(o1w, W, W, W, lay.out1.W, W);
            b.red(c1w, Cd, W, W, lay.cond_out1.W, W);
            b.red(o1b + 3 * W, 1, W, W, lay.out1.b, W);
            b.red(o1b + 3 * W, 1, W, W, lay.cond_out1.b, W);
            if (int rc = b.run(h, run, st)) return rc;
        }
        if (d_encoding) denc_gemm(fl.cond_out1_t, dh1, W, Tp);
        {   // d l_final = W_out1^T d h1, masked by l_final > 0
            TgArgs a = args(fl.out1_t, dl, Tp, 0, W);
            a.seg[0] = tg_seg_g4(dh1, (long long)W * Tp, Tp, 0, W); a.nseg = 1;
            a.tape = at<float>(tp, fo.lf); a.tape_bstride = (long long)W * Tp; a.tape_nmb = W / 16;
            wn_tg_launch(TG_EPI_MASK, a, fl.out1_t.mtiles, B, Tp, st);
        }
        for (size_t li = fl.layers.size(); li-- > 0;) {
            const IafTrainLayer& tl = fl.layers[li];
            const IafLayerOff& lo = lay.layers[li];
            const float* gt = at<float>(tp, fo.g) + li * (size_t)B * W * Tp;
            {   // dm = W_res^T dl -> dd through the gate derivative
                TgArgs a = args(tl.res_t, dd, RD, 0, W);
                a.seg[0] = seg_dl; a.nseg = 1;
                a.tape = const_cast<float*>(gt); a.tape_bstride = (long long)W * Tp; a.tape_nmb = W / 16; a.tape_hoff = H / 16;
                a.bg_rows = H % 64 ? H : 0;             // width 64: the tile's upper 32 rows are padding
                wn_tg_launch(TG_EPI_BGATE, a, tl.res_t.mtiles, B, Tp, st);
            }
            if (wg) {
                wn_tw_act(gt, (long long)W * Tp, W / 16, H / 16, xa, B, T, Tp, H, 1, st);           // m_i = sigma * tanh
                TwBatch b;
                const long long rw = b.add(dl, W, Tp, xa, H, Tp, 0);
                const long long rb = b.add(dl, W, Tp, aux, TW_AUXC, Tp, 0);
                long long dw[3];
                for (int tap = 0; tap < 3; ++tap)
                    dw[tap] = b.add(dd, W, RD, slot(li), W, RS, IAF_LP - (long long)(2 - tap) * tl.dilation);
                const long long cw = b.add(dd, W, RD, enc, Cd, TL.TE, TL.c0);
                const long long db = b.add(dd, W, RD, aux, TW_AUXC, Tp, 0);
                b.red(rw, H, W, W, lo.res.W, W);
                b.red(rb + 3 * W, 1, W, W, lo.res.b, W);
                for (int tap = 0; tap < 3; ++tap) b.red(dw[tap], W, W, W, lo.dil.W + (size_t)tap * W * W, W);
                b.red(cw, Cd, W, W, lo.cond.W, W);
                b.red(db + 3 * W, 1, W, W, lo.dil.b, W);
                b.red(db + 3 * W, 1, W, W, lo.cond.b, W);
                if (int rc = b.run(h, run, st)) return rc;
            }
            if (d_encoding) denc_gemm(tl.cond_t, dd, W, RD);
            {   // dl += sum_k W_dil[k]^T dd(t + (2 - k) dilation)
                TgArgs a = args(tl.gate_t, dl, Tp, 0, W);
                for (int tap = 0; tap < 3; ++tap) a.seg[tap] = tg_seg_g4(dd, (long long)W * RD, RD, (long long)(2 - tap) * tl.dilation, W);
                a.nseg = 3;
                a.res_mtiles = W / 64;
                wn_tg_launch(TG_EPI_RS, a, tl.gate_t.mtiles, B, Tp, st);
            }
        }
        if (wg) {   // dl = d l_0: the start conv's variables, and its transpose into d x_{k-1}
            TwBatch b;
            const long long cs = b.add(dl, W, Tp, aux, TW_AUXC, Tp, 0);
            b.red(cs, 3, W, W, lay.start.W, W);
            b.red(cs + 3 * W, 1, W, W, lay.start.b, W);
            if (int rc = b.run(h, run, st)) return rc;
        }
        if (k > 0 || d_noise)   // flow 1's input is the noise
            wn_tb_dx(dl, h->d_blob + fl.start_off, scal, dx, B, W, T, Tp, true, st);
        if (d_encoding) {
            // flows that share a stack accumulate into its slice: the last flow stores, the ones before it add
            const int add = c.share_deconv && k + 1 < NF;
            wn_tw_denc(denc, scal, d_encoding + (size_t)fl.deconv_stack * B * TL.TE * Cd, B, TL.TE, RE, Cd, add, st);
        }
    }
    if (d_noise) {
        const size_t n = (size_t)B * T;
        hipLaunchKernelGGL(it_dnoise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dx, d_x,
                           at<float>(tp, TL.f[NF - 1].S), d_noise, n);
    }
    WN_HIP(h, hipGetLastError());
    return WN_OK;
}

int it_reverse(wn_handle* h, const char* fn, const void* tape, size_t tape_bytes, const float* d_x, const float* d_mean_tot,
               const float* d_scale_tot, int B, int F, int64_t T, float* grads, size_t grads_floats, float* d_noise,
               float* d_encoding, void* ws, size_t ws_bytes, void* stream) {
    const bool wg = grads != nullptr;
    if (int rc = it_check(h, fn)) return rc;
    if (int rc = it_shape_check(h, fn, B, F, T)) return rc;
    if (!tape || !d_x || !d_mean_tot || !d_scale_tot || (!grads && !d_noise) || !ws)
        return wn_fail(h, WN_EINVAL, "%s: bad argument", fn);
    const ItLayout TL = it_layout(h, B, F, T);
    if (int rc = it_tape_check(h, fn, tape, tape_bytes, TL, B, F, T)) return rc;
    if (wg && grads_floats < h->iaf_train.lay.table.floats)
        return wn_fail(h, WN_ENOMEM, "%s: grads holds %zu floats, the gradients need %zu", fn, grads_floats,
                       h->iaf_train.lay.table.floats);
    const ItBwdLayout BL = it_bwd_layout(h, TL, B, wg);
    if (wg && (long long)B * BL.nchunk > 65535) return wn_fail(h, WN_EINVAL, "%s: B = %d needs more than 65535 slabs", fn, B);
    if (ws_bytes < BL.total) return wn_fail(h, WN_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, BL.total);
    const WnWork work(h);
    return it_reverse_run(h, fn, tape, TL, BL, d_x, d_mean_tot, d_scale_tot, B, T, grads, d_noise, d_encoding, ws, stream);
}
}  // namespace

// ---- for wn_iaf_adjoint (wn_iaf_nll.hip): the checks of a reverse pass by name, and its data path alone ----
int wn_iaf_reverse_check(wn_handle* h, const char* fn, int B, int F, int64_t T) {
    if (int rc = it_check(h, fn)) return rc;
    return it_shape_check(h, fn, B, F, T);
}
int wn_iaf_reverse_tape_check(wn_handle* h, const char* fn, const void* tape, size_t tape_bytes, int B, int F, int64_t T) {
    return it_tape_check(h, fn, tape, tape_bytes, it_layout(h, B, F, T), B, F, T);
}
const float* wn_iaf_tape_scale_prod(const wn_handle* h, const void* tape, int B, int F, int64_t T) {
    return at<float>(const_cast<void*>(tape), it_layout(h, B, F, T).f[h->cfg.n_flows - 1].S);
}
int wn_iaf_reverse_input_run(wn_handle* h, const char* fn, const void* tape, const float* d_x, const float* d_mean_tot,
                             const float* d_scale_tot, int B, int F, int64_t T, float* d_noise, void* ws, void* stream) {
    const ItLayout TL = it_layout(h, B, F, T);
    return it_reverse_run(h, fn, tape, TL, it_bwd_layout(h, TL, B, false), d_x, d_mean_tot, d_scale_tot, B, T, nullptr, d_noise,
                          nullptr, ws, stream);
}

extern "C" int wn_iaf_backward_weights(wn_handle* h, const void* tape, size_t tape_bytes, const float* d_x,
                                       const float* d_mean_tot, const float* d_scale_tot, int B, int F, int64_t T, float* grads,
                                       size_t grads_floats, float* d_encoding, void* ws, size_t ws_bytes, void* stream) {
    return it_reverse(h, "wn_iaf_backward_weights", tape, tape_bytes, d_x, d_mean_tot, d_scale_tot, B, F, T, grads, grads_floats,
                      nullptr, d_encoding, ws, ws_bytes, stream);
}

extern "C" int wn_iaf_backward_input(wn_handle* h, const void* tape, size_t tape_bytes, const float* d_x, const float* d_mean_tot,
                                     const float* d_scale_tot, int B, int F, int64_t T, float* d_noise, float* d_encoding, void* ws,
                                     size_t ws_bytes, void* stream) {
    return it_reverse(h, "wn_iaf_backward_input", tape, tape_bytes, d_x, d_mean_tot, d_scale_tot, B, F, T, nullptr, 0, d_noise,
                      d_encoding, ws, ws_bytes, stream);
}
