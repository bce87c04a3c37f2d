// Internal declarations shared by the teacher's translation units:
//   wn_teacher.hip        the GEMM kernel, the packing, the forward, log_prob and its gradient
//   wn_teacher_bwd.hip    the tape and its registry, the reverse pass (input VJP)
//   wn_teacher_wgrad.hip  the weight-gradient GEMM, its product tables and the training tape
//   wn_teacher_dropout.hip  the dropout mask kernels of the training forward and the reverse pass
#pragma once
#include "wn_internal.h"

constexpr int TG_NT = 4;                 // 16-column blocks per wave
constexpr int TG_TN = 4 * 16 * TG_NT;    // columns per workgroup
constexpr int TG_KC = 4;                 // K-steps of weights per LDS stage
constexpr int TG_XP = 64;                // zero left pad of the scaled input row

enum { TG_SRC_G4 = 0, TG_SRC_ACC_RELU = 1 };
enum { TG_EPI_GATE = 0, TG_EPI_RS = 1, TG_EPI_ACC = 2, TG_EPI_OUT = 3, TG_EPI_GATE_TAPE = 4, TG_EPI_BGATE = 5, TG_EPI_MASK = 6 };

struct TgSeg {
    const unsigned* base;   // G4 words or accumulator-layout floats
    long long bstride;      // words per batch element
    int rowlen;             // G4: columns per group row; ACC: 16-row blocks per column block
    int col0;               // G4: column of t = 0 (left pad, tap shift, centre crop)
    int nks;                // 32-channel K-steps in this segment
    int ng;                 // G4: group rows per plane
    int kind;
};

struct TgArgs {
    TgSeg seg[4];
    int nseg, nks;
    const unsigned* wp;     // A fragments [m-tile][K-step][4 row blocks][plane][lane][4]
    const float* bias;      // [m-tile][64], tile-local row order
    float inv_scale;
    long long T;            // valid columns (only the time-major store is guarded)
    unsigned* og4;          // GATE: m;  RS: l (updated in place)
    long long og4_bstride;
    int og4_rowlen, og4_col0, og4_ng;
    float* oacc;            // RS: s (accumulated);  ACC: destination
    long long oacc_bstride;
    int oacc_nmb;
    int res_mtiles;         // RS: m-tiles below this are residual rows, the rest skip rows
    float* otm;             // OUT: [B][T][ow]
    int ow;
    // tape (accumulator layout [t/16][row block][lane][4] per batch element):  GATE_TAPE writes sigma at row block
    // hb and tanh at tape_hoff + hb, BGATE reads them;  MASK reads the pre-ReLU rows of its own row blocks
    float* tape;
    long long tape_bstride;
    int tape_nmb, tape_hoff;
};

// tg_gemm_kernel<epi, U> on a grid of Tp / TG_TN x mtiles / U x B workgroups (U = 2 for an even number of m-tiles)
void wn_tg_launch(int epi, const TgArgs& a, int mtiles, int B, long long Tp, hipStream_t st);
// G4 rows of C channels as an operand segment, and the fields of a launch that its weight pack fixes
inline TgSeg tg_seg_g4(const unsigned* p, long long bstride, long long rowlen, long long col0, int C) {
    TgSeg sg;
    sg.base = p; sg.bstride = bstride; sg.rowlen = (int)rowlen; sg.col0 = (int)col0; sg.nks = C / 32; sg.ng = C / 8;
    sg.kind = TG_SRC_G4;
    return sg;
}
inline TgArgs tg_pack_args(const wn_handle* h, const TeacherGemmPack& g, long long T) {
    TgArgs a{};
    a.wp = reinterpret_cast<const unsigned*>(h->d_blob + g.w_off);
    a.bias = h->d_blob + g.b_off;
    a.inv_scale = g.inv_scale;
    a.nks = g.nks;
    a.T = T;
    return a;
}

// ---- workspace of the forward ----
struct TLayout {
    long long T, Tp, TE, RS;
    int c0;
    size_t enc, l, m, s, h1, xs, scratch, total;
};
inline TLayout t_layout(const wn_handle* h, int B, int F, long long T) {
    const wn_config& c = h->cfg;
    TLayout L;
    L.T = T;
    L.Tp = (T + TG_TN - 1) / TG_TN * TG_TN;
    L.TE = (long long)F * h->frame_shift;
    L.c0 = (int)((L.TE - T) / 2);                           // wavenet.py:76-85
    L.RS = IAF_LP + L.Tp;
    size_t o = 0;
    auto carve = [&](size_t floats) { size_t r = o; o += align_up(floats * sizeof(float), 256); return r; };
    L.enc = carve((size_t)B * c.deconv_width * (L.TE + TG_TN) + 64);
    L.l = carve((size_t)B * c.width * L.RS);
    L.m = carve((size_t)B * (c.gate_width / 2) * L.Tp);
    L.s = carve((size_t)B * c.skip_width * L.Tp);
    L.h1 = carve((size_t)B * c.skip_width * L.Tp);
    L.xs = carve((size_t)B * (TG_XP + L.Tp));
    L.scratch = o;
    o += wn_deconv_scratch_bytes(h, B, F);
    L.total = o;
    return L;
}

// ---- the tape: a header, the pre-ReLU skip sum and out1 rows, sigma / tanh of every gate ----
constexpr uint32_t TB_MAGIC = 0x31505457u;         // "WTP1"
constexpr uint32_t TB_MAGIC_TRAIN = 0x32505457u;   // "WTP2": a training tape (wn_teacher_forward_train_tape)
constexpr size_t TB_HEAD = 256;
struct TapeLayout {
    long long Tp;
    size_t s, h1, g, total;
};
inline TapeLayout tape_layout(const wn_handle* h, int B, long long T) {
    const wn_config& c = h->cfg;
    TapeLayout L;
    L.Tp = (T + TG_TN - 1) / TG_TN * TG_TN;
    const size_t cols = (size_t)B * L.Tp;
    L.s = TB_HEAD;
    L.h1 = L.s + cols * c.skip_width * sizeof(float);
    L.g = L.h1 + cols * c.skip_width * sizeof(float);
    L.total = L.g + h->teacher.layers.size() * cols * c.gate_width * sizeof(float);
    return L;
}
// dropout of a training forward and of the reverse passes over its tape (mode 0: none)
struct TgDropout {
    int mode = 0;               // WN_DROPOUT_INPUTS / WN_DROPOUT_ALL
    uint64_t seed = 0;
    uint32_t thr = 0;           // an element is kept where its hash word is >= thr
    float keep = 1.0f;          // fp32(1 - rate): a kept element is v / keep
};
// where the forward writes what a tape keeps; a null member stays in the call's workspace (all null: wn_teacher_forward)
struct TgTape {
    float *s = nullptr, *h1 = nullptr, *g = nullptr;      // plain tape
    unsigned* l = nullptr;                                // training tape: the layer inputs l_i, one slot per layer
    float *enc = nullptr, *xs = nullptr;                  //   ... the conditioning and the scaled input row
    unsigned* lraw = nullptr;                             // dropout_inputs: the undropped l_0 (slot 0 of l holds the dropped one)
    TgDropout drop;
};
inline TgTape tape_regions(const TapeLayout& TL, void* tape) {
    char* tb = reinterpret_cast<char*>(tape);
    return TgTape{reinterpret_cast<float*>(tb + TL.s), reinterpret_cast<float*>(tb + TL.h1), reinterpret_cast<float*>(tb + TL.g)};
}

// ---- workspace of the reverse pass ----
struct BLayout {
    long long Tp, RD;
    int Kp;
    size_t scal, dout, dh1, ds, dl, dd, total;
};
BLayout b_layout(const wn_handle* h, int B, long long T);
struct TbWork {
    float* scal;                        // scale pair, then the partial maxima
    unsigned *dout, *dh1, *ds, *dl, *dd;   // cotangents as G4 rows of Tp columns (dd: RD, with the zero right pad)
    long long RD;
    int Kp;                             // channels of dout: out_width padded to 32
};
inline TbWork tb_work(const BLayout& L, void* ws) {
    char* base = reinterpret_cast<char*>(ws);
    auto at = [&](size_t off) { return reinterpret_cast<unsigned*>(base + off); };
    return TbWork{reinterpret_cast<float*>(base + L.scal), at(L.dout), at(L.dh1), at(L.ds), at(L.dl), at(L.dd), L.RD, L.Kp};
}

// ---- wn_teacher.hip ----
// checks of the forward calls (message prefix fn)
int tg_forward_check(wn_handle* h, const char* fn, const float* wav, const float* mel, int B, int F, int64_t T,
                     const float* out_params, const void* ws);
int tg_forward(wn_handle* h, const char* fn, const float* wav, const float* mel, int B, int F, int64_t T, float* out_params,
               void* ws, size_t ws_bytes, const TgTape& tape, void* stream);

// ---- wn_teacher_bwd.hip ----
// what the VJP-side calls refuse (the distillation losses' own refusals, wn_distill.hip)
int tb_check(wn_handle* h, const char* fn);
// registry check shared by the reverse-pass calls; *F receives the frame count of a training tape (0: a plain tape)
// and *drop the dropout its forward applied
int tb_tape_check(wn_handle* h, const char* fn, const void* tape, size_t tape_bytes, int B, int64_t T, int* F,
                  TgDropout* drop = nullptr);
// a tape-writing forward once its checks have passed: the header (magic, B, T, F), the forward into `regions`, and -- if that
// succeeded -- the registry entry of the tape (a training tape under TB_MAGIC_TRAIN, a plain one otherwise)
int tb_tape_forward(wn_handle* h, const char* fn, uint32_t magic, const float* wav, const float* mel, int B, int F, int64_t T,
                    float* out_params, void* tape, const TgTape& regions, void* ws, size_t ws_bytes, void* stream);
// The reverse pass.  wg == nullptr: the input VJP alone, launch for launch what wn_teacher_backward_input always ran.
// With wg the weight-gradient products, the d enc GEMMs and their reductions are issued between those launches, where
// the cotangents they read are complete; they write nothing the input VJP reads, so d_wav is the same bits.
struct TwCtx;
// dr: the dropout of the tape's forward; its masks are applied to the cotangents where the forward applied them.
int tb_reverse(wn_handle* h, const void* tape, const float* d_out_params, int B, int64_t T, float* d_wav, void* ws,
               void* stream, const TwCtx* wg, const TgDropout& dr);

// ---- wn_teacher_wgrad.hip: the weight-gradient side of the reverse pass, called where its operands are complete ----
int tw_aux(wn_handle* h, const TwCtx& w, hipStream_t st);                  // before anything else: aux rows, d enc zeroed
int tw_head(wn_handle* h, const TwCtx& w, hipStream_t st, int stage);      // stage 0: d h1 is complete;  1: ds is complete
int tw_layer(wn_handle* h, const TwCtx& w, size_t li, hipStream_t st);     // dl = d l_{li+1} and dd_li are complete
int tw_tail(wn_handle* h, const TwCtx& w, hipStream_t st);                 // dl = d l_0

// ---- wn_teacher_dropout.hip: the mask kernels ----
uint32_t wn_dropout_threshold(double rate);     // min(2^32 - 1, floor(rate 2^32 + 0.5))
// G4 rows [B][C][rowlen] with t = 0 at column col0 (a multiple of 4): dst = mask(src) on columns [col0, col0 + T), the left
// pad copied, zeros from column col0 + T on.  dst == src: in place.
void wn_dropout_g4(const unsigned* src, unsigned* dst, int B, int C, long long rowlen, long long col0, long long T,
                   const TgDropout& dr, int site, hipStream_t st);
// accumulator-layout rows [B][Tp / 16][C / 16][64][4] in place, on columns < T
void wn_dropout_acc(float* s, int B, int C, long long Tp, long long T, const TgDropout& dr, int site, hipStream_t st);
