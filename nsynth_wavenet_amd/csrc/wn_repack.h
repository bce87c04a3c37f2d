// The in-place re-packs: the index maps of wn_finalize's host packs as __device__ functions, one
// statement of each, shared by wn_teacher_set_weights (wn_train.hip: one launch per pack) and wn_iaf_set_weights
// (wn_iaf_repack.hip: one launch per KIND of pack over a descriptor table), and the per-stack host code of the upsampler's
// re-pack that both calls run.
#pragma once
#include "wn_internal.h"
#include "wn_pack_h.h"

constexpr int TR_NT = 256;
inline unsigned tr_blocks(size_t n) { return (unsigned)((n + TR_NT - 1) / TR_NT); }

// ---- plain fp32 parts ----
// HWIO [1,1,cin,cout] -> dst[o * ld + col0 + ci] (pack_T of wn_pack_ar); cin = 1, ld = 1 is a plain copy of cout floats
struct ScatterArgs {
    const float* src;
    float* dst;
    int cin, cout, ld, col0;
};
__device__ inline void tr_scatter_word(const ScatterArgs& a, size_t i) {
    if (i >= (size_t)a.cin * a.cout) return;
    const int o = (int)(i / a.cin), ci = (int)(i % a.cin);
    a.dst[(size_t)o * a.ld + a.col0 + ci] = a.src[(size_t)ci * a.cout + o];
}
// A-fragment order [row block][k-group of 16][lane][4] of a row-major [rows][KA] matrix; rows beyond `rows` are zero (frag of
// wn_pack_ar)
__device__ inline void tr_frag_word(const float* __restrict__ a, float* __restrict__ dst, int rows, int KA, size_t i) {
    const int nks4 = KA / 16, mbs = (rows + 15) / 16;
    if (i >= (size_t)mbs * nks4 * 256) return;
    const int jj = i & 3, lane = (i >> 2) & 63;
    const size_t blk = i >> 8;
    const int k4 = (int)(blk % nks4), mb = (int)(blk / nks4);
    const int row = 16 * mb + (lane & 15), k = 16 * k4 + 4 * jj + (lane >> 4);
    dst[i] = row >= rows ? 0.f : a[(size_t)row * KA + k];
}
// fp32 A fragments of one transposed-conv layer: [S][tap, block][mb][lane][4] of W [K][cout][cin] (wn_pack_deconv)
__device__ inline void tr_deconv_frag_word(const float* __restrict__ W, float* __restrict__ P, int S, int taps, int cin, int cout,
                                           size_t i) {
    const int nmb = cout / 16, cblk = cin / 16, nks4 = taps * cblk;
    if (i >= (size_t)S * nks4 * nmb * 256) return;
    const int jj = i & 3, lane = (i >> 2) & 63;
    size_t rest = i >> 8;
    const int mb = (int)(rest % nmb);
    rest /= nmb;
    const int ks4 = (int)(rest % nks4), r = (int)(rest / nks4);
    const int tap = ks4 / cblk, c4 = ks4 % cblk;
    const int co = 16 * mb + (lane & 15), ci = 16 * c4 + 4 * jj + (lane >> 4), k = S * tap + r;
    P[i] = W[((size_t)k * cout + co) * cin + ci];
}
// fp32 fragments of a student layer or head of width 64 (wn_pack_iaf): word [K-step / 4][mb][lane][K-step % 4] holds row
// 16 (j / 4) + 4 (lane / 16) + j % 4 of 64-row segment ks / 16 (j = ks % 16) of the TF kernels [rows][64] a (its first nA rows)
// and b (the rest), at output 16 mb + lane % 16
__device__ inline void iaf_frag32_word(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ dst, int nA,
                                       int nks, size_t i) {
    if (i >= (size_t)nks * 256) return;
    const int e = i & 3, lane = (i >> 2) & 63, mb = (i >> 8) & 3, ks = 4 * (int)(i >> 10) + e;
    const int seg = ks / 16, j = ks % 16, o = 16 * mb + (lane & 15);
    const int R = 64 * seg + 16 * (j >> 2) + 4 * (lane >> 4) + (j & 3);
    dst[i] = R < nA ? a[(size_t)R * 64 + o] : b[(size_t)(R - nA) * 64 + o];
}
// the 64 per-channel values behind a width-64 student pack (wn_pack_iaf, wn_pack_iaf_h): slot [q][mb][r] holds channel
// 16 mb + 4 q + r
__device__ inline int iaf_lane_row(int i) { return 16 * ((i >> 2) & 3) + 4 * (i >> 4) + (i & 3); }

// largest |x| of n floats, as the bit pattern of a non-negative float (exact in any order); NaNs are passed over like
// std::max does in pick_scale.  *out starts at zero.  Block `bid` of `nblk`, TR_NT threads.
__device__ inline void tr_absmax_block(const float* __restrict__ x, size_t n, unsigned* __restrict__ out, unsigned bid,
                                       unsigned nblk) {
    float mx = 0.f;
    for (size_t i = (size_t)bid * TR_NT + threadIdx.x; i < n; i += (size_t)nblk * TR_NT) {
        const float v = fabsf(x[i]);
        if (v > mx) mx = v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0 && mx > 0.f) atomicMax(out, __float_as_uint(mx));
}

// ---- split-fp16 packs.  One thread per packed word of pack_afrag's layout [fragment][plane][lane][4]. ----
enum { ROW_IDENT = 0, ROW_GATE = 1 };              // rowfn of wn_pack_teacher / wn_pack_iaf_train
// the matrix as stored, a transposed column range, gate_t's tap-major form (the teacher's [out][in] matrices); the student's
// TF kernels [rows][ld]: the transpose of `src` (nA rows) followed by `src2`, gate_t's [w][tap, g] of a [3][W][W] kernel, the
// two rows src | src2, the two columns src | src2 and zeros
enum { SRC_DIRECT = 0, SRC_T = 1, SRC_GATE_T = 2, SRC_CAT_T = 3, SRC_TAP_T = 4, SRC_ROWS2 = 5, SRC_COLS2 = 6 };
__device__ inline int tr_row(int kind, int M, int H, int i) {
    if (kind == ROW_IDENT) return i < M ? i : -1;
    const int j = i / 64, lr = i % 64;
    return lr < 32 ? 32 * j + lr : H + 32 * j + lr - 32;
}
struct TileArgs {
    const float* src;      // row-major matrix
    unsigned* dst;
    float sc;
    int ld, nks, mtiles;
    int rowkind, M, H;     // ROW_*: rows of the pack (ident) / half gate width (gate)
    int srckind;           // SRC_*
    int R, c0;             // SRC_T: rows of the source, first column taken
    int G, W;              // SRC_GATE_T; W: SRC_TAP_T
    const float* src2;     // SRC_CAT_T, SRC_ROWS2, SRC_COLS2
    int nA;                // SRC_CAT_T: rows of src
};
__device__ inline float tile_elem(const TileArgs& a, int row, int col) {
    if (a.srckind == SRC_DIRECT) return a.src[(size_t)row * a.ld + col];
    if (a.srckind == SRC_T) return col < a.R ? a.src[(size_t)col * a.ld + a.c0 + row] : 0.f;
    if (a.srckind == SRC_GATE_T) {
        const int k = col / a.G, g = col % a.G;
        return a.src[(size_t)g * a.ld + k * a.W + row];
    }
    if (a.srckind == SRC_CAT_T) return col < a.nA ? a.src[(size_t)col * a.ld + row] : a.src2[(size_t)(col - a.nA) * a.ld + row];
    if (a.srckind == SRC_TAP_T) return a.src[((size_t)(col / a.W) * a.W + row) * a.W + col % a.W];
    if (a.srckind == SRC_ROWS2) return (row == 0 ? a.src : a.src2)[col];
    return col == 0 ? a.src[row] : col == 1 ? a.src2[row] : 0.f;
}
// word i of [m-tile][K-step][4 row blocks][plane][lane][4] (pack_tiles / pack_afrag)
__device__ inline void tr_tile_word(const TileArgs& a, size_t i) {
    if (i >= (size_t)a.mtiles * a.nks * 4 * 512) return;
    const int ii = i & 3, lane = (i >> 2) & 63, plane = (i >> 8) & 1;
    const size_t f = i >> 9;
    const int mb = f & 3, ks = (int)((f >> 2) % a.nks), mt = (int)((f >> 2) / a.nks);
    const int i16 = lane & 15, kg = lane >> 4;
    const int row = tr_row(a.rowkind, a.M, a.H, mt * 64 + 16 * mb + i16);
    uint16_t hh[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int e = 2 * ii + p;
        const float v = row < 0 ? 0.f : __fmul_rn(a.sc, tile_elem(a, row, 32 * ks + 16 * (e >> 2) + 4 * kg + (e & 3)));
        hh[p] = split_half(v, plane);
    }
    a.dst[i] = (uint32_t)hh[0] | ((uint32_t)hh[1] << 16);
}

// ---- the upsampler's stack (wn_train.hip): what both calls run for one stack whose variables `up` hold, in the stack's own
// layout (sp.lay).  amax / mx: one slot per layer.
// the absolute maxima of the kernels, reduced into amax[j] (zeroed by the caller)
void wn_repack_deconv_absmax(const DeconvStackPack& sp, const float* up, unsigned* amax, hipStream_t st);
// the fp32 fragments and the bias
void wn_repack_deconv_plain(wn_handle* h, const DeconvStackPack& sp, const float* up, hipStream_t st);
// the split-fp16, phase-group and transposed packs under pick_scale(mx[j]), and their scales in the host structs
void wn_repack_deconv_split(wn_handle* h, DeconvStackPack& sp, const float* up, const float* mx, hipStream_t st);
uint64_t wn_repack_serial_next();   // tape serials of re-packed handles: apart from wn_finalize's counter
