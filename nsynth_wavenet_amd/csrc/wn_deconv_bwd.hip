// Reverse pass of the transposed-conv upsampler (wn_deconv.hip): gradients of trans_conv_j/kernel and trans_conv_j/bias
// from a cotangent of the stack's output.
//
// Per layer (stride S, filter length K, taps = K / S, pL = (K - S) / 2; x [cin][L] in, y = act(z) [C][S L] out):
//   z[co][t] = b[co] + sum_{ci,k,q : t = S q + k - pL} W[k][co][ci] x[ci][q]
// With t = S f + p, DZ_p[co][f] = dz[co][S f + p], dz = dy * act'(y), r = (p + pL) mod S, d = (p + pL) div S:
//   dW[S j + r][co][ci] = sum_{b,f} DZ_p[co][f] x[ci][f + d - j]          GEMM over the frame axis
//   db[co]              = sum_{b,t} dz[co][t]
//   dx[ci][f']          = sum_{p,j,co} W[S j + r][co][ci] DZ_p[co][f' - d + j]   GEMM over (p, j, co)
// Both GEMMs are "NT" products C[m][n] = sum_k A[m][k] B[n][k] of operands whose reduction index is contiguous, held as two
// planes of fp16 halves (hi = f16(v), lo = f16(v - hi), wn_codec.h) and multiplied as hi.hi + hi.lo + lo.hi on
// v_mfma_f32_16x16x32_f16 with fp32 accumulation.  One kernel body (nt_tile_step) serves both:
//   dW: A = DZ_p rows (channel-major, frames contiguous),  B = x rows SHIFTED by d - j (one copy of x per shift, so that
//       every 16-byte operand load is aligned), result rows co, columns ci = the TF order [1,K,Cout,Cin];
//   dx: A = W^T rows [k][ci][co] (packed at wn_finalize), B = DZ_p rows in FRAME-major order [f][co] (the tap shift is a
//       row offset), result rows ci, columns f'.
// wn_deconv_backward_input runs the dx chain alone, down to d mel: the first layer's W^T is packed with its rows
// padded to cinp, and db_dmel_kernel drops the padding columns.
// The forward is recomputed by wn_run_deconv into the call's workspace; nothing is taped.  Every output element has one
// writer, partial sums are added in a fixed order, no float atomics: repeated calls give identical bits.
#include <algorithm>

#include "wn_internal.h"
#include "wn_g4.h"
#include "wn_mfma_h.h"
#include "wn_pack_h.h"

namespace {

typedef unsigned short hf;            // storage of one fp16 half

constexpr int DB_FT = 16;             // frames per de-interleave tile
constexpr int DB_CT = 32;             // channels per de-interleave tile (one 32-channel block = four G4 groups)
constexpr int DB_MAXS = 30;           // largest stride: S * DB_FT * (DB_CT + 1) words of LDS
constexpr int DB_LP = 32;             // frames per batch row are padded to a multiple of the 32-wide K-step
constexpr int DB_SLAB = 4096;         // columns (batch x padded frames) per partial sum of a weight-gradient GEMM
constexpr int DB_WGS = 1024;          // workgroups the data-gradient GEMM aims at (four per CU)

struct LayerDims {
    int cin, cinp, C, K, S, pL, taps, dmax, nsh;
    int L, Lp, R;                     // input frames, padded, rows of a frame-major DZ image per (phase, batch row)
    long long N;                      // B * Lp
    int nslab;
    int pchunk, npc;                  // phases per workgroup of the data-gradient GEMM, number of such chunks
};

LayerDims layer_dims(const DeconvLayerPack& lp, int B, int L) {
    LayerDims d;
    d.cin = lp.cin; d.cinp = (lp.cin + 63) / 64 * 64; d.C = lp.cout; d.K = lp.K; d.S = lp.S; d.pL = lp.pL; d.taps = lp.taps;
    d.dmax = (lp.S - 1 + lp.pL) / lp.S;
    d.nsh = lp.taps + d.dmax;
    d.L = L; d.Lp = (L + DB_LP - 1) / DB_LP * DB_LP;
    d.R = d.dmax + (L + 63) / 64 * 64 + lp.taps;
    d.N = (long long)B * d.Lp;
    d.nslab = (int)((d.N + DB_SLAB - 1) / DB_SLAB);
    // enough phase chunks for about DB_WGS workgroups, from B and the frame count alone
    const long long tiles = (long long)(d.cinp / 64) * ((L + 63) / 64) * B;      // cinp = cin for every layer but the first
    const int want = (int)std::min<long long>(lp.S, std::max<long long>(1, (DB_WGS + tiles - 1) / std::max<long long>(tiles, 1)));
    d.pchunk = (lp.S + want - 1) / want;
    d.npc = (lp.S + d.pchunk - 1) / d.pchunk;
    return d;
}

struct BwdLayout {
    size_t scal, part_amax, enc, fwd, dzc, dzt, xs, dx, part, total;
};

BwdLayout bwd_layout(const wn_handle* h, const DeconvStackPack& sp, int B, int F) {
    BwdLayout o{};
    size_t dzc = 0, dzt = 0, xs = 0, dx = 0, part = 0;
    int L = F;
    for (size_t j = 0; j < sp.layers.size(); ++j) {
        const LayerDims d = layer_dims(sp.layers[j], B, L);
        dzc = std::max<size_t>(dzc, (size_t)2 * d.S * d.C * d.N * sizeof(hf));
        xs = std::max<size_t>(xs, (size_t)2 * d.nsh * d.cinp * d.N * sizeof(hf));
        part = std::max<size_t>(part, (size_t)d.nslab * d.K * d.C * d.cin * sizeof(float));
        if (j > 0) {
            part = std::max<size_t>(part, (size_t)d.npc * B * d.L * d.cin * sizeof(float));
            dzt = std::max<size_t>(dzt, (size_t)2 * d.S * B * d.R * d.C * sizeof(hf));
            dx = std::max<size_t>(dx, (size_t)B * d.L * d.cin * sizeof(float));
        }
        L *= d.S;
    }
    size_t p = 0;
    auto take = [&](size_t bytes) { const size_t at = p; p += align_up(std::max<size_t>(bytes, 16), 256); return at; };
    o.scal = take(sp.layers.size() * 4 * sizeof(float));
    o.part_amax = take(WN_NPART * sizeof(float));
    o.enc = take((size_t)B * h->cfg.deconv_width * (size_t)L * sizeof(float));
    o.fwd = take(wn_deconv_scratch_bytes(h, B, F));
    o.dzc = take(dzc);
    o.dzt = take(dzt);
    o.xs = take(xs);
    o.dx = take(dx);
    o.part = take(part);
    o.total = p;
    return o;
}

// wn_deconv_backward_input: no weight-gradient operands (dzc, xs, slabs); dzt and the phase chunks for the first layer too,
// whose chunks hold cinp columns per frame
struct BwdInLayout {
    size_t scal, part_amax, enc, fwd, dzt, dx, part, total;
};

BwdInLayout bwd_in_layout(const wn_handle* h, const DeconvStackPack& sp, int B, int F) {
    BwdInLayout o{};
    size_t dzt = 0, dx = 0, part = 0;
    int L = F;
    for (size_t j = 0; j < sp.layers.size(); ++j) {
        const LayerDims d = layer_dims(sp.layers[j], B, L);
        part = std::max<size_t>(part, (size_t)d.npc * B * d.L * d.cinp * sizeof(float));
        dzt = std::max<size_t>(dzt, (size_t)2 * d.S * B * d.R * d.C * sizeof(hf));
        if (j > 0) dx = std::max<size_t>(dx, (size_t)B * d.L * d.cin * sizeof(float));
        L *= d.S;
    }
    size_t p = 0;
    auto take = [&](size_t bytes) { const size_t at = p; p += align_up(std::max<size_t>(bytes, 16), 256); return at; };
    o.scal = take(sp.layers.size() * 4 * sizeof(float));
    o.part_amax = take(WN_NPART * sizeof(float));
    o.enc = take((size_t)B * h->cfg.deconv_width * (size_t)L * sizeof(float));
    o.fwd = take(wn_deconv_scratch_bytes(h, B, F));
    o.dzt = take(dzt);
    o.dx = take(dx);
    o.part = take(part);
    o.total = p;
    return o;
}

// ---- shifted split-fp16 images of a layer's input: xs[plane][s][ci][b Lp + f] = x[ci][f + s - (taps - 1)] ----
// G4: the hidden activation as the forward's interleave kernel wrote it (the halves it multiplied); otherwise mel [B,F,cin].
// One thread = 8 consecutive columns of one (shift, channel) row: one 16-byte store per plane.
template <bool G4>
__global__ __launch_bounds__(256) void db_xs_kernel(const void* __restrict__ src, int64_t ys, int yoff, int cin, int cinp, int C_src,
                                                    int L, int Lp, int taps, int nsh, int B, hf* __restrict__ xs) {
    const long long N = (long long)B * Lp;
    const long long item = (long long)blockIdx.x * 256 + threadIdx.x;     // (s, ci, n / 8)
    const long long per_row = N / 8;
    if (item >= (long long)nsh * cinp * per_row) return;
    const int s = (int)(item / (cinp * per_row));
    const long long rem = item - (long long)s * cinp * per_row;
    const int ci = (int)(rem / per_row);
    const long long n0 = (rem - (long long)ci * per_row) * 8;
    const int b = (int)(n0 / Lp), f0 = (int)(n0 - (long long)b * Lp);
    const int shift = s - (taps - 1);
    wn_u4 hw = {0u, 0u, 0u, 0u}, lw = {0u, 0u, 0u, 0u};
    if (ci < cin) {
        if (G4) {
            const unsigned* y = reinterpret_cast<const unsigned*>(src) + (size_t)b * C_src * ys;
            int g, slot, sh;
            wn_g4_slot(ci, g, slot, sh);
            const size_t lo_plane = (size_t)(C_src / 8) * ys * 4;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int f = f0 + e, q = f + shift;
                if (f < L && q >= 0 && q < L) {
                    const size_t at = ((size_t)g * ys + yoff + q) * 4 + slot;
                    hw[e >> 1] |= ((y[at] >> sh) & 0xffffu) << (16 * (e & 1));
                    lw[e >> 1] |= ((y[at + lo_plane] >> sh) & 0xffffu) << (16 * (e & 1));
                }
            }
        } else {
            const float* m = reinterpret_cast<const float*>(src) + (size_t)b * L * cin + ci;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int f = f0 + e, q = f + shift;
                v[e] = (f < L && q >= 0 && q < L) ? m[(size_t)q * cin] : 0.f;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned a, c2;
                wn_split_pair(v[2 * e], v[2 * e + 1], a, c2);
                hw[e] = a; lw[e] = c2;
            }
        }
    }
    const size_t row = ((size_t)s * cinp + ci) * N + n0;
    *reinterpret_cast<wn_u4*>(xs + row) = hw;
    *reinterpret_cast<wn_u4*>(xs + (size_t)nsh * cinp * N + row) = lw;
}

__device__ inline float db_act_grad(float y, int act) {
    if (act == WN_ACT_LEAKY_RELU) return y > 0.f ? 1.f : 0.4f;      // the sign of y is the sign of z
    if (act == WN_ACT_RELU) return y > 0.f ? 1.f : 0.f;
    return 1.f - y * y;                                             // tanh
}

// ---- de-interleave: cotangent [B][S L][C] (time-major) x act'(y) -> the phase rows DZ_p, split fp16 ----
//   dzc[plane][p][co][b Lp + f]            channel-major, for the weight-gradient GEMMs (zeros for f >= L; null: not wanted)
//   dzt[plane][p][b][dmax + f][co]         frame-major, for the data-gradient GEMM (null: not wanted; the rows outside
//                                          [dmax, dmax + Lp) are zeroed by the caller)
// One workgroup = DB_FT frames x DB_CT channels of one batch row = S DB_FT consecutive samples, through LDS; every store is
// a 16-byte word, 32 contiguous bytes per dzc row and 64 per dzt row.
// y: the layer's output in the forward's G4 layout (hidden layers in the forward's scratch, the last layer's in `enc`).
__global__ __launch_bounds__(256) void db_deint_kernel(const float* __restrict__ g, const float* __restrict__ scal,
                                                       const unsigned* __restrict__ yv, int64_t ys, int yoff, int C, int L, int Lp,
                                                       int S, int B, int R, int dmax, int act, hf* __restrict__ dzc,
                                                       hf* __restrict__ dzt) {
    __shared__ unsigned tile[DB_MAXS * DB_FT][DB_CT + 1];
    const int f0 = blockIdx.x * DB_FT, c0 = blockIdx.y * DB_CT, b = blockIdx.z;
    const int nt = S * DB_FT;
    const long long T = (long long)S * L, t0 = (long long)S * f0;
    const float sc = scal[0];
    for (int i = threadIdx.x; i < nt * DB_CT; i += 256) {
        const int tl = i / DB_CT, c = i - tl * DB_CT;
        const long long t = t0 + tl;
        const float v = t < T ? g[((size_t)b * T + t) * C + c0 + c] * sc : 0.f;
        tile[tl][c] = __builtin_bit_cast(unsigned, v);
    }
    __syncthreads();
    // channel pairs: (cc, cc + 1) share a word of the G4 layout; the split of a pair is one packed conversion
    for (int i = threadIdx.x; i < nt * (DB_CT / 2); i += 256) {
        const int pr = i / nt, tl = i - pr * nt, cc = 2 * pr;
        const long long t = t0 + tl;
        float y0 = 0.f, y1 = 0.f;
        if (t < T) {
            const unsigned* y = yv + (size_t)b * C * ys;
            int gq, slot, sh;                                       // sh = 0: cc is even
            wn_g4_slot(c0 + cc, gq, slot, sh);
            const size_t at = ((size_t)gq * ys + yoff + t) * 4 + slot;
            wn_join_pair(y[at], y[at + (size_t)(C / 8) * ys * 4], y0, y1);
        }
        const float d0 = __builtin_bit_cast(float, tile[tl][cc]) * db_act_grad(y0, act);
        const float d1 = __builtin_bit_cast(float, tile[tl][cc + 1]) * db_act_grad(y1, act);
        unsigned hw, lw;
        wn_split_pair(d0, d1, hw, lw);
        tile[tl][cc] = (hw & 0xffffu) | (lw << 16);                 // {hi, lo} of channel cc
        tile[tl][cc + 1] = (hw >> 16) | (lw & 0xffff0000u);
    }
    __syncthreads();
    const long long N = (long long)B * Lp;
    // channel-major rows: (plane, p, c, run of 8 frames)
    for (int i = threadIdx.x; dzc && i < 2 * S * DB_CT * (DB_FT / 8); i += 256) {      // (skipped without dzc)
        const int fr = i % (DB_FT / 8), c = (i / (DB_FT / 8)) % DB_CT, p = (i / (DB_FT / 8 * DB_CT)) % S,
                  plane = i / (DB_FT / 8 * DB_CT * S);
        wn_u4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned a = tile[S * (8 * fr + 2 * e) + p][c], c2 = tile[S * (8 * fr + 2 * e + 1) + p][c];
            w[e] = plane ? (a >> 16) | (c2 & 0xffff0000u) : (a & 0xffffu) | (c2 << 16);
        }
        *reinterpret_cast<wn_u4*>(dzc + (size_t)plane * S * C * N + ((size_t)p * C + c0 + c) * N + (size_t)b * Lp + f0 + 8 * fr) = w;
    }
    if (!dzt) return;
    // frame-major rows: (plane, p, f, run of 8 channels)
    for (int i = threadIdx.x; i < 2 * S * DB_FT * (DB_CT / 8); i += 256) {
        const int cq = i % (DB_CT / 8), f = (i / (DB_CT / 8)) % DB_FT, p = (i / (DB_CT / 8 * DB_FT)) % S,
                  plane = i / (DB_CT / 8 * DB_FT * S);
        wn_u4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned a = tile[S * f + p][8 * cq + 2 * e], c2 = tile[S * f + p][8 * cq + 2 * e + 1];
            w[e] = plane ? (a >> 16) | (c2 & 0xffff0000u) : (a & 0xffffu) | (c2 << 16);
        }
        *reinterpret_cast<wn_u4*>(dzt + (size_t)plane * S * B * R * C + (((size_t)p * B + b) * R + dmax + f0 + f) * C + c0 + 8 * cq) = w;
    }
}

// ---- the shared GEMM body: a wave owns 32 x 32 of the workgroup's 64 x 64 tile (2 x 2 MFMA blocks) ----
// a / b: this lane's row of the first block of each operand at the lane's k offset (8 halves = one 16-byte load);
// a16 / b16: halves between the two blocks' rows (16 rows); alo / blo: halves from the hi plane to the lo plane.
__device__ inline void nt_tile_steps(const hf* __restrict__ a, size_t a16, size_t alo, const hf* __restrict__ b, size_t b16,
                                     size_t blo, int nks, f4 (&acc)[2][2]) {
    // operands one K-step ahead of the MFMAs that consume them
    wn_u4 nah[2], nal[2], nbh[2], nbl[2];
    auto load = [&](int ks) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            nah[i] = *reinterpret_cast<const wn_u4*>(a + i * a16 + 32 * ks);
            nal[i] = *reinterpret_cast<const wn_u4*>(a + alo + i * a16 + 32 * ks);
            nbh[i] = *reinterpret_cast<const wn_u4*>(b + i * b16 + 32 * ks);
            nbl[i] = *reinterpret_cast<const wn_u4*>(b + blo + i * b16 + 32 * ks);
        }
    };
    if (nks > 0) load(0);
    for (int ks = 0; ks < nks; ++ks) {
        wn_u4 ah[2], al[2], bh[2], bl[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) { ah[i] = nah[i]; al[i] = nal[i]; bh[i] = nbh[i]; bl[i] = nbl[i]; }
        if (ks + 1 < nks) load(ks + 1);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                f4 c = acc[i][j];
                c = mfma_h(ah[i], bh[j], c);
                c = mfma_h(ah[i], bl[j], c);
                c = mfma_h(al[i], bh[j], c);
                acc[i][j] = c;
            }
    }
}

// Weight gradient: grid (C / 64 * cinp / 64, S * taps, slabs).  part[slab][k][co][ci], k = S j + r.
__global__ __launch_bounds__(256) void db_wgrad_kernel(const hf* __restrict__ dzc, const hf* __restrict__ xs, int C, int cin, int cinp,
                                                       long long N, int S, int taps, int pL, int nsh, int slab_cols,
                                                       float* __restrict__ part, size_t part_stride) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l16 = lane & 15, kg = lane >> 4;
    const int ntn = cinp / 64;
    const int m0 = (blockIdx.x / ntn) * 64 + 32 * (wave >> 1), n0 = (blockIdx.x % ntn) * 64 + 32 * (wave & 1);
    const int p = blockIdx.y / taps, jt = blockIdx.y - p * taps;
    const int r = (p + pL) % S, d = (p + pL) / S;
    const int k = S * jt + r, s = d - jt + taps - 1;
    const long long col0 = (long long)blockIdx.z * slab_cols;
    const long long left = N - col0;
    const int nks = (int)((left < slab_cols ? left : slab_cols) / 32);
    f4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f4){0.f, 0.f, 0.f, 0.f};
    const hf* a = dzc + ((size_t)p * C + m0 + l16) * N + col0 + 8 * kg;
    const hf* b = xs + ((size_t)s * cinp + n0 + l16) * N + col0 + 8 * kg;
    nt_tile_steps(a, (size_t)16 * N, (size_t)S * C * N, b, (size_t)16 * N, (size_t)nsh * cinp * N, nks, acc);
    float* out = part + (size_t)blockIdx.z * part_stride + (size_t)k * C * cin;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ci = n0 + 16 * j + l16;
            if (ci < cin)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) out[(size_t)(m0 + 16 * i + 4 * kg + rr) * cin + ci] = acc[i][j][rr];
        }
}

// Data gradient: grid (cin / 64 * ceil(L / 64), B, phase chunks).  part[chunk][b][f'][ci] (time-major fp32); a workgroup
// walks (phase of its chunk, tap, channel) in a fixed order, db_dxsum_kernel adds the chunks in order into the cotangent
// of the layer below.  The frame axis alone (10 F columns for the shipped last layer) would leave most of the machine idle
// on a reduction of S taps Cout = 20 480.
__global__ __launch_bounds__(256) void db_dgrad_kernel(const hf* __restrict__ wt, const hf* __restrict__ dzt, int C, int cin, int K,
                                                       int S, int taps, int pL, int dmax, int L, int R, int B, int pchunk,
                                                       float inv_scale, float* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l16 = lane & 15, kg = lane >> 4;
    const int ntm = cin / 64;
    const int m0 = (blockIdx.x % ntm) * 64 + 32 * (wave >> 1), f0 = (blockIdx.x / ntm) * 64 + 32 * (wave & 1);
    const int b = blockIdx.y;
    f4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f4){0.f, 0.f, 0.f, 0.f};
    const size_t wlo = (size_t)K * cin * C, zlo = (size_t)S * B * R * C;
    const int p1 = min(S, ((int)blockIdx.z + 1) * pchunk);
    float* dx = part + (size_t)blockIdx.z * B * L * cin;
    for (int p = blockIdx.z * pchunk; p < p1; ++p) {
        const int r = (p + pL) % S, d = (p + pL) / S;
        for (int jt = 0; jt < taps; ++jt) {
            const int k = S * jt + r;
            const hf* a = wt + ((size_t)k * cin + m0 + l16) * C + 8 * kg;
            const hf* bp = dzt + (((size_t)p * B + b) * R + dmax + f0 + l16 - d + jt) * C + 8 * kg;
            nt_tile_steps(a, (size_t)16 * C, wlo, bp, (size_t)16 * C, zlo, C / 32, acc);
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int f = f0 + 16 * j + l16;
            if (f < L)
                *reinterpret_cast<f4*>(dx + ((size_t)b * L + f) * cin + m0 + 16 * i + 4 * kg) = acc[i][j] * inv_scale;
        }
}

// dx[i] = sum over the phase chunks, in order
__global__ __launch_bounds__(256) void db_dxsum_kernel(const float* __restrict__ part, size_t n4, int nchunk, float* __restrict__ dx) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    f4 s = reinterpret_cast<const f4*>(part)[i];
    for (int k = 1; k < nchunk; ++k) s += reinterpret_cast<const f4*>(part)[(size_t)k * n4 + i];
    reinterpret_cast<f4*>(dx)[i] = s;
}

// d mel: the first layer's phase chunks [chunk][B F][cinp] summed in order, the padding columns cin .. cinp - 1 dropped, times
// scal[1] (what undoes every scale applied so far) -> float32 [B F][cin].  One thread = four columns of one frame; VEC: cin is
// a multiple of 4 and d_mel 16-byte aligned, one 16-byte store
template <bool VEC>
__global__ __launch_bounds__(256) void db_dmel_kernel(const float* __restrict__ part, size_t rows, int cin, int cinp, int nchunk,
                                                      const float* __restrict__ scal, float* __restrict__ d_mel) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int q = cinp / 4;
    if (i >= rows * q) return;
    const size_t row = i / q;
    const int c0 = 4 * (int)(i - row * q);
    if (c0 >= cin) return;
    f4 s = reinterpret_cast<const f4*>(part)[i];
    for (int k = 1; k < nchunk; ++k) s += reinterpret_cast<const f4*>(part)[(size_t)k * rows * q + i];
    s = s * scal[1];
    float* o = d_mel + row * cin + c0;
    if (VEC) *reinterpret_cast<f4*>(o) = s;
    else
        for (int e = 0; e < 4; ++e)
            if (c0 + e < cin) o[e] = s[e];
}

// grads[i] = (sum over the slabs, in order) * scal[1]
__global__ __launch_bounds__(256) void db_reduce_kernel(const float* __restrict__ part, size_t n, int nslab, const float* __restrict__ scal,
                                                        float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (int k = 1; k < nslab; ++k) s += part[(size_t)k * n + i];
    out[i] = s * scal[1];
}

// db[co] = sum over (phase, column) of hi + lo, one workgroup per channel, fixed order
__global__ __launch_bounds__(256) void db_bias_kernel(const hf* __restrict__ dzc, int C, int S, long long N, const float* __restrict__ scal,
                                                      float* __restrict__ out) {
    __shared__ float sh[256];
    const int co = blockIdx.x;
    const size_t lo = (size_t)S * C * N;
    float s = 0.f;
    for (int p = 0; p < S; ++p) {
        const hf* row = dzc + ((size_t)p * C + co) * N;
        for (long long n = threadIdx.x; n < N; n += 256)
            s += (float)__builtin_bit_cast(_Float16, row[n]) + (float)__builtin_bit_cast(_Float16, row[lo + n]);
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[co] = sh[0] * scal[1];
}

int find_stack(const wn_handle* h, const char* scope) {
    for (size_t i = 0; i < h->stacks.size(); ++i)
        if (h->stacks[i].prefix == (scope ? scope : "")) return (int)i;
    return -1;
}

// what the call refuses about the handle and the scope; quiet: no message (the size queries return 0)
int bwd_check(const wn_handle* h, const char* fn, const char* scope, int* si, bool quiet) {
#define DB_REFUSE(...) return quiet ? WN_EINVAL : wn_fail(h, WN_EINVAL, __VA_ARGS__)
    if (!h) DB_REFUSE("%s: null handle", fn);
    if (!h->finalized) return quiet ? WN_ESTATE : wn_fail(h, WN_ESTATE, "%s: call wn_finalize first", fn);
    const wn_config& c = h->cfg;
    if (c.use_resize_conv) DB_REFUSE("%s: use_resize_conv: the backward of the resize-conv upsampler is not implemented", fn);
    if (c.use_weight_norm) DB_REFUSE("%s: use_weight_norm: the gradients of W_V / W_g are not implemented", fn);
    *si = find_stack(h, scope);
    if (*si < 0) DB_REFUSE("%s: no deconv stack with scope '%s'", fn, scope ? scope : "");
    if (c.deconv_width % 64) DB_REFUSE("%s: deconv_width %d is not a multiple of 64", fn, c.deconv_width);
    for (const DeconvLayerPack& lp : h->stacks[*si].layers) {
        if (!lp.w_off_h) DB_REFUSE("%s: a layer of the stack has no split-fp16 pack (filter %d, stride %d, %d inputs)", fn, lp.K, lp.S, lp.cin);
        if (lp.S > DB_MAXS) DB_REFUSE("%s: stride %d above %d", fn, lp.S, DB_MAXS);
    }
    return WN_OK;
#undef DB_REFUSE
}

}  // namespace

// W^T of every layer but the first as two planes of halves [k][ci][co], prescaled like the forward's packs; called by
// wn_finalize after every other pack, so that no existing offset moves.  Behind those, the first layer's W^T with its rows
// padded to cinp (zero rows behind cin) for wn_deconv_backward_input.
int wn_pack_deconv_bwd(wn_handle* h, std::vector<float>& blob) {
    const wn_config& c = h->cfg;
    if (c.use_resize_conv || c.use_weight_norm || c.deconv_width % 64) return WN_OK;
    // rows: the row count of the packed planes (cin, or cinp for the first layer); returns the pack's offset and 1 / scale
    auto pack_t = [&](const DeconvStackPack& sp, size_t j, int rows, size_t* off, float* inv_scale) {
        const DeconvLayerPack& lp = sp.layers[j];
        const std::string scope = (sp.prefix.empty() ? std::string() : sp.prefix + "/") + "trans_conv_" + std::to_string(j + 1);
        const std::vector<float> W = wn_get_kernel(h, scope, "kernel", true);              // [K][cout][cin]
        const float sc = pick_scale(W.data(), W.size());
        const size_t n = (size_t)lp.K * rows * lp.cout;
        blob.resize(align_up(blob.size(), 64));
        *off = blob.size();
        *inv_scale = 1.0f / sc;
        blob.resize(blob.size() + n);                                                      // 2 planes of n halves, zero
        uint16_t* P = reinterpret_cast<uint16_t*>(blob.data() + *off);
        for (int k = 0; k < lp.K; ++k)
            for (int co = 0; co < lp.cout; ++co)
                for (int ci = 0; ci < lp.cin; ++ci) {
                    const float v = sc * W[((size_t)k * lp.cout + co) * lp.cin + ci];
                    const uint16_t hi = f2h(v);
                    const size_t at = ((size_t)k * rows + ci) * lp.cout + co;
                    P[at] = hi;
                    P[n + at] = f2h(v - h2f(hi));
                }
    };
    for (auto& sp : h->stacks)
        for (size_t j = 1; j < sp.layers.size(); ++j) {
            DeconvLayerPack& lp = sp.layers[j];
            if (lp.w_off_h) pack_t(sp, j, lp.cin, &lp.wt_off, &lp.wt_inv_scale);
        }
    for (auto& sp : h->stacks) {
        if (sp.layers.empty() || !sp.layers[0].w_off_h) continue;
        DeconvLayerPack& lp = sp.layers[0];
        pack_t(sp, 0, (lp.cin + 63) / 64 * 64, &lp.wt_in_off, &lp.wt_in_inv_scale);
    }
    return WN_OK;
}

// the parameter layout of every stack: per layer the kernel [1][K][cout][cin], then the bias
void wn_deconv_build_layout(wn_handle* h) {
    for (DeconvStackPack& sp : h->stacks) {
        sp.lay.clear();
        sp.table = WnGradTable();
        for (size_t j = 0; j < sp.layers.size(); ++j) {
            const DeconvLayerPack& lp = sp.layers[j];
            const std::string scope = (sp.prefix.empty() ? std::string() : sp.prefix + "/") + "trans_conv_" + std::to_string(j + 1);
            sp.lay.push_back(sp.table.conv(scope, "/kernel", "/bias", lp.K, lp.cout, lp.cin, lp.cout));
        }
    }
}

extern "C" int wn_deconv_grad_count(const wn_handle* h, const char* scope) {
    int si;
    if (bwd_check(h, "wn_deconv_grad_count", scope, &si, true)) return 0;
    return (int)h->stacks[si].table.entries.size();
}

extern "C" int wn_deconv_grad_info(const wn_handle* h, const char* scope, int i, char* name, size_t name_cap, int64_t* offset,
                                   int64_t* shape4, int* ndim) {
    int si;
    if (int rc = bwd_check(h, "wn_deconv_grad_info", scope, &si, false)) return rc;
    return wn_grad_info(h, "wn_deconv_grad_info", h->stacks[si].table.entries, i, name, name_cap, offset, shape4, ndim);
}

extern "C" size_t wn_deconv_grad_floats(const wn_handle* h, const char* scope) {
    int si;
    if (bwd_check(h, "wn_deconv_grad_floats", scope, &si, true)) return 0;
    return h->stacks[si].table.floats;
}

extern "C" size_t wn_deconv_backward_workspace_bytes(const wn_handle* h, const char* scope, int B, int F) {
    int si;
    if (B < 1 || F < 1 || bwd_check(h, "wn_deconv_backward_workspace_bytes", scope, &si, true)) return 0;
    return bwd_layout(h, h->stacks[si], B, F).total;
}

extern "C" int wn_deconv_backward(wn_handle* h, const char* scope, const float* mel, const float* d_enc, int B, int F, float* grads,
                                  size_t grads_floats, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "wn_deconv_backward";
    int si;
    if (int rc = bwd_check(h, fn, scope, &si, false)) return rc;
    if (!mel || !d_enc || !grads || !ws || B < 1 || F < 1) return wn_fail(h, WN_EINVAL, "%s: bad argument", fn);
    if (B > 65535) return wn_fail(h, WN_EINVAL, "%s: B = %d above 65535", fn, B);
    const DeconvStackPack& sp = h->stacks[si];
    if (grads_floats < sp.table.floats)
        return wn_fail(h, WN_EINVAL, "%s: grads holds %zu floats, the gradients need %zu", fn, grads_floats, sp.table.floats);
    const BwdLayout BL = bwd_layout(h, sp, B, F);
    if (ws_bytes < BL.total) return wn_fail(h, WN_EINVAL, "%s: workspace %zu < %zu bytes", fn, ws_bytes, BL.total);
    const int nl = (int)sp.layers.size();
    {
        int L = F;
        for (int j = 0; j < nl; ++j) {
            const LayerDims d = layer_dims(sp.layers[j], B, L);
            if (d.N > (1ll << 30) || d.nslab > 65535 || (long long)d.S * d.L > (1ll << 30))
                return wn_fail(h, WN_EINVAL, "%s: B = %d, F = %d is too long for one call", fn, B, F);
            if (j > 0 && !sp.layers[j].wt_off) return wn_fail(h, WN_EINVAL, "%s: a layer of the stack has no split-fp16 pack", fn);
            L *= d.S;
        }
    }
    const WnWork work(h);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* base = reinterpret_cast<char*>(ws);
    float* scal = reinterpret_cast<float*>(base + BL.scal);
    float* pamax = reinterpret_cast<float*>(base + BL.part_amax);
    float* enc = reinterpret_cast<float*>(base + BL.enc);
    void* fwd = base + BL.fwd;
    hf* dzc = reinterpret_cast<hf*>(base + BL.dzc);
    hf* dzt = reinterpret_cast<hf*>(base + BL.dzt);
    hf* xs = reinterpret_cast<hf*>(base + BL.xs);
    float* dx = reinterpret_cast<float*>(base + BL.dx);
    float* part = reinterpret_cast<float*>(base + BL.part);
    const int64_t Tn = (int64_t)F * h->frame_shift;
    // the forward, with the forward's kernels, in split-fp16 whatever the handle's precision: hidden activations stay in
    // `fwd`, the last layer's output goes to `enc`, all as the G4 halves the forward multiplies
    if (int rc = wn_run_deconv(h, si, mel, B, F, enc, Tn, fwd, st, true, nullptr, WN_PREC_F16X3)) return rc;
    std::vector<int> Lin(nl);
    {
        int L = F;
        for (int j = 0; j < nl; ++j) { Lin[j] = L; L *= sp.layers[j].S; }
    }
    const float* g = d_enc;
    for (int j = nl - 1; j >= 0; --j) {
        const DeconvLayerPack& lp = sp.layers[j];
        const LayerDims d = layer_dims(lp, B, Lin[j]);
        float* sj = scal + 4 * j;
        // scal[0] = 2^k applied to this layer's cotangent, scal[1] = what undoes every scale applied so far (the layer above's)
        wn_pow2_scale(g, (long long)B * d.S * d.L * d.C, pamax, sj, j + 1 < nl ? sj + 4 : nullptr, st);
        // shifted images of the layer's input
        {
            const long long items = (long long)d.nsh * d.cinp * (d.N / 8);
            const unsigned nbx = (unsigned)((items + 255) / 256);
            if (j == 0) {
                hipLaunchKernelGGL(db_xs_kernel<false>, dim3(nbx), dim3(256), 0, st, (const void*)mel, (int64_t)0, 0, d.cin, d.cinp, d.cin, d.L,
                                   d.Lp, d.taps, d.nsh, B, xs);
            } else {
                int64_t ys; int yoff;
                const void* hid = wn_deconv_hidden(h, B, F, j - 1, fwd, &ys, &yoff);
                hipLaunchKernelGGL(db_xs_kernel<true>, dim3(nbx), dim3(256), 0, st, hid, ys, yoff, d.cin, d.cinp, d.cin, d.L, d.Lp, d.taps,
                                   d.nsh, B, xs);
            }
        }
        hf* zt = j > 0 ? dzt : nullptr;
        if (zt) WN_HIP(h, hipMemsetAsync(zt, 0, (size_t)2 * d.S * B * d.R * d.C * sizeof(hf), st));
        const dim3 gd(d.Lp / DB_FT, d.C / DB_CT, B);
        {
            int64_t ys = Tn; int yoff = 0;
            const void* y = enc;
            if (j + 1 < nl) y = wn_deconv_hidden(h, B, F, j, fwd, &ys, &yoff);
            hipLaunchKernelGGL(db_deint_kernel, gd, dim3(256), 0, st, g, sj, reinterpret_cast<const unsigned*>(y), ys, yoff, d.C, d.L,
                               d.Lp, d.S, B, d.R, d.dmax, h->cfg.upsample_act, dzc, zt);
        }
        const size_t nw = (size_t)d.K * d.C * d.cin;
        hipLaunchKernelGGL(db_wgrad_kernel, dim3((d.C / 64) * (d.cinp / 64), d.S * d.taps, d.nslab), dim3(256), 0, st, dzc, xs, d.C,
                           d.cin, d.cinp, d.N, d.S, d.taps, d.pL, d.nsh, DB_SLAB, part, nw);
        hipLaunchKernelGGL(db_reduce_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, part, nw, d.nslab, sj,
                           grads + sp.lay[j].W);
        hipLaunchKernelGGL(db_bias_kernel, dim3(d.C), dim3(256), 0, st, dzc, d.C, d.S, d.N, sj, grads + sp.lay[j].b);
        if (j > 0) {
            // the slabs of the weight gradient are reduced by now: `part` holds the phase chunks of dx next
            hipLaunchKernelGGL(db_dgrad_kernel, dim3((d.cin / 64) * ((d.L + 63) / 64), B, d.npc), dim3(256), 0, st,
                               reinterpret_cast<const hf*>(h->d_blob + lp.wt_off), dzt, d.C, d.cin, d.K, d.S, d.taps, d.pL, d.dmax, d.L,
                               d.R, B, d.pchunk, lp.wt_inv_scale, part);
            const size_t n4 = (size_t)B * d.L * d.cin / 4;
            hipLaunchKernelGGL(db_dxsum_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, part, n4, d.npc, dx);
            g = dx;
        }
    }
    WN_HIP(h, hipGetLastError());
    return WN_OK;
}

// ---- d mel: the data-gradient chain alone, down to the first layer ----
extern "C" size_t wn_deconv_backward_input_workspace_bytes(const wn_handle* h, const char* scope, int B, int F) {
    int si;
    if (B < 1 || F < 1 || bwd_check(h, "wn_deconv_backward_input_workspace_bytes", scope, &si, true)) return 0;
    if (!h->stacks[si].layers[0].wt_in_off) return 0;
    return bwd_in_layout(h, h->stacks[si], B, F).total;
}

extern "C" int wn_deconv_backward_input(wn_handle* h, const char* scope, const float* mel, const float* d_enc, int B, int F,
                                        float* d_mel, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "wn_deconv_backward_input";
    int si;
    if (int rc = bwd_check(h, fn, scope, &si, false)) return rc;
    if (!mel || !d_enc || !d_mel || !ws || B < 1 || F < 1) return wn_fail(h, WN_EINVAL, "%s: bad argument", fn);
    if (B > 65535) return wn_fail(h, WN_EINVAL, "%s: B = %d above 65535", fn, B);
    const DeconvStackPack& sp = h->stacks[si];
    const int nl = (int)sp.layers.size();
    std::vector<int> Lin(nl);
    {
        int L = F;
        for (int j = 0; j < nl; ++j) {
            const LayerDims d = layer_dims(sp.layers[j], B, L);
            if (d.N > (1ll << 30) || d.nslab > 65535 || (long long)d.S * d.L > (1ll << 30))
                return wn_fail(h, WN_EINVAL, "%s: B = %d, F = %d is too long for one call", fn, B, F);
            if (!(j ? sp.layers[j].wt_off : sp.layers[j].wt_in_off))
                return wn_fail(h, WN_EINVAL, "%s: a layer of the stack has no split-fp16 pack", fn);
            Lin[j] = L;
            L *= d.S;
        }
    }
    const BwdInLayout BL = bwd_in_layout(h, sp, B, F);
    if (ws_bytes < BL.total) return wn_fail(h, WN_EINVAL, "%s: workspace %zu < %zu bytes", fn, ws_bytes, BL.total);
    const WnWork work(h);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* base = reinterpret_cast<char*>(ws);
    float* scal = reinterpret_cast<float*>(base + BL.scal);
    float* pamax = reinterpret_cast<float*>(base + BL.part_amax);
    float* enc = reinterpret_cast<float*>(base + BL.enc);
    void* fwd = base + BL.fwd;
    hf* dzt = reinterpret_cast<hf*>(base + BL.dzt);
    float* dx = reinterpret_cast<float*>(base + BL.dx);
    float* part = reinterpret_cast<float*>(base + BL.part);
    const int64_t Tn = (int64_t)F * h->frame_shift;
    // the forward as wn_deconv_backward recomputes it: split-fp16 whatever the handle's precision
    if (int rc = wn_run_deconv(h, si, mel, B, F, enc, Tn, fwd, st, true, nullptr, WN_PREC_F16X3)) return rc;
    const float* g = d_enc;
    for (int j = nl - 1; j >= 0; --j) {
        const DeconvLayerPack& lp = sp.layers[j];
        const LayerDims d = layer_dims(lp, B, Lin[j]);
        float* sj = scal + 4 * j;
        wn_pow2_scale(g, (long long)B * d.S * d.L * d.C, pamax, sj, j + 1 < nl ? sj + 4 : nullptr, st);
        WN_HIP(h, hipMemsetAsync(dzt, 0, (size_t)2 * d.S * B * d.R * d.C * sizeof(hf), st));
        {
            int64_t ys = Tn; int yoff = 0;
            const void* y = enc;
            if (j + 1 < nl) y = wn_deconv_hidden(h, B, F, j, fwd, &ys, &yoff);
            hipLaunchKernelGGL(db_deint_kernel, dim3(d.Lp / DB_FT, d.C / DB_CT, B), dim3(256), 0, st, g, sj,
                               reinterpret_cast<const unsigned*>(y), ys, yoff, d.C, d.L, d.Lp, d.S, B, d.R, d.dmax, h->cfg.upsample_act,
                               (hf*)nullptr, dzt);
        }
        // rows of the result: cin, or for the first layer cinp -- the rows behind cin are the pack's zero rows
        const int rows = j ? d.cin : d.cinp;
        hipLaunchKernelGGL(db_dgrad_kernel, dim3((rows / 64) * ((d.L + 63) / 64), B, d.npc), dim3(256), 0, st,
                           reinterpret_cast<const hf*>(h->d_blob + (j ? lp.wt_off : lp.wt_in_off)), dzt, d.C, rows, d.K, d.S, d.taps,
                           d.pL, d.dmax, d.L, d.R, B, d.pchunk, j ? lp.wt_inv_scale : lp.wt_in_inv_scale, part);
        if (j > 0) {
            const size_t n4 = (size_t)B * d.L * d.cin / 4;
            hipLaunchKernelGGL(db_dxsum_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, part, n4, d.npc, dx);
            g = dx;
        } else {
            const size_t nrow = (size_t)B * d.L, items = nrow * (d.cinp / 4);
            const dim3 gd((unsigned)((items + 255) / 256));
            if (d.cin % 4 == 0 && (reinterpret_cast<uintptr_t>(d_mel) & 15) == 0)
                hipLaunchKernelGGL(db_dmel_kernel<true>, gd, dim3(256), 0, st, part, nrow, d.cin, d.cinp, d.npc, sj, d_mel);
            else
                hipLaunchKernelGGL(db_dmel_kernel<false>, gd, dim3(256), 0, st, part, nrow, d.cin, d.cinp, d.npc, sj, d_mel);
        }
    }
    WN_HIP(h, hipGetLastError());
    return WN_OK;
}
