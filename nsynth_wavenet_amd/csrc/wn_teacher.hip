// Full-sequence (teacher-forced) forward of the WaveNet teacher: wavenet/wavenet.py:180-291.
//
// The autoregressive path (wn_ar.hip) evaluates one sample per step; scoring or checking a
// whole utterance that way costs T dependent steps.  Given the audio, every layer is a dense
// GEMM over time, so the same network runs here as a chain of split-fp16 MFMA GEMMs on
// channel-major activations (the layouts of the IAF path):
//   l, m, enc : G4 words (wn_iaf_h.hip) -- the MFMA B operand of a lane is one 16-byte load
//   s, out1   : fp32 in the MFMA accumulator layout [t/16][16-row block][lane][4] -- written and
//               read-modify-written with one 16-byte access per lane, and the accumulator
//               registers of two row blocks ARE the B operand of a K-step of the next GEMM
// One kernel template: C[64 or 128 rows][256 columns] per workgroup, K walked over up to four operand
// segments (three dilated taps of l + enc; m; relu(s) + enc; relu(out1)), weights as A fragments
// staged through LDS in double-buffered chunks shared by the four waves.  Epilogues: gate ->
// m; residual add -> l and skip accumulate -> s; plain store; time-major out_params.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <mutex>
#include <unordered_map>

#include "wn_internal.h"
#include "wn_codec.h"
#include "wn_mol.h"
#include "wn_pack_h.h"
#include "wn_mfma_h.h"

namespace {

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

// U = 64-row m-tiles per workgroup (1 or 2): two tiles halve the re-reads of the activation operand,
// which bound the kernel (each operand word is fetched once per workgroup row of the grid).
template <int EPI, int U>
__global__ __launch_bounds__(256, 2) void tg_gemm_kernel(const TgArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned lds[2][TG_KC * 4 * 512];
    constexpr int KC = TG_KC / U;                 // K-steps per LDS stage (64 KB in both shapes)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 15, q = lane >> 4;
    const int mt0 = blockIdx.y * U, b = blockIdx.z;
    const int t0 = blockIdx.x * TG_TN + wave * 16 * TG_NT;      // first column of this wave
    const int nchunk = (a.nks + KC - 1) / KC;

    f4 acc[4 * U][TG_NT];
#pragma unroll
    for (int mb = 0; mb < 4 * U; ++mb)
#pragma unroll
        for (int e = 0; e < TG_NT; ++e) acc[mb][e] = (f4){0.f, 0.f, 0.f, 0.f};

    const wn_u4* wsrc = reinterpret_cast<const wn_u4*>(a.wp);
    auto stage = [&](int chunk, int buf) {
#pragma unroll
        for (int kl = 0; kl < KC; ++kl) {
            const int ks = chunk * KC + kl;
            if (ks < a.nks) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const wn_u4* src = wsrc + ((size_t)(mt0 + u) * a.nks + ks) * 512;
                    wn_u4* dst = reinterpret_cast<wn_u4*>(lds[buf]) + (kl * U + u) * 512;
                    dst[threadIdx.x] = src[threadIdx.x];
                    dst[threadIdx.x + 256] = src[threadIdx.x + 256];
                }
            }
        }
    };
    // operand words of K-step ks for the TG_NT column blocks of this lane
    auto loadB = [&](int ks, wn_u4 (&vh)[TG_NT], wn_u4 (&vl)[TG_NT]) {
        int si = 0, ksl = ks;
        while (si + 1 < a.nseg && ksl >= a.seg[si].nks) { ksl -= a.seg[si].nks; ++si; }
        const TgSeg& s = a.seg[si];
        if (s.kind == TG_SRC_G4) {
            const wn_u4* p = reinterpret_cast<const wn_u4*>(s.base + (size_t)b * s.bstride) +
                             (size_t)(4 * ksl + q) * s.rowlen + s.col0 + t0 + n;
            const size_t lo = (size_t)s.ng * s.rowlen;
#pragma unroll
            for (int e = 0; e < TG_NT; ++e) {
                vh[e] = p[16 * e];
                vl[e] = p[lo + 16 * e];
            }
        } else {
            // accumulator layout: the registers of row blocks 2ksl, 2ksl+1 of lane (q, n) are the 8 k-slots
            const f4* p = reinterpret_cast<const f4*>(reinterpret_cast<const float*>(s.base) + (size_t)b * s.bstride) +
                          ((size_t)(t0 >> 4) * s.rowlen + 2 * ksl) * 64 + lane;
#pragma unroll
            for (int e = 0; e < TG_NT; ++e) {
                const f4 v0 = p[(size_t)e * s.rowlen * 64], v1 = p[(size_t)e * s.rowlen * 64 + 64];
                unsigned h0, l0, h1, l1, h2, l2, h3, l3;
                wn_split_pair(fmaxf(v0[0], 0.f), fmaxf(v0[1], 0.f), h0, l0);
                wn_split_pair(fmaxf(v0[2], 0.f), fmaxf(v0[3], 0.f), h1, l1);
                wn_split_pair(fmaxf(v1[0], 0.f), fmaxf(v1[1], 0.f), h2, l2);
                wn_split_pair(fmaxf(v1[2], 0.f), fmaxf(v1[3], 0.f), h3, l3);
                vh[e] = (wn_u4){h0, h1, h2, h3};
                vl[e] = (wn_u4){l0, l1, l2, l3};
            }
        }
    };

    stage(0, 0);
    wn_u4 b1h[TG_NT], b1l[TG_NT];
    loadB(0, b1h, b1l);
    __syncthreads();
    for (int chunk = 0; chunk < nchunk; ++chunk) {
        const int buf = chunk & 1;
        if (chunk + 1 < nchunk) stage(chunk + 1, buf ^ 1);
        const wn_u4* Al = reinterpret_cast<const wn_u4*>(lds[buf]) + lane;
#pragma unroll
        for (int kl = 0; kl < KC; ++kl) {
            const int ks = chunk * KC + kl;
            if (ks < a.nks) {
                wn_u4 vh[TG_NT], vl[TG_NT];
#pragma unroll
                for (int e = 0; e < TG_NT; ++e) { vh[e] = b1h[e]; vl[e] = b1l[e]; }
                if (ks + 1 < a.nks) loadB(ks + 1, b1h, b1l);
#ifndef WN_TG_APIPE
#define WN_TG_APIPE 1
#endif
                if (WN_TG_APIPE) {
                    // weight fragments one row block (12 MFMAs) ahead of their use: read where they are used, each pair of
                    // ds_read_b128 sat in front of its own MFMAs and the wave waited out the LDS latency twelve MFMAs at a time
                    wn_u4 ahn = Al[(kl * 4 * U) * 128], aln = Al[(kl * 4 * U) * 128 + 64];
                    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
                    for (int mb = 0; mb < 4 * U; ++mb) {
                        const wn_u4 ah = ahn, al = aln;
                        if (mb + 1 < 4 * U) {
                            ahn = Al[(kl * 4 * U + mb + 1) * 128];
                            aln = Al[(kl * 4 * U + mb + 1) * 128 + 64];
                        }
#pragma unroll
                        for (int e = 0; e < TG_NT; ++e) acc[mb][e] = mfma3(ah, al, vh[e], vl[e], acc[mb][e]);
                        if (mb + 1 < 4 * U) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
                        __builtin_amdgcn_sched_group_barrier(0x008, 3 * TG_NT, 0);
                    }
                } else {
#pragma unroll
                for (int mb = 0; mb < 4 * U; ++mb) {
                    const wn_u4 ah = Al[(kl * 4 * U + mb) * 128], al = Al[(kl * 4 * U + mb) * 128 + 64];
#pragma unroll
                    for (int e = 0; e < TG_NT; ++e) acc[mb][e] = mfma3(ah, al, vh[e], vl[e], acc[mb][e]);
                }
                }
            }
        }
        __syncthreads();
    }

    // ---- epilogue per 64-row tile: row 16 mb + 4 q + r of the tile, column t0 + 16 e + n ----
    const float inv = a.inv_scale;
#pragma unroll
    for (int u = 0; u < U; ++u) {
    const int mt = mt0 + u;
    const f4* bias4 = reinterpret_cast<const f4*>(a.bias + (size_t)mt * 64) + q;
    f4 bv[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) bv[mb] = bias4[mb * 4];
    f4 (&ac)[4][TG_NT] = *reinterpret_cast<f4 (*)[4][TG_NT]>(&acc[4 * u]);
    if (EPI == TG_EPI_GATE || EPI == TG_EPI_GATE_TAPE) {
        // rows 0-31: sigmoid half of gate channels 32 mt .. +31, rows 32-63: their tanh half
        // (GATE_TAPE: the same arithmetic, and both activations go to the tape for the input VJP)
        wn_u4* o = reinterpret_cast<wn_u4*>(a.og4 + (size_t)b * a.og4_bstride) +
                   (size_t)(4 * mt + q) * a.og4_rowlen + a.og4_col0 + t0 + n;
        const size_t lo = (size_t)a.og4_ng * a.og4_rowlen;
#pragma unroll
        for (int e = 0; e < TG_NT; ++e) {
            wn_u4 gh, gl;
#pragma unroll
            for (int mg = 0; mg < 2; ++mg) {
                f4 sg, th;
#pragma unroll
                for (int rp = 0; rp < 2; ++rp) {
                    float g[2];
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const float sv = sigmoidf_(fmaf(ac[mg][e][2 * rp + k], inv, bv[mg][2 * rp + k]));
                        const float tv = tanhf_(fmaf(ac[mg + 2][e][2 * rp + k], inv, bv[mg + 2][2 * rp + k]));
                        g[k] = sv * tv;
                        sg[2 * rp + k] = sv;
                        th[2 * rp + k] = tv;
                    }
                    unsigned hw, lw;
                    wn_split_pair(g[0], g[1], hw, lw);
                    gh[2 * mg + rp] = hw;
                    gl[2 * mg + rp] = lw;
                }
                if (EPI == TG_EPI_GATE_TAPE) {
                    f4* tp = reinterpret_cast<f4*>(a.tape + (size_t)b * a.tape_bstride) +
                             ((size_t)((t0 >> 4) + e) * a.tape_nmb + 2 * mt + mg) * 64 + lane;
                    tp[0] = sg;
                    tp[(size_t)a.tape_hoff * 64] = th;
                }
            }
            o[16 * e] = gh;
            o[lo + 16 * e] = gl;
        }
    } else if (EPI == TG_EPI_RS && mt < a.res_mtiles) {
        // residual rows 64 mt .. +63: l += res  (wavenet.py:272-274), two 32-channel operand groups
        const size_t lo = (size_t)a.og4_ng * a.og4_rowlen;
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            wn_u4* o = reinterpret_cast<wn_u4*>(a.og4 + (size_t)b * a.og4_bstride) +
                       (size_t)(4 * (2 * mt + st) + q) * a.og4_rowlen + a.og4_col0 + t0 + n;
#pragma unroll
            for (int e = 0; e < TG_NT; ++e) {
                const wn_u4 oh = o[16 * e], ol = o[lo + 16 * e];
                wn_u4 nh, nl;
#pragma unroll
                for (int mg = 0; mg < 2; ++mg)
#pragma unroll
                    for (int rp = 0; rp < 2; ++rp) {
                        const int mb = 2 * st + mg;
                        float l0, l1;
                        wn_join_pair(oh[2 * mg + rp], ol[2 * mg + rp], l0, l1);
                        l0 += fmaf(ac[mb][e][2 * rp], inv, bv[mb][2 * rp]);
                        l1 += fmaf(ac[mb][e][2 * rp + 1], inv, bv[mb][2 * rp + 1]);
                        unsigned hw, lw;
                        wn_split_pair(l0, l1, hw, lw);
                        nh[2 * mg + rp] = hw;
                        nl[2 * mg + rp] = lw;
                    }
                o[16 * e] = nh;
                o[lo + 16 * e] = nl;
            }
        }
    } else if (EPI == TG_EPI_RS || EPI == TG_EPI_ACC) {
        // accumulator-layout destination: s += skip (wavenet.py:275-277) or a plain store
        const int mrow = EPI == TG_EPI_RS ? mt - a.res_mtiles : mt;
        f4* o = reinterpret_cast<f4*>(a.oacc + (size_t)b * a.oacc_bstride) +
                ((size_t)(t0 >> 4) * a.oacc_nmb + 4 * mrow) * 64 + lane;
#pragma unroll
        for (int e = 0; e < TG_NT; ++e)
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) {
                f4* p = o + ((size_t)e * a.oacc_nmb + mb) * 64;
                f4 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaf(ac[mb][e][r], inv, bv[mb][r]);
                if (EPI == TG_EPI_RS) v += *p;
                *p = v;
            }
    } else if (EPI == TG_EPI_BGATE) {
        // input VJP of the gate: dm rows h = 64 mt + 16 mb + 4 q + r (wavenet.py:264-269 transposed) ->
        // dd_sigma[h] = dm tanh sigma (1 - sigma) and dd_tanh[h] = dm sigma (1 - tanh^2), G4 channels h and H + h
        const size_t lo = (size_t)a.og4_ng * a.og4_rowlen;
        const f4* tp = reinterpret_cast<const f4*>(a.tape + (size_t)b * a.tape_bstride) + lane;
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            wn_u4* os = reinterpret_cast<wn_u4*>(a.og4 + (size_t)b * a.og4_bstride) +
                        (size_t)(4 * (2 * mt + st) + q) * a.og4_rowlen + a.og4_col0 + t0 + n;
            wn_u4* ot = os + (size_t)(2 * a.tape_hoff) * a.og4_rowlen;
#pragma unroll
            for (int e = 0; e < TG_NT; ++e) {
                // columns >= T: the tape holds what the forward made of its pad operands (possibly NaN) and dm is 0 --
                // a select, not the product, so dd is 0 there and the anti-causal taps of the next GEMM read zeros
                const bool live = t0 + 16 * e + n < a.T;
                wn_u4 sh, sl, th, tl;
#pragma unroll
                for (int mg = 0; mg < 2; ++mg) {
                    const int mb = 2 * st + mg;
                    const size_t ti = ((size_t)((t0 >> 4) + e) * a.tape_nmb + 4 * mt + mb) * 64;
                    const f4 sg = tp[ti], tg = tp[ti + (size_t)a.tape_hoff * 64];
                    float vs[4], vt[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float dm = ac[mb][e][r] * inv;
                        vs[r] = live ? dm * tg[r] * (sg[r] * (1.f - sg[r])) : 0.f;
                        vt[r] = live ? dm * sg[r] * (1.f - tg[r] * tg[r]) : 0.f;
                    }
#pragma unroll
                    for (int rp = 0; rp < 2; ++rp) {
                        unsigned hw, lw;
                        wn_split_pair(vs[2 * rp], vs[2 * rp + 1], hw, lw);
                        sh[2 * mg + rp] = hw;
                        sl[2 * mg + rp] = lw;
                        wn_split_pair(vt[2 * rp], vt[2 * rp + 1], hw, lw);
                        th[2 * mg + rp] = hw;
                        tl[2 * mg + rp] = lw;
                    }
                }
                os[16 * e] = sh;
                os[lo + 16 * e] = sl;
                ot[16 * e] = th;
                ot[lo + 16 * e] = tl;
            }
        }
    } else if (EPI == TG_EPI_MASK) {
        // ReLU transposed: G4 rows 64 mt + ... = acc where the taped pre-ReLU value of the same row is > 0, else 0
        const size_t lo = (size_t)a.og4_ng * a.og4_rowlen;
        const f4* tp = reinterpret_cast<const f4*>(a.tape + (size_t)b * a.tape_bstride) + lane;
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            wn_u4* o = reinterpret_cast<wn_u4*>(a.og4 + (size_t)b * a.og4_bstride) +
                       (size_t)(4 * (2 * mt + st) + q) * a.og4_rowlen + a.og4_col0 + t0 + n;
#pragma unroll
            for (int e = 0; e < TG_NT; ++e) {
                wn_u4 nh, nl;
#pragma unroll
                for (int mg = 0; mg < 2; ++mg) {
                    const int mb = 2 * st + mg;
                    const f4 mk = tp[((size_t)((t0 >> 4) + e) * a.tape_nmb + 4 * mt + mb) * 64];
                    float v[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = mk[r] > 0.f ? ac[mb][e][r] * inv : 0.f;
#pragma unroll
                    for (int rp = 0; rp < 2; ++rp) {
                        unsigned hw, lw;
                        wn_split_pair(v[2 * rp], v[2 * rp + 1], hw, lw);
                        nh[2 * mg + rp] = hw;
                        nl[2 * mg + rp] = lw;
                    }
                }
                o[16 * e] = nh;
                o[lo + 16 * e] = nl;
            }
        }
    } else {
        // out_params, the reference's [B][T][out_width]
#pragma unroll
        for (int e = 0; e < TG_NT; ++e) {
            const long long t = t0 + 16 * e + n;
            if (t >= a.T) continue;
            float* o = a.otm + ((size_t)b * a.T + t) * a.ow;
#pragma unroll
            for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = 64 * mt + 16 * mb + 4 * q + r;
                    if (c < a.ow) o[c] = fmaf(ac[mb][e][r], inv, bv[mb][r]);
                }
        }
    }
    }
}

// scaled input row: zero pad | encode(wav)  (wavenet.py:412-418 encoding, masked.py:39-52 shift by reading t-1)
__global__ void tg_input_kernel(const float* __restrict__ wav, float* __restrict__ xs, long long T, long long Tp,
                                int mu) {
    const int b = blockIdx.y;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= TG_XP + Tp) return;
    const long long t = i - TG_XP;
    float v = 0.f;
    if (t >= 0 && t < T) {
        v = wav[(size_t)b * T + t];
        if (mu) v = wn_mu_law_scaled(v);
    }
    xs[(size_t)b * (TG_XP + Tp) + i] = v;
}

// conv_start over shift_right(x) (wavenet.py:223-226) -> l in G4, plus the zero left pad of the rows
__global__ __launch_bounds__(256) void tg_start_kernel(const float* __restrict__ xs, const float* __restrict__ wb,
                                                       unsigned* __restrict__ l, int W, long long Tp, long long RS) {
    const int b = blockIdx.z, g = blockIdx.y, NG = W / 8;
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // column incl. left pad
    if (c >= RS) return;
    const long long t = c - IAF_LP;
    wn_u4 hw = (wn_u4){0u, 0u, 0u, 0u}, lw = hw;
    if (t >= 0) {
        const float* xp = xs + (size_t)b * (TG_XP + Tp) + TG_XP + t;
        const float x0 = xp[-3], x1 = xp[-2], x2 = xp[-1];
        const int s = g >> 2, kg = g & 3;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ch = 2 * (16 * s + 8 * (i >> 1) + 2 * kg + (i & 1));
            float o[2];
#pragma unroll
            for (int hh = 0; hh < 2; ++hh)
                o[hh] = wb[3 * W + ch + hh] + wb[ch + hh] * x0 + wb[W + ch + hh] * x1 + wb[2 * W + ch + hh] * x2;
            unsigned a, c2;
            wn_split_pair(o[0], o[1], a, c2);
            hw[i] = a;
            lw[i] = c2;
        }
    }
    unsigned* base = l + (size_t)b * W * RS;
    *reinterpret_cast<wn_u4*>(base + ((size_t)g * RS + c) * 4) = hw;
    *reinterpret_cast<wn_u4*>(base + ((size_t)(NG + g) * RS + c) * 4) = lw;
}

struct TLayout {
    long long T, Tp, TE, RS;
    int c0;
    size_t enc, l, m, s, h1, xs, scratch, total;
};

TLayout t_layout(const wn_handle* h, int B, int F, long long T) {
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

template <int EPI>
void tg_launch(const TgArgs& a, int mtiles, int B, long long Tp, hipStream_t st) {
    if (mtiles % 2 == 0) {
        dim3 g((unsigned)(Tp / TG_TN), mtiles / 2, B);
        hipLaunchKernelGGL((tg_gemm_kernel<EPI, 2>), g, dim3(256), 0, st, a);
    } else {
        dim3 g((unsigned)(Tp / TG_TN), mtiles, B);
        hipLaunchKernelGGL((tg_gemm_kernel<EPI, 1>), g, dim3(256), 0, st, a);
    }
}

}  // namespace

// ---- packing: A fragments of a row-major [M][K] matrix, 64-row tiles, rows picked by rowfn ----
template <class RowFn>
static void pack_tiles(std::vector<float>& blob, size_t dst_off, const float* src, int ld, int K, int mtiles, float scale,
                       RowFn rowfn) {
    const int nks = K / 32;
    unsigned* P = reinterpret_cast<unsigned*>(blob.data() + dst_off);
    for (int mt = 0; mt < mtiles; ++mt)
        for (int ks = 0; ks < nks; ++ks)
            for (int mb = 0; mb < 4; ++mb)
                pack_afrag(P + (((size_t)mt * nks + ks) * 4 + mb) * 512, [&](int e, int kg, int i16) {
                    const int row = rowfn(mt * 64 + 16 * mb + i16);
                    if (row < 0) return 0.f;
                    return scale * src[(size_t)row * ld + 32 * ks + 16 * (e >> 2) + 4 * kg + (e & 3)];
                });
}

int wn_pack_teacher(wn_handle* h, std::vector<float>& blob) {
    const wn_config& c = h->cfg;
    const int W = c.width, S = c.skip_width, G = c.gate_width, H = G / 2, Cd = c.deconv_width, OW = c.out_width;
    TeacherPack& T = h->teacher;
    const ArPack& A = h->ar;
    auto reserve = [&](size_t words) {
        blob.resize(align_up(blob.size(), 64));
        const size_t off = blob.size();
        blob.resize(off + words);
        return off;
    };
    // one GEMM: fragments + tile-ordered bias from the row-major matrices wn_pack_ar already built
    auto gemm = [&](size_t w_off, size_t b_off, int M, int K, int mtiles, auto rowfn) {
        TeacherGemmPack g;
        std::vector<float> src(blob.begin() + w_off, blob.begin() + w_off + (size_t)M * K);
        std::vector<float> bsrc(blob.begin() + b_off, blob.begin() + b_off + M);
        const float sc = pick_scale(src.data(), src.size());
        g.inv_scale = 1.0f / sc;
        g.nks = K / 32;
        g.mtiles = mtiles;
        g.w_off = reserve((size_t)mtiles * g.nks * 4 * 512);
        pack_tiles(blob, g.w_off, src.data(), K, K, mtiles, sc, rowfn);
        g.b_off = reserve((size_t)mtiles * 64);
        for (int i = 0; i < mtiles * 64; ++i) {
            const int row = rowfn(i);
            blob[g.b_off + i] = row < 0 ? 0.f : bsrc[row];
        }
        return g;
    };
    auto ident = [](int M) { return [M](int i) { return i < M ? i : -1; }; };
    T.skip_start = gemm(A.wss_off, A.bss_off, S, W, S / 64, ident(S));
    for (const ArLayerPack& lp : A.layers) {
        TeacherLayerPack tl;
        tl.dilation = lp.dilation;
        // m-tile j: sigmoid rows 32j..32j+31 then their tanh partners H+32j.. (wavenet.py:264-269)
        tl.gate = gemm(lp.wd_off, lp.bd_off, G, 3 * W + Cd, H / 32,
                       [H](int i) { const int j = i / 64, lr = i % 64; return lr < 32 ? 32 * j + lr : H + 32 * j + lr - 32; });
        tl.rs = gemm(lp.wrs_off, lp.brs_off, W + S, H, (W + S) / 64, ident(W + S));
        T.layers.push_back(tl);
    }
    T.out1 = gemm(A.wo1_off, A.bo1_off, S, S + Cd, S / 64, ident(S));
    T.out2 = gemm(A.wo2_off, A.bo2_off, OW, S, (OW + 63) / 64, ident(OW));

    // transposed packs of the input VJP (wn_teacher_backward_input): A = W^T, zero bias, same fragment order and scaling
    static std::atomic<uint64_t> next_serial{1};
    T.serial = next_serial++;
    T.vjp_ok = W % 64 == 0 && S % 64 == 0 && H % 64 == 0 && OW <= 64;
    if (!T.vjp_ok) return WN_OK;
    auto gemm_t = [&](const std::vector<float>& src, int M, int K) {
        TeacherGemmPack g;
        const float sc = pick_scale(src.data(), src.size());
        g.inv_scale = 1.0f / sc;
        g.nks = K / 32;
        g.mtiles = M / 64;
        g.w_off = reserve((size_t)g.mtiles * g.nks * 4 * 512);
        pack_tiles(blob, g.w_off, src.data(), K, K, g.mtiles, sc, ident(M));
        g.b_off = reserve((size_t)g.mtiles * 64);             // zeros
        return g;
    };
    // [nc][Kp] transpose of columns c0 .. c0 + nc - 1 of the R x C row-major matrix at `off` (columns R .. Kp - 1 zero)
    auto transpose = [&](size_t off, int R, int C, int c0, int nc, int Kp) {
        std::vector<float> t((size_t)nc * Kp, 0.f);
        for (int r = 0; r < R; ++r)
            for (int j = 0; j < nc; ++j) t[(size_t)j * Kp + r] = blob[off + (size_t)r * C + c0 + j];
        return t;
    };
    const int OWp = (OW + 31) / 32 * 32;
    T.skip_start_t = gemm_t(transpose(A.wss_off, S, W, 0, W, S), W, S);
    T.out1_t = gemm_t(transpose(A.wo1_off, S, S + Cd, 0, S, S), S, S);
    T.out2_t = gemm_t(transpose(A.wo2_off, OW, S, 0, S, OWp), S, OWp);
    for (size_t i = 0; i < A.layers.size(); ++i) {
        const ArLayerPack& lp = A.layers[i];
        T.layers[i].rs_t = gemm_t(transpose(lp.wrs_off, W + S, H, 0, H, W + S), H, W + S);
        // [width][tap 0 gate | tap 1 gate | tap 2 gate]: dl(t) += sum_k W_dil[k]^T dd(t + (2 - k) dilation)
        std::vector<float> t((size_t)W * 3 * G);
        const int ld = 3 * W + Cd;
        for (int g = 0; g < G; ++g)
            for (int k = 0; k < 3; ++k)
                for (int w = 0; w < W; ++w) t[(size_t)w * 3 * G + k * G + g] = blob[lp.wd_off + (size_t)g * ld + k * W + w];
        T.layers[i].gate_t = gemm_t(t, W, 3 * G);
    }
    // d enc = sum_i W_cond_i^T dd_i + W_cond_out1^T d h1 (wn_teacher_backward_weights): the conditioning columns transposed.
    // Packed after everything above, so no earlier offset moves.
    T.denc_ok = Cd % 64 == 0;
    if (T.denc_ok) {
        for (size_t i = 0; i < A.layers.size(); ++i)
            T.layers[i].cond_t = gemm_t(transpose(A.layers[i].wd_off, G, 3 * W + Cd, 3 * W, Cd, G), Cd, G);
        T.cond_out1_t = gemm_t(transpose(A.wo1_off, S, S + Cd, S, Cd, S), Cd, S);
    }
    return WN_OK;
}

namespace {
// Teacher scoring: log-likelihood per sample of the (encoded) audio under the output parameters of Wavenet.feed_forward --
// the per-sample term of Wavenet.calculate_loss (wavenet/wavenet.py:293-316): loss_func.mol_log_probs (loss_func.py:22-63),
// gauss_log_prob (:66-75,104-119) and the cross entropy of ce_loss (:128-133), on the targets Wavenet.encode_signal derives
// from the raw audio (wavenet.py:157-178).  One wave per sample; lane i owns mixture i / strides over the classes.
// The discretised-logistic mass cdf(x + 1/Q) - cdf(x - 1/Q) is evaluated as sigma(a) sigma(-b) (1 - exp(-(a - b))) with
// a - b = 2 inv_s / Q formed directly: the difference of two float32 sigmoids the reference's formula takes loses all but
// two digits of it at Q = 65 536 (the float64 evaluation of the reference's formula is what the tests compare with).
// The per-component arithmetic is wn_mol.h's, shared with the distillation cross entropy (wn_distill.hip).
__device__ inline float tl_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ inline float tl_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__global__ __launch_bounds__(256) void tg_log_prob_kernel(const float* __restrict__ out, const float* __restrict__ wav,
                                                          float* __restrict__ lp, long long n, int ow, int loss, int Q, int mu) {
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (i >= n) return;
    const float* o = out + (size_t)i * ow;
    const float x = wav[i];
    const float xt = mu ? wn_mu_law_scaled(x) : x;                 // real_targets (wavenet.py:165-174)
    const float NEG = -__builtin_inff();
    float res;
    if (loss == WN_LOSS_MOL) {
        const int M = ow / 3;
        float v = NEG, lg = NEG;
        if (lane < M) {
            lg = o[lane];
            const float mean = o[M + lane], ls = fmaxf(o[2 * M + lane], -7.0f);
            const float inv = expf(-ls), c = xt - mean, iq = 1.0f / (float)Q;
            float min_thres, max_thres;
            wn_mol_thresholds(Q, min_thres, max_thres);
            v = wn_mol_component_lp(xt, c, inv, iq, wn_mol_bin_factor(inv, iq), min_thres, max_thres);
        }
        const float lmax = tl_wave_max(lg);
        const float lse = lmax + logf(tl_wave_sum(lane < M ? expf(lg - lmax) : 0.f));
        v = lane < M ? v + (lg - lse) : NEG;
        const float vmax = tl_wave_max(v);
        res = vmax + logf(tl_wave_sum(lane < M ? expf(v - vmax) : 0.f));
    } else if (loss == WN_LOSS_GAUSS) {
        const float ls = fmaxf(o[1], -7.0f), z = (xt - o[0]) * expf(-ls);
        res = -0.5f * z * z - ls - 0.9189385332046727f;             // Normal(mean, exp(ls)).log_prob(x)
    } else {
        // cate_targets (wavenet.py:166-176): the quantised audio shifted to [0, Q)
        int label = (mu ? (int)floorf(wn_mu_law_scaled(x) * 128.0f) : (int)floorf(x * (float)Q * 0.5f)) + Q / 2;
        label = min(max(label, 0), Q - 1);
        float m = NEG;
        for (int k = lane; k < ow; k += 64) m = fmaxf(m, o[k]);
        m = tl_wave_max(m);
        float sum = 0.f;
        for (int k = lane; k < ow; k += 64) sum += expf(o[k] - m);
        res = o[label] - (m + logf(tl_wave_sum(sum)));
    }
    if (lane == 0) lp[i] = res;
}

// Gradient of tg_log_prob_kernel: g = d_log_prob[i] -> d out_params[i, :] and d wav[i], in the forward's
// layout (one wave per sample; lane i owns mixture i / the lanes stride over the classes) on the forward's xt, Q,
// thresholds and bin factor, so it differentiates the function the forward evaluates.  Tie conventions as in wnhip.h:
// max(log_s, -7) passes the gradient at the tie, the 1e-12 floor passes none below it, the edge bins differentiate the
// selected branch only.  Every output element is written by exactly one lane: no atomics.
template <int W>
__device__ inline void tl_load(const float* __restrict__ p, float (&v)[W]) {
    if constexpr (W == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = *p;
    }
}
template <int W>
__device__ inline void tl_store(float* __restrict__ p, const float (&v)[W]) {
    if constexpr (W == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        *p = v[0];
    }
}
// d logit_k = g (onehot_k - softmax_k) of one row, W consecutive classes per lane and step (ow % W == 0).  A row of 64 W
// classes (256 at W = 4) stays in registers and is read once; a longer one is reduced with a running max / sum per lane
// and read a second time for the softmax: two reads and one write of the row.
template <int W>
__device__ inline void tl_ce_grad_row(const float* __restrict__ o, float* __restrict__ d, int ow, int label, float g, int lane) {
    float v[W], m = -__builtin_inff(), s = 0.f;
#pragma unroll 4
    for (int k = lane * W; k < ow; k += 64 * W) {
        tl_load<W>(o + k, v);
        float mn = m, a = 0.f;
#pragma unroll
        for (int j = 0; j < W; ++j) mn = fmaxf(mn, v[j]);
#pragma unroll
        for (int j = 0; j < W; ++j) a += expf(v[j] - mn);
        s = s * expf(m - mn) + a;
        m = mn;
    }
    const float mx = tl_wave_max(m);
    const float rinv = 1.0f / tl_wave_sum(s * expf(m - mx));     // a lane without classes holds s = 0
    const bool once = ow <= 64 * W;                              // v still holds the lane's only classes
#pragma unroll 4
    for (int k = lane * W; k < ow; k += 64 * W) {
        if (!once) tl_load<W>(o + k, v);
#pragma unroll
        for (int j = 0; j < W; ++j) v[j] = g * ((k + j == label ? 1.0f : 0.0f) - expf(v[j] - mx) * rinv);
        tl_store<W>(d + k, v);
    }
}
__global__ __launch_bounds__(256) void tg_log_prob_grad_kernel(const float* __restrict__ out, const float* __restrict__ wav,
                                                               const float* __restrict__ dlp, float* __restrict__ dout,
                                                               float* __restrict__ dwav, long long n, int ow, int loss, int Q,
                                                               int mu, int vec) {
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (i >= n) return;
    const float* o = out + (size_t)i * ow;
    float* d = dout + (size_t)i * ow;
    const float x = wav[i], g = dlp[i];
    const float xt = mu ? wn_mu_law_scaled(x) : x;
    const float NEG = -__builtin_inff();
    float dx_tot = 0.f;                                            // d log_prob / d xt
    if (loss == WN_LOSS_MOL) {
        const int M = ow / 3;
        float v = NEG, lg = NEG, raw = 0.f, inv = 0.f, dx = 0.f, dinv = 0.f;
        if (lane < M) {
            lg = o[lane];
            raw = o[2 * M + lane];
            const float mean = o[M + lane], ls = fmaxf(raw, -7.0f);
            inv = expf(-ls);
            const float c = xt - mean, iq = 1.0f / (float)Q, bf = wn_mol_bin_factor(inv, iq);
            float min_thres, max_thres;
            wn_mol_thresholds(Q, min_thres, max_thres);
            v = wn_mol_component_lp(xt, c, inv, iq, bf, min_thres, max_thres);
            wn_mol_component_grad(xt, c, inv, iq, bf, min_thres, max_thres, dx, dinv);
        }
        const float lmax = tl_wave_max(lg);
        const float lse = lmax + logf(tl_wave_sum(lane < M ? expf(lg - lmax) : 0.f));
        v = lane < M ? v + (lg - lse) : NEG;
        const float vmax = tl_wave_max(v);
        const float res = vmax + logf(tl_wave_sum(lane < M ? expf(v - vmax) : 0.f));
        const float r = lane < M ? expf(v - res) : 0.f;           // responsibility of the component
        dx_tot = tl_wave_sum(r * dx);
        if (lane < M) {
            d[lane] = g * (r - expf(lg - lse));
            d[M + lane] = -g * r * dx;
            d[2 * M + lane] = raw >= -7.0f ? -g * r * dinv * inv : 0.f;
        }
    } else if (loss == WN_LOSS_GAUSS) {
        const float raw = o[1], einv = expf(-fmaxf(raw, -7.0f)), z = (xt - o[0]) * einv;
        dx_tot = -z * einv;
        if (lane == 0) {
            d[0] = g * z * einv;
            d[1] = raw >= -7.0f ? g * (z * z - 1.0f) : 0.f;
        }
    } else {
        int label = (mu ? (int)floorf(wn_mu_law_scaled(x) * 128.0f) : (int)floorf(x * (float)Q * 0.5f)) + Q / 2;
        label = min(max(label, 0), Q - 1);
        if (vec) tl_ce_grad_row<4>(o, d, ow, label, g, lane);
        else tl_ce_grad_row<1>(o, d, ow, label, g, lane);
    }
    // a mu-law or class target is piecewise constant in the audio (encode_signal quantises first): zero
    if (dwav && lane == 0) dwav[i] = (mu || loss == WN_LOSS_CE) ? 0.f : g * dx_tot;
}
}  // namespace

size_t wn_teacher_ws_bytes(const wn_handle* h, int B, int F, long long T) { return t_layout(h, B, F, T).total; }

extern "C" size_t wn_teacher_workspace_bytes(const wn_handle* h, int B, int F, int64_t T) {
    if (!h || !h->finalized || h->cfg.kind != WN_KIND_TEACHER || B < 1 || F < 1 || T < 1) return 0;
    return wn_teacher_ws_bytes(h, B, F, T);
}

// checks of the forward calls (message prefix fn)
static int tg_forward_check(wn_handle* h, const char* fn, const float* wav, const float* mel, int B, int F, int64_t T,
                            const float* out_params, const void* ws) {
    if (!h) return wn_fail(nullptr, WN_EINVAL, "%s: null handle", fn);
    if (!h->finalized) return wn_fail(h, WN_ESTATE, "%s: call wn_finalize first", fn);
    const wn_config& c = h->cfg;
    if (c.kind != WN_KIND_TEACHER) return wn_fail(h, WN_EINVAL, "%s: handle is not a Wavenet teacher", fn);
    if (B < 1 || F < 1 || T < 1 || !wav || !mel || !out_params || !ws)
        return wn_fail(h, WN_EINVAL, "%s: bad argument", fn);
    const long long TE = (long long)F * h->frame_shift, md = 1ll << (c.num_stages - 1);
    if (T > TE) return wn_fail(h, WN_EINVAL, "%s: %lld samples need more than %d mel frames "
                               "(wavenet.py:79 assert cond_len >= x_len)", fn, (long long)T, F);
    if (T % md) return wn_fail(h, WN_EINVAL, "%s: length %lld is not a multiple of the largest "
                               "dilation %lld (masked.py:188)", fn, (long long)T, md);
    if (TE > 2000000) return wn_fail(h, WN_EINVAL, "%s: utterance too long (32-bit row offsets)", fn);
    return WN_OK;
}

// the forward; with tape_s != nullptr the skip sum and out1 rows land in the tape and every gate stores its activations
// to tape_g (layer i at i * B * gate * Tp floats) -- the same arithmetic, so out_params are the same bits either way.
// With tape_l (training tape) the conditioning and the scaled input row are written to the tape instead of the
// workspace and layer i reads its input l_i from slot i of tape_l: l_i is copied to the next slot (the workspace row for the
// last layer) before the residual GEMM updates that copy in place -- the same kernels on the same values.
static int tg_forward(wn_handle* h, const char* fn, const float* wav, const float* mel, int B, int F, int64_t T,
                      float* out_params, void* ws, size_t ws_bytes, float* tape_s, float* tape_h1, float* tape_g,
                      void* stream, unsigned* tape_l = nullptr, float* tape_enc = nullptr, float* tape_xs = nullptr) {
    const wn_config& c = h->cfg;
    const TLayout L = t_layout(h, B, F, T);
    if (ws_bytes < L.total)
        return wn_fail(h, WN_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, L.total);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* base = reinterpret_cast<char*>(ws);
    float* enc = tape_enc ? tape_enc : reinterpret_cast<float*>(base + L.enc);
    unsigned* lws = reinterpret_cast<unsigned*>(base + L.l);
    unsigned* l = tape_l ? tape_l : lws;
    unsigned* m = reinterpret_cast<unsigned*>(base + L.m);
    float* s = tape_s ? tape_s : reinterpret_cast<float*>(base + L.s);
    float* h1 = tape_h1 ? tape_h1 : reinterpret_cast<float*>(base + L.h1);
    float* xs = tape_xs ? tape_xs : reinterpret_cast<float*>(base + L.xs);
    const int W = c.width, S = c.skip_width, H = c.gate_width / 2, Cd = c.deconv_width;
    const TeacherPack& P = h->teacher;

    // conditioning (wavenet.py:214-216), G4 rows of TE columns
    int rc = wn_run_deconv(h, 0, mel, B, F, enc, L.TE, base + L.scratch, st, true);
    if (rc) return rc;
    // l0 = conv_start(shift_right(x_scaled))  (wavenet.py:223-226)
    {
        dim3 g((unsigned)((TG_XP + L.Tp + 255) / 256), B);
        hipLaunchKernelGGL(tg_input_kernel, g, dim3(256), 0, st, wav, xs, (long long)T, L.Tp, c.use_mu_law);
        dim3 g2((unsigned)((L.RS + 255) / 256), W / 8, B);
        hipLaunchKernelGGL(tg_start_kernel, g2, dim3(256), 0, st, xs, h->d_blob + h->ar.start_off, l, W, L.Tp, L.RS);
    }
    auto seg_g4 = [](const unsigned* p, long long bstride, long long rowlen, int col0, int nks, int ng) {
        TgSeg sg;
        sg.base = p; sg.bstride = bstride; sg.rowlen = (int)rowlen; sg.col0 = col0; sg.nks = nks; sg.ng = ng;
        sg.kind = TG_SRC_G4;
        return sg;
    };
    auto seg_acc = [&](const float* p, int nks) {
        TgSeg sg;
        sg.base = reinterpret_cast<const unsigned*>(p); sg.bstride = (long long)S * L.Tp; sg.rowlen = S / 16;
        sg.col0 = 0; sg.nks = nks; sg.ng = 0; sg.kind = TG_SRC_ACC_RELU;
        return sg;
    };
    auto base_args = [&](const TeacherGemmPack& g) {
        TgArgs a{};
        a.wp = reinterpret_cast<const unsigned*>(h->d_blob + g.w_off);
        a.bias = h->d_blob + g.b_off;
        a.inv_scale = g.inv_scale;
        a.nks = g.nks;
        a.T = T;
        return a;
    };
    TgSeg seg_l = seg_g4(l, (long long)W * L.RS, L.RS, IAF_LP, W / 32, W / 8);
    const size_t l_words = (size_t)B * W * L.RS;
    const TgSeg seg_enc = seg_g4(reinterpret_cast<const unsigned*>(enc), (long long)Cd * L.TE, L.TE, L.c0, Cd / 32, Cd / 8);
    const TgSeg seg_m = seg_g4(m, (long long)H * L.Tp, L.Tp, 0, H / 32, H / 8);
    // s = skip_start(l)  (wavenet.py:231-233)
    {
        TgArgs a = base_args(P.skip_start);
        a.seg[0] = seg_l; a.nseg = 1;
        a.oacc = s; a.oacc_bstride = (long long)S * L.Tp; a.oacc_nmb = S / 16;
        tg_launch<TG_EPI_ACC>(a, P.skip_start.mtiles, B, L.Tp, st);
    }
    for (size_t li = 0; li < P.layers.size(); ++li) {
        const TeacherLayerPack& tl = P.layers[li];
        if (tape_l) {
            seg_l.base = l;
            unsigned* next = li + 1 < P.layers.size() ? l + l_words : lws;
            WN_HIP(h, hipMemcpyAsync(next, l, l_words * 4, hipMemcpyDeviceToDevice, st));
            l = next;                     // the gate below reads seg_l (slot li); the residual GEMM updates the copy
        }
        {   // d = dilated_conv(l) + mel_cond(enc); m = sigmoid(d[:H]) * tanh(d[H:])  (wavenet.py:243-269)
            TgArgs a = base_args(tl.gate);
            for (int tap = 0; tap < 3; ++tap) {
                a.seg[tap] = seg_l;
                a.seg[tap].col0 = IAF_LP - (2 - tap) * tl.dilation;
            }
            a.seg[3] = seg_enc; a.nseg = 4;
            a.og4 = m; a.og4_bstride = (long long)H * L.Tp; a.og4_rowlen = (int)L.Tp; a.og4_col0 = 0; a.og4_ng = H / 8;
            if (tape_g) {
                a.tape = tape_g + li * (size_t)B * 2 * H * L.Tp;
                a.tape_bstride = 2ll * H * L.Tp; a.tape_nmb = 2 * H / 16; a.tape_hoff = H / 16;
                tg_launch<TG_EPI_GATE_TAPE>(a, tl.gate.mtiles, B, L.Tp, st);
            } else {
                tg_launch<TG_EPI_GATE>(a, tl.gate.mtiles, B, L.Tp, st);
            }
        }
        {   // l += res(m); s += skip(m)  (wavenet.py:271-277)
            TgArgs a = base_args(tl.rs);
            a.seg[0] = seg_m; a.nseg = 1;
            a.og4 = l; a.og4_bstride = (long long)W * L.RS; a.og4_rowlen = (int)L.RS; a.og4_col0 = IAF_LP; a.og4_ng = W / 8;
            a.oacc = s; a.oacc_bstride = (long long)S * L.Tp; a.oacc_nmb = S / 16;
            a.res_mtiles = W / 64;
            tg_launch<TG_EPI_RS>(a, tl.rs.mtiles, B, L.Tp, st);
        }
    }
    {   // out1(relu(s)) + mel_cond_out1(enc)  (wavenet.py:283-289)
        TgArgs a = base_args(P.out1);
        a.seg[0] = seg_acc(s, S / 32); a.seg[1] = seg_enc; a.nseg = 2;
        a.oacc = h1; a.oacc_bstride = (long long)S * L.Tp; a.oacc_nmb = S / 16;
        tg_launch<TG_EPI_ACC>(a, P.out1.mtiles, B, L.Tp, st);
    }
    {   // out2(relu(.))  (wavenet.py:290-292)
        TgArgs a = base_args(P.out2);
        a.seg[0] = seg_acc(h1, S / 32); a.nseg = 1;
        a.otm = out_params; a.ow = c.out_width;
        tg_launch<TG_EPI_OUT>(a, P.out2.mtiles, B, L.Tp, st);
    }
    WN_HIP(h, hipGetLastError());
    return WN_OK;
}

extern "C" int wn_teacher_forward(wn_handle* h, const float* wav, const float* mel, int B, int F, int64_t T,
                                  float* out_params, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "wn_teacher_forward";
    if (int rc = tg_forward_check(h, fn, wav, mel, B, F, T, out_params, ws)) return rc;
    const WnWork work(h);
    return tg_forward(h, fn, wav, mel, B, F, T, out_params, ws, ws_bytes, nullptr, nullptr, nullptr, stream);
}

extern "C" int wn_teacher_log_prob(wn_handle* h, const float* out_params, const float* wav, int B, int64_t T, float* log_prob,
                                   void* stream) {
    if (!h) return wn_fail(nullptr, WN_EINVAL, "wn_teacher_log_prob: null handle");
    const wn_config& c = h->cfg;
    if (c.kind != WN_KIND_TEACHER) return wn_fail(h, WN_EINVAL, "wn_teacher_log_prob: handle is not a Wavenet teacher");
    if (B < 1 || T < 1 || !out_params || !wav || !log_prob) return wn_fail(h, WN_EINVAL, "wn_teacher_log_prob: bad argument");
    const int Q = c.use_mu_law ? 256 : 65536;
    if (c.loss_type == WN_LOSS_CE && c.out_width != Q)
        return wn_fail(h, WN_EINVAL, "wn_teacher_log_prob: %d logits for %d classes", c.out_width, Q);
    const long long n = (long long)B * T;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(tg_log_prob_kernel, dim3((unsigned)((n * 64 + 255) / 256)), dim3(256), 0, st, out_params, wav, log_prob,
                       n, c.out_width, c.loss_type, Q, c.use_mu_law);
    WN_HIP(h, hipGetLastError());
    return WN_OK;
}

extern "C" int wn_teacher_log_prob_grad(wn_handle* h, const float* out_params, const float* wav, int B, int64_t T,
                                        const float* d_log_prob, float* d_out_params, float* d_wav, void* stream) {
    const char* fn = "wn_teacher_log_prob_grad";
    if (!h) return wn_fail(nullptr, WN_EINVAL, "%s: null handle", fn);
    const wn_config& c = h->cfg;
    if (c.kind != WN_KIND_TEACHER) return wn_fail(h, WN_EINVAL, "%s: handle is not a Wavenet teacher", fn);
    if (B < 1 || T < 1 || !out_params || !wav || !d_log_prob || !d_out_params) return wn_fail(h, WN_EINVAL, "%s: bad argument", fn);
    const int Q = c.use_mu_law ? 256 : 65536;
    if (c.loss_type == WN_LOSS_CE && c.out_width != Q)
        return wn_fail(h, WN_EINVAL, "%s: %d logits for %d classes", fn, c.out_width, Q);
    const WnWork work(h);
    const long long n = (long long)B * T;
    // four classes per lane and load when the rows are 16-byte aligned (any torch tensor); one otherwise
    const int vec = c.out_width % 4 == 0 &&
                    ((reinterpret_cast<uintptr_t>(out_params) | reinterpret_cast<uintptr_t>(d_out_params)) & 15) == 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(tg_log_prob_grad_kernel, dim3((unsigned)((n * 64 + 255) / 256)), dim3(256), 0, st, out_params, wav,
                       d_log_prob, d_out_params, d_wav, n, c.out_width, c.loss_type, Q, c.use_mu_law, vec);
    WN_HIP(h, hipGetLastError());
    return WN_OK;
}

// ---- input VJP of the teacher: d out_params [B,T,ow] -> d wav [B,T], weights frozen ----
// The tape (wn_teacher_forward_tape) holds what the reverse pass reads: a header, the pre-ReLU skip sum s and out1 rows
// (accumulator layout, as the forward keeps them), and sigma / tanh of every gate.  The reverse pass runs the forward's
// GEMM kernel on the transposed packs: d out2 and d out1 through the ReLU masks (MASK), then per layer from the last one
// dm = W_res^T dl + W_skip^T ds with the gate derivative in the epilogue (BGATE) and dl += sum_k W_dil[k]^T dd(t + (2-k) d)
// in place (RS, anti-causal taps: dd rows carry a zero right pad of 2 * max dilation), then skip_start^T and the start
// conv transposed.  The operands are split-fp16 like the forward's, so d out_params enter scaled by a power of two that
// brings their largest magnitude to [1, 2) (found on the device) and d wav leaves unscaled: the VJP is linear.
namespace {
constexpr uint32_t TB_MAGIC = 0x31505457u;      // "WTP1"
constexpr uint32_t TB_MAGIC_TRAIN = 0x32505457u;   // "WTP2": a training tape (wn_teacher_forward_train_tape)
constexpr size_t TB_HEAD = 256;
constexpr int TB_NMAX = 1024;                   // workgroups of the max-magnitude pass

struct TapeRec {
    uint64_t serial;
    int B;
    long long T;
    int F;              // > 0: a training tape (wn_teacher_forward_train_tape) for F mel frames
};
std::mutex g_tape_mu;
std::unordered_map<const void*, TapeRec> g_tapes;   // tape address -> the handle and shape that last wrote it

struct TapeLayout {
    long long Tp;
    size_t s, h1, g, total;
};
TapeLayout tape_layout(const wn_handle* h, int B, long long T) {
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

struct BLayout {
    long long Tp, RD;
    int Kp;
    size_t scal, dout, dh1, ds, dl, dd, total;
};
BLayout b_layout(const wn_handle* h, int B, long long T) {
    const wn_config& c = h->cfg;
    BLayout L;
    L.Tp = (T + TG_TN - 1) / TG_TN * TG_TN;
    L.RD = L.Tp + 2 * (1ll << (c.num_stages - 1));
    L.Kp = h->teacher.out2_t.nks * 32;
    size_t o = 0;
    auto carve = [&](size_t words) { size_t r = o; o += align_up(words * 4, 256); return r; };
    L.scal = carve(4 + TB_NMAX);
    L.dout = carve((size_t)B * L.Kp * L.Tp);
    L.dh1 = carve((size_t)B * c.skip_width * L.Tp);
    L.ds = carve((size_t)B * c.skip_width * L.Tp);
    L.dl = carve((size_t)B * c.width * L.Tp);
    L.dd = carve((size_t)B * c.gate_width * L.RD);
    L.total = o;
    return L;
}

struct TbHead {
    unsigned w[8];
};
__global__ void tb_header_kernel(TbHead v, unsigned* __restrict__ dst) {
    if (threadIdx.x < 8) dst[threadIdx.x] = v.w[threadIdx.x];
}

__device__ inline float tb_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
// largest |x| per workgroup, then one workgroup: scal[0] = 2^k with max |x| 2^k in [1, 2), scal[1] = 2^-k
__global__ __launch_bounds__(256) void tb_absmax_kernel(const float* __restrict__ x, long long n, float* __restrict__ part) {
    __shared__ float sh[4];
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) m = fmaxf(m, fabsf(x[i]));
    m = tb_wave_max(m);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}
__global__ __launch_bounds__(256) void tb_scale_kernel(const float* __restrict__ part, int np, float* __restrict__ scal) {
    __shared__ float sh[4];
    float m = 0.f;
    for (int i = threadIdx.x; i < np; i += 256) m = fmaxf(m, part[i]);
    m = tb_wave_max(m);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
        int k = 0;
        if (m > 0.f && m < __builtin_inff()) k = min(max(-ilogbf(m), -100), 100);
        scal[0] = ldexpf(1.f, k);
        scal[1] = ldexpf(1.f, -k);
    }
}

// d out_params [B,T,ow] (scaled by scal[0]) -> G4 rows of Kp channels (zero beyond ow and from column T on)
__global__ __launch_bounds__(256) void tb_dout_kernel(const float* __restrict__ dout, const float* __restrict__ scal,
                                                      unsigned* __restrict__ g4, long long T, long long Tp, int ow, int Kp) {
    const int b = blockIdx.z, gr = blockIdx.y, NG = Kp / 8;
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= Tp) return;
    const float sc = scal[0];
    const int s4 = gr >> 2, kg = gr & 3;
    wn_u4 hw, lw;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float o[2];
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const int ch = 32 * s4 + 16 * (i >> 1) + 4 * kg + 2 * (i & 1) + hh;
            o[hh] = c < T && ch < ow ? dout[((size_t)b * T + c) * ow + ch] * sc : 0.f;
        }
        unsigned a, a2;
        wn_split_pair(o[0], o[1], a, a2);
        hw[i] = a;
        lw[i] = a2;
    }
    unsigned* base = g4 + (size_t)b * Kp * Tp;
    *reinterpret_cast<wn_u4*>(base + ((size_t)gr * Tp + c) * 4) = hw;
    *reinterpret_cast<wn_u4*>(base + ((size_t)(NG + gr) * Tp + c) * 4) = lw;
}

// conv_start transposed (tg_start_kernel: l0(t) = b + w0 x(t-3) + w1 x(t-2) + w2 x(t-1)):
// d wav(t) = scal[1] sum_c (w0[c] dl0[c](t+3) + w1[c] dl0[c](t+2) + w2[c] dl0[c](t+1)); 64 columns x 4 waves of channels
__global__ __launch_bounds__(256) void tb_dx_kernel(const unsigned* __restrict__ dl, const float* __restrict__ wb,
                                                    const float* __restrict__ scal, float* __restrict__ dwav, int W,
                                                    long long T, long long Tp) {
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y, NG = W / 8;
    const long long t = (long long)blockIdx.x * 64 + lane;
    float acc = 0.f;
    if (t < T) {
        const unsigned* base = dl + (size_t)b * W * Tp;
        for (int gr = wave; gr < NG; gr += 4) {
            const int s4 = gr >> 2, kg = gr & 3;
            for (int k = 0; k < 3; ++k) {
                const long long col = t + 3 - k;
                if (col >= T) continue;
                const wn_u4 hw = *reinterpret_cast<const wn_u4*>(base + ((size_t)gr * Tp + col) * 4);
                const wn_u4 lw = *reinterpret_cast<const wn_u4*>(base + ((size_t)(NG + gr) * Tp + col) * 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float v0, v1;
                    wn_join_pair(hw[i], lw[i], v0, v1);
                    const int ch = 32 * s4 + 16 * (i >> 1) + 4 * kg + 2 * (i & 1);
                    acc = fmaf(wb[k * W + ch], v0, acc);
                    acc = fmaf(wb[k * W + ch + 1], v1, acc);
                }
            }
        }
    }
    red[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && t < T) dwav[(size_t)b * T + t] = (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]) * scal[1];
}

// what the two VJP-side calls refuse (the distillation losses' own refusals, wn_distill.hip)
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
}  // namespace

extern "C" size_t wn_teacher_tape_bytes(const wn_handle* h, int B, int64_t T) {
    if (!h || !h->finalized || h->cfg.kind != WN_KIND_TEACHER || B < 1 || T < 1) return 0;
    return tape_layout(h, B, T).total;
}

extern "C" size_t wn_teacher_backward_workspace_bytes(const wn_handle* h, int B, int64_t T) {
    if (!h || !h->finalized || h->cfg.kind != WN_KIND_TEACHER || !h->teacher.vjp_ok || B < 1 || T < 1) return 0;
    return b_layout(h, B, T).total;
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
    char* tb = reinterpret_cast<char*>(tape);
    TbHead hd;
    const uint64_t ser = h->teacher.serial;
    hd.w[0] = TB_MAGIC; hd.w[1] = (unsigned)ser; hd.w[2] = (unsigned)(ser >> 32); hd.w[3] = (unsigned)B;
    hd.w[4] = (unsigned)T; hd.w[5] = (unsigned)((uint64_t)T >> 32); hd.w[6] = (unsigned)h->teacher.layers.size();
    hd.w[7] = (unsigned)F;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(tb_header_kernel, dim3(1), dim3(64), 0, st, hd, reinterpret_cast<unsigned*>(tb));
    const int rc = tg_forward(h, fn, wav, mel, B, F, T, out_params, ws, ws_bytes, reinterpret_cast<float*>(tb + TL.s),
                              reinterpret_cast<float*>(tb + TL.h1), reinterpret_cast<float*>(tb + TL.g), stream);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g_tape_mu);
    g_tapes[tape] = TapeRec{ser, B, (long long)T, 0};
    return WN_OK;
}

// registry check shared by the reverse-pass calls; *F receives the frame count of a training tape (0: a plain tape)
static int tb_tape_check(wn_handle* h, const char* fn, const void* tape, size_t tape_bytes, int B, int64_t T, int* F) {
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
    return WN_OK;
}

namespace {
struct TwCtx;                                   // weight-gradient side of the reverse pass (below)
int tw_aux(wn_handle* h, const TwCtx& w, hipStream_t st);
int tw_head(wn_handle* h, const TwCtx& w, hipStream_t st, int stage);
int tw_layer(wn_handle* h, const TwCtx& w, size_t li, hipStream_t st);
int tw_tail(wn_handle* h, const TwCtx& w, hipStream_t st);
}  // namespace

// The reverse pass.  wg == nullptr: the input VJP alone, launch for launch what wn_teacher_backward_input always ran.
// With wg the weight-gradient products, the d enc GEMMs and their reductions are issued between those launches, where
// the cotangents they read are complete; they write nothing the input VJP reads, so d_wav is the same bits.
static int tb_reverse(wn_handle* h, const void* tape, const float* d_out_params, int B, int64_t T, float* d_wav, void* ws,
                      void* stream, const TwCtx* wg) {
    const TapeLayout TL = tape_layout(h, B, T);
    const BLayout L = b_layout(h, B, T);
    const wn_config& c = h->cfg;
    const int W = c.width, S = c.skip_width, G = c.gate_width, H = G / 2;
    const TeacherPack& P = h->teacher;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* base = reinterpret_cast<char*>(ws);
    float* scal = reinterpret_cast<float*>(base + L.scal);
    unsigned* dout = reinterpret_cast<unsigned*>(base + L.dout);
    unsigned* dh1 = reinterpret_cast<unsigned*>(base + L.dh1);
    unsigned* ds = reinterpret_cast<unsigned*>(base + L.ds);
    unsigned* dl = reinterpret_cast<unsigned*>(base + L.dl);
    unsigned* dd = reinterpret_cast<unsigned*>(base + L.dd);
    const char* tb = reinterpret_cast<const char*>(tape);
    float* tape_s = const_cast<float*>(reinterpret_cast<const float*>(tb + TL.s));
    float* tape_h1 = const_cast<float*>(reinterpret_cast<const float*>(tb + TL.h1));
    float* tape_g = const_cast<float*>(reinterpret_cast<const float*>(tb + TL.g));
    const long long Tp = L.Tp;

    // operand scale
    const long long n = (long long)B * T * c.out_width;
    const int nb = (int)std::min<long long>(TB_NMAX, (n + 255) / 256);
    hipLaunchKernelGGL(tb_absmax_kernel, dim3(nb), dim3(256), 0, st, d_out_params, n, scal + 4);
    hipLaunchKernelGGL(tb_scale_kernel, dim3(1), dim3(256), 0, st, scal + 4, nb, scal);
    hipLaunchKernelGGL(tb_dout_kernel, dim3((unsigned)((Tp + 255) / 256), L.Kp / 8, B), dim3(256), 0, st, d_out_params, scal,
                       dout, (long long)T, Tp, c.out_width, L.Kp);
    WN_HIP(h, hipMemsetAsync(dl, 0, (size_t)B * W * Tp * 4, st));
    WN_HIP(h, hipMemsetAsync(dd, 0, (size_t)B * G * L.RD * 4, st));

    auto seg = [](const unsigned* p, long long bstride, long long rowlen, long long col0, int C) {
        TgSeg sg;
        sg.base = p; sg.bstride = bstride; sg.rowlen = (int)rowlen; sg.col0 = (int)col0; sg.nks = C / 32; sg.ng = C / 8;
        sg.kind = TG_SRC_G4;
        return sg;
    };
    auto args = [&](const TeacherGemmPack& g, unsigned* og4, long long obstride, long long orowlen, int C) {
        TgArgs a{};
        a.wp = reinterpret_cast<const unsigned*>(h->d_blob + g.w_off);
        a.bias = h->d_blob + g.b_off;
        a.inv_scale = g.inv_scale;
        a.nks = g.nks;
        a.T = T;
        a.og4 = og4; a.og4_bstride = obstride; a.og4_rowlen = (int)orowlen; a.og4_col0 = 0; a.og4_ng = C / 8;
        return a;
    };
    const TgSeg seg_ds = seg(ds, (long long)S * Tp, Tp, 0, S), seg_dl = seg(dl, (long long)W * Tp, Tp, 0, W);
    {   // d relu(h1) = W_out2^T d out, masked by h1 > 0  (wavenet.py:290-292)
        TgArgs a = args(P.out2_t, dh1, (long long)S * Tp, Tp, S);
        a.seg[0] = seg(dout, (long long)L.Kp * Tp, Tp, 0, L.Kp); a.nseg = 1;
        a.tape = tape_h1; a.tape_bstride = (long long)S * Tp; a.tape_nmb = S / 16;
        tg_launch<TG_EPI_MASK>(a, P.out2_t.mtiles, B, Tp, st);
    }
    if (wg) {
        if (int rc = tw_aux(h, *wg, st)) return rc;
        if (int rc = tw_head(h, *wg, st, 0)) return rc;
    }
    {   // ds = W_out1^T d h1 (its skip columns), masked by s > 0  (wavenet.py:283-289)
        TgArgs a = args(P.out1_t, ds, (long long)S * Tp, Tp, S);
        a.seg[0] = seg(dh1, (long long)S * Tp, Tp, 0, S); a.nseg = 1;
        a.tape = tape_s; a.tape_bstride = (long long)S * Tp; a.tape_nmb = S / 16;
        tg_launch<TG_EPI_MASK>(a, P.out1_t.mtiles, B, Tp, st);
    }
    if (wg)
        if (int rc = tw_head(h, *wg, st, 1)) return rc;
    for (size_t li = P.layers.size(); li-- > 0;) {
        const TeacherLayerPack& tl = P.layers[li];
        {   // dm = W_res^T dl + W_skip^T ds -> dd through the gate derivative  (wavenet.py:264-277 transposed)
            TgArgs a = args(tl.rs_t, dd, (long long)G * L.RD, L.RD, G);
            a.seg[0] = seg_dl; a.seg[1] = seg_ds; a.nseg = 2;
            a.tape = tape_g + li * (size_t)B * G * Tp; a.tape_bstride = (long long)G * Tp; a.tape_nmb = G / 16;
            a.tape_hoff = H / 16;
            tg_launch<TG_EPI_BGATE>(a, tl.rs_t.mtiles, B, Tp, st);
        }
        if (wg)     // dl = d l_{li+1} and dd_li are complete here, before the dilated step overwrites dl
            if (int rc = tw_layer(h, *wg, li, st)) return rc;
        {   // dl += sum_k W_dil[k]^T dd(t + (2 - k) dilation)  (wavenet.py:243-262 transposed)
            TgArgs a = args(tl.gate_t, dl, (long long)W * Tp, Tp, W);
            for (int k = 0; k < 3; ++k) a.seg[k] = seg(dd, (long long)G * L.RD, L.RD, (long long)(2 - k) * tl.dilation, G);
            a.nseg = 3;
            a.res_mtiles = W / 64;
            tg_launch<TG_EPI_RS>(a, tl.gate_t.mtiles, B, Tp, st);
        }
    }
    {   // dl0 += W_skip_start^T ds  (wavenet.py:231-233)
        TgArgs a = args(P.skip_start_t, dl, (long long)W * Tp, Tp, W);
        a.seg[0] = seg_ds; a.nseg = 1;
        a.res_mtiles = W / 64;
        tg_launch<TG_EPI_RS>(a, P.skip_start_t.mtiles, B, Tp, st);
    }
    if (wg)
        if (int rc = tw_tail(h, *wg, st)) return rc;
    if (d_wav)
        hipLaunchKernelGGL(tb_dx_kernel, dim3((unsigned)((T + 63) / 64), B), dim3(256), 0, st, dl,
                           h->d_blob + h->ar.start_off, scal, d_wav, W, (long long)T, Tp);
    WN_HIP(h, hipGetLastError());
    return WN_OK;
}

extern "C" int wn_teacher_backward_input(wn_handle* h, const void* tape, size_t tape_bytes, const float* d_out_params,
                                         int B, int64_t T, float* d_wav, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "wn_teacher_backward_input";
    if (int rc = tb_check(h, fn)) return rc;
    if (B < 1 || T < 1 || !tape || !d_out_params || !d_wav || !ws) return wn_fail(h, WN_EINVAL, "%s: bad argument", fn);
    int F = 0;
    if (int rc = tb_tape_check(h, fn, tape, tape_bytes, B, T, &F)) return rc;
    const BLayout L = b_layout(h, B, T);
    if (ws_bytes < L.total) return wn_fail(h, WN_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, L.total);
    const WnWork work(h);
    return tb_reverse(h, tape, d_out_params, B, T, d_wav, ws, stream, nullptr);
}


// ---- weight gradients of the teacher: d out_params -> d of every variable of the residual stack and head ----
// The reverse pass above already holds every cotangent a weight gradient needs as G4 rows (d out, d h1, ds, and per layer dl
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
namespace {
constexpr int TW_SLABS = 64;        // slabs (batch elements x chunks) aimed at
constexpr int TW_KT = 32;           // columns per LDS stage (one K-step)
constexpr int TW_LD = TW_KT + 8;    // halves per LDS row: 80 bytes, 16 lanes of a ds_read_b128 hit 16 distinct bank quads
constexpr int TW_MAXOP = 10;
constexpr int TW_MAXRED = 12;
constexpr int TW_AUXC = 32;         // channels of aux: x(t-3), x(t-2), x(t-1), 1, zeros

struct TwOp {
    const unsigned* dy;             // G4 rows of M channels (cotangent)
    const unsigned* x;              // G4 rows of N channels (activation)
    long long dy_bs, x_bs;          // words per batch element
    long long out_off;              // floats inside a slab, [N][M]
    int dy_rowlen, dy_col0, M;
    int x_rowlen, x_col0, N;
};
struct TwArgs {
    TwOp op[TW_MAXOP];
    float* slab;
    long long slab_stride;          // floats per slab
    long long T;
    int nchunk, chunk;              // chunks per batch element, columns per chunk
};
struct TwRed {
    long long src_off, dst_off;     // floats inside a slab / inside grads
    int rows, cols, src_ld, dst_ld;
};
struct TwRedArgs {
    TwRed r[TW_MAXRED];
    const float* slab;
    long long slab_stride;
    int nslab;
    const float* scal;
    float* grads;
};

// eight columns of one G4 group -> eight rows [channel][8 columns] of an LDS operand image.  r[j] = the four words of
// column j: word i holds channels 16 (i >> 1) + 2 (i & 1) + {0, 1} (+ 4 kg + 32 s4) of the group (tb_dout_kernel's order)
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
            const int c = 32 * (g >> 2) + 16 * (i >> 1) + 4 * (g & 3) + 2 * (i & 1) + p;
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
    unsigned* base = g4 + (size_t)b * C * Tp;
    *reinterpret_cast<wn_u4*>(base + ((size_t)gr * Tp + t) * 4) = hw;
    *reinterpret_cast<wn_u4*>(base + ((size_t)(NG + gr) * Tp + t) * 4) = lw;
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
    unsigned* base = g4 + (size_t)b * TW_AUXC * Tp;
    *reinterpret_cast<wn_u4*>(base + ((size_t)gr * Tp + t) * 4) = hw;
    *reinterpret_cast<wn_u4*>(base + ((size_t)(NG + gr) * Tp + t) * 4) = lw;
}

// d enc: G4 rows [B][Cd][RE] (scaled) -> float32 [B][TE][Cd]
__global__ __launch_bounds__(256) void tw_denc_kernel(const unsigned* __restrict__ g4, const float* __restrict__ scal,
                                                      float* __restrict__ out, long long TE, long long RE, int Cd) {
    const int b = blockIdx.z, gr = blockIdx.y, NG = Cd / 8;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= TE) return;
    const unsigned* base = g4 + (size_t)b * Cd * RE;
    const wn_u4 hw = *reinterpret_cast<const wn_u4*>(base + ((size_t)gr * RE + t) * 4);
    const wn_u4 lw = *reinterpret_cast<const wn_u4*>(base + ((size_t)(NG + gr) * RE + t) * 4);
    const float sc = scal[1];
    const int s4 = gr >> 2, kg = gr & 3;
    float* o = out + ((size_t)b * TE + t) * Cd;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float v0, v1;
        wn_join_pair(hw[i], lw[i], v0, v1);
        const int ch = 32 * s4 + 16 * (i >> 1) + 4 * kg + 2 * (i & 1);
        o[ch] = v0 * sc;
        o[ch + 1] = v1 * sc;
    }
}

struct TrainLayout {
    size_t l, enc, xs, total;       // after the plain tape's regions
    long long RS, TE;
};
TrainLayout train_layout(const wn_handle* h, int B, int F, long long T) {
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
    L.total = o;
    return L;
}

struct WLayout {
    long long Tp, TE, RE;
    int c0, nchunk, chunk;
    size_t aux, xa, xb, denc, slab, slab_floats, total;
};
WLayout w_layout(const wn_handle* h, int B, int F, long long T) {
    const wn_config& c = h->cfg;
    const int W = c.width, S = c.skip_width, G = c.gate_width, H = G / 2, Cd = c.deconv_width;
    const BLayout BL = b_layout(h, B, T);
    WLayout L;
    L.Tp = BL.Tp;
    L.TE = (long long)F * h->frame_shift;
    L.c0 = (int)((L.TE - T) / 2);
    L.RE = std::max<long long>(L.TE, L.c0 + L.Tp);
    const long long ntiles = L.Tp / TG_TN, want = std::min<long long>(ntiles, std::max(1, TW_SLABS / B));
    L.chunk = (int)((ntiles + want - 1) / want) * TG_TN;
    L.nchunk = (int)((T + L.chunk - 1) / L.chunk);
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
struct GradEntry {
    std::string name;
    size_t off;
    int64_t shape[4];
    int ndim;
};
std::vector<GradEntry> grad_table(const wn_handle* h) {
    const wn_config& c = h->cfg;
    const int W = c.width, S = c.skip_width, G = c.gate_width, H = G / 2, Cd = c.deconv_width, OW = c.out_width;
    std::vector<GradEntry> t;
    size_t off = 0;
    auto conv = [&](const std::string& scope, int K, int cin, int cout) {
        t.push_back({scope + "/W", off, {1, K, cin, cout}, 4});
        off += (size_t)K * cin * cout;
        t.push_back({scope + "/biases", off, {cout, 0, 0, 0}, 1});
        off += cout;
    };
    conv("conv_start", 3, 1, W);
    conv("skip_start", 1, W, S);
    for (size_t i = 0; i < h->teacher.layers.size(); ++i) {
        const std::string n = std::to_string(i + 1);
        conv("dilated_conv_" + n, 3, W, G);
        conv("mel_cond_" + n, 1, Cd, G);
        conv("res_" + n, 1, H, W);
        conv("skip_" + n, 1, H, S);
    }
    conv("out1", 1, S, S);
    conv("mel_cond_out1", 1, Cd, S);
    conv("out2", 1, S, OW);
    return t;
}
size_t grad_floats(const std::vector<GradEntry>& t) { return t.back().off + (size_t)t.back().shape[0]; }
constexpr size_t GRAD_NONE = ~(size_t)0;
size_t grad_off(const std::vector<GradEntry>& t, const std::string& name) {
    for (const GradEntry& e : t)
        if (e.name == name) return e.off;
    return GRAD_NONE;       // an unknown name: TwBatch::red records it and run() refuses to launch
}

struct TwCtx {
    int B;
    long long T;
    WLayout L;
    TrainLayout TR;
    std::vector<GradEntry> tab;
    // workspace (reverse pass)
    float* scal;
    unsigned *dout, *dh1, *ds, *dl, *dd;
    long long RD;
    int Kp;
    // workspace (weight side)
    unsigned *aux, *xa, *xb, *denc;
    float* slab;
    // tape
    const float *tape_s, *tape_h1, *tape_g, *xs;
    const unsigned *tl, *enc;
    float* grads;
    bool want_denc;
};

// one batch of products and the reduction of their slabs
struct TwBatch {
    TwArgs a{};
    TwRedArgs r{};
    int nop = 0, nred = 0;
    long long used = 0;
    int max_tiles = 0;
    // dY (M channels, rows of rowlen) x X (N channels): returns the slab offset of the [N][M] product
    bool bad = false;               // a table overflow or an unknown gradient name: nothing was written, run() refuses
    long long add(const unsigned* dy, int M, long long dy_rowlen, const unsigned* x, int N, long long x_rowlen, long long x_col0) {
        if (nop >= TW_MAXOP) { bad = true; return 0; }
        TwOp& o = a.op[nop++];
        o.dy = dy; o.dy_bs = (long long)M * dy_rowlen; o.dy_rowlen = (int)dy_rowlen; o.dy_col0 = 0; o.M = M;
        o.x = x; o.x_bs = (long long)N * x_rowlen; o.x_rowlen = (int)x_rowlen; o.x_col0 = (int)x_col0; o.N = N;
        o.out_off = used;
        used += (long long)M * N;
        max_tiles = std::max(max_tiles, ((M + 127) / 128) * ((N + 127) / 128));
        return o.out_off;
    }
    void red(long long src_off, int rows, int cols, int src_ld, size_t dst_off, int dst_ld) {
        if (nred >= TW_MAXRED || dst_off == GRAD_NONE) { bad = true; return; }
        TwRed& q = r.r[nred++];
        q.src_off = src_off; q.dst_off = (long long)dst_off; q.rows = rows; q.cols = cols; q.src_ld = src_ld; q.dst_ld = dst_ld;
    }
    int run(wn_handle* h, const TwCtx& w, hipStream_t st) {
        if (bad || used > (long long)w.L.slab_floats)
            return wn_fail(h, WN_EIO, "wn_teacher_backward_weights: internal product table overflow or unknown gradient name");
        a.slab = w.slab; a.slab_stride = (long long)w.L.slab_floats; a.T = w.T; a.nchunk = w.L.nchunk; a.chunk = w.L.chunk;
        hipLaunchKernelGGL(tw_gemm_kernel, dim3(max_tiles, nop, w.B * w.L.nchunk), dim3(256), 0, st, a);
        r.slab = w.slab; r.slab_stride = a.slab_stride; r.nslab = w.B * w.L.nchunk; r.scal = w.scal; r.grads = w.grads;
        int most = 0;
        for (int i = 0; i < nred; ++i) most = std::max(most, r.r[i].rows * r.r[i].cols);
        hipLaunchKernelGGL(tw_reduce_kernel, dim3(std::min(1024, (most + 255) / 256), nred), dim3(256), 0, st, r);
        WN_HIP(h, hipGetLastError());
        return WN_OK;
    }
};

// in-place accumulation of W^T dY into the d enc rows (tg_gemm_kernel, RS epilogue with residual rows only)
void tw_denc_gemm(wn_handle* h, const TwCtx& w, const TeacherGemmPack& g, const unsigned* dy, int C, long long rowlen,
                  hipStream_t st) {
    const int Cd = h->cfg.deconv_width;
    TgArgs a{};
    a.wp = reinterpret_cast<const unsigned*>(h->d_blob + g.w_off);
    a.bias = h->d_blob + g.b_off;
    a.inv_scale = g.inv_scale;
    a.nks = g.nks;
    a.T = w.T;
    a.og4 = w.denc; a.og4_bstride = (long long)Cd * w.L.RE; a.og4_rowlen = (int)w.L.RE; a.og4_col0 = w.L.c0; a.og4_ng = Cd / 8;
    a.seg[0].base = dy; a.seg[0].bstride = (long long)C * rowlen; a.seg[0].rowlen = (int)rowlen; a.seg[0].col0 = 0;
    a.seg[0].nks = C / 32; a.seg[0].ng = C / 8; a.seg[0].kind = TG_SRC_G4;
    a.nseg = 1;
    a.res_mtiles = g.mtiles;
    tg_launch<TG_EPI_RS>(a, g.mtiles, w.B, w.L.Tp, st);
}

int tw_aux(wn_handle* h, const TwCtx& w, hipStream_t st) {
    const long long Tp = w.L.Tp;
    hipLaunchKernelGGL(tw_aux_kernel, dim3((unsigned)(Tp / 256), TW_AUXC / 8, w.B), dim3(256), 0, st, w.xs, w.aux, w.T, Tp);
    if (w.want_denc) WN_HIP(h, hipMemsetAsync(w.denc, 0, (size_t)w.B * h->cfg.deconv_width * w.L.RE * 4, st));
    return WN_OK;
}

// stage 0 (d h1 is complete): relu(h1) rows;  stage 1 (ds is complete): the head's products
int tw_head(wn_handle* h, const TwCtx& w, hipStream_t st, int stage) {
    const wn_config& c = h->cfg;
    const int S = c.skip_width, Cd = c.deconv_width, OW = c.out_width, Kp = w.Kp;
    const long long Tp = w.L.Tp;
    const dim3 ga((unsigned)(Tp / 256), S / 8, w.B);
    if (stage == 0) {
        hipLaunchKernelGGL(tw_act_kernel, ga, dim3(256), 0, st, w.tape_h1, (long long)S * Tp, S / 16, 0, w.xa, w.T, Tp, S, 0);
        return WN_OK;
    }
    hipLaunchKernelGGL(tw_act_kernel, ga, dim3(256), 0, st, w.tape_s, (long long)S * Tp, S / 16, 0, w.xb, w.T, Tp, S, 0);
    TwBatch k;
    const long long o2w = k.add(w.dout, Kp, Tp, w.xa, S, Tp, 0);
    const long long o2b = k.add(w.dout, Kp, Tp, w.aux, TW_AUXC, Tp, 0);
    const long long o1w = k.add(w.dh1, S, Tp, w.xb, S, Tp, 0);
    const long long c1w = k.add(w.dh1, S, Tp, w.enc, Cd, w.L.TE, w.L.c0);
    const long long o1b = k.add(w.dh1, S, Tp, w.aux, TW_AUXC, Tp, 0);
    k.red(o2w, S, OW, Kp, grad_off(w.tab, "out2/W"), OW);
    k.red(o2b + 3 * Kp, 1, OW, Kp, grad_off(w.tab, "out2/biases"), OW);
    k.red(o1w, S, S, S, grad_off(w.tab, "out1/W"), S);
    k.red(c1w, Cd, S, S, grad_off(w.tab, "mel_cond_out1/W"), S);
    k.red(o1b + 3 * S, 1, S, S, grad_off(w.tab, "out1/biases"), S);
    k.red(o1b + 3 * S, 1, S, S, grad_off(w.tab, "mel_cond_out1/biases"), S);
    if (int rc = k.run(h, w, st)) return rc;
    if (w.want_denc) tw_denc_gemm(h, w, h->teacher.cond_out1_t, w.dh1, S, Tp, st);
    return WN_OK;
}

int tw_layer(wn_handle* h, const TwCtx& w, size_t li, hipStream_t st) {
    const wn_config& c = h->cfg;
    const int W = c.width, S = c.skip_width, G = c.gate_width, H = G / 2, Cd = c.deconv_width;
    const long long Tp = w.L.Tp, RS = w.TR.RS;
    const TeacherLayerPack& tl = h->teacher.layers[li];
    const std::string n = std::to_string(li + 1);
    // m_i = sigma * tanh of the gate tape
    hipLaunchKernelGGL(tw_act_kernel, dim3((unsigned)(Tp / 256), H / 8, w.B), dim3(256), 0, st,
                       w.tape_g + li * (size_t)w.B * G * Tp, (long long)G * Tp, G / 16, H / 16, w.xa, w.T, Tp, H, 1);
    const unsigned* l = w.tl + li * (size_t)w.B * W * RS;
    TwBatch k;
    const long long rw = k.add(w.dl, W, Tp, w.xa, H, Tp, 0);
    const long long sw = k.add(w.ds, S, Tp, w.xa, H, Tp, 0);
    const long long rb = k.add(w.dl, W, Tp, w.aux, TW_AUXC, Tp, 0);
    const long long sb = k.add(w.ds, S, Tp, w.aux, TW_AUXC, Tp, 0);
    long long dw[3];
    for (int tap = 0; tap < 3; ++tap) dw[tap] = k.add(w.dd, G, w.RD, l, W, RS, IAF_LP - (long long)(2 - tap) * tl.dilation);
    const long long cw = k.add(w.dd, G, w.RD, w.enc, Cd, w.L.TE, w.L.c0);
    const long long db = k.add(w.dd, G, w.RD, w.aux, TW_AUXC, Tp, 0);
    k.red(rw, H, W, W, grad_off(w.tab, "res_" + n + "/W"), W);
    k.red(sw, H, S, S, grad_off(w.tab, "skip_" + n + "/W"), S);
    k.red(rb + 3 * W, 1, W, W, grad_off(w.tab, "res_" + n + "/biases"), W);
    k.red(sb + 3 * S, 1, S, S, grad_off(w.tab, "skip_" + n + "/biases"), S);
    for (int tap = 0; tap < 3; ++tap)
        k.red(dw[tap], W, G, G, grad_off(w.tab, "dilated_conv_" + n + "/W") + (size_t)tap * W * G, G);
    k.red(cw, Cd, G, G, grad_off(w.tab, "mel_cond_" + n + "/W"), G);
    k.red(db + 3 * G, 1, G, G, grad_off(w.tab, "dilated_conv_" + n + "/biases"), G);
    k.red(db + 3 * G, 1, G, G, grad_off(w.tab, "mel_cond_" + n + "/biases"), G);
    if (int rc = k.run(h, w, st)) return rc;
    if (w.want_denc) tw_denc_gemm(h, w, tl.cond_t, w.dd, G, w.RD, st);
    return WN_OK;
}

// dl = d l_0: skip_start and conv_start
int tw_tail(wn_handle* h, const TwCtx& w, hipStream_t st) {
    const wn_config& c = h->cfg;
    const int W = c.width, S = c.skip_width;
    const long long Tp = w.L.Tp, RS = w.TR.RS;
    TwBatch k;
    const long long sw = k.add(w.ds, S, Tp, w.tl, W, RS, IAF_LP);
    const long long sb = k.add(w.ds, S, Tp, w.aux, TW_AUXC, Tp, 0);
    const long long cs = k.add(w.dl, W, Tp, w.aux, TW_AUXC, Tp, 0);
    k.red(sw, W, S, S, grad_off(w.tab, "skip_start/W"), S);
    k.red(sb + 3 * S, 1, S, S, grad_off(w.tab, "skip_start/biases"), S);
    k.red(cs, 3, W, W, grad_off(w.tab, "conv_start/W"), W);
    k.red(cs + 3 * W, 1, W, W, grad_off(w.tab, "conv_start/biases"), W);
    return k.run(h, w, st);
}

// what the weight-gradient calls refuse beyond tb_check
int tw_check(wn_handle* h, const char* fn) {
    if (int rc = tb_check(h, fn)) return rc;
    if (h->cfg.use_weight_norm)
        return wn_fail(h, WN_EINVAL, "%s: weight-norm teacher: the gradients of W_V / W_g are not implemented", fn);
    return WN_OK;
}
}  // namespace

extern "C" int wn_teacher_grad_count(const wn_handle* h) {
    if (!h || !h->finalized || h->cfg.kind != WN_KIND_TEACHER) return 0;
    return (int)grad_table(h).size();
}

extern "C" int wn_teacher_grad_info(const wn_handle* h, int i, char* name, size_t name_cap, int64_t* offset, int64_t* shape4,
                                    int* ndim) {
    if (!h || !h->finalized || h->cfg.kind != WN_KIND_TEACHER)
        return wn_fail(h, WN_EINVAL, "wn_teacher_grad_info: needs a finalized teacher handle");
    const std::vector<GradEntry> t = grad_table(h);
    if (i < 0 || i >= (int)t.size() || !name || !offset || !shape4 || !ndim || name_cap <= t[i].name.size())
        return wn_fail(h, WN_EINVAL, "wn_teacher_grad_info: bad argument (index %d of %zu)", i, t.size());
    memcpy(name, t[i].name.c_str(), t[i].name.size() + 1);
    *offset = (int64_t)t[i].off;
    for (int k = 0; k < 4; ++k) shape4[k] = t[i].shape[k];
    *ndim = t[i].ndim;
    return WN_OK;
}

extern "C" size_t wn_teacher_grad_floats(const wn_handle* h) {
    if (!h || !h->finalized || h->cfg.kind != WN_KIND_TEACHER) return 0;
    return grad_floats(grad_table(h));
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
    const TapeLayout TL = tape_layout(h, B, T);
    const TrainLayout TR = train_layout(h, B, F, T);
    if (tape_bytes < TR.total) return wn_fail(h, WN_ENOMEM, "%s: tape %zu < %zu bytes", fn, tape_bytes, TR.total);
    const WnWork work(h);
    char* tb = reinterpret_cast<char*>(tape);
    TbHead hd;
    const uint64_t ser = h->teacher.serial;
    hd.w[0] = TB_MAGIC_TRAIN; hd.w[1] = (unsigned)ser; hd.w[2] = (unsigned)(ser >> 32); hd.w[3] = (unsigned)B;
    hd.w[4] = (unsigned)T; hd.w[5] = (unsigned)((uint64_t)T >> 32); hd.w[6] = (unsigned)h->teacher.layers.size();
    hd.w[7] = (unsigned)F;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(tb_header_kernel, dim3(1), dim3(64), 0, st, hd, reinterpret_cast<unsigned*>(tb));
    const int rc = tg_forward(h, fn, wav, mel, B, F, T, out_params, ws, ws_bytes, reinterpret_cast<float*>(tb + TL.s),
                              reinterpret_cast<float*>(tb + TL.h1), reinterpret_cast<float*>(tb + TL.g), stream,
                              reinterpret_cast<unsigned*>(tb + TR.l), reinterpret_cast<float*>(tb + TR.enc),
                              reinterpret_cast<float*>(tb + TR.xs));
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g_tape_mu);
    g_tapes[tape] = TapeRec{ser, B, (long long)T, F};
    return WN_OK;
}

extern "C" int wn_teacher_backward_weights(wn_handle* h, const void* tape, size_t tape_bytes, const float* d_out_params, int B,
                                           int F, int64_t T, float* grads, size_t grads_floats, float* d_encoding, float* d_wav,
                                           void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "wn_teacher_backward_weights";
    if (int rc = tw_check(h, fn)) return rc;
    if (B < 1 || F < 1 || T < 1 || !tape || !d_out_params || !grads || !ws) return wn_fail(h, WN_EINVAL, "%s: bad argument", fn);
    int tape_F = 0;
    if (int rc = tb_tape_check(h, fn, tape, tape_bytes, B, T, &tape_F)) return rc;
    if (tape_F == 0)
        return wn_fail(h, WN_EINVAL, "%s: a plain tape of wn_teacher_forward_tape holds no layer inputs and no conditioning; "
                       "the weight gradients need a tape of wn_teacher_forward_train_tape", fn);
    if (tape_F != F) return wn_fail(h, WN_EINVAL, "%s: the tape holds F = %d mel frames, not %d", fn, tape_F, F);
    TwCtx w;
    w.TR = train_layout(h, B, F, T);
    if (tape_bytes < w.TR.total)
        return wn_fail(h, WN_EINVAL, "%s: a tape of %zu bytes cannot hold the training tape of B = %d, F = %d, T = %lld "
                       "(%zu bytes)", fn, tape_bytes, B, F, (long long)T, w.TR.total);
    w.tab = grad_table(h);
    if (grads_floats < grad_floats(w.tab))
        return wn_fail(h, WN_ENOMEM, "%s: grads holds %zu floats, the gradients need %zu", fn, grads_floats, grad_floats(w.tab));
    if (d_encoding && !h->teacher.denc_ok)
        return wn_fail(h, WN_EINVAL, "%s: d_encoding needs deconv_width %d to be a multiple of 64", fn, h->cfg.deconv_width);
    w.L = w_layout(h, B, F, T);
    if ((long long)B * w.L.nchunk > 65535) return wn_fail(h, WN_EINVAL, "%s: B = %d needs more than 65535 slabs", fn, B);
    if (ws_bytes < w.L.total) return wn_fail(h, WN_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, w.L.total);
    const WnWork work(h);
    const TapeLayout TL = tape_layout(h, B, T);
    const BLayout BL = b_layout(h, B, T);
    char* base = reinterpret_cast<char*>(ws);
    const char* tb = reinterpret_cast<const char*>(tape);
    w.B = B; w.T = T;
    w.scal = reinterpret_cast<float*>(base + BL.scal);
    w.dout = reinterpret_cast<unsigned*>(base + BL.dout);
    w.dh1 = reinterpret_cast<unsigned*>(base + BL.dh1);
    w.ds = reinterpret_cast<unsigned*>(base + BL.ds);
    w.dl = reinterpret_cast<unsigned*>(base + BL.dl);
    w.dd = reinterpret_cast<unsigned*>(base + BL.dd);
    w.RD = BL.RD; w.Kp = BL.Kp;
    w.aux = reinterpret_cast<unsigned*>(base + w.L.aux);
    w.xa = reinterpret_cast<unsigned*>(base + w.L.xa);
    w.xb = reinterpret_cast<unsigned*>(base + w.L.xb);
    w.denc = reinterpret_cast<unsigned*>(base + w.L.denc);
    w.slab = reinterpret_cast<float*>(base + w.L.slab);
    w.tape_s = reinterpret_cast<const float*>(tb + TL.s);
    w.tape_h1 = reinterpret_cast<const float*>(tb + TL.h1);
    w.tape_g = reinterpret_cast<const float*>(tb + TL.g);
    w.tl = reinterpret_cast<const unsigned*>(tb + w.TR.l);
    w.enc = reinterpret_cast<const unsigned*>(tb + w.TR.enc);
    w.xs = reinterpret_cast<const float*>(tb + w.TR.xs);
    w.grads = grads;
    w.want_denc = d_encoding != nullptr;
    if (int rc = tb_reverse(h, tape, d_out_params, B, T, d_wav, ws, stream, &w)) return rc;
    if (d_encoding) {
        hipStream_t st = reinterpret_cast<hipStream_t>(stream);
        const int Cd = h->cfg.deconv_width;
        hipLaunchKernelGGL(tw_denc_kernel, dim3((unsigned)((w.L.TE + 255) / 256), Cd / 8, B), dim3(256), 0, st, w.denc, w.scal,
                           d_encoding, w.L.TE, w.L.RE, Cd);
        WN_HIP(h, hipGetLastError());
    }
    return WN_OK;
}
