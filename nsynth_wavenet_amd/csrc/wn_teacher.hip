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

#include "wn_teacher.h"
#include "wn_g4.h"
#include "wn_mol.h"
#include "wn_pack_h.h"
#include "wn_mfma_h.h"

namespace {

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
    } else if ((EPI == TG_EPI_RS || EPI == TG_EPI_RSC) && mt < a.res_mtiles) {
        // residual rows 64 mt .. +63: l += res  (wavenet.py:272-274), two 32-channel operand groups
        // (RSC: the sum goes to og4 and the rows at ig4 stay as they are -- a training tape keeps every layer's input)
        const size_t lo = (size_t)a.og4_ng * a.og4_rowlen;
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const size_t oo = (size_t)b * a.og4_bstride + ((size_t)(4 * (2 * mt + st) + q) * a.og4_rowlen + a.og4_col0 + t0 + n) * 4;
            wn_u4* o = reinterpret_cast<wn_u4*>(a.og4 + oo);
            const wn_u4* in = EPI == TG_EPI_RSC ? reinterpret_cast<const wn_u4*>(a.ig4 + oo) : o;
#pragma unroll
            for (int e = 0; e < TG_NT; ++e) {
                const wn_u4 oh = in[16 * e], ol = in[lo + 16 * e];
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
            if (a.bg_rows && 64 * mt + 32 * st >= a.bg_rows) continue;      // zero rows of a padded pack: no gate channel
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
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ch = wn_g4_channel(g, i);
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
    wn_g4_store(l + (size_t)b * W * RS, NG, RS, g, c, hw, lw);
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

void wn_tg_input(const float* wav, float* xs, int B, long long T, long long Tp, int mu, hipStream_t st) {
    hipLaunchKernelGGL(tg_input_kernel, dim3((unsigned)((TG_XP + Tp + 255) / 256), B), dim3(256), 0, st, wav, xs, T, Tp, mu);
}
void wn_tg_start(const float* xs, const float* wb, unsigned* l, int B, int W, long long Tp, long long RS, hipStream_t st) {
    hipLaunchKernelGGL(tg_start_kernel, dim3((unsigned)((RS + 255) / 256), W / 8, B), dim3(256), 0, st, xs, wb, l, W, Tp, RS);
}
uint64_t wn_tape_serial_next() {
    static std::atomic<uint64_t> next_serial{1};
    return next_serial++;
}

void wn_tg_launch(int epi, const TgArgs& a, int mtiles, int B, long long Tp, hipStream_t st) {
    switch (epi) {
        case TG_EPI_GATE: return tg_launch<TG_EPI_GATE>(a, mtiles, B, Tp, st);
        case TG_EPI_RS: return tg_launch<TG_EPI_RS>(a, mtiles, B, Tp, st);
        case TG_EPI_ACC: return tg_launch<TG_EPI_ACC>(a, mtiles, B, Tp, st);
        case TG_EPI_OUT: return tg_launch<TG_EPI_OUT>(a, mtiles, B, Tp, st);
        case TG_EPI_GATE_TAPE: return tg_launch<TG_EPI_GATE_TAPE>(a, mtiles, B, Tp, st);
        case TG_EPI_BGATE: return tg_launch<TG_EPI_BGATE>(a, mtiles, B, Tp, st);
        case TG_EPI_MASK: return tg_launch<TG_EPI_MASK>(a, mtiles, B, Tp, st);
        case TG_EPI_RSC: return tg_launch<TG_EPI_RSC>(a, mtiles, B, Tp, st);
    }
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
    T.serial = wn_tape_serial_next();
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
        const float lmax = wn_wave_max(lg);
        const float lse = lmax + logf(tl_wave_sum(lane < M ? expf(lg - lmax) : 0.f));
        v = lane < M ? v + (lg - lse) : NEG;
        const float vmax = wn_wave_max(v);
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
        m = wn_wave_max(m);
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
    const float mx = wn_wave_max(m);
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
        const float lmax = wn_wave_max(lg);
        const float lse = lmax + logf(tl_wave_sum(lane < M ? expf(lg - lmax) : 0.f));
        v = lane < M ? v + (lg - lse) : NEG;
        const float vmax = wn_wave_max(v);
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

extern "C" size_t wn_teacher_workspace_bytes(const wn_handle* h, int B, int F, int64_t T) {
    if (!h || !h->finalized || h->cfg.kind != WN_KIND_TEACHER || B < 1 || F < 1 || T < 1) return 0;
    return t_layout(h, B, F, T).total;
}

int tg_forward_check(wn_handle* h, const char* fn, const float* wav, const float* mel, int B, int F, int64_t T,
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
    if (TE > WN_MAX_ROW_SAMPLES) return wn_fail(h, WN_EINVAL, "%s: utterance too long (32-bit row offsets)", fn);
    return WN_OK;
}

// the forward; with tape.s the skip sum and out1 rows land in the tape and every gate stores its activations
// to tape.g (layer i at i * B * gate * Tp floats) -- the same arithmetic, so out_params are the same bits either way.
// With tape.l (training tape) the conditioning and the scaled input row are written to the tape instead of the
// workspace and layer i reads its input l_i from slot i of tape.l: l_i is copied to the next slot (the workspace row for the
// last layer) before the residual GEMM updates that copy in place -- the same kernels on the same values.
int tg_forward(wn_handle* h, const char* fn, const float* wav, const float* mel, int B, int F, int64_t T, float* out_params,
               void* ws, size_t ws_bytes, const TgTape& tape, void* stream) {
    const wn_config& c = h->cfg;
    const TLayout L = t_layout(h, B, F, T);
    if (ws_bytes < L.total)
        return wn_fail(h, WN_ENOMEM, "%s: workspace %zu < %zu bytes", fn, ws_bytes, L.total);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* base = reinterpret_cast<char*>(ws);
    float* enc = tape.enc ? tape.enc : reinterpret_cast<float*>(base + L.enc);
    unsigned* lws = reinterpret_cast<unsigned*>(base + L.l);
    unsigned* l = tape.l ? tape.l : lws;
    unsigned* m = reinterpret_cast<unsigned*>(base + L.m);
    float* s = tape.s ? tape.s : reinterpret_cast<float*>(base + L.s);
    float* h1 = tape.h1 ? tape.h1 : reinterpret_cast<float*>(base + L.h1);
    float* xs = tape.xs ? tape.xs : reinterpret_cast<float*>(base + L.xs);
    const int W = c.width, S = c.skip_width, H = c.gate_width / 2, Cd = c.deconv_width;
    const TeacherPack& P = h->teacher;
    // dropout (training tapes only).  dropout_inputs: conv_start writes the raw l_0 row, skip_start reads it, and
    // slot 0 receives its masked copy;  dropout_all: slot 0 and every layer's output are masked in place
    const TgDropout& dr = tape.drop;
    const bool drop_in = dr.mode == WN_DROPOUT_INPUTS, drop_all = dr.mode == WN_DROPOUT_ALL;
    unsigned* l_start = drop_in ? tape.lraw : l;

    // conditioning (wavenet.py:214-216), G4 rows of TE columns
    int rc = wn_run_deconv(h, 0, mel, B, F, enc, L.TE, base + L.scratch, st, true);
    if (rc) return rc;
    // l0 = conv_start(shift_right(x_scaled))  (wavenet.py:223-226)
    {
        wn_tg_input(wav, xs, B, T, L.Tp, c.use_mu_law, st);
        wn_tg_start(xs, h->d_blob + h->ar.start_off, l_start, B, W, L.Tp, L.RS, st);
    }
    if (drop_all) wn_dropout_g4(l, l, B, W, L.RS, IAF_LP, T, dr, 0, st);        // conv_dropout (wavenet.py:229-230)
    auto seg_acc = [&](const float* p, int nks) {
        TgSeg sg;
        sg.base = reinterpret_cast<const unsigned*>(p); sg.bstride = (long long)S * L.Tp; sg.rowlen = S / 16;
        sg.col0 = 0; sg.nks = nks; sg.ng = 0; sg.kind = TG_SRC_ACC_RELU;
        return sg;
    };
    TgSeg seg_l = tg_seg_g4(l, (long long)W * L.RS, L.RS, IAF_LP, W);
    const size_t l_words = (size_t)B * W * L.RS;
    const TgSeg seg_enc = tg_seg_g4(reinterpret_cast<const unsigned*>(enc), (long long)Cd * L.TE, L.TE, L.c0, Cd);
    const TgSeg seg_m = tg_seg_g4(m, (long long)H * L.Tp, L.Tp, 0, H);
    // s = skip_start(l)  (wavenet.py:231-233)
    {
        TgArgs a = tg_pack_args(h, P.skip_start, T);
        a.seg[0] = seg_l; a.seg[0].base = l_start; a.nseg = 1;
        a.oacc = s; a.oacc_bstride = (long long)S * L.Tp; a.oacc_nmb = S / 16;
        wn_tg_launch(TG_EPI_ACC, a, P.skip_start.mtiles, B, L.Tp, st);
    }
    if (drop_in) {      // conv_dropout on l, skip_dropout on s (wavenet.py:204-206, 237-239)
        wn_dropout_g4(l_start, l, B, W, L.RS, IAF_LP, T, dr, 0, st);
        wn_dropout_acc(s, B, S, L.Tp, T, dr, 1, st);
    }
    for (size_t li = 0; li < P.layers.size(); ++li) {
        const TeacherLayerPack& tl = P.layers[li];
        if (tape.l) {
            seg_l.base = l;
            unsigned* next = li + 1 < P.layers.size() ? l + l_words : lws;
            WN_HIP(h, hipMemcpyAsync(next, l, l_words * 4, hipMemcpyDeviceToDevice, st));
            l = next;                     // the gate below reads seg_l (slot li); the residual GEMM updates the copy
        }
        {   // d = dilated_conv(l) + mel_cond(enc); m = sigmoid(d[:H]) * tanh(d[H:])  (wavenet.py:243-269)
            TgArgs a = tg_pack_args(h, tl.gate, T);
            for (int tap = 0; tap < 3; ++tap) {
                a.seg[tap] = seg_l;
                a.seg[tap].col0 = IAF_LP - (2 - tap) * tl.dilation;
            }
            a.seg[3] = seg_enc; a.nseg = 4;
            a.og4 = m; a.og4_bstride = (long long)H * L.Tp; a.og4_rowlen = (int)L.Tp; a.og4_col0 = 0; a.og4_ng = H / 8;
            if (tape.g) {
                a.tape = tape.g + li * (size_t)B * 2 * H * L.Tp;
                a.tape_bstride = 2ll * H * L.Tp; a.tape_nmb = 2 * H / 16; a.tape_hoff = H / 16;
                wn_tg_launch(TG_EPI_GATE_TAPE, a, tl.gate.mtiles, B, L.Tp, st);
            } else {
                wn_tg_launch(TG_EPI_GATE, a, tl.gate.mtiles, B, L.Tp, st);
            }
        }
        {   // l += res(m); s += skip(m)  (wavenet.py:271-277)
            TgArgs a = tg_pack_args(h, tl.rs, T);
            a.seg[0] = seg_m; a.nseg = 1;
            a.og4 = l; a.og4_bstride = (long long)W * L.RS; a.og4_rowlen = (int)L.RS; a.og4_col0 = IAF_LP; a.og4_ng = W / 8;
            a.oacc = s; a.oacc_bstride = (long long)S * L.Tp; a.oacc_nmb = S / 16;
            a.res_mtiles = W / 64;
            wn_tg_launch(TG_EPI_RS, a, tl.rs.mtiles, B, L.Tp, st);
        }
        // res_dropout (wavenet.py:276-278); the last layer's output is read by nothing
        if (drop_all && li + 1 < P.layers.size()) wn_dropout_g4(l, l, B, W, L.RS, IAF_LP, T, dr, (int)li + 1, st);
    }
    {   // out1(relu(s)) + mel_cond_out1(enc)  (wavenet.py:283-289)
        TgArgs a = tg_pack_args(h, P.out1, T);
        a.seg[0] = seg_acc(s, S / 32); a.seg[1] = seg_enc; a.nseg = 2;
        a.oacc = h1; a.oacc_bstride = (long long)S * L.Tp; a.oacc_nmb = S / 16;
        wn_tg_launch(TG_EPI_ACC, a, P.out1.mtiles, B, L.Tp, st);
    }
    {   // out2(relu(.))  (wavenet.py:290-292)
        TgArgs a = tg_pack_args(h, P.out2, T);
        a.seg[0] = seg_acc(h1, S / 32); a.nseg = 1;
        a.otm = out_params; a.ow = c.out_width;
        wn_tg_launch(TG_EPI_OUT, a, P.out2.mtiles, B, L.Tp, st);
    }
    WN_HIP(h, hipGetLastError());
    return WN_OK;
}

extern "C" int wn_teacher_forward(wn_handle* h, const float* wav, const float* mel, int B, int F, int64_t T,
                                  float* out_params, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "wn_teacher_forward";
    if (int rc = tg_forward_check(h, fn, wav, mel, B, F, T, out_params, ws)) return rc;
    const WnWork work(h);
    return tg_forward(h, fn, wav, mel, B, F, T, out_params, ws, ws_bytes, TgTape{}, stream);
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
