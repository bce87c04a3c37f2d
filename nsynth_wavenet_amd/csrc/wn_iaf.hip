// Parallel-WaveNet (IAF) student generation on gfx950:
//   wavenet/parallel_wavenet.py:200-287 (_create_iaf), :289-345 (feed_forward),
//   :347-359 (_clip_quant_scale), :172-184 (noise sources).
//
// Device data layout (all fp32, caller-provided workspace):
//   l   ping/pong  [B][64][LP + T]   residual stream, CHANNEL-MAJOR rows, LP zero
//                                    columns on the left so t-d / t-2d never branch
//   enc            [B][256][TE]      upsampled mel (wn_deconv.hip), channel-major
//   x              [B][XP + T]       flow input/output, XP zero columns on the left
//   x0, M, S       [B][T]            noise, mean_tot, scale_tot
//
// One residual layer (parallel_wavenet.py:227-254) is ONE kernel:
//   h[o,t]  = bd+bc + sum_k Wd[tap k] l[:, t-(2-k)d] + Wc enc[:, t+c0]     (K = 448)
//   g[c,t]  = sigmoid(h[c,t]) * tanh(h[c+32,t])
//   l'[o,t] = l[o,t] + br + Wr g[:, t]                                       (K = 32)
// as v_mfma_f32_16x16x4_f32 with the WEIGHTS as the A operand (M = output channel)
// and the ACTIVATIONS as the B operand (N = time).  With that orientation
//   * B-operand loads are time-contiguous (coalesced) rows, dilation is a column
//     offset, the centre crop (wavenet.py:76-85) is a pointer offset;
//   * the accumulator holds, per lane, one time step and channels {16mb+4q+r}:
//     sigmoid channel c and tanh channel c+32 sit in the same lane and register
//     index (row blocks mb and mb+2), so the gate is lane-local;
//   * the gated registers ARE the B operand of the residual 1x1 (K order is
//     chosen to match the accumulator layout), and the tap-t loads ARE its C-in.
// Weights are packed on the host in A-fragment order and staged once per
// workgroup in LDS (120.5 KB); workgroups are persistent over 64-sample tiles.
//
// This unit: the fp32 MFMA kernels, their host pack and their launch functions.  The call that uses them: wn_iaf_call.hip.
#include "wn_internal.h"

namespace {

constexpr float EXP_M9 = 1.2340980408667956e-4f;
constexpr float EXP_7 = 1096.6331584284585f;

__device__ inline f4 mfma4(float a, float b, f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ inline float sigmoidf_(float a) { return __builtin_amdgcn_rcpf(1.f + __expf(-a)); }
__device__ inline float tanhf_(float a) { return 1.f - 2.f * __builtin_amdgcn_rcpf(__expf(2.f * a) + 1.f); }

// ---------------- start conv (parallel_wavenet.py:222-225; masked.py:39-52) ----------------
// l[c,t] = b[c] + W0[c] x[t-3] + W1[c] x[t-2] + W2[c] x[t-1]   (shift_right folded into the taps)
__global__ void iaf_start_kernel(const float* __restrict__ x, const float* __restrict__ wb,
                                 float* __restrict__ l, int64_t T, int XR, int64_t RS) {
    const int b = blockIdx.y;
    const int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (t >= T) return;
    const float* xp = x + (size_t)b * XR + IAF_XP + t;
    float xv[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) xv[i] = xp[i - 3];
    float* lp = l + (size_t)b * IAF_W * RS + IAF_LP + t;
    for (int c = 0; c < IAF_W; ++c) {
        const float w0 = wb[c], w1 = wb[IAF_W + c], w2 = wb[2 * IAF_W + c], bb = wb[3 * IAF_W + c];
        f4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = bb + w0 * xv[e] + w1 * xv[e + 1] + w2 * xv[e + 2];
        *reinterpret_cast<f4*>(lp + (size_t)c * RS) = o;
    }
}

// The same into the "Q4" rows of the hoisted fp32 form: l[b][group g = c / 4][column][4 channels] -- one 16-byte word is
// the MFMA B operand of a lane for a whole K-group, so a layer issues 12 operand loads per block instead of 48 (the vector
// memory instructions of the planar form cost the K loop 16 % and the launch's first 4 000 cycles: r06 cycle stamps).
__global__ void iaf_start_q4_kernel(const float* __restrict__ x, const float* __restrict__ wb,
                                    float* __restrict__ l, int64_t T, int XR, int64_t RS) {
    const int b = blockIdx.y;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const float* xp = x + (size_t)b * XR + IAF_XP + t;
    const float x0 = xp[-3], x1 = xp[-2], x2 = xp[-1];
    f4* lp = reinterpret_cast<f4*>(l + (size_t)b * IAF_W * RS) + IAF_LP + t;
    for (int g = 0; g < IAF_W / 4; ++g) {
        f4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * g + e;
            o[e] = wb[3 * IAF_W + c] + wb[c] * x0 + wb[IAF_W + c] * x1 + wb[2 * IAF_W + c] * x2;
        }
        lp[(size_t)g * RS] = o;
    }
}

// ---------------- fused residual layer ----------------
// Buffer-addressed loads: base pointer + size live in a scalar resource descriptor, the
// per-lane part of the address is ONE VGPR per tap that stays constant for a tile, and the
// row (channel) offset is a scalar soffset -- no per-load 64-bit VALU address arithmetic.
__device__ inline float buf_ld(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
// NOTE: pass the value as a plain float.  hipcc (ROCm 7.2) miscompiles
// raw_buffer_store_b32(__builtin_bit_cast(unsigned, vec[r]), ...) on an MFMA accumulator
// vector: every r stores element 0 (seen in the ISA as four stores of a0).
__device__ inline void buf_st(float v, __amdgpu_buffer_rsrc_t r, int voff, int soff) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, voff, soff, 0);
}

// 16-byte accesses of the hoisted fp32 form's residual stream ("Q4" rows: four channels of one sample per word).  The store
// goes through the same guard as every wide residual-stream store of the library (wn_mfma_h.h: buf_st4): gfx950 loses lanes
// of a buffer_store_dwordx4 whose data a VALU instruction overwrites right behind it.
__device__ inline f4 buf_ld16(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
typedef unsigned u4_t __attribute__((ext_vector_type(4)));
template <int AUX = 0>
__device__ inline void buf_st16(f4 v, __amdgpu_buffer_rsrc_t r, int voff, int soff) {
    const u4_t w = __builtin_bit_cast(u4_t, v);
    __builtin_amdgcn_raw_buffer_store_b128(w, r, voff, soff, AUX);
    asm volatile("s_nop 1" ::"v"(w));
}

// One-shot staging of a packed weight image into LDS: ALL loads of a thread are issued
// before the first LDS store (a load->store loop serialises ~30 L2 round trips per thread,
// which cost more than the layer's MFMA time).
template <int NFLOATS>
__device__ inline void stage_weights(const float* __restrict__ wpack, float* lds) {
    constexpr int NF4 = NFLOATS / 4, NCHUNK = NF4 / 256, REM = NF4 - NCHUNK * 256;
    const f4* src = reinterpret_cast<const f4*>(wpack) + threadIdx.x;
    f4* dst = reinterpret_cast<f4*>(lds) + threadIdx.x;
    f4 tmp[NCHUNK + 1];
#pragma unroll
    for (int k = 0; k < NCHUNK; ++k) tmp[k] = src[k * 256];
    if (REM && (int)threadIdx.x < REM) tmp[NCHUNK] = src[NCHUNK * 256];
#pragma unroll
    for (int k = 0; k < NCHUNK; ++k) dst[k * 256] = tmp[k];
    if (REM && (int)threadIdx.x < REM) dst[NCHUNK * 256] = tmp[NCHUNK];
    __syncthreads();
}

// two pieces of a pack (NA floats from srcA, NB from srcB) back to back into LDS, all loads before the first store
template <int NA, int NB, int NT = 256, bool SYNC = true>
__device__ inline void stage_weights_part(const float* __restrict__ srcA, const float* __restrict__ srcB, float* lds) {
    constexpr int NF4 = (NA + NB) / 4, NA4 = NA / 4, NCHUNK = (NF4 + NT - 1) / NT;
    static_assert(NA % 4 == 0 && NB % 4 == 0, "16-byte pieces");
    f4 tmp[NCHUNK];
#pragma unroll
    for (int k = 0; k < NCHUNK; ++k) {
        const int i = k * NT + (int)threadIdx.x;
        if (i < NF4) tmp[k] = i < NA4 ? reinterpret_cast<const f4*>(srcA)[i] : reinterpret_cast<const f4*>(srcB)[i - NA4];
    }
#pragma unroll
    for (int k = 0; k < NCHUNK; ++k) {
        const int i = k * NT + (int)threadIdx.x;
        if (i < NF4) reinterpret_cast<f4*>(lds)[i] = tmp[k];
    }
    if (SYNC) __syncthreads();
}

// LDS-DMA the compiler does not see (16 B per lane: lane i's bytes land at lds_byte_addr + 16 i), issued from inline asm:
// through the builtin every later LDS access of the wave would be preceded by s_waitcnt vmcnt(0) (wn_iaf_g.hip has the
// same helper and the measurement).  Completion is the caller's business: s_waitcnt vmcnt(0) before the barrier.
__device__ inline void f_dma16(const float* gsrc, unsigned lds_byte_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(__builtin_amdgcn_readfirstlane(lds_byte_addr)) : "memory");
}
// `floats` (a multiple of 4) from src to LDS byte address dst, 1 KB per instruction, spread over the workgroup's waves
__device__ inline void f_dma_image(const float* src, unsigned dst, int floats, int wave, int lane, int nwaves) {
    const int full = floats >> 8, rem = (floats & 255) >> 2;
    for (int i = wave; i < full; i += nwaves) f_dma16(src + (size_t)(i * 64 + lane) * 4, dst + i * 1024);
    if (rem && wave == full % nwaves && lane < rem) f_dma16(src + (size_t)(full * 64 + lane) * 4, dst + full * 1024);
}

struct TileSrc {                      // where one wave finds the B operands of one tile
    __amdgpu_buffer_rsrc_t rl, re;    // residual stream rows / upsampled-mel rows of the batch element
    int vo[3];                        // per-lane byte offset for taps t-2d, t-d, t
    int ve;                           // per-lane byte offset into enc
};

// HOIST (round 6): the conditioning 1x1 of every layer and head is evaluated by ONE fp32 GEMM per deconv stack
// (gemm_f32_kernel, wn_iaf_f.hip) and arrives as the term C in the accumulator layout, bias included -- the kernel then
// walks the 12 K-groups of the dilated conv only (K = 192 instead of 448: 53 % of a layer's MACs leave the 60 per-layer
// launches for a GEMM that keeps the matrix pipe busy), its weight image shrinks to 57 KB and it no longer reads enc.
constexpr int IAF_LAYER_F_FLOATS = 12 * 1024 + IAF_PR_FLOATS + 64 + 64;   // hoisted form: dilated-conv K-groups | PR | bgate | bres
constexpr int IAF_HEAD_F_FLOATS = 4 * 1024 + 64 * 3 + 4;   // hoisted form: out1 K-groups | bias, wmean, wscale, bmean / bscale
__device__ inline float softplus_tf(float p);

// LAST (hoisted form): the layer closes a flow and the flow head (parallel_wavenet.py:256-277, :319-324) runs in its epilogue.
// The head is column-local -- out1 over relu(l), relu, two 64-wide dots, softplus, x <- x s + mean, mean_tot / scale_tot --
// and the layer's output words ARE its MFMA B operand as they stand in the registers (channel 16 cg + 4 q + jj of lane group q:
// the K order of the packs): the flow's last l is neither written nor read back and the flow loses a launch (16.8 us each).
struct HeadF {
    const float* whead;      // head pack (out1 K-groups at 0, tail at IAF_PH_FLOATS)
    const float* Ch;         // hoisted term of the head's row block (batch row 0)
    float* x;
    float* Mt;
    float* St;
    int XR;
    int64_t T;
    int first;
};

// Hoisted form: EIGHT waves per workgroup, two per SIMD, one weight image.  The two waves of a SIMD (w and w + 4) take the
// workgroup's tiles alternately: with one wave per SIMD the gate (transcendentals), the dependent start of the residual
// 1x1 and the stores of every tile sat bare between two K loops; now one wave's epilogue runs under the other's MFMAs.
// One utterance is 1 200 tiles on 256 workgroups = 4.69 per SIMD: five rounds either way (3 + 2 per wave pair).
#ifndef WN_F32_NH
#define WN_F32_NH 2
#endif
constexpr int iaf_layer_threads(bool hoist) { return hoist ? 256 * WN_F32_NH : 256; }
// Cache policy of the hoisted form's residual-stream stores: 16 = sc1, written through.  A launch writes 19.7 MB per
// utterance that the NEXT launch reads from every XCD: left dirty in the L2s they are flushed at the kernel boundary, with
// the matrix pipes idle (timing-only ablation: a launch without its stores is 2.65 us shorter); written through as they are
// produced the launch is 1.9 us shorter (25.96 -> 24.03 us under rocprofv3; 3.21 -> 3.07 ms per call, A/B on one box).  The
// same policy on the f16x3 group kernels (WN_G_ST_AUX) costs 4.5 %: their stores are a burst at the end of a long launch.
#ifndef WN_F32_ST_AUX
#define WN_F32_ST_AUX 16
#endif

// START (hoisted form): the layer opens a flow (dilation 1) and computes its own input instead of loading it -- l0 =
// start_conv(shift_right(x)) (parallel_wavenet.py:222-225): l0[c][t'] = b[c] + w0[c] x[t'-3] + w1[c] x[t'-2] + w2[c] x[t'-1],
// 0 left of the utterance -- from five x values per column and the lane's 16 x 4 coefficients held in registers: the flow's first
// l is neither written (iaf_start_q4_kernel, a launch per flow) nor read back (12 of the block's 16 operand loads).
struct StartF {
    const float* x;          // flow input rows [B][XR], IAF_XP zero columns in front
    const float* w;          // start conv: w0[64] | w1[64] | w2[64] | b[64]
    int XR;
};

template <bool HOIST, bool LAST = false, bool START = false>
__global__ __launch_bounds__(iaf_layer_threads(HOIST), 1) void iaf_layer_kernel(
    const float* __restrict__ lin, float* __restrict__ lout, const float* __restrict__ enc,
    const float* __restrict__ wpack, int64_t RS, int64_t TE, int d, int tiles_per_row, int ntiles,
    const float* __restrict__ C, int64_t c_bstride, const HeadF hd, const StartF sf) {
    static_assert(HOIST || !LAST, "the head runs in the epilogue of the hoisted form only");
    static_assert((HOIST && !LAST) || !START, "the start conv runs in front of a plain hoisted layer only");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NG = HOIST ? 12 : 28;                 // K-groups of four K-steps
    constexpr int P_FLOATS = NG * 1024;
    constexpr int NH = HOIST ? WN_F32_NH : 1;           // wave sets that walk the tiles alternately
    // wave-uniform values through readfirstlane: a tile index the compiler takes for divergent makes every buffer
    // descriptor "divergent" and wraps each operand load in a waterfall loop (28 -> 37 us per launch when that happened)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((threadIdx.x >> 6) & 3),
              half = __builtin_amdgcn_readfirstlane(threadIdx.x >> 8);
    const int n = lane & 15, q = lane >> 4;
    const f4* Pl = reinterpret_cast<const f4*>(lds) + lane;
    const f4* PRl = Pl + P_FLOATS / 4;
    const float* bg = lds + P_FLOATS + IAF_PR_FLOATS + q * 16;
    const float* br = bg + 64;
    // fused form: planar rows [64][RS] (4 bytes per column); hoisted form: Q4 rows [16 groups][RS][4] (16 bytes per column)
    constexpr int CB = HOIST ? 16 : 4;                   // bytes per column of a row
    const int RS4 = (int)RS * CB, TE4 = (int)TE * 4;
    const int lane_l = ((HOIST ? q : 4 * q) * (int)RS + wave * 16 + n + IAF_LP) * CB;
    const int lane_e = (4 * q * (int)TE + wave * 16 + n) * 4;
    const int tile0 = (int)blockIdx.x + half * (int)gridDim.x, tstep = NH * (int)gridDim.x;

    auto tile_src = [&](int tile) -> TileSrc {
        const int b = tile / tiles_per_row;
        const int tt = (tile - b * tiles_per_row) * 64;
        TileSrc s;
        s.rl = __builtin_amdgcn_make_buffer_rsrc((void*)(lin + (size_t)b * IAF_W * RS), 0, IAF_W * (int)RS * 4, 0x00020000);
        s.re = __builtin_amdgcn_make_buffer_rsrc((void*)(enc + (size_t)b * IAF_CD * TE), 0, 0x7ffffff0, 0x00020000);
        s.vo[0] = lane_l + (tt - 2 * d) * CB;
        s.vo[1] = lane_l + (tt - d) * CB;
        s.vo[2] = lane_l + tt * CB;
        s.ve = lane_e + tt * 4;
        return s;
    };
    // hoisted term of this wave's column block of a tile: [row block][t / 16][mb][lane][4], one 16-byte load per mb
    auto load_c = [&](int tile, f4 (&cv)[4], const float* Cb = nullptr) {
        const int b = tile / tiles_per_row;
        const int cb = (tile - b * tiles_per_row) * 4 + wave;
        const f4* cp = reinterpret_cast<const f4*>((Cb ? Cb : C) + (size_t)b * c_bstride) + (size_t)cb * 256 + lane;
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) cv[mb] = __builtin_nontemporal_load(cp + mb * 64);
    };
    // 28 K-groups of 4 K-steps (16 MFMAs each): groups 0-11 = the three causal taps t-2d,
    // t-d, t of the dilated conv (4 groups of 16 channels each), groups 12-27 = the
    // conditioning 1x1 over the 256 upsampled-mel channels (not in the hoisted form).
    auto loadB = [&](const TileSrc& s, int g) -> f4 {
        f4 v;
        if (HOIST) return buf_ld16(s.rl, s.vo[g >> 2], 4 * (g & 3) * RS4);     // group row 4 cg + q: one word = the K-group's operand
        if (g < 12) {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) v[jj] = buf_ld(s.rl, s.vo[g >> 2], (16 * (g & 3) + jj) * RS4);
        } else {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) v[jj] = buf_ld(s.re, s.ve, (16 * (g - 12) + jj) * TE4);
        }
        return v;
    };
    // START: the lane's coefficients (channels 16 cg + 4 q + jj) and the operand of K-group g (tap t - 2 + g / 4) from
    // xv[j] = x[t - 5 + j]; the expression is iaf_start_q4_kernel's, term for term
    f4 sw0[4], sw1[4], sw2[4], sbs[4];
    if (START) {
#pragma unroll
        for (int cg = 0; cg < 4; ++cg)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int c = 16 * cg + 4 * q + jj;
                sw0[cg][jj] = sf.w[c];
                sw1[cg][jj] = sf.w[IAF_W + c];
                sw2[cg][jj] = sf.w[2 * IAF_W + c];
                sbs[cg][jj] = sf.w[3 * IAF_W + c];
            }
    }
    struct XV { float v[5]; int t; };
    auto load_x = [&](int tile) -> XV {
        const int b = tile / tiles_per_row;
        const int t = (tile - b * tiles_per_row) * 64 + wave * 16 + n;
        const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(sf.x + (size_t)b * sf.XR), 0, sf.XR * 4, 0x00020000);
        XV r;
        r.t = t;
#pragma unroll
        for (int j = 0; j < 5; ++j) r.v[j] = buf_ld(rx, (IAF_XP + t - 5 + j) * 4, 0);
        return r;
    };
    auto start_op = [&](const XV& xv, int g) -> f4 {
        const int k = g >> 2, cg = g & 3;
        f4 o;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
            o[jj] = sbs[cg][jj] + sw0[cg][jj] * xv.v[k] + sw1[cg][jj] * xv.v[k + 1] + sw2[cg][jj] * xv.v[k + 2];
        return xv.t - 2 + k >= 0 ? o : (f4){0.f, 0.f, 0.f, 0.f};
    };
    // The f32 MFMA is slow (32 cycles per instruction per SIMD) and this kernel runs one wave
    // per SIMD, so memory latency is hidden by distance, not occupancy: as soon as K-group g of
    // tile i has been multiplied, the B operands of group g of the wave's NEXT tile are loaded
    // into the same registers -- every load is issued one whole tile (~15k cycles) before its
    // use, with a single 112-register operand set and no copies.  Weights (A) are read from
    // LDS one K-group ahead into the other half of a register double buffer.
    f4 bcur[NG], ccur[4], hcur[4];
    if (HOIST) {
        // the weight image by LDS-DMA, requested FIRST (no registers, no wait): the image of the hoisted form skips the 16
        // conditioning K-groups of the pack; LAST: the head's image behind it.  It lands while the first tile's operands load.
        const unsigned lds_base = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) float*)lds);
        const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        constexpr int NWV = 4 * NH;
        f_dma_image(wpack, lds_base, 12 * 1024, wv, lane, NWV);
        f_dma_image(wpack + IAF_P_FLOATS, lds_base + 12 * 1024 * 4, IAF_PR_FLOATS + 128, wv, lane, NWV);
        if (LAST) {
            f_dma_image(hd.whead, lds_base + IAF_LAYER_F_FLOATS * 4, 4 * 1024, wv, lane, NWV);
            f_dma_image(hd.whead + IAF_PH_FLOATS, lds_base + (IAF_LAYER_F_FLOATS + 4 * 1024) * 4, 64 * 3 + 4, wv, lane, NWV);
        }
    }
    XV xn{};
    if (tile0 < ntiles) {
        const TileSrc s0 = tile_src(tile0);
        if (START) {
            xn = load_x(tile0);
#pragma unroll
            for (int g = 0; g < NG; ++g) bcur[g] = start_op(xn, g);
        } else {
#pragma unroll
            for (int g = 0; g < NG; ++g) bcur[g] = loadB(s0, g);
        }
        if (HOIST) load_c(tile0, ccur);
        if (LAST) load_c(tile0, hcur, hd.Ch);
    }
    if (HOIST) {
        // the DMA requests are older than the tile loads and vmcnt retires in order: waiting for everything is the wait
        // for the tile's operands, which the first K-group needs anyway
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    } else {
        // the weight image AFTER the first tile's operand loads are in flight (the two latencies overlap)
        stage_weights<IAF_LAYER_FLOATS>(wpack, lds);
    }
    for (int tile = tile0; tile < ntiles; tile += tstep) {
        const int b = tile / tiles_per_row;
        const int tt = (tile - b * tiles_per_row) * 64;
        const int next = tile + tstep;
        const bool has_next = next < ntiles;
        const TileSrc sn = tile_src(has_next ? next : tile);

        f4 acc[4], cur[4], a[2][4];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) acc[mb] = HOIST ? ccur[mb] : *reinterpret_cast<const f4*>(bg + mb * 4);
        if (HOIST && has_next) load_c(next, ccur);
        if (START) xn = load_x(has_next ? next : tile);
        f4 hacc[4];
        if (LAST) {
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) hacc[mb] = hcur[mb];
            if (has_next) load_c(next, hcur, hd.Ch);
        }
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) a[0][mb] = Pl[mb * 64];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g + 1 < NG) {
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) a[(g + 1) & 1][mb] = Pl[((g + 1) * 4 + mb) * 64];
            }
            if (g >= 8 && g < 12) cur[g - 8] = bcur[g];      // tap t is also the residual C-in
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) acc[mb] = mfma4(a[g & 1][mb][jj], bcur[g][jj], acc[mb]);
            // pin the order inside the group: next group's 4 LDS weight reads FIRST (so their
            // latency hides under this group's 16 MFMAs), then the MFMAs
            __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
            // START: the next tile's operands from its x values, four groups behind the loads issued at the top of this tile
            // (their round trip) -- group g - 4 here, the last four behind the loop
            if (START) { if (g >= 4) bcur[g - 4] = start_op(xn, g - 4); }
            else if (has_next) bcur[g] = loadB(sn, g);
            // keep the schedule group-by-group: without this fence the scheduler hoists every
            // LDS weight read of the unrolled loop to the top and spills hundreds of registers
            __builtin_amdgcn_sched_barrier(0);
        }
        if (START) {
#pragma unroll
            for (int g = NG - 4; g < NG; ++g) bcur[g] = start_op(xn, g);
        }
        // gate: sigmoid(first half) * tanh(second half)  (parallel_wavenet.py:246-250)
        f4 gt[2];
#pragma unroll
        for (int mg = 0; mg < 2; ++mg)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                gt[mg][r] = sigmoidf_(acc[mg][r]) * tanhf_(acc[mg + 2][r]);
        // residual 1x1 accumulated onto l: the tap-t operands (groups 8-11) are the C-in
        f4 d2[4];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) d2[mb] = cur[mb] + *reinterpret_cast<const f4*>(br + mb * 4);
#pragma unroll
        for (int j4 = 0; j4 < 2; ++j4) {
            f4 ar[4];
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) ar[mb] = PRl[(j4 * 4 + mb) * 64];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) d2[mb] = mfma4(ar[mb][jj], gt[j4][jj], d2[mb]);
        }
        if (LAST) {
            // flow head on the registers: out1 over relu(l') on top of the head's hoisted tile, then the two projections
            const f4* PHl = reinterpret_cast<const f4*>(lds + IAF_LAYER_F_FLOATS) + lane;
            const float* ht = lds + IAF_LAYER_F_FLOATS + 4 * 1024;
            const float* wm = ht + 64 + q * 16;
            const float* wsc = wm + 64;
#pragma unroll
            for (int cg = 0; cg < 4; ++cg) {
                f4 ah[4];
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) ah[mb] = PHl[(cg * 4 + mb) * 64];
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const float bv = fmaxf(d2[cg][jj], 0.f);                           // relu(l), :256
#pragma unroll
                    for (int mb = 0; mb < 4; ++mb) hacc[mb] = mfma4(ah[mb][jj], bv, hacc[mb]);
                }
            }
            float pm = 0.f, ps = 0.f;
#pragma unroll
            for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float o = fmaxf(hacc[mb][r], 0.f);
                    pm = fmaf(wm[mb * 4 + r], o, pm);
                    ps = fmaf(wsc[mb * 4 + r], o, ps);
                }
            pm += __shfl_xor(pm, 16);
            ps += __shfl_xor(ps, 16);
            pm += __shfl_xor(pm, 32);
            ps += __shfl_xor(ps, 32);
            if (q == 0) {
                const int64_t t = tt + wave * 16 + n;
                const float mean = pm + ht[192];
                const float sc = fminf(fmaxf(softplus_tf(ps + ht[193]), EXP_M9), EXP_7);   // :105-114
                float* xp = hd.x + (size_t)b * hd.XR + IAF_XP + t;
                *xp = *xp * sc + mean;                                                  // :277
                float* mp = hd.Mt + (size_t)b * hd.T + t;
                float* sp = hd.St + (size_t)b * hd.T + t;
                if (hd.first) { *mp = mean; *sp = sc; }
                else { *mp = mean + *mp * sc; *sp = *sp * sc; }                         // :322-323
            }
            continue;
        }
        const __amdgpu_buffer_rsrc_t ro =
            __builtin_amdgcn_make_buffer_rsrc((void*)(lout + (size_t)b * IAF_W * RS), 0, IAF_W * (int)RS * 4, 0x00020000);
        const int vo_out = lane_l + tt * CB;
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {
            if (HOIST) {                                   // channels 16 mb + 4 q + (0..3) = one word of group row 4 mb + q
                buf_st16<WN_F32_ST_AUX>(d2[mb], ro, vo_out, 4 * mb * RS4);
                continue;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) buf_st(d2[mb][r], ro, vo_out, (16 * mb + r) * RS4);
        }
    }
}

// ---------------- flow head (parallel_wavenet.py:256-277, :319-324) ----------------
__device__ inline float softplus_tf(float p) {
    // tf.nn.softplus (Eigen): threshold = log(eps) + 2
    const float thr = -13.942384719848633f;
    if (p > -thr) return p;
    if (p < thr) return expf(p);
    return log1pf(expf(p));
}

template <bool HOIST>
__global__ __launch_bounds__(256, 1) void iaf_head_kernel(
    const float* __restrict__ lin, const float* __restrict__ enc, const float* __restrict__ wpack,
    float* __restrict__ x, float* __restrict__ Mt, float* __restrict__ St,
    int64_t RS, int64_t TE, int XR, int64_t T, int first, int tiles_per_row, int ntiles,
    const float* __restrict__ C, int64_t c_bstride) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NG = HOIST ? 4 : 20;
    constexpr int PH_FLOATS = NG * 1024;
    if (HOIST) stage_weights_part<4 * 1024, 64 * 3 + 4>(wpack, wpack + IAF_PH_FLOATS, lds);
    else stage_weights<IAF_HEAD_FLOATS>(wpack, lds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 15, q = lane >> 4;
    const f4* Pl = reinterpret_cast<const f4*>(lds) + lane;
    const float* bo = lds + PH_FLOATS + q * 16;
    const float* wm = bo + 64;
    const float* wsc = wm + 64;
    const float bmean = lds[PH_FLOATS + 192], bscale = lds[PH_FLOATS + 193];
    constexpr int CB = HOIST ? 16 : 4;                   // bytes per column of an l row (Q4 rows in the hoisted form)
    const int RS4 = (int)RS * CB, TE4 = (int)TE * 4;
    const int lane_l = ((HOIST ? q : 4 * q) * (int)RS + wave * 16 + n + IAF_LP) * CB;
    const int lane_e = (4 * q * (int)TE + wave * 16 + n) * 4;

    // 20 K-groups: 0-3 = out1 over relu(l), 4-19 = mel_cond_out1 over the 256 enc channels (hoisted form: those arrive
    // in C, bias included); same one-tile-ahead operand prefetch as iaf_layer_kernel.
    auto tile_src = [&](int tile) -> TileSrc {
        const int b = tile / tiles_per_row;
        const int tt = (tile - b * tiles_per_row) * 64;
        TileSrc s;
        s.rl = __builtin_amdgcn_make_buffer_rsrc((void*)(lin + (size_t)b * IAF_W * RS), 0, IAF_W * (int)RS * 4, 0x00020000);
        s.re = __builtin_amdgcn_make_buffer_rsrc((void*)(enc + (size_t)b * IAF_CD * TE), 0, 0x7ffffff0, 0x00020000);
        s.vo[0] = s.vo[1] = s.vo[2] = lane_l + tt * CB;
        s.ve = lane_e + tt * 4;
        return s;
    };
    auto load_c = [&](int tile, f4 (&cv)[4]) {
        const int b = tile / tiles_per_row;
        const int cb = (tile - b * tiles_per_row) * 4 + wave;
        const f4* cp = reinterpret_cast<const f4*>(C + (size_t)b * c_bstride) + (size_t)cb * 256 + lane;
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) cv[mb] = __builtin_nontemporal_load(cp + mb * 64);
    };
    auto loadB = [&](const TileSrc& s, int g) -> f4 {
        f4 v;
        if (HOIST) return buf_ld16(s.rl, s.vo[2], 4 * g * RS4);
        if (g < 4) {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) v[jj] = buf_ld(s.rl, s.vo[2], (16 * g + jj) * RS4);
        } else {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) v[jj] = buf_ld(s.re, s.ve, (16 * (g - 4) + jj) * TE4);
        }
        return v;
    };
    f4 bcur[NG], ccur[4];
    if ((int)blockIdx.x < ntiles) {
        const TileSrc s0 = tile_src(blockIdx.x);
#pragma unroll
        for (int g = 0; g < NG; ++g) bcur[g] = loadB(s0, g);
        if (HOIST) load_c(blockIdx.x, ccur);
    }
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int b = tile / tiles_per_row;
        const int t0 = (tile - b * tiles_per_row) * 64 + wave * 16;
        const int next = tile + gridDim.x;
        const bool has_next = next < ntiles;
        const TileSrc sn = tile_src(has_next ? next : tile);
        f4 acc[4], a[2][4];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) acc[mb] = HOIST ? ccur[mb] : *reinterpret_cast<const f4*>(bo + mb * 4);
        if (HOIST && has_next) load_c(next, ccur);
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) a[0][mb] = Pl[mb * 64];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g + 1 < NG) {
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) a[(g + 1) & 1][mb] = Pl[((g + 1) * 4 + mb) * 64];
            }
            f4 bv = bcur[g];
            if (g < 4) {
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) bv[jj] = fmaxf(bv[jj], 0.f);        // relu(l), :256
            }
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) acc[mb] = mfma4(a[g & 1][mb][jj], bv[jj], acc[mb]);
            __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
            if (has_next) bcur[g] = loadB(sn, g);
            __builtin_amdgcn_sched_barrier(0);
        }
        float pm = 0.f, ps = 0.f;
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float o = fmaxf(acc[mb][r], 0.f);
                pm = fmaf(wm[mb * 4 + r], o, pm);
                ps = fmaf(wsc[mb * 4 + r], o, ps);
            }
        pm += __shfl_xor(pm, 16);
        ps += __shfl_xor(ps, 16);
        pm += __shfl_xor(pm, 32);
        ps += __shfl_xor(ps, 32);
        if (q == 0) {
            const int64_t t = t0 + n;
            const float mean = pm + bmean;
            const float s = fminf(fmaxf(softplus_tf(ps + bscale), EXP_M9), EXP_7);   // :105-114
            float* xp = x + (size_t)b * XR + IAF_XP + t;
            *xp = *xp * s + mean;                                                    // :277
            float* mp = Mt + (size_t)b * T + t;
            float* sp = St + (size_t)b * T + t;
            if (first) { *mp = mean; *sp = s; }
            else { *mp = mean + *mp * s; *sp = *sp * s; }                            // :322-323
        }
    }
}

}  // namespace

// ---------------------------------------------------------------------------
int wn_pack_iaf(wn_handle* h, std::vector<float>& blob) {
    const wn_config& c = h->cfg;
    auto var = [&](const std::string& nme) -> const std::vector<float>& { return h->vars.at(nme).data; };
    for (int k = 0; k < c.n_flows; ++k) {
        const std::string p = "iaf_" + std::to_string(k + 1);
        IafFlowPack fp;
        fp.deconv_stack = c.share_deconv ? 0 : k;
        // start conv: W [1,3,1,64] -> w[tap][c], then bias
        blob.resize(align_up(blob.size(), 64));
        fp.start_off = blob.size();
        {
            std::vector<float> W = wn_get_kernel(h, p + "/start_conv", "W", false);
            blob.insert(blob.end(), W.begin(), W.end());
            const auto& b = var(p + "/start_conv/biases");
            blob.insert(blob.end(), b.begin(), b.end());
        }
        for (int i = 0; i < c.iaf_layers[k]; ++i) {
            const std::string s = std::to_string(i + 1);
            std::vector<float> Wd = wn_get_kernel(h, p + "/dilated_conv_" + s, "W", false);   // [3][64][64]
            std::vector<float> Wc = wn_get_kernel(h, p + "/mel_cond_" + s, "W", false);       // [256][64]
            std::vector<float> Wr = wn_get_kernel(h, p + "/res_" + s, "W", false);            // [32][64]
            const auto& bd = var(p + "/dilated_conv_" + s + "/biases");
            const auto& bc = var(p + "/mel_cond_" + s + "/biases");
            const auto& br = var(p + "/res_" + s + "/biases");
            IafLayerPack lp;
            lp.dilation = 1 << (i % c.num_stages);          // parallel_wavenet.py:228
            blob.resize(align_up(blob.size(), 64));
            lp.off = blob.size();
            blob.resize(blob.size() + IAF_LAYER_FLOATS);
            float* P = blob.data() + lp.off;
            float* PR = P + IAF_P_FLOATS;
            float* bg = PR + IAF_PR_FLOATS;
            float* brp = bg + 64;
            for (int ks = 0; ks < 112; ++ks) {
                const int seg = ks / 16, j = ks % 16;
                for (int mb = 0; mb < 4; ++mb)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int i16 = lane & 15, q = lane >> 4;
                        const int o = 16 * mb + i16;
                        const int kch = 16 * (j >> 2) + 4 * q + (j & 3);
                        const float v = seg < 3 ? Wd[((size_t)seg * 64 + kch) * 64 + o]
                                                : Wc[((size_t)(seg - 3) * 64 + kch) * 64 + o];
                        P[((((ks >> 2) * 4 + mb) * 64) + lane) * 4 + (ks & 3)] = v;
                    }
            }
            for (int j = 0; j < 8; ++j)
                for (int mb = 0; mb < 4; ++mb)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int i16 = lane & 15, q = lane >> 4;
                        const int o = 16 * mb + i16;
                        const int cch = 16 * (j >> 2) + 4 * q + (j & 3);
                        PR[((((j >> 2) * 4 + mb) * 64) + lane) * 4 + (j & 3)] = Wr[(size_t)cch * 64 + o];
                    }
            for (int q = 0; q < 4; ++q)
                for (int mb = 0; mb < 4; ++mb)
                    for (int r = 0; r < 4; ++r) {
                        const int o = 16 * mb + 4 * q + r;
                        bg[q * 16 + mb * 4 + r] = bd[o] + bc[o];
                        brp[q * 16 + mb * 4 + r] = br[o];
                    }
            fp.layers.push_back(lp);
        }
        // head
        {
            std::vector<float> Wo = wn_get_kernel(h, p + "/out1", "W", false);            // [64][64]
            std::vector<float> Wco = wn_get_kernel(h, p + "/mel_cond_out1", "W", false);  // [256][64]
            std::vector<float> Wm = wn_get_kernel(h, p + "/out2_mean", "W", false);       // [64][1]
            std::vector<float> Ws = wn_get_kernel(h, p + "/out2_scale", "W", false);
            const auto& bo = var(p + "/out1/biases");
            const auto& bco = var(p + "/mel_cond_out1/biases");
            blob.resize(align_up(blob.size(), 64));
            fp.head_off = blob.size();
            blob.resize(blob.size() + IAF_HEAD_FLOATS);
            float* P = blob.data() + fp.head_off;
            float* tb = P + IAF_PH_FLOATS;
            for (int ks = 0; ks < 80; ++ks) {
                const int seg = ks / 16, j = ks % 16;
                for (int mb = 0; mb < 4; ++mb)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int i16 = lane & 15, q = lane >> 4;
                        const int o = 16 * mb + i16;
                        const int kch = 16 * (j >> 2) + 4 * q + (j & 3);
                        const float v = seg == 0 ? Wo[(size_t)kch * 64 + o]
                                                 : Wco[((size_t)(seg - 1) * 64 + kch) * 64 + o];
                        P[((((ks >> 2) * 4 + mb) * 64) + lane) * 4 + (ks & 3)] = v;
                    }
            }
            for (int q = 0; q < 4; ++q)
                for (int mb = 0; mb < 4; ++mb)
                    for (int r = 0; r < 4; ++r) {
                        const int o = 16 * mb + 4 * q + r;
                        tb[q * 16 + mb * 4 + r] = bo[o] + bco[o];
                        tb[64 + q * 16 + mb * 4 + r] = Wm[o];
                        tb[128 + q * 16 + mb * 4 + r] = Ws[o];
                    }
            tb[192] = var(p + "/out2_mean/biases")[0];
            tb[193] = var(p + "/out2_scale/biases")[0];
            tb[194] = tb[195] = 0.f;
        }
        h->flows.push_back(fp);
    }
    // row-block table of the fp32 conditioning GEMM (wn_iaf_f.hip): the 16 cond K-groups of each pack (layer: K-groups
    // 12-27, head: 4-19) are contiguous 16 x 1024 floats; the biases (dilated + cond / out1 + cond) sit in lane order
    // behind the fragments
    {
        std::vector<unsigned> tab;
        for (const IafFlowPack& fp : h->flows) {
            for (const IafLayerPack& lp : fp.layers) {
                tab.push_back((unsigned)(lp.off + 12 * 1024));
                tab.push_back((unsigned)(lp.off + IAF_P_FLOATS + IAF_PR_FLOATS));
            }
            tab.push_back((unsigned)(fp.head_off + 4 * 1024));
            tab.push_back((unsigned)(fp.head_off + IAF_PH_FLOATS));
        }
        if (blob.size() >= 0x1ff00000u) return wn_fail(h, WN_EINVAL, "weight blob too large");
        blob.resize(align_up(blob.size(), 64));
        h->cond_tab_f_off = blob.size();
        blob.resize(blob.size() + align_up(tab.size(), 4));
        memcpy(blob.data() + h->cond_tab_f_off, tab.data(), tab.size() * sizeof(unsigned));
    }
    return WN_OK;
}

// ---------------------------------------------------------------------------
// Launches, plain arguments (as wn_iaf_c_layer / wn_iaf_h_head): persistent workgroups over the 64-sample tiles of B rows.
// The hoisted kernels start their accumulators from the C rows instead of streaming enc.
namespace {

template <bool HOIST, bool LAST = false, bool START = false>
void launch_layer(const float* lin, float* lout, const float* enc, int64_t TE, const float* C, int64_t c_bstride,
                  const float* wpack, int64_t RS, int d, int B, int64_t T, int num_cu, hipStream_t st,
                  const HeadF& hd = HeadF{}, const StartF& sf = StartF{}) {
    constexpr size_t lds = (HOIST ? IAF_LAYER_F_FLOATS + (LAST ? IAF_HEAD_F_FLOATS : 0) : IAF_LAYER_FLOATS) * sizeof(float);
    const int tiles_per_row = (int)(T / 64), ntiles = B * tiles_per_row;
    hipLaunchKernelGGL((iaf_layer_kernel<HOIST, LAST, START>), dim3(std::min(ntiles, num_cu)), dim3(iaf_layer_threads(HOIST)),
                       lds, st, lin, lout, enc, wpack, RS, TE, d, tiles_per_row, ntiles, C, c_bstride, hd, sf);
}
template <bool HOIST>
void launch_head(const float* lin, const float* enc, int64_t TE, const float* C, int64_t c_bstride, const float* wpack,
                 float* x, float* Mt, float* St, int64_t RS, int XR, int64_t T, int first, int B, int num_cu, hipStream_t st) {
    const int tiles_per_row = (int)(T / 64), ntiles = B * tiles_per_row;
    hipLaunchKernelGGL(iaf_head_kernel<HOIST>, dim3(std::min(ntiles, num_cu)), dim3(256),
                       (HOIST ? IAF_HEAD_F_FLOATS : IAF_HEAD_FLOATS) * sizeof(float), st, lin, enc, wpack, x, Mt, St, RS, TE, XR,
                       T, first, tiles_per_row, ntiles, C, c_bstride);
}

}  // namespace

void wn_iaf_f32_start(const float* x, const float* wb, float* l, int64_t T, int XR, int64_t RS, int B, bool q4, hipStream_t st) {
    if (q4)
        hipLaunchKernelGGL(iaf_start_q4_kernel, dim3((unsigned)((T + 255) / 256), B), dim3(256), 0, st, x, wb, l, T, XR, RS);
    else
        hipLaunchKernelGGL(iaf_start_kernel, dim3((unsigned)((T / 4 + 255) / 256), B), dim3(256), 0, st, x, wb, l, T, XR, RS);
}

void wn_iaf_f32_layer(const float* lin, float* lout, const float* enc, const float* wpack, int64_t RS, int64_t TE, int c0,
                      int d, int B, int64_t T, int num_cu, hipStream_t st) {
    launch_layer<false>(lin, lout, enc + c0, TE, nullptr, 0, wpack, RS, d, B, T, num_cu, st);
}

void wn_iaf_f32_layer_c(const float* lin, float* lout, const float* C, int64_t c_bstride, const float* wpack, int64_t RS,
                        int d, int B, int64_t T, int num_cu, hipStream_t st, const float* x, int XR, const float* wstart) {
    if (x) launch_layer<true, false, true>(lin, lout, nullptr, 0, C, c_bstride, wpack, RS, d, B, T, num_cu, st, HeadF{},
                                           StartF{x, wstart, XR});
    else launch_layer<true>(lin, lout, nullptr, 0, C, c_bstride, wpack, RS, d, B, T, num_cu, st);
}

void wn_iaf_f32_layer_head(const float* lin, const float* C, const float* Ch, int64_t c_bstride, const float* wpack,
                           const float* wpack_head, float* x, float* Mt, float* St, int64_t RS, int XR, int d, int first,
                           int B, int64_t T, int num_cu, hipStream_t st) {
    launch_layer<true, true>(lin, nullptr, nullptr, 0, C, c_bstride, wpack, RS, d, B, T, num_cu, st,
                             HeadF{wpack_head, Ch, x, Mt, St, XR, T, first});
}

void wn_iaf_f32_head(const float* lin, const float* enc, const float* wpack, float* x, float* Mt, float* St, int64_t RS,
                     int64_t TE, int c0, int XR, int64_t T, int first, int B, int num_cu, hipStream_t st) {
    launch_head<false>(lin, enc + c0, TE, nullptr, 0, wpack, x, Mt, St, RS, XR, T, first, B, num_cu, st);
}

void wn_iaf_f32_head_c(const float* lin, const float* C, int64_t c_bstride, const float* wpack, float* x, float* Mt,
                       float* St, int64_t RS, int XR, int64_t T, int first, int B, int num_cu, hipStream_t st) {
    launch_head<true>(lin, nullptr, 0, C, c_bstride, wpack, x, Mt, St, RS, XR, T, first, B, num_cu, st);
}

int wn_iaf_f32_set_attrs(wn_handle* h) {
    const std::pair<const void*, int> lds_floats[] = {
        {reinterpret_cast<const void*>(iaf_layer_kernel<false, false>), IAF_LAYER_FLOATS},
        {reinterpret_cast<const void*>(iaf_head_kernel<false>), IAF_HEAD_FLOATS},
        {reinterpret_cast<const void*>(iaf_layer_kernel<true, false>), IAF_LAYER_F_FLOATS},
        {reinterpret_cast<const void*>(iaf_layer_kernel<true, false, true>), IAF_LAYER_F_FLOATS},
        {reinterpret_cast<const void*>(iaf_layer_kernel<true, true>), IAF_LAYER_F_FLOATS + IAF_HEAD_F_FLOATS}};
    for (const auto& k : lds_floats)
        WN_HIP(h, hipFuncSetAttribute(k.first, hipFuncAttributeMaxDynamicSharedMemorySize, k.second * sizeof(float)));
    return WN_OK;
}
