// wn_iaf_set_weights: the in-place re-pack of a finalized STUDENT handle from device-resident fp32 masters --
// the generation packs of all three launch forms (wn_pack_iaf_x, or wn_pack_iaf and wn_pack_iaf_h), the training packs of
// wn_pack_iaf_train, and, through wn_train.hip's per-stack code, the forward and backward packs of the deconv stacks.
//
// A student has some hundred packs of a handful of KINDS, so the call is table-driven: the host builds one descriptor array
// per kind (source and destination pointers, dimensions, row and source kind, scale slot), uploads them into the caller's
// workspace and launches one kernel per kind with one workgroup column (blockIdx.y) per descriptor.  The index maps are
// wn_repack.h's, the roundings wn_pack_h.h's; the scales come from exact absolute maxima and the host's pick_scale after the
// call's one read-back, and reach the kernels through a small device table uploaded after it.
#include <memory>

#include "wn_repack.h"

namespace {

// ---- descriptors ----
struct RpAbs {            // amax[slot] = max(amax[slot], max |src[0 .. n)|)
    const float* src;
    unsigned n, slot;
};
struct RpCopy {           // dst[0 .. n) = src[0 .. n)
    const float* src;
    float* dst;
    unsigned n;
    unsigned rb;          // host side only: 1 + index of the read-back float dst stands for until layout() resolves it
};
struct RpFrag32 {         // iaf_frag32_word
    const float *a, *b;
    float* dst;
    int nA, nks;
};
enum { BIAS_LANE = 0, BIAS_TILE = 1 };
struct RpBias {           // dst[i] = a[row(i)] (+ b[row(i)]), a zero for a pad row; row(i): iaf_lane_row or tr_row
    const float *a, *b;
    float* dst;
    int order, n, rowkind, M, H;
    int gate_scaled;      // BIAS_LANE: times -log2 e on sigmoid rows (channels < 32), 2 log2 e on tanh rows (gate_scaled of wn_iaf_h.hip)
};
struct RpTile {           // tr_tile_word under the scale sctab[slot]
    TileArgs a;
    int slot, pad;
};

__global__ __launch_bounds__(TR_NT) void rp_absmax_kernel(const RpAbs* __restrict__ tab, unsigned* __restrict__ amax) {
    const RpAbs d = tab[blockIdx.y];
    tr_absmax_block(d.src, d.n, amax + d.slot, blockIdx.x, gridDim.x);
}
__global__ __launch_bounds__(TR_NT) void rp_copy_kernel(const RpCopy* __restrict__ tab) {
    const RpCopy d = tab[blockIdx.y];
    for (size_t i = (size_t)blockIdx.x * TR_NT + threadIdx.x; i < d.n; i += (size_t)gridDim.x * TR_NT) d.dst[i] = d.src[i];
}
__global__ __launch_bounds__(TR_NT) void rp_frag32_kernel(const RpFrag32* __restrict__ tab) {
    const RpFrag32 d = tab[blockIdx.y];
    iaf_frag32_word(d.a, d.b, d.dst, d.nA, d.nks, (size_t)blockIdx.x * TR_NT + threadIdx.x);
}
__global__ __launch_bounds__(TR_NT) void rp_bias_kernel(const RpBias* __restrict__ tab) {
    const RpBias d = tab[blockIdx.y];
    const int i = blockIdx.x * TR_NT + threadIdx.x;
    if (i >= d.n) return;
    const int row = d.order == BIAS_LANE ? iaf_lane_row(i) : tr_row(d.rowkind, d.M, d.H, i);
    float v = 0.f;
    if (row >= 0) v = d.b ? __fadd_rn(d.a[row], d.b[row]) : d.a[row];
    if (d.gate_scaled) v = __fmul_rn(v, row < 32 ? -1.4426950408889634f : 2.8853900817779268f);
    d.dst[i] = v;
}
__global__ __launch_bounds__(TR_NT) void rp_tile_kernel(const RpTile* __restrict__ tab, const float* __restrict__ sctab) {
    TileArgs a = tab[blockIdx.y].a;
    a.sc = sctab[tab[blockIdx.y].slot];
    tr_tile_word(a, (size_t)blockIdx.x * TR_NT + threadIdx.x);
}

// a scale of the device table: pick_scale of the larger of two maxima (one source matrix cut in two), or the smaller of
// their two scales (wn_pack_iaf_h)
struct ScaleRule {
    int s0, s1;           // amax slots; s1 < 0: none
    bool min_of_picks;
};
// a host float that follows a scale: 1 / scale
struct InvTarget {
    float* host;
    int rule;
};

// Everything the call launches, built on the host from the handle and the base addresses alone (null bases: the size query)
struct Plan {
    std::vector<RpAbs> abs;
    std::vector<RpCopy> copy, post_copy;      // post_copy: 1 / scale words of the split-fp16 blobs, out of the device table
    std::vector<RpFrag32> frag;
    std::vector<RpBias> bias;
    std::vector<RpTile> tile;
    std::vector<ScaleRule> rules;
    std::vector<InvTarget> inv;
    std::vector<int> post_rule;               // rule whose reciprocal post_copy[i] delivers
    std::vector<float> post;                  // the device table's host copy: the scales, then the reciprocals
    int nslots = 0, n_rb = 0;                 // maxima; floats read back besides them (bmean, bscale of every generic flow)
    unsigned max_abs = 0, max_copy = 0, max_frag = 0, max_bias = 0, max_tile = 0;
    // workspace
    size_t o_rb = 0, o_post = 0, o_abs = 0, o_copy = 0, o_pcopy = 0, o_frag = 0, o_bias = 0, o_tile = 0, total = 0;
};

void build_plan(wn_handle* h, const float* params, Plan& P) {
    const wn_config& c = h->cfg;
    const int W = c.width, H = W / 2, Cd = c.deconv_width;
    float* blob = h->d_blob;
    // a source variable: params + its offset in the handle's layout
    auto Wp = [&](const WnConvOff& o) { return params + o.W; };
    auto bp = [&](const WnConvOff& o) { return params + o.b; };
    auto absmax = [&](const float* src, size_t n) {
        P.abs.push_back(RpAbs{src, (unsigned)n, (unsigned)P.nslots});
        P.max_abs = std::max(P.max_abs, (unsigned)n);
        return P.nslots++;
    };
    auto copy = [&](const float* src, float* dst, size_t n) {
        P.copy.push_back(RpCopy{src, dst, (unsigned)n, 0});
        P.max_copy = std::max(P.max_copy, (unsigned)n);
    };
    auto rule = [&](int s0, int s1, bool min_of_picks) {
        P.rules.push_back(ScaleRule{s0, s1, min_of_picks});
        return (int)P.rules.size() - 1;
    };
    auto frag32 = [&](const float* a, const float* b, int nA, size_t dst_off, int nks) {
        P.frag.push_back(RpFrag32{a, b, blob + dst_off, nA, nks});
        P.max_frag = std::max(P.max_frag, (unsigned)nks * 256u);
    };
    auto lane_bias = [&](const float* a, const float* b, size_t dst_off, int gate_scaled) {
        P.bias.push_back(RpBias{a, b, blob + dst_off, BIAS_LANE, 64, 0, 0, 0, gate_scaled});
        P.max_bias = std::max(P.max_bias, 64u);
    };
    // one TeacherGemmPack: the fragments under rule r, the tile-ordered bias (a null: the zeros it was packed with stay)
    auto gemm = [&](TeacherGemmPack& g, int r, int srckind, const float* src, const float* src2, int nA, int ld, int rowkind, int M,
                    const float* ba, const float* bb) {
        TileArgs a{};
        a.src = src; a.src2 = src2; a.nA = nA; a.ld = ld; a.srckind = srckind;
        a.dst = reinterpret_cast<unsigned*>(blob + g.w_off);
        a.nks = g.nks; a.mtiles = g.mtiles; a.rowkind = rowkind; a.M = M; a.H = H; a.W = W;
        P.tile.push_back(RpTile{a, r, 0});
        P.max_tile = std::max(P.max_tile, (unsigned)g.mtiles * g.nks * 2048u);
        P.inv.push_back(InvTarget{&g.inv_scale, r});
        if (ba) {
            P.bias.push_back(RpBias{ba, bb, blob + g.b_off, BIAS_TILE, g.mtiles * 64, rowkind, M, H, 0});
            P.max_bias = std::max(P.max_bias, (unsigned)g.mtiles * 64u);
        }
    };
    // a fragment array of the width-64 split-fp16 packs: pack_tiles' one m-tile of 64 rows
    auto frag_h = [&](size_t dst_off, int r, const float* a, const float* b, int nA, int nks) {
        TileArgs t{};
        t.src = a; t.src2 = b; t.nA = nA; t.ld = 64; t.srckind = SRC_CAT_T;
        t.dst = reinterpret_cast<unsigned*>(blob + dst_off);
        t.nks = nks; t.mtiles = 1; t.rowkind = ROW_IDENT; t.M = 64; t.H = H; t.W = W;
        P.tile.push_back(RpTile{t, r, 0});
        P.max_tile = std::max(P.max_tile, (unsigned)nks * 2048u);
    };
    auto post_inv = [&](size_t dst_off, int r) {
        P.post_copy.push_back(RpCopy{nullptr, blob + dst_off, 1, 0});      // src: inside the device table, set in layout()
        P.post_rule.push_back(r);
    };
    auto read_back = [&](const float* src) {
        P.copy.push_back(RpCopy{src, nullptr, 1, 1u + (unsigned)P.n_rb});
        ++P.n_rb;
    };

    for (int f = 0; f < c.n_flows; ++f) {
        const int nl = c.iaf_layers[f];
        const IafFlowLayout& fo = h->iaf_train.lay.flows[f];
        const std::vector<IafLayerOff>& lo = fo.layers;
        // ---- the absolute maxima, per source variable
        std::vector<int> s_d(nl), s_c(nl), s_r(nl);
        for (int i = 0; i < nl; ++i) {
            s_d[i] = absmax(Wp(lo[i].dil), (size_t)3 * W * W);
            s_c[i] = absmax(Wp(lo[i].cond), (size_t)Cd * W);
            s_r[i] = absmax(Wp(lo[i].res), (size_t)H * W);
        }
        const int s_o = absmax(Wp(fo.out1), (size_t)W * W), s_co = absmax(Wp(fo.cond_out1), (size_t)Cd * W);
        const int s_m = absmax(Wp(fo.out2_mean), W), s_s = absmax(Wp(fo.out2_scale), W);
        // ---- generation packs
        if (h->generic_student) {                        // wn_pack_iaf_x: plain copies; the two head biases are host floats
            IafFlowX& fx = h->flows_x[f];
            copy(Wp(fo.start), blob + fx.start, (size_t)4 * W);      // W [3][1][W] and the biases are neighbours in the table
            for (int i = 0; i < nl; ++i) {
                const IafLayerX& lx = fx.layers[i];
                copy(Wp(lo[i].dil), blob + lx.wd, (size_t)3 * W * W);
                copy(Wp(lo[i].cond), blob + lx.wc, (size_t)Cd * W);
                copy(Wp(lo[i].res), blob + lx.wr, (size_t)H * W);
                copy(bp(lo[i].dil), blob + lx.bd, W);
                copy(bp(lo[i].cond), blob + lx.bc, W);
                copy(bp(lo[i].res), blob + lx.br, W);
            }
            copy(Wp(fo.out1), blob + fx.wo, (size_t)W * W);
            copy(Wp(fo.cond_out1), blob + fx.wco, (size_t)Cd * W);
            copy(bp(fo.out1), blob + fx.bo, W);
            copy(bp(fo.cond_out1), blob + fx.bco, W);
            copy(Wp(fo.out2_mean), blob + fx.wm, W);
            copy(Wp(fo.out2_scale), blob + fx.ws, W);
            read_back(bp(fo.out2_mean));
            read_back(bp(fo.out2_scale));
        } else {                                         // wn_pack_iaf and wn_pack_iaf_h, width 64 and deconv_width 256
            IafFlowPack& fp = h->flows[f];
            copy(Wp(fo.start), blob + fp.start_off, (size_t)4 * W);
            for (int i = 0; i < nl; ++i) {
                const IafLayerPack& lp = fp.layers[i];
                frag32(Wp(lo[i].dil), Wp(lo[i].cond), 3 * IAF_W, lp.off, 112);
                frag32(Wp(lo[i].res), nullptr, IAF_W / 2, lp.off + IAF_P_FLOATS, 8);
                const size_t tb = lp.off + IAF_P_FLOATS + IAF_PR_FLOATS;
                lane_bias(bp(lo[i].dil), bp(lo[i].cond), tb, 0);
                lane_bias(bp(lo[i].res), nullptr, tb + 64, 0);
                const int rm = rule(s_d[i], s_c[i], true), rr = rule(s_r[i], -1, false);
                frag_h(lp.off_h, rm, Wp(lo[i].dil), Wp(lo[i].cond), 3 * IAF_W, 14);
                frag_h(lp.off_h + IAF_P_FLOATS, rr, Wp(lo[i].res), nullptr, IAF_W / 2, 1);
                const size_t th = lp.off_h + IAF_P_FLOATS + IAF_PR_FLOATS;
                lane_bias(bp(lo[i].dil), bp(lo[i].cond), th, 1);
                lane_bias(bp(lo[i].res), nullptr, th + 64, 0);
                post_inv(th + 128, rm);
                post_inv(th + 129, rr);
            }
            for (int form = 0; form < 2; ++form) {       // the head of the fp32 pack, then of the split-fp16 pack
                const size_t head = form == 0 ? fp.head_off : fp.head_off_h, tb = head + IAF_PH_FLOATS;
                if (form == 0) frag32(Wp(fo.out1), Wp(fo.cond_out1), IAF_W, head, 80);
                else {
                    const int rh = rule(s_o, s_co, true);
                    frag_h(head, rh, Wp(fo.out1), Wp(fo.cond_out1), IAF_W, 10);
                    post_inv(tb + 194, rh);
                }
                lane_bias(bp(fo.out1), bp(fo.cond_out1), tb, 0);
                lane_bias(Wp(fo.out2_mean), nullptr, tb + 64, 0);
                lane_bias(Wp(fo.out2_scale), nullptr, tb + 128, 0);
                copy(bp(fo.out2_mean), blob + tb + 192, 1);
                copy(bp(fo.out2_scale), blob + tb + 193, 1);
            }
        }
        // ---- training packs (wn_pack_iaf_train): each scale over the sources the host hands to pick_scale
        IafTrainFlow& fl = h->iaf_train.flows[f];
        copy(Wp(fo.start), blob + fl.start_off, (size_t)4 * W);
        for (int i = 0; i < nl; ++i) {
            IafTrainLayer& tl = fl.layers[i];
            gemm(tl.gate, rule(s_d[i], s_c[i], false), SRC_CAT_T, Wp(lo[i].dil), Wp(lo[i].cond), 3 * W, W, ROW_GATE, W, bp(lo[i].dil),
                 bp(lo[i].cond));
            gemm(tl.res, rule(s_r[i], -1, false), SRC_CAT_T, Wp(lo[i].res), nullptr, H, W, ROW_IDENT, W, bp(lo[i].res), nullptr);
            gemm(tl.gate_t, rule(s_d[i], -1, false), SRC_TAP_T, Wp(lo[i].dil), nullptr, 0, 0, ROW_IDENT, W, nullptr, nullptr);
            gemm(tl.res_t, rule(s_r[i], -1, false), SRC_DIRECT, Wp(lo[i].res), nullptr, 0, W, ROW_IDENT, H, nullptr, nullptr);
            gemm(tl.cond_t, rule(s_c[i], -1, false), SRC_DIRECT, Wp(lo[i].cond), nullptr, 0, W, ROW_IDENT, Cd, nullptr, nullptr);
        }
        gemm(fl.out1, rule(s_o, s_co, false), SRC_CAT_T, Wp(fo.out1), Wp(fo.cond_out1), W, W, ROW_IDENT, W, bp(fo.out1),
             bp(fo.cond_out1));
        const int r2 = rule(s_m, s_s, false);
        gemm(fl.out2, r2, SRC_ROWS2, Wp(fo.out2_mean), Wp(fo.out2_scale), 0, W, ROW_IDENT, 2, nullptr, nullptr);
        copy(bp(fo.out2_mean), blob + fl.out2.b_off, 1);     // its bias rows 0 and 1; the other 62 stay zero
        copy(bp(fo.out2_scale), blob + fl.out2.b_off + 1, 1);
        gemm(fl.out1_t, rule(s_o, -1, false), SRC_DIRECT, Wp(fo.out1), nullptr, 0, W, ROW_IDENT, W, nullptr, nullptr);
        gemm(fl.out2_t, r2, SRC_COLS2, Wp(fo.out2_mean), Wp(fo.out2_scale), 0, 32, ROW_IDENT, W, nullptr, nullptr);
        gemm(fl.cond_out1_t, rule(s_co, -1, false), SRC_DIRECT, Wp(fo.cond_out1), nullptr, 0, W, ROW_IDENT, Cd, nullptr, nullptr);
    }
}

// the workspace: [maxima | read-back floats] [scale table | reciprocals] [the descriptor arrays]
void layout(Plan& P, int n_up_slots, char* ws) {
    size_t o = 0;
    auto carve = [&](size_t bytes) { const size_t r = o; o += align_up(std::max<size_t>(bytes, 4), 256); return r; };
    P.o_rb = carve((size_t)(P.nslots + n_up_slots + P.n_rb) * 4);
    P.o_post = carve((P.rules.size() + P.post_copy.size()) * 4);
    P.o_abs = carve(P.abs.size() * sizeof(RpAbs));
    P.o_copy = carve(P.copy.size() * sizeof(RpCopy));
    P.o_pcopy = carve(P.post_copy.size() * sizeof(RpCopy));
    P.o_frag = carve(P.frag.size() * sizeof(RpFrag32));
    P.o_bias = carve(P.bias.size() * sizeof(RpBias));
    P.o_tile = carve(P.tile.size() * sizeof(RpTile));
    P.total = o;
    // the read-back floats sit behind every maximum, the reciprocals behind the scales
    float* rb = reinterpret_cast<float*>(ws + P.o_rb) + P.nslots + n_up_slots;
    for (RpCopy& d : P.copy)
        if (d.rb) d.dst = rb + (d.rb - 1);
    const float* post = reinterpret_cast<const float*>(ws + P.o_post) + P.rules.size();
    for (size_t i = 0; i < P.post_copy.size(); ++i) P.post_copy[i].src = post + i;
}

int up_slots(const wn_handle* h) {
    int n = 0;
    for (const DeconvStackPack& sp : h->stacks) n += (int)sp.layers.size();
    return n;
}
bool supported(const wn_handle* h) {
    return h && h->finalized && h->cfg.kind == WN_KIND_STUDENT && !h->cfg.use_mu_law && !h->cfg.use_weight_norm && h->iaf_train.ok;
}

template <class D>
int upload(wn_handle* h, const std::vector<D>& v, char* ws, size_t off, hipStream_t st) {
    if (!v.empty()) WN_HIP(h, hipMemcpyAsync(ws + off, v.data(), v.size() * sizeof(D), hipMemcpyHostToDevice, st));
    return WN_OK;
}
inline unsigned grid_x(unsigned words, unsigned cap = 0) {
    const unsigned nb = tr_blocks(std::max(words, 1u));
    return cap ? std::min(nb, cap) : nb;
}

}  // namespace

extern "C" size_t wn_iaf_set_weights_workspace_bytes(const wn_handle* h) {
    if (!supported(h)) return 0;
    Plan P;
    build_plan(const_cast<wn_handle*>(h), nullptr, P);
    layout(P, up_slots(h), nullptr);
    return P.total;
}

extern "C" int wn_iaf_set_weights(wn_handle* h, const float* params, size_t params_floats, const float* const* up_params,
                                  const size_t* up_floats, int n_up, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "wn_iaf_set_weights";
    if (h && h->cfg.kind != WN_KIND_STUDENT)
        return wn_fail(h, WN_EINVAL, "%s: this is a teacher handle; wn_teacher_set_weights re-packs a teacher", fn);
    if (int rc = wn_iaf_train_check(h, fn)) return rc;
    if (!params || !ws) return wn_fail(h, WN_EINVAL, "%s: null argument", fn);
    const wn_config& c = h->cfg;
    if (params_floats != h->iaf_train.lay.table.floats)
        return wn_fail(h, WN_EINVAL, "%s: params holds %zu floats, the layout of wn_iaf_grad_info has %zu", fn, params_floats,
                       h->iaf_train.lay.table.floats);
    const int NS = (int)h->stacks.size();
    if (n_up != 0 && n_up != NS)
        return wn_fail(h, WN_EINVAL, "%s: n_up = %d, the student has %d deconv stack%s (or pass 0)", fn, n_up, NS, NS == 1 ? "" : "s");
    if (n_up && (!up_params || !up_floats)) return wn_fail(h, WN_EINVAL, "%s: null argument", fn);
    for (int s = 0; s < n_up; ++s) {
        if (!up_params[s]) continue;
        const std::string& scope = h->stacks[s].prefix;
        if (c.use_resize_conv)
            return wn_fail(h, WN_EINVAL, "%s: use_resize_conv: the resize-conv upsampler has no parameter layout; pass no up_params", fn);
        if (wn_deconv_grad_floats(h, scope.c_str()) == 0)
            return wn_fail(h, WN_EINVAL, "%s: the upsampler '%s' has no parameter layout (wn_deconv_grad_floats is 0)", fn, scope.c_str());
        if (up_floats[s] != h->stacks[s].table.floats)
            return wn_fail(h, WN_EINVAL, "%s: up_params[%d] holds %zu floats, the layout of wn_deconv_grad_info has %zu", fn, s,
                           up_floats[s], h->stacks[s].table.floats);
    }
    // the tables and the scale table are read by asynchronous uploads: the handle keeps them until its next re-pack
    std::shared_ptr<Plan> keep = std::make_shared<Plan>();
    Plan& P = *keep;
    char* wsb = reinterpret_cast<char*>(ws);
    build_plan(h, params, P);
    const int NU = up_slots(h);
    layout(P, NU, wsb);
    if (ws_bytes < P.total) return wn_fail(h, WN_EINVAL, "%s: workspace %zu < %zu bytes", fn, ws_bytes, P.total);
    WN_SWITCH(h, "wn_iaf_set_weights");

    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // From here on the handle changes: tapes written under the old weights are refused, also after a failure below
    h->iaf_train.serial = wn_repack_serial_next();
    h->repack_keep = keep;

    // ---- 1. the descriptor tables; the maxima; every part that needs no scale
    unsigned* amax = reinterpret_cast<unsigned*>(wsb + P.o_rb);
    const int n_rb_all = P.nslots + NU + P.n_rb;
    WN_HIP(h, hipMemsetAsync(amax, 0, (size_t)n_rb_all * 4, st));
    if (int rc = upload(h, P.abs, wsb, P.o_abs, st)) return rc;
    if (int rc = upload(h, P.copy, wsb, P.o_copy, st)) return rc;
    if (int rc = upload(h, P.post_copy, wsb, P.o_pcopy, st)) return rc;
    if (int rc = upload(h, P.frag, wsb, P.o_frag, st)) return rc;
    if (int rc = upload(h, P.bias, wsb, P.o_bias, st)) return rc;
    if (int rc = upload(h, P.tile, wsb, P.o_tile, st)) return rc;
    hipLaunchKernelGGL(rp_absmax_kernel, dim3(grid_x((P.max_abs + 3) / 4, 16), (unsigned)P.abs.size()), dim3(TR_NT), 0, st,
                       reinterpret_cast<const RpAbs*>(wsb + P.o_abs), amax);
    hipLaunchKernelGGL(rp_copy_kernel, dim3(grid_x(P.max_copy, 64), (unsigned)P.copy.size()), dim3(TR_NT), 0, st,
                       reinterpret_cast<const RpCopy*>(wsb + P.o_copy));
    if (!P.frag.empty())
        hipLaunchKernelGGL(rp_frag32_kernel, dim3(grid_x(P.max_frag), (unsigned)P.frag.size()), dim3(TR_NT), 0, st,
                           reinterpret_cast<const RpFrag32*>(wsb + P.o_frag));
    hipLaunchKernelGGL(rp_bias_kernel, dim3(grid_x(P.max_bias), (unsigned)P.bias.size()), dim3(TR_NT), 0, st,
                       reinterpret_cast<const RpBias*>(wsb + P.o_bias));
    int slot0 = P.nslots;
    std::vector<int> up_slot0(NS, 0);
    for (int s = 0; s < n_up; ++s) {
        up_slot0[s] = slot0;
        slot0 += (int)h->stacks[s].layers.size();
        if (!up_params[s]) continue;
        wn_repack_deconv_absmax(h->stacks[s], up_params[s], amax + up_slot0[s], st);
        wn_repack_deconv_plain(h, h->stacks[s], up_params[s], st);
    }

    // ---- 2. the maxima and the generic flows' head biases come back (the call's one read-back: it synchronises the stream)
    std::vector<float> mx(n_rb_all);
    WN_HIP(h, hipMemcpyAsync(mx.data(), amax, mx.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    WN_HIP(h, hipStreamSynchronize(st));
    std::vector<float>& post = P.post;
    post.resize(P.rules.size() + P.post_copy.size());
    for (size_t r = 0; r < P.rules.size(); ++r) {
        const ScaleRule& q = P.rules[r];
        const float a = mx[q.s0], b = q.s1 >= 0 ? mx[q.s1] : 0.f;
        if (q.min_of_picks) post[r] = std::min(pick_scale(&a, 1), pick_scale(&b, 1));
        else { const float m = std::max(a, b); post[r] = pick_scale(&m, 1); }
    }
    for (size_t i = 0; i < P.post_copy.size(); ++i) post[P.rules.size() + i] = 1.0f / post[P.post_rule[i]];
    for (const InvTarget& t : P.inv) *t.host = 1.0f / post[t.rule];
    if (h->generic_student)
        for (int f = 0; f < c.n_flows; ++f) {
            h->flows_x[f].bmean = mx[P.nslots + NU + 2 * f];
            h->flows_x[f].bscale = mx[P.nslots + NU + 2 * f + 1];
        }

    // ---- 3. the split-fp16 packs under the scale table
    if (int rc = upload(h, post, wsb, P.o_post, st)) return rc;
    hipLaunchKernelGGL(rp_tile_kernel, dim3(grid_x(P.max_tile), (unsigned)P.tile.size()), dim3(TR_NT), 0, st,
                       reinterpret_cast<const RpTile*>(wsb + P.o_tile), reinterpret_cast<const float*>(wsb + P.o_post));
    if (!P.post_copy.empty())
        hipLaunchKernelGGL(rp_copy_kernel, dim3(1, (unsigned)P.post_copy.size()), dim3(TR_NT), 0, st,
                           reinterpret_cast<const RpCopy*>(wsb + P.o_pcopy));
    for (int s = 0; s < n_up; ++s)
        if (up_params[s]) wn_repack_deconv_split(h, h->stacks[s], up_params[s], mx.data() + up_slot0[s], st);
    WN_HIP(h, hipGetLastError());
    return WN_OK;
}
