"""The upsampler geometries of tests/test_gpu_deconv_geometries.py and tests/test_deconv_geometry_oracle.py:
deconv_configs off the two the rest of the suite runs, chosen so that every kernel and instantiation of csrc/wn_deconv.hip and
the frame-axis GEMM of csrc/wn_iaf_f.hip runs at least once, with the shapes (B, F) that cross each kernel's tile seams.

Every geometry has n_mel 80.  The student handles are parallel_wavenet.json (width 64, deconv_width 256, ten stages,
use_share_deconv) with num_iaf_layers [10]; the teacher handles a 64-channel wavenet_mol.json.  Per layer: taps = K / S,
pL = (K - S) / 2 (resize-conv: taps = ceil((K - 1) / S) + 1, rounded up where taps x cin / 16 would be odd, pL = K - 1 - (K - 1) // 2).
"pg" = the phase groups of deconv_pg_kernel (phases per group) and its row groups at 256 channels.

The kernel columns are what wn_run_deconv launches per layer.  tests/test_gpu_deconv_geometries.py asserts every cell against
Engine.deconv_forms, which prints the plan the runner launches from (dc_plan, csrc/wn_deconv.hip):
  rows   Engine.deconv, split-fp16 GEMMs, fp32 rows out           g4   the same stack writing G4 words for a consumer
  f32    Engine(precision='f32'): fp32 GEMMs, fp32 rows out       no_pg   g4 on a handle created under WN_DC_NO_PG=1
  no_pg_rows   rows on such a handle, where they differ from rows (the switch also keeps the frame-axis GEMM out)
TEACHER_KERNELS: the 64-channel teachers (and the 256-channel one of hop256), default handle and precision='f32'.
front = deconv_front_kernel, pg = deconv_pg_kernel (one launch each, no weave behind them), h<..> = deconv_mfma_h_kernel<G4IN>,
hs<T> = deconv_mfma_hs_kernel<TAPS>, mfma = deconv_mfma_kernel, fa = gemm_f32_kernel<4, true> (the frame-axis GEMM),
il = deconv_interleave_kernel, g4<S> = deconv_interleave_g4_kernel<S>.
"""
import json
import os

import numpy as np

CONFIG_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'config_jsons')
N_MEL = 80
DC_QW = 256          # q columns per workgroup of the split-fp16 GEMMs (csrc/wn_deconv.hip)
PG_FRAMES = 640      # frames per workgroup of deconv_pg_kernel

# tag: deconv_config, hop, (taps, pL) per layer, pg phase groups of the last layer (None: no pack), frame-axis table on the
# last layer, and the kernels per layer: (rows, G4, f32, G4 under WN_DC_NO_PG)
GEOMETRIES = {
    'hop256': dict(deconv_config=[[64, 16], [64, 16]], hop=256, layers=[(4, 24), (4, 24)], pg=[4, 4, 4, 4], pg_rg=32, fa=True,
                   kernels=dict(rows=['h<false> g4<0>', 'hs<4> il'], g4=['front', 'pg'], f32=['mfma il', 'fa il'],
                                no_pg=['h<false> g4<0>', 'hs<4> g4<0>'])),
    'taps6': dict(deconv_config=[[40, 10], [48, 8]], hop=80, layers=[(4, 15), (6, 20)], pg=None, pg_rg=0, fa=False,
                  kernels=dict(rows=['h<false> g4<10>', 'hs<6> il'], g4=['h<false> g4<10>', 'hs<6> g4<0>'],
                               f32=['mfma il', 'mfma il'], no_pg=['h<false> g4<10>', 'hs<6> g4<0>'])),
    'three': dict(deconv_config=[[8, 2], [20, 4], [16, 4]], hop=32, layers=[(4, 3), (5, 8), (4, 6)], pg=[2, 2], pg_rg=8, fa=True,
                  kernels=dict(rows=['h<false> g4<0>', 'hs<5> g4<0>', 'hs<4> il'], g4=['front', 'hs<5> g4<0>', 'pg'],
                               f32=['mfma il', 'fa il', 'fa il'], no_pg=['h<false> g4<0>', 'hs<5> g4<0>', 'hs<4> g4<0>'])),
    # layer 1: 3 taps x 5 blocks of 16 mel channels is odd -> no split-fp16 pack -> the whole stack on the fp32 GEMMs
    'oddtap': dict(deconv_config=[[24, 8], [16, 8]], hop=64, layers=[(3, 8), (2, 4)], pg=None, pg_rg=0, fa=True,
                   kernels=dict(rows=['mfma il', 'fa il'], g4=['mfma il', 'fa g4<0>'], f32=['mfma il', 'fa il'],
                                no_pg=['mfma il', 'mfma g4<0>'], no_pg_rows=['mfma il', 'mfma il'])),
    'one': dict(deconv_config=[[64, 32]], hop=32, layers=[(2, 16)], pg=None, pg_rg=0, fa=False,
                kernels=dict(rows=['h<false> il'], g4=['h<false> g4<0>'], f32=['mfma il'], no_pg=['h<false> g4<0>'])),
    'taps8': dict(deconv_config=[[40, 10], [160, 20]], hop=200, layers=[(4, 15), (8, 70)], pg=None, pg_rg=0, fa=False,
                  kernels=dict(rows=['h<false> g4<10>', 'h<true> il'], g4=['h<false> g4<10>', 'h<true> g4<20>'],
                               f32=['mfma il', 'mfma il'], no_pg=['h<false> g4<10>', 'h<true> g4<20>'])),
    's12': dict(deconv_config=[[40, 10], [48, 12]], hop=120, layers=[(4, 15), (4, 18)], pg=[4, 2, 4, 2], pg_rg=24, fa=True,
                kernels=dict(rows=['h<false> g4<10>', 'hs<4> il'], g4=['front', 'pg'], f32=['mfma il', 'fa il'],
                             no_pg=['h<false> g4<10>', 'hs<4> g4<0>'])),
    # stride 6, pL 9: three phases per input shift d -> the pack refuses the phase groups
    's6': dict(deconv_config=[[40, 10], [24, 6]], hop=60, layers=[(4, 15), (4, 9)], pg=None, pg_rg=0, fa=True,
               kernels=dict(rows=['h<false> g4<10>', 'hs<4> il'], g4=['h<false> g4<10>', 'hs<4> g4<0>'], f32=['mfma il', 'fa il'],
                            no_pg=['h<false> g4<10>', 'hs<4> g4<0>'])),
    's32': dict(deconv_config=[[40, 10], [128, 32]], hop=320, layers=[(4, 15), (4, 48)], pg=[4] * 8, pg_rg=64, fa=True,
                kernels=dict(rows=['h<false> g4<10>', 'hs<4> il'], g4=['front', 'pg'], f32=['mfma il', 'fa il'],
                             no_pg=['h<false> g4<10>', 'hs<4> g4<0>'])),
    'resize': dict(deconv_config=[[9, 4], [5, 2]], hop=8, layers=[(4, 4), (3, 2)], pg=None, pg_rg=0, fa=False, resize=True,
                   kernels=dict(rows=['h<false> g4<0>', 'h<true> il'], g4=['h<false> g4<0>', 'h<true> g4<0>'],
                                f32=['mfma il', 'mfma il'], no_pg=['h<false> g4<0>', 'h<true> g4<0>'])),
}
TAGS = list(GEOMETRIES)
TEACHER_TAGS = ['hop256', 'three', 's12', 'oddtap']
# teacher_cfg(tag) (64 channels: no deconv_front_kernel, which needs 256, and no frame-axis table, which needs 256 input
# channels), default handle and precision='f32': fp32 rows and G4 words (what teacher_forward asks for)
TEACHER_KERNELS = {
    'hop256': dict(rows=['h<false> g4<0>', 'hs<4> il'], g4=['h<false> g4<0>', 'pg'],
                   f32_rows=['mfma il', 'mfma il'], f32_g4=['mfma il', 'mfma g4<0>']),
    'three': dict(rows=['h<false> g4<0>', 'hs<5> g4<0>', 'hs<4> il'], g4=['h<false> g4<0>', 'hs<5> g4<0>', 'pg'],
                  f32_rows=['mfma il', 'mfma il', 'mfma il'], f32_g4=['mfma il', 'mfma il', 'mfma g4<0>']),
    's12': dict(rows=['h<false> g4<10>', 'hs<4> il'], g4=['h<false> g4<10>', 'pg'],
                f32_rows=['mfma il', 'mfma il'], f32_g4=['mfma il', 'mfma g4<0>']),
    'oddtap': dict(rows=['mfma il', 'mfma il'], g4=['mfma il', 'mfma g4<0>'],
                   f32_rows=['mfma il', 'mfma il'], f32_g4=['mfma il', 'mfma g4<0>']),
}
# ... and hop256 with deconv_width 256: the first layer is the front launch, the fp32 last layer the frame-axis GEMM
TEACHER_256_KERNELS = dict(rows=['h<false> g4<0>', 'hs<4> il'], g4=['front', 'pg'],
                           f32_rows=['mfma il', 'fa il'], f32_g4=['mfma il', 'fa g4<0>'])
DF_STORE_LIMIT = 1 << 31     # deconv_front_kernel addresses its output with 32-bit byte offsets: 64 x 16 x row stride below this


def load_json(name):
    with open(os.path.join(CONFIG_DIR, name), 'rt') as f:
        return json.load(f)


def pack_facts(deconv_config, resize=False, n_mel=N_MEL, width=256):
    """wn_pack_deconv's formulas, restated: per layer (taps, pL); the last layer's phase groups (None where the pack has none),
    its row groups, and whether it gets a frame-axis table."""
    layers, cin = [], n_mel
    for K, S in deconv_config:
        if resize:
            taps = (K - 1 + S - 1) // S + 1
            if (taps * (cin // 16)) % 2:
                taps += 1
            pL = K - 1 - (K - 1) // 2
        else:
            taps, pL = K // S, (K - S) // 2
        layers.append((taps, pL))
        last_cin, cin = cin, width
    (taps, pL), S = layers[-1], deconv_config[-1][1]
    split_ok = all((t * (c // 16)) % 2 == 0 for (t, _), c in zip(layers, [n_mel] + [width] * (len(layers) - 1)))
    pg, rg = None, 0
    if split_ok and not resize and taps == 4 and last_cin % 32 == 0:
        groups, p, ok = [], 0, True
        while p < S and ok:
            d, q = (p + pL) // S, p
            while q < S and (q + pL) // S == d:
                q += 1
            if (q - p) & 1:
                ok = False
                break
            while q - p >= 4:
                groups.append(4)
                p += 4
            if q - p == 2:
                groups.append(2)
                p += 2
        if ok and len(groups) <= 8:
            pg, rg = groups, sum(width // 32 if g == 4 else width // 64 for g in groups)
    fa = (not resize) and last_cin == 256 and 1 <= taps <= 5 and (pL + S - 1) // S <= 4
    return layers, pg, rg, fa


def hop(tag):
    return int(np.prod([s for _, s in GEOMETRIES[tag]['deconv_config']]))


def frames_in(tag, F):
    """L_in: frames entering the last layer"""
    return F * int(np.prod([s for _, s in GEOMETRIES[tag]['deconv_config'][:-1]], dtype=np.int64))


def f_over(tag, n):
    """smallest F with L_in > n"""
    return n // frames_in(tag, 1) + 1


def f_a(tag):
    return f_over(tag, DC_QW)


def f_b(tag):
    """... past one PG_FRAMES tile, where the last layer has a phase-group pack or a frame-axis table (else None)"""
    g = GEOMETRIES[tag]
    return f_over(tag, PG_FRAMES) if (g['pg'] or g['fa']) else None


def row_stride(L):
    """dc_row_stride (csrc/wn_deconv.hip): DC_XOFF zero columns, the q columns of L frames in whole workgroups, 8 more"""
    return 8 + (L + 5 + DC_QW - 1) // DC_QW * DC_QW + 8


def f_past_front(tag):
    """smallest F at which the first layer's G4 rows are too long for deconv_front_kernel's 32-bit store offsets"""
    S = GEOMETRIES[tag]['deconv_config'][0][1]
    F = (DF_STORE_LIMIT // (64 * 16) - 16 - 5) // S - DC_QW
    while 64 * 16 * row_stride(F * S) < DF_STORE_LIMIT:
        F += 1
    return F


def f_crop(tag, num_stages=10):
    """smallest F with T > 0 and a non-zero centre crop of the conditioning"""
    md, h = 2 ** (num_stages - 1), hop(tag)
    F = 1
    while not (F * h // md > 0 and (F * h - F * h // md * md) // 2 > 0):
        F += 1
    return F


def rows_shapes(tag):
    s = [(1, 1), (3, 2), (2, f_a(tag))]
    return s + ([(1, f_b(tag))] if f_b(tag) else [])


def f_b_seen(tag, num_stages=10):
    """smallest F >= F_b at which a student's centre crop keeps both sides of the L_in = 640 seam (s6: at F_b = 65 the
    generated length is 3584 of 3900 samples and the crop ends at 3741, short of the seam at 3840; F = 69 keeps it)"""
    F = f_b(tag)
    if F is None:
        return None
    md, h, S = 2 ** (num_stages - 1), hop(tag), GEOMETRIES[tag]['deconv_config'][-1][1]
    while True:
        T = F * h // md * md
        c0 = (F * h - T) // 2
        if c0 <= S * PG_FRAMES - 1 and S * PG_FRAMES < c0 + T:
            return F
        F += 1


def student_shapes(tag):
    s = [(2, f_a(tag))] + ([(1, f_b(tag))] if f_b(tag) else [])
    if f_b_seen(tag) != f_b(tag):
        s.append((1, f_b_seen(tag)))
    return s + [(1, f_crop(tag))]


def student_cfg(tag, **extra):
    g = GEOMETRIES[tag]
    return dict(load_json('parallel_wavenet.json'), deconv_config=g['deconv_config'], use_resize_conv=bool(g.get('resize')),
                num_iaf_layers=[10], **extra)


def teacher_cfg(tag):
    """the tiny teacher: wavenet_mol.json at width 64 (gate 128: the narrowest wn_create takes), skip 64, deconv_width 64,
    three layers in two stages"""
    g = GEOMETRIES[tag]
    return dict(load_json('wavenet_mol.json'), deconv_config=g['deconv_config'], width=64, double_gate_width=True, skip_width=64,
                deconv_width=64, num_layers=3, num_stages=2)


def seam_columns(tag, F, c0, T):
    """Conditioning columns (time index into the upsampler's output) a consumer of T samples behind a centre crop of c0 reads
    first and last, and the two on either side of every L_in = 256 / 640 seam of the last layer that lies inside that range."""
    S = GEOMETRIES[tag]['deconv_config'][-1][1]
    cols = {'first': c0, 'last': c0 + T - 1}
    for n in (DC_QW, PG_FRAMES):
        if frames_in(tag, F) > n:
            for name, t in (('{}-'.format(n), S * n - 1), ('{}+'.format(n), S * n)):
                if c0 <= t < c0 + T:
                    cols[name] = t
    return cols


# the consumers' weights, shared by the GPU tests and the sensitivity condition that is proved for them on the CPU
STUDENT_INIT, STUDENT_SEED = 'unit', 4321
TEACHER_INIT, TEACHER_SEED = 'unit', 1234


def student_weights(tag):
    from oracle import wavenet_np as O
    cfgd = student_cfg(tag)
    return cfgd, O.synth_weights(O.HP(cfgd), 'student', seed=STUDENT_SEED, init=STUDENT_INIT)


def teacher_weights(tag):
    from oracle import wavenet_np as O
    cfgd = teacher_cfg(tag)
    return cfgd, O.synth_weights(O.HP(cfgd), 'teacher', seed=TEACHER_SEED, init=TEACHER_INIT)


def student_inputs(tag, B, F, seed=0):
    from oracle import wavenet_np as O
    rs = np.random.RandomState(1000 * seed + 17 * B + F)
    T = F * hop(tag) // 512 * 512
    mel = rs.uniform(0, 1, [B, F, N_MEL]).astype(np.float32)
    return mel, O.logistic_from_uniform(rs.uniform(1e-5, 1 - 1e-5, [B, T])), T


def teacher_inputs(tag, B, F, seed=0):
    rs = np.random.RandomState(2000 * seed + 17 * B + F)
    mel = rs.uniform(0, 1, [B, F, N_MEL]).astype(np.float32)
    return mel, rs.uniform(-1, 1, [B, F * hop(tag)]).astype(np.float32)
