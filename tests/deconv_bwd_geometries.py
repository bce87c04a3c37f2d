"""The upsampler geometries of tests/test_gpu_deconv_backward_geometries.py and tests/test_gpu_deconv_repack_geometries.py
(DESIGN.md 25): deconv_configs off [[40, 10], [80, 20]], the one every other test of wn_deconv_backward
(csrc/wn_deconv_bwd.hip) and of the device re-pack of an upsampler stack (csrc/wn_train.hip) runs.  The configs shared with
the forward suite come from tests/deconv_geometries.py; 's30', 'single' and 'base' are added here (GEOMETRIES there
parametrises the forward suite and stays as it is).

layer_dims() restates layer_dims of csrc/wn_deconv_bwd.hip as pack_facts restates wn_pack_deconv: per layer Lp, nslab, dmax,
nsh, R, pchunk, npc.  Every shape below is asserted on that restatement (tests/test_deconv_grad_oracle.py, on the CPU) to
hit the seam it is there for, so a later change of DB_SLAB or DB_WGS fails loudly instead of leaving a test that no longer
tests.
"""
import numpy as np

import deconv_geometries as G

N_MEL = G.N_MEL
DB_FT = 16            # frames per de-interleave tile
DB_LP = 32            # frames per batch row are padded to a multiple of the 32-wide K-step
DB_SLAB = 4096        # columns per partial sum of a weight-gradient GEMM
DB_WGS = 1024         # workgroups the data-gradient GEMM aims at
DB_MAXS = 30          # largest stride the call takes

# tag: deconv_config, and what only it exercises
ACCEPTED = {
    'hop256': G.GEOMETRIES['hop256']['deconv_config'],     # S = 16 in both layers, pL 24, a hidden layer with stride 16
    'taps6': G.GEOMETRIES['taps6']['deconv_config'],       # 6 taps, dmax 3, nsh 9
    'taps8': G.GEOMETRIES['taps8']['deconv_config'],       # 8 taps, dmax 4, nsh 12, K = 160
    'three': G.GEOMETRIES['three']['deconv_config'],       # three layers, 5 taps in the middle one, S = 2 in the first
    's12': G.GEOMETRIES['s12']['deconv_config'],           # phase groups 4,2,4,2 in the re-pack
    's6': G.GEOMETRIES['s6']['deconv_config'],             # odd pL (9), no phase-group pack
    's30': [[40, 10], [60, 30]],                           # the largest admitted stride: all 480 rows of the de-interleave tile
    'single': [[40, 20]],                                  # one layer: no data gradient at all
    'base': [[40, 10], [80, 20]],                          # control, and the carrier of the relu cases
}
TAGS = list(ACCEPTED)
MULTI = [t for t in TAGS if len(ACCEPTED[t]) > 1]
# tag: (deconv_config, use_resize_conv, what deconv_backward names as the reason)
REFUSED = {
    'one': (G.GEOMETRIES['one']['deconv_config'], False, 'stride 32 above 30'),
    's32': (G.GEOMETRIES['s32']['deconv_config'], False, 'stride 32 above 30'),
    'oddtap': (G.GEOMETRIES['oddtap']['deconv_config'], False, 'no split-fp16 pack'),
    'resize': (G.GEOMETRIES['resize']['deconv_config'], True, 'use_resize_conv'),
}
STUDENT_SCOPE = 'iaf_share'
SEED, INIT = 1234, 'unit'


def config_of(tag):
    """(deconv_config, use_resize_conv)"""
    if tag in ACCEPTED:
        return ACCEPTED[tag], False
    return REFUSED[tag][0], REFUSED[tag][1]


def hop(tag):
    return int(np.prod([s for _, s in config_of(tag)[0]]))


def student_cfg(tag, **extra):
    """deconv_geometries.student_cfg for every tag of this file: deconv_width 256, one flow of ten layers, 'iaf_share'"""
    dc, resize = config_of(tag)
    return dict(G.student_cfg('hop256'), deconv_config=dc, use_resize_conv=resize, **extra)


def teacher_cfg(tag, **extra):
    """deconv_geometries.teacher_cfg for every tag of this file: the tiny teacher with deconv_width 64, scope ''"""
    dc, resize = config_of(tag)
    return dict(G.teacher_cfg('hop256'), deconv_config=dc, use_resize_conv=resize, **extra)


def cfg_of(kind, tag, **extra):
    return (student_cfg if kind == 'student' else teacher_cfg)(tag, **extra)


def scope_of(kind):
    return STUDENT_SCOPE if kind == 'student' else ''


def weights(kind, cfgd, seed=SEED):
    from oracle import wavenet_np as O
    return O.synth_weights(O.HP(cfgd), kind, seed=seed, init=INIT)


def layer_dims(deconv_config, width, B, F, n_mel=N_MEL):
    """layer_dims of csrc/wn_deconv_bwd.hip, restated: one dict per layer.  pchunk / npc are those of the data-gradient GEMM,
    which every layer but the first runs (None for the first)."""
    out, L, cin = [], F, n_mel
    for j, (K, S) in enumerate(deconv_config):
        taps, pL = K // S, (K - S) // 2
        dmax = (S - 1 + pL) // S
        Lp = (L + DB_LP - 1) // DB_LP * DB_LP
        N = B * Lp
        nslab = (N + DB_SLAB - 1) // DB_SLAB
        tiles = (cin // 64) * ((L + 63) // 64) * B
        want = min(S, max(1, (DB_WGS + tiles - 1) // max(tiles, 1)))
        pchunk = (S + want - 1) // want
        out.append(dict(K=K, S=S, taps=taps, pL=pL, dmax=dmax, nsh=taps + dmax, cin=cin, cinp=(cin + 63) // 64 * 64, L=L, Lp=Lp,
                        R=dmax + (L + 63) // 64 * 64 + taps, N=N, nslab=nslab, last_slab=N - (nslab - 1) * DB_SLAB,
                        pchunk=pchunk if j else None, npc=(S + pchunk - 1) // pchunk if j else None,
                        deint_tiles=Lp // DB_FT))
        L, cin = L * S, width
    return out


WIDTH = {'student': 256, 'teacher': 64}

# (3, F_slab): B Lp of the last layer is 4128 -- two slabs of the weight-gradient GEMM, the second a single 32-column K-step
F_SLAB = {'hop256': 86, 'taps6': 135, 'taps8': 135, 'three': 169, 's12': 135, 's6': 135, 's30': 135, 'single': 1345, 'base': 135}
SLAB_FRAMES = {'hop256': 1376, 'three': 1352, 'single': 1345}          # last-layer input frames; 1350 for every other tag


def tanh_shapes(tag):
    return [(1, 1), (3, 2), (3, F_SLAB[tag])]


def f_pchunk(tag, width, B, layer=-1, pchunk=2):
    """smallest F at which the data-gradient GEMM of `layer` runs `pchunk` phases per workgroup"""
    dc = ACCEPTED[tag]
    for F in range(1, 1 << 14):
        if layer_dims(dc, width, B, F)[layer]['pchunk'] == pchunk:
            return F
    raise AssertionError((tag, width, B, layer, pchunk))


# phase chunks of the data-gradient GEMM, on the 256-wide student handle: (B, F), the layer the shape is for, (pchunk, npc)
PCHUNK_SHAPES = [
    ('hop256', (3, 49), -1, (3, 6)),          # 16 phases: five chunks of 3 and a ragged one of 1
    ('taps6', (3, 180), -1, (3, 3)),          # 8 phases: 3, 3 and a ragged 2
    ('taps8', (3, 58), -1, (3, 7)),           # 20 phases: six chunks of 3 and a ragged 2
    ('three', (3, f_pchunk('three', 256, 3)), -1, (2, 2)),           # the last layer (S = 4, L = 8 F)
    ('three', (3, f_pchunk('three', 256, 3, 1)), 1, (2, 2)),         # the middle layer (S = 4, L = 2 F)
    ('s12', (3, f_pchunk('s12', 256, 3)), -1, (2, 6)),
    ('s6', (3, f_pchunk('s6', 256, 3)), -1, (2, 3)),
    ('s30', (3, f_pchunk('s30', 256, 3)), -1, (2, 15)),
    ('base', (3, f_pchunk('base', 256, 3)), -1, (2, 10)),
]


def f_second_tile(tag):
    """smallest F >= 2 at which sample S_last * 16 -- the first of the second de-interleave tile -- exists in the output"""
    S = ACCEPTED[tag][-1][1]
    return max(2, S * DB_FT // hop(tag) + 1)


# leaky-relu and relu cases: (kind, tag) -> shapes.  The rule of tests/deconv_grad_oracle64.py is a condition: the one case
# that cannot meet it (the 64-wide 's6' at (1, 1): 6 of its 3 840 last-layer pre-activations are near ties, 1.6e-3, above the
# cap of 1e-3) is left to the next shape
LEAKY_SHAPES = [(1, 1), (3, 2)]
LEAKY_SKIP = {('teacher', 's6', (1, 1))}
RELU_TAGS = ['base', 'three']
RELU_SHAPES = [(1, 1), (3, 2), (2, 7)]


def leaky_cases():
    return [(kind, tag, s) for tag in TAGS for kind in ('teacher', 'student') for s in LEAKY_SHAPES
            if (kind, tag, s) not in LEAKY_SKIP]


def f_crop(tag, num_stages=10):
    """deconv_geometries.f_crop for this file's tags: smallest F with T > 0 and a non-zero centre crop of the conditioning"""
    md, h = 2 ** (num_stages - 1), hop(tag)
    F = 1
    while not (F * h // md > 0 and (F * h - F * h // md * md) // 2 > 0):
        F += 1
    return F


def f_a(tag):
    """smallest F whose last layer has more than one DC_QW = 256 column tile of the forward GEMM"""
    dc = ACCEPTED[tag]
    return G.DC_QW // int(np.prod([s for _, s in dc[:-1]], dtype=np.int64)) + 1


def student_inputs(tag, B, F, seed=0, num_stages=10):
    from oracle import wavenet_np as O
    rs = np.random.RandomState(1000 * seed + 17 * B + F)
    md = 2 ** (num_stages - 1)
    T = F * hop(tag) // md * md
    mel = rs.uniform(0, 1, [B, F, N_MEL]).astype(np.float32)
    return mel, O.logistic_from_uniform(rs.uniform(1e-5, 1 - 1e-5, [B, T])), T


def teacher_inputs(tag, B, F, seed=0):
    rs = np.random.RandomState(2000 * seed + 17 * B + F)
    mel = rs.uniform(0, 1, [B, F, N_MEL]).astype(np.float32)
    return mel, rs.uniform(-1, 1, [B, F * hop(tag)]).astype(np.float32)
