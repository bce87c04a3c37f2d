"""The cases of the input-gradient tests, shared by tests/test_input_grad_oracle.py -- which asserts on the
CPU that every shape hits the seam it is there for and that the tie rules hold for the chosen seeds -- and the GPU tests
test_gpu_deconv_input_grad.py, test_gpu_iaf_input_grad.py, test_gpu_feed_forward_grad.py and test_gpu_input_grad_repack.py."""
import numpy as np
import torch

import deconv_bwd_geometries as BG
import deconv_grad_oracle64 as DG
import student_grad_oracle64 as S

KINDS = ('teacher', 'student')

# ---- d mel of a stack: every accepted tag on both handle kinds ----
SHAPES = [(1, 1), (3, 2), (2, 7)]
# layer 0's frame axis is F itself: 67 frames cross the 64-frame tile of db_dgrad_kernel with a ragged second tile of 3
TILE_TAGS, TILE_SHAPE = ('base', 'three'), (2, 67)


def first_layer_chunks(tag, width, B, F):
    """(pchunk, npc) of the FIRST layer's data-gradient GEMM, which only wn_deconv_backward_input runs: layer_dims of
    csrc/wn_deconv_bwd.hip on the padded row count cinp (BG.layer_dims leaves the first layer's None)"""
    d = BG.layer_dims(BG.ACCEPTED[tag], width, B, F)[0]
    tiles = (d['cinp'] // 64) * ((d['L'] + 63) // 64) * B
    want = min(d['S'], max(1, (BG.DB_WGS + tiles - 1) // max(tiles, 1)))
    pchunk = (d['S'] + want - 1) // want
    return pchunk, (d['S'] + pchunk - 1) // pchunk


def b_first_pchunk(tag, width, pchunk=2):
    """smallest B at which, at F = 1, the first layer runs `pchunk` phases per workgroup (batch rows are the cheap way to the
    DB_WGS workgroups behind which phases start to share one)"""
    for B in range(1, 1 << 12):
        if first_layer_chunks(tag, width, B, 1)[0] == pchunk:
            return B
    raise AssertionError((tag, width, pchunk))


def chunk_shape(tag):
    """(B, 1) on the 256-wide student handle: the first layer's phase chunks hold two phases each"""
    return (b_first_pchunk(tag, BG.WIDTH['student']), 1)


def tanh_cases():
    out = [(kind, tag, s) for tag in BG.TAGS for kind in KINDS for s in SHAPES]
    return out + [(kind, tag, TILE_SHAPE) for tag in TILE_TAGS for kind in KINDS]


# leaky-relu (the shipped activation) and relu under the tie rules of deconv_grad_oracle64: the cases of
# deconv_bwd_geometries, whose one left-out case cannot meet the rule
LEAKY = BG.leaky_cases()
RELU = [(kind, tag, s) for tag in BG.RELU_TAGS for kind in KINDS for s in BG.RELU_SHAPES]


class DeconvCase(object):
    """mel rows by deconv_grad_oracle64.pick_rows, a dense standard-normal cotangent masked at the last layer's near ties by
    mask_last -- which asserts that at most MAX_ZEROED of it is zeroed and that no hidden pre-activation is a near tie.  As
    _Case of tests/test_gpu_deconv_backward_geometries.py, without a device."""

    def __init__(self, kind, tag, act, shape, gseed=101, w32=None):
        self.kind, self.tag, self.act, (self.B, self.F) = kind, tag, act, shape
        self.cfgd = BG.cfg_of(kind, tag, upsample_act=act)
        self.dc, self.width, self.scope = self.cfgd['deconv_config'], int(self.cfgd['deconv_width']), BG.scope_of(kind)
        self.w32 = BG.weights(kind, self.cfgd) if w32 is None else w32
        self.w64 = DG.weights64(self.w32, len(self.dc), self.scope)
        self.mel, self.seeds = DG.pick_rows(self.B, self.F, self.w64, self.dc, act, self.scope)
        g = torch.as_tensor(np.random.RandomState(gseed).standard_normal([self.B, self.F * BG.hop(tag), self.width]).astype(np.float32))
        self.g, self.zeroed, hidden = DG.mask_last(g, self.mel, self.w64, self.dc, act, self.scope)
        assert hidden == 0

    def ref(self, g=None):
        import input_grad_oracle64 as IG
        return IG.stack_d_mel(self.mel, self.w64, self.dc, self.act, (self.g if g is None else g).double(), self.scope)


# ---- d noise of the student: the models, shapes and seed of tests/test_gpu_student_grad.py ----
IAF_SEED = 11
IAF_CASES = {'S1a': ('S1', (2, 25, 200)),       # one partial 256-column tile: T is no multiple of 256
             'S1b': ('S1', (3, 33, 264)),       # a second, ragged tile
             'S2': ('S2', (1, 64, 512))}
IAF_CFG = {'S1': S.S1, 'S2': S.S2}


def iaf_weights(model, seed=IAF_SEED):
    from oracle import wavenet_np as O
    hp = O.HP(IAF_CFG[model])
    return hp, O.synth_weights(hp, 'student', seed=seed, init='unit')


def iaf_inputs(tag):
    """mel, noise, dense cotangents: test_gpu_student_grad._oracle's"""
    B, F, T = IAF_CASES[tag][1]
    return S.case_inputs(B, F, T, seed=IAF_SEED + 100)


# ---- the two composed.  Mel rows: the first seeds from FF_FIRST_SEED whose hidden pre-activations are clear in every stack
# (input_grad_oracle64.pick_rows_stacks; found from deconv_grad_oracle64.FIRST_SEED once, the CPU test asserts them clear)
FF_CASES = {'S1': ('S1', (2, 25, 200), 2005), 'S2': ('S2', (1, 64, 512), 11456)}


def ff_inputs(tag):
    """(hp, weights, oracle, mel, mel seeds, noise, cotangents) of a composed case"""
    import input_grad_oracle64 as IG
    model, (B, F, T), first = FF_CASES[tag]
    hp, w = iaf_weights(model)
    ora = S.StudentGrad64(w, hp)
    mel, seeds = IG.pick_rows_stacks(ora, B, F, first=first)
    _, noise, cot = S.case_inputs(B, F, T, seed=IAF_SEED + 100)
    return hp, w, ora, mel, seeds, noise, cot
