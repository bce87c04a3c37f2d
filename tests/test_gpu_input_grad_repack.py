"""The device re-pack rewrites the first layer's transposed pack too: after Engine.iaf_set_weights(params,
up_params) / Engine.teacher_set_weights(P, U) with changed upsampler weights, deconv_backward_input -- the only reader of that
pack -- returns the bits of a fresh handle loaded with the same weights, and bits that differ from those before the update.
The form and the weight sets w0 / w1 / wz of tests/test_gpu_deconv_repack_geometries.py: w1 moves every scale of the stack
(the first kernel times 2^-3), wz has one kernel all zero (pick_scale's 1; the first one, except on 'three')."""
import numpy as np
import pytest

import deconv_bwd_geometries as BG
import test_gpu_deconv_repack_geometries as RG

pytestmark = pytest.mark.gpu
TAGS = ['base', 'three', 'single', 's6']
SHAPE = (2, 3)


def _d_mel(eng, kind, tag):
    import torch
    B, F = SHAPE
    mel = torch.as_tensor(np.random.RandomState(3).uniform(0, 1, [B, F, BG.N_MEL]).astype(np.float32)).cuda()
    g = torch.as_tensor(np.random.RandomState(5).standard_normal([B, F * BG.hop(tag), int(eng.hp.deconv_width)]).astype(np.float32)).cuda()
    scopes = eng.iaf_stack_scopes() if kind == 'student' else ['']
    return {s: eng.deconv_backward_input(mel, g, s).clone() for s in scopes}


def _same(a, b):
    import torch
    return all(torch.equal(a[s].view(torch.int32), b[s].view(torch.int32)) for s in a)


@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('kind', RG.KINDS)
def test_repacked_first_layer_pack_equals_a_fresh_handles(kind, tag):
    import torch
    cfgd = BG.cfg_of(kind, tag)
    n = len(cfgd['deconv_config'])
    w0 = BG.weights(kind, cfgd)
    made = []

    def new(w):
        made.append(RG._engine(kind, cfgd, w))
        return made[-1]
    try:
        a = new(w0)
        scopes = a.iaf_stack_scopes() if kind == 'student' else ['']
        w1 = RG._w1(w0, n, scopes)
        wz = RG._wz(w1, n, scopes)
        before = _d_mel(a, kind, tag)
        assert all(float(v.abs().max()) > 0 and bool(torch.isfinite(v).all()) for v in before.values())
        RG._set(a, kind, w1, scopes)
        got = _d_mel(a, kind, tag)
        assert _same(got, _d_mel(new(w1), kind, tag)), 're-packed to w1'
        assert not any(torch.equal(got[s], before[s]) for s in got), 'the re-pack left d_mel where it was'
        # the flows / the stack alone go back to w0: the upsampler's packs stay those of w1
        RG._set(a, kind, w0, [])
        assert _same(_d_mel(a, kind, tag), got), 'up_params=None'
        RG._set(a, kind, wz, scopes)
        assert _same(_d_mel(a, kind, tag), _d_mel(new(wz), kind, tag)), 're-packed to wz'
    finally:
        for e in made:
            e.close()
