"""CPU pin of the float64 oracle the upsampler-backward tests compare with (tests/deconv_grad_oracle64.py):
its forward is oracle.wavenet_np.deconv_stack in float64 for both activations, and torch.autograd's gradient of
sum(enc * g) agrees with float64 central differences on a handful of entries of every variable (the bar of
tests/test_teacher_wgrad_oracle.py)."""
import json
import os

import numpy as np
import pytest
import torch

import deconv_grad_oracle64 as DG
import distill_oracle64 as D

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_distill.npz')


def _model(act):
    from oracle import wavenet_np as O
    cfgd, seed, init = D.golden_case(np.load(GOLD), 'mol')[1]
    cfgd = dict(json.loads(json.dumps(cfgd)), upsample_act=act)
    hp = O.HP(cfgd)
    return cfgd, hp, O.synth_weights(hp, 'teacher', seed=seed, init=init)


@pytest.mark.parametrize('act', ['leaky_relu', 'tanh'])
def test_forward_is_the_numpy_oracle(act):
    from oracle import wavenet_np as O
    cfgd, hp, w = _model(act)
    mel = np.random.RandomState(7).uniform(0, 1, [2, 3, 80])
    ref = O.deconv_stack(mel, w, hp, '', np.float64)
    _, enc = DG.stack_ff(mel, DG.weights64(w, 2), cfgd['deconv_config'], act)
    assert tuple(enc.shape) == ref.shape == (2, 600, 64)
    assert float(np.abs(enc.numpy() - ref).max()) <= 1e-12 * float(np.abs(ref).max())


@pytest.mark.parametrize('act', ['leaky_relu', 'tanh'])
def test_autograd_gradients_match_central_differences(act):
    cfgd, hp, w = _model(act)
    dc = cfgd['deconv_config']
    rs = np.random.RandomState(5)
    mel = rs.uniform(0, 1, [2, 2, 80])
    g = rs.standard_normal([2, 400, 64])
    w64 = DG.weights64(w, 2)
    got = DG.grads(mel, w64, dc, act, g)

    def val(weights):
        with torch.no_grad():
            return float((DG.stack_ff(mel, weights, dc, act)[1] * torch.as_tensor(g)).sum())
    h = 1e-6
    for k in DG.names(2):
        flat = w64[k].reshape(-1)
        for idx in sorted(set(int(i) for i in rs.randint(0, flat.numel(), 4))):
            vals = []
            for sgn in (1.0, -1.0):
                wp = dict(w64)
                t = w64[k].clone()
                t.reshape(-1)[idx] += sgn * h
                wp[k] = t
                vals.append(val(wp))
            fd = (vals[0] - vals[1]) / (2 * h)
            a = float(got[k].reshape(-1)[idx])
            assert abs(fd - a) <= 1e-6 * max(1.0, float(got[k].abs().max())) + 1e-5 * abs(a), (act, k, idx, fd, a)


def test_tie_handling_is_on_the_oracle_alone():
    """pick_rows finds rows whose hidden layers have no near tie -- the FIRST such seeds; mask_last zeroes at most 0.1 % of a
    dense cotangent"""
    cfgd, hp, w = _model('leaky_relu')
    w64 = DG.weights64(w, 2)
    mel, seeds = DG.pick_rows(3, 2, w64, cfgd['deconv_config'], 'leaky_relu')
    assert len(seeds) == 3 and seeds[0] >= DG.FIRST_SEED and list(seeds) == sorted(set(seeds))
    skipped = [s for s in range(DG.FIRST_SEED, seeds[-1]) if s not in seeds]
    if skipped:
        rows = np.stack([np.random.RandomState(s).uniform(0, 1, [2, 80]).astype(np.float32) for s in skipped])
        assert min(DG.hidden_ties(rows, w64, cfgd['deconv_config'])) > 0
    assert DG.hidden_ties(mel, w64, cfgd['deconv_config']) == [0, 0, 0]
    g = torch.as_tensor(np.random.RandomState(1).standard_normal([3, 400, 64]))
    gm, n, nh = DG.mask_last(g, mel, w64, cfgd['deconv_config'], 'leaky_relu')
    assert nh == 0 and int((gm != g).sum()) == n <= 1e-3 * g.numel()


def test_hidden_ties_without_a_clear_seed_are_projected_out():
    """A row whose hidden layer does have near ties: after mask_last the float64 cotangent of those hidden elements is zero
    (to rounding), so flipping leaky-relu's slope there leaves every gradient where it was."""
    cfgd, hp, w = _model('leaky_relu')
    dc = cfgd['deconv_config']
    w64 = DG.weights64(w, 2)
    seed = next(s for s in range(1, 400) if DG.hidden_ties(
        np.random.RandomState(s).uniform(0, 1, [1, 3, 80]).astype(np.float32), w64, dc)[0] > 0)
    mel = np.random.RandomState(seed).uniform(0, 1, [1, 3, 80]).astype(np.float32)
    with pytest.raises(AssertionError, match='hidden pre-activation'):
        DG.mask_last(torch.zeros(1, 600, 64), mel, w64, dc, 'leaky_relu')
    g = torch.as_tensor(np.random.RandomState(2).standard_normal([1, 600, 64]).astype(np.float32))
    gm, n, nh = DG.mask_last(g, mel, w64, dc, 'leaky_relu', project=True)
    assert nh > 0 and float((gm - g).abs().max()) > 0
    h = torch.as_tensor(mel, dtype=torch.float64).transpose(1, 2)
    z1 = torch.nn.functional.conv_transpose1d(h, w64['trans_conv_1/kernel'][0].permute(2, 1, 0).contiguous(),
                                              w64['trans_conv_1/bias'], stride=dc[0][1], padding=(dc[0][0] - dc[0][1]) // 2)
    h1 = torch.nn.functional.leaky_relu(z1, 0.4).detach().requires_grad_(True)
    z2 = torch.nn.functional.conv_transpose1d(h1, w64['trans_conv_2/kernel'][0].permute(2, 1, 0).contiguous(),
                                              w64['trans_conv_2/bias'], stride=dc[1][1], padding=(dc[1][0] - dc[1][1]) // 2)
    enc = torch.nn.functional.leaky_relu(z2, 0.4).transpose(1, 2)
    dh, = torch.autograd.grad((enc * gm.double()).sum(), [h1])
    ties = DG.near(z1)
    assert int(ties.sum()) == nh
    assert float(dh[ties].abs().max()) <= 1e-6 * float(dh.abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# the geometries of tests/deconv_bwd_geometries.py: the oracle on n-layer stacks and relu, and the
# restatement of csrc/wn_deconv_bwd.hip's layer_dims asserting that every shape hits the seam it is there for
# ---------------------------------------------------------------------------------------------------------------------
import deconv_bwd_geometries as BG                                                  # noqa: E402

GEO_FORWARD = [(tag, 'tanh') for tag in BG.TAGS] + [(tag, 'relu') for tag in BG.RELU_TAGS] + [('taps6', 'leaky_relu')]


def _geo_model(tag, act, kind='teacher'):
    from oracle import wavenet_np as O
    cfgd = BG.cfg_of(kind, tag, upsample_act=act)
    return cfgd, O.HP(cfgd), BG.weights(kind, cfgd)


@pytest.mark.parametrize('tag,act', GEO_FORWARD, ids=['{}-{}'.format(*c) for c in GEO_FORWARD])
def test_forward_is_the_numpy_oracle_on_every_geometry(tag, act):
    from oracle import wavenet_np as O
    cfgd, hp, w = _geo_model(tag, act)
    dc = cfgd['deconv_config']
    mel = np.random.RandomState(7).uniform(0, 1, [2, 3, 80])
    ref = O.deconv_stack(mel, w, hp, '', np.float64)
    pre, enc = DG.stack_ff(mel, DG.weights64(w, len(dc)), dc, act)
    assert len(pre) == len(dc) and tuple(enc.shape) == ref.shape == (2, 3 * BG.hop(tag), 64)
    assert float(np.abs(enc.numpy() - ref).max()) <= 1e-12 * float(np.abs(ref).max())
    if act == 'relu':
        assert float(enc.min()) == 0.0 and float((enc == 0).double().mean()) > 0.05, 'relu, not tanh'


def test_an_unknown_activation_raises():
    cfgd, hp, w = _geo_model('base', 'tanh')
    mel = np.random.RandomState(7).uniform(0, 1, [1, 1, 80])
    with pytest.raises(ValueError, match='Unsupported activation'):
        DG.stack_ff(mel, DG.weights64(w, 2), cfgd['deconv_config'], 'elu')
    with pytest.raises(ValueError, match='Unsupported activation'):
        DG.pick_rows(1, 1, DG.weights64(w, 2), cfgd['deconv_config'], 'elu')


GEO_FD = [('three', 'tanh'), ('single', 'tanh'), ('taps8', 'tanh'), ('base', 'relu'), ('three', 'relu')]


@pytest.mark.parametrize('tag,act', GEO_FD, ids=['{}-{}'.format(*c) for c in GEO_FD])
def test_autograd_gradients_match_central_differences_on_the_geometries(tag, act):
    cfgd, hp, w = _geo_model(tag, act)
    dc = cfgd['deconv_config']
    rs = np.random.RandomState(5)
    w64 = DG.weights64(w, len(dc))
    # relu: rows whose hidden pre-activations keep clear of zero, so that no step of 1e-6 crosses a kink there
    mel = DG.pick_rows(2, 2, w64, dc, act)[0].astype(np.float64)
    g = torch.as_tensor(rs.standard_normal([2, 2 * BG.hop(tag), 64]))
    g = DG.mask_last(g, mel, w64, dc, act)[0].numpy()
    got = DG.grads(mel, w64, dc, act, g)
    assert sorted(got) == sorted(DG.names(len(dc)))

    def val(weights):
        with torch.no_grad():
            return float((DG.stack_ff(mel, weights, dc, act)[1] * torch.as_tensor(g)).sum())
    h = 1e-6
    for k in DG.names(len(dc)):
        flat = w64[k].reshape(-1)
        for idx in sorted(set(int(i) for i in rs.randint(0, flat.numel(), 4))):
            vals = []
            for sgn in (1.0, -1.0):
                wp = dict(w64)
                t = w64[k].clone()
                t.reshape(-1)[idx] += sgn * h
                wp[k] = t
                vals.append(val(wp))
            fd = (vals[0] - vals[1]) / (2 * h)
            a = float(got[k].reshape(-1)[idx])
            assert abs(fd - a) <= 1e-6 * max(1.0, float(got[k].abs().max())) + 1e-5 * abs(a), (tag, act, k, idx, fd, a)


def test_relu_ties_follow_torch_relu():
    """no gradient at exactly 0, and the tie rules apply to relu's pre-activations as to leaky-relu's"""
    z = torch.tensor([-1.0, 0.0, 2.0], dtype=torch.float64, requires_grad=True)
    d, = torch.autograd.grad(DG.activation(z, 'relu').sum(), [z])
    assert d.tolist() == [0.0, 0.0, 1.0]
    cfgd, hp, w = _geo_model('base', 'relu')
    w64 = DG.weights64(w, 2)
    mel, seeds = DG.pick_rows(3, 2, w64, cfgd['deconv_config'], 'relu')
    assert DG.hidden_ties(mel, w64, cfgd['deconv_config'], '', 'relu') == [0, 0, 0]
    g = torch.as_tensor(np.random.RandomState(1).standard_normal([3, 400, 64]))
    gm, n, nh = DG.mask_last(g, mel, w64, cfgd['deconv_config'], 'relu')
    assert nh == 0 and int((gm != g).sum()) == n <= DG.MAX_ZEROED * g.numel()


def test_layer_dims_of_the_control_geometry():
    """what the issue of DESIGN.md 25 says [[40, 10], [80, 20]] pins, on the restatement"""
    for d, (S, pL) in zip(BG.layer_dims(BG.ACCEPTED['base'], 64, 1, 27), ((10, 15), (20, 30))):
        assert (d['S'], d['pL'], d['taps'], d['dmax'], d['nsh']) == (S, pL, 4, 2, 6)
    d = BG.layer_dims(BG.ACCEPTED['base'], 64, 15, 27)[1]                 # tests/test_gpu_deconv_backward.py's slab shape
    assert (d['Lp'], d['N'], d['nslab'], d['pchunk'], d['npc']) == (288, 4320, 2, 2, 10)
    d = BG.layer_dims(BG.ACCEPTED['base'], 64, 30, 27)[1]
    assert (d['nslab'], d['pchunk'], d['npc']) == (3, 3, 7)


def test_every_geometry_is_what_its_table_row_says():
    want = {'hop256': [(16, 4, 24, 2)] * 2, 'taps6': [(10, 4, 15, 2), (8, 6, 20, 3)], 'taps8': [(10, 4, 15, 2), (20, 8, 70, 4)],
            'three': [(2, 4, 3, 2), (4, 5, 8, 2), (4, 4, 6, 2)], 's12': [(10, 4, 15, 2), (12, 4, 18, 2)],
            's6': [(10, 4, 15, 2), (6, 4, 9, 2)], 's30': [(10, 4, 15, 2), (30, 2, 15, 1)], 'single': [(20, 2, 10, 1)],
            'base': [(10, 4, 15, 2), (20, 4, 30, 2)]}
    assert sorted(want) == sorted(BG.TAGS)
    for tag in BG.TAGS:
        got = [(d['S'], d['taps'], d['pL'], d['dmax']) for d in BG.layer_dims(BG.ACCEPTED[tag], 256, 1, 1)]
        assert got == want[tag], (tag, got)
        assert all(d['nsh'] == d['taps'] + d['dmax'] and d['S'] <= BG.DB_MAXS for d in BG.layer_dims(BG.ACCEPTED[tag], 256, 1, 1))
    assert [d['nsh'] for d in BG.layer_dims(BG.ACCEPTED['taps6'], 256, 1, 1)] == [6, 9]
    assert [d['nsh'] for d in BG.layer_dims(BG.ACCEPTED['taps8'], 256, 1, 1)] == [6, 12]
    for tag, (dc, resize, why) in BG.REFUSED.items():
        strides = [s for _, s in dc]
        if 'stride' in why:
            assert max(strides) > BG.DB_MAXS
        else:                                  # the pack's own reasons are the GPU refusal test's, by message
            assert max(strides) <= BG.DB_MAXS and (resize or 'split' in why)


def test_the_leaky_case_left_out_cannot_meet_the_rule():
    """('teacher', 's6', (1, 1)): more than 0.1 % of its last-layer pre-activations are near ties, so it runs at (3, 2) only.
    A change of weights or seeds that makes the case eligible fails here, and the case goes back in."""
    assert BG.LEAKY_SKIP == {('teacher', 's6', (1, 1))}
    cfgd = BG.teacher_cfg('s6', upsample_act='leaky_relu')
    w64 = DG.weights64(BG.weights('teacher', cfgd), 2)
    mel, _ = DG.pick_rows(1, 1, w64, cfgd['deconv_config'], 'leaky_relu')
    pre, _ = DG.stack_ff(mel, w64, cfgd['deconv_config'], 'leaky_relu')
    n = int(DG.near(pre[-1]).sum())
    print('teacher s6 B1-F1: {} of {} last-layer pre-activations are near ties'.format(n, pre[-1].numel()))
    assert n > DG.MAX_ZEROED * pre[-1].numel()
    g = torch.zeros(1, BG.hop('s6'), 64)
    with pytest.raises(AssertionError):
        DG.mask_last(g, mel, w64, cfgd['deconv_config'], 'leaky_relu')


@pytest.mark.parametrize('tag', BG.TAGS)
def test_slab_shape_crosses_a_slab_and_leaves_ragged_tiles(tag):
    B, F = BG.tanh_shapes(tag)[-1]
    for width in (64, 256):
        d = BG.layer_dims(BG.ACCEPTED[tag], width, B, F)[-1]
        assert d['L'] == BG.SLAB_FRAMES.get(tag, 1350)
        assert (d['N'], d['nslab'], d['last_slab']) == (4128, 2, 32)           # the second slab is one 32-column K-step
        assert d['L'] % 64 != 0                                                 # a ragged last data-gradient tile
        assert (d['L'] % BG.DB_FT != 0) == (tag != 'hop256')                    # a partly filled de-interleave tile
        assert B * F * BG.hop(tag) * width * 4 <= (125e6 if tag == 's30' else 83e6)      # the cotangent (hop 300: 124 MB)
    for s in BG.tanh_shapes(tag)[:2]:
        assert all(x['nslab'] == 1 for x in BG.layer_dims(BG.ACCEPTED[tag], 256, *s))


def test_phase_chunk_shapes_run_several_phases_per_workgroup():
    assert sorted(set(t for t, _, _, _ in BG.PCHUNK_SHAPES)) == sorted(BG.MULTI)
    for tag, (B, F), layer, (pchunk, npc) in BG.PCHUNK_SHAPES:
        d = BG.layer_dims(BG.ACCEPTED[tag], 256, B, F)[layer]
        assert (d['pchunk'], d['npc']) == (pchunk, npc) and pchunk >= 2, (tag, d)
        assert B * F * BG.hop(tag) * 256 * 4 <= 89e6, tag
    ragged = {t: BG.layer_dims(BG.ACCEPTED[t], 256, B, F)[-1] for t, (B, F), l, _ in BG.PCHUNK_SHAPES[:3]}
    assert all(d['S'] % d['pchunk'] for d in ragged.values())                   # a ragged last chunk
    assert any(l == 1 for t, _, l, _ in BG.PCHUNK_SHAPES if t == 'three')       # the middle layer of 'three' has its own shape
    # the small shapes give every phase a workgroup of its own
    for tag in BG.MULTI:
        assert all(d['pchunk'] == 1 for d in BG.layer_dims(BG.ACCEPTED[tag], 256, 3, 2)[1:])


@pytest.mark.parametrize('tag', BG.TAGS)
def test_second_tile_sample_exists(tag):
    F, S = BG.f_second_tile(tag), BG.ACCEPTED[tag][-1][1]
    d = BG.layer_dims(BG.ACCEPTED[tag], 256, 1, F)[-1]
    assert S * BG.DB_FT < F * BG.hop(tag) and d['deint_tiles'] >= 2 and d['L'] > BG.DB_FT
    assert F == 2 or (F - 1) * BG.hop(tag) <= S * BG.DB_FT
    assert (F == 2) == (tag not in ('three', 'single'))
    assert BG.layer_dims(BG.ACCEPTED['s30'], 256, 1, 2)[-1]['S'] * BG.DB_FT == 480   # all rows of the LDS tile
