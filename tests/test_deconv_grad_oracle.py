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
