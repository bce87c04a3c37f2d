"""CPU tests of tests/teacher_nll_oracle64.py, the float64 torch restatement of the teacher's scoring that the GPU gradient
tests compare with: its values against oracle.wavenet_np.teacher_log_prob in float64, its autograd gradient
against central finite differences, and the tie conditions of the GPU tests' inputs."""
import numpy as np
import pytest
import torch

import teacher_nll_oracle64 as N

CASES = sorted(N.KERNEL_CASES)


def _hp(tag):
    from oracle import wavenet_np as O
    loss, mu, M, _, _ = N.KERNEL_CASES[tag]
    return O.HP({'loss_type': loss, 'use_mu_law': mu, 'mol_mix': M})


@pytest.mark.parametrize('tag', CASES)
def test_values_match_the_numpy_oracle(tag):
    """mol (Q = 65536 and 256), gauss and ce (256 and 65536 classes): 1e-10 against the float64 numpy oracle"""
    from oracle import wavenet_np as O
    loss, mu = N.KERNEL_CASES[tag][:2]
    par, wav, _ = N.kernel_case(tag)
    ref = O.teacher_log_prob(par.astype(np.float64), wav.astype(np.float64), _hp(tag), np.float64)
    got = N.teacher_log_prob(torch.as_tensor(par.astype(np.float64)), torch.as_tensor(wav.astype(np.float64)), loss, mu).numpy()
    assert got.shape == ref.shape == wav.shape
    assert np.all(np.isfinite(ref))
    assert np.abs(got - ref).max() <= 1e-10, np.abs(got - ref).max()
    # the targets themselves
    real, cate = N.encode_targets(torch.as_tensor(wav.astype(np.float64)), mu)
    r_ref, c_ref = O.encode_targets(wav.astype(np.float64), _hp(tag), np.float64)
    assert np.array_equal(real.numpy(), r_ref) and np.array_equal(cate.numpy(), c_ref)


@pytest.mark.parametrize('tag', CASES)
def test_autograd_matches_central_differences(tag):
    """d sum(g log_prob) / d (out_params, wav) against (f(p + e) - f(p - e)) / 2e, e = 1e-6, element by element on the first
    eight samples of the first utterance (three and two for the 256- and 65 536-class heads: edge bins, log-scales below -7
    and a component below the floor among them; the one exact tie at -7 lies in the second utterance: a central difference
    straddles it).  Truncation error: the sharpest component has inv_s = e^7, so (e inv_s)^2 / 6 = 2e-7 of the gradient; the
    bound is 1e-5 of the largest magnitude."""
    loss, mu = N.KERNEL_CASES[tag][:2]
    par, wav, g = N.kernel_case(tag)
    n = {'ce_mulaw': 3, 'ce_16bit': 2}.get(tag, 8)
    par, wav, g = (np.asarray(v[:1, :n], np.float64) for v in (par, wav, g))
    assert N.tie_report(tag, par, wav)['scale_at_tie'] == 0
    _, dp, dx = N.grads(par, wav, g, loss, mu)
    gt = torch.as_tensor(g)

    def f(p, x):
        return float((N.teacher_log_prob(torch.as_tensor(p), torch.as_tensor(x), loss, mu) * gt).sum())
    eps = 1e-6
    rs = np.random.RandomState(0)
    for arr, grad, which in ((par, dp.numpy(), 0), (wav, dx.numpy(), 1)):
        idx = list(np.ndindex(*arr.shape))
        if len(idx) > 4096:                                     # 65 536 logits: the labels' and 60 others
            _, cate = N.encode_targets(torch.as_tensor(wav), mu)
            idx = [(0, t, int(cate[0, t])) for t in range(arr.shape[1])] + \
                  [(0, int(t), int(k)) for t, k in zip(rs.randint(0, arr.shape[1], 60), rs.randint(0, arr.shape[2], 60))]
        fd = np.zeros(len(idx))
        for j, i in enumerate(idx):
            a, b = arr.copy(), arr.copy()
            a[i] += eps
            b[i] -= eps
            fd[j] = ((f(a, wav) - f(b, wav)) if which == 0 else (f(par, a) - f(par, b))) / (2 * eps)
        an = np.array([grad[i] for i in idx])
        scale = max(np.abs(grad).max(), 1e-30)
        if which == 1 and (mu or loss == 'ce'):
            assert np.all(an == 0) and np.abs(fd).max() <= 1e-9 * max(1.0, np.abs(dp.numpy()).max())
        else:
            assert np.abs(grad).max() > 0
            assert np.abs(fd - an).max() <= 1e-5 * scale, (tag, which, np.abs(fd - an).max(), scale)


@pytest.mark.parametrize('tag', CASES)
def test_gpu_case_inputs_hit_every_edge_and_no_tie(tag):
    """the conditions under which tests/test_gpu_teacher_nll_grad.py excludes no element, checked before a GPU sees the seed"""
    loss = N.KERNEL_CASES[tag][0]
    par, wav, _ = N.kernel_case(tag)
    r = N.tie_report(tag, par, wav)
    assert r['mass_in_band'] == 0 and r['target_near_threshold'] == 0 and r['scale_near_tie'] == 0, r
    if loss != 'gauss':
        assert r['low_bin'] >= 1 and r['high_bin'] >= 1, r
    if loss != 'ce':
        assert r['scale_at_tie'] == 1 and r['scale_below'] >= 3, r
    if loss == 'mol':
        assert r['mass_below_floor'] >= 4, r
    else:
        spread = par.max() - par.min()
        assert loss == 'gauss' or spread > 39.0
