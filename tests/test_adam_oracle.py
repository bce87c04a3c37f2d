"""Pins tests/adam_oracle64.py on the CPU: against torch.optim.Adam in float64 at eps = 0 on nonzero gradients (there
TensorFlow's epsilon, outside the bias-corrected square root, and torch's, inside it, coincide), against values worked out
by hand for t = 1, and for the global-norm clip on both sides of the bound."""
import numpy as np
import torch

import adam_oracle64 as A


def test_matches_torch_adam_at_eps_zero():
    rs = np.random.RandomState(5)
    n, lr, b1, b2 = 37, 3e-3, 0.9, 0.999
    p = rs.standard_normal(n)
    tp = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([tp], lr=lr, betas=(b1, b2), eps=0.0)
    m, v = np.zeros(n), np.zeros(n)
    for t in range(1, 6):
        g = rs.standard_normal(n)
        g[np.abs(g) < 1e-3] = 0.5
        tp.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        r = A.adam_ema_step(p, g, m, v, None, A.lr_t(lr, b1, b2, t), b1, b2, 0.0, 0.0)
        p, m, v = r['p'], r['m'], r['v']
        assert np.abs(p - tp.detach().numpy()).max() <= 1e-14 * np.abs(p).max(), t


def test_first_step_by_hand():
    """t = 1 from m = v = 0: m = 0.1 g, v = 0.001 g^2, lr_t = lr sqrt(0.001) / 0.1, so the update is lr g / (|g| + eps
    sqrt(1000)) up to rounding -- lr sign(g) at eps = 0; the shadow moves 0.9 of the way at num_updates = 0."""
    lr, b1, b2 = 0.01, 0.9, 0.999
    p, g = np.array([1.0, -2.0, 0.5]), np.array([0.3, -4.0, 0.0])
    lt = A.lr_t(lr, b1, b2, 1)
    assert abs(lt - lr * np.sqrt(0.001) / 0.1) < 1e-15 * lt
    r = A.adam_ema_step(p, g, np.zeros(3), np.zeros(3), p.copy(), lt, b1, b2, 0.0 + 1e-300, A.ema_decay(0.9999, 0))
    assert np.allclose(r['m'], [0.03, -0.4, 0.0], rtol=1e-13, atol=1e-18)
    assert np.allclose(r['v'], [0.00009, 0.016, 0.0], rtol=1e-13, atol=0)
    assert np.allclose(r['p'], [1.0 - lr, -2.0 + lr, 0.5], rtol=1e-13, atol=1e-18)
    assert A.ema_decay(0.9999, 0) == 0.1 and A.ema_decay(0.9999, 10 ** 9) == 0.9999
    assert np.allclose(r['ema'], p - 0.9 * (p - r['p']), rtol=1e-13, atol=1e-18)
    # eps outside the square root: with eps = sqrt(v) the update halves
    r2 = A.adam_ema_step(p[:1], g[:1], np.zeros(1), np.zeros(1), None, lt, b1, b2, np.sqrt(0.00009), 0.0)
    assert abs(r2["u"][0] - 0.5 * lr) < 1e-13 * lr


def test_clip_on_both_sides_of_the_bound():
    g = np.array([3.0, -4.0])                      # norm 5
    assert A.clip_factor(25.0, 1.0) == 0.2 and A.clip_factor(25.0, 10.0) == 1.0 and A.clip_factor(25.0, 5.0) == 1.0
    z = np.zeros(2)
    above = A.adam_ema_step(z, g, z, z, None, 1.0, 0.9, 0.999, 1e-8, 0.0, sumsq=25.0, clip_norm=1.0)
    assert np.allclose(above['g'], [0.6, -0.8], rtol=1e-13, atol=1e-18) and np.allclose(above['m'], [0.06, -0.08], rtol=1e-13, atol=1e-18)
    below = A.adam_ema_step(z, g, z, z, None, 1.0, 0.9, 0.999, 1e-8, 0.0, sumsq=25.0, clip_norm=10.0)
    assert np.array_equal(below['g'], g)
    plain = A.adam_ema_step(z, g, z, z, None, 1.0, 0.9, 0.999, 1e-8, 0.0)
    assert all(np.array_equal(below[k], plain[k]) for k in ('p', 'm', 'v'))
