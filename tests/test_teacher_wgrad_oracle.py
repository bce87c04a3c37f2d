"""CPU pin of the float64 oracle the weight-gradient tests compare with (tests/test_gpu_teacher_wgrad.py):
with requires_grad on the weight tensors of distill_oracle64.teacher_weights, torch.autograd's gradient of mean(-log p) agrees
with float64 central differences on a handful of entries of every kind of variable of the residual stack and output head."""
import os

import numpy as np
import pytest
import torch

import distill_oracle64 as D
import teacher_nll_oracle64 as N

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_distill.npz')
KINDS = ['conv_start/W', 'conv_start/biases', 'skip_start/W', 'skip_start/biases', 'dilated_conv_3/W', 'dilated_conv_3/biases',
         'mel_cond_3/W', 'mel_cond_3/biases', 'res_3/W', 'res_3/biases', 'skip_7/W', 'skip_7/biases', 'out1/W', 'out1/biases',
         'mel_cond_out1/W', 'mel_cond_out1/biases', 'out2/W', 'out2/biases']


@pytest.mark.parametrize('tag', ['mol', 'gauss'])
def test_autograd_weight_gradients_match_central_differences(tag):
    R = np.load(GOLD)
    cfgd, seed, init = D.golden_case(R, tag)[1]
    B, F, T = 2, 1, 64
    rs = np.random.RandomState(5)
    mel = rs.uniform(0, 1, [B, F, 80]).astype(np.float32)
    x = torch.as_tensor(np.clip(0.5 * np.sin(0.05 * np.arange(T)) + 0.1 * rs.standard_normal([B, T]), -0.95, 0.95))
    thp, w = D.teacher_weights(cfgd, seed, init)
    enc = D.teacher_enc(mel, cfgd, seed, init)

    def loss(weights):
        return -N.teacher_log_prob(D.teacher_ff(x, enc, weights, thp), x, tag, False).mean()

    leaves = {k: w[k].clone().requires_grad_(True) for k in KINDS}
    wl = dict(w)
    wl.update(leaves)
    grads = dict(zip(KINDS, torch.autograd.grad(loss(wl), [leaves[k] for k in KINDS])))
    h = 1e-6
    for k in KINDS:
        flat = w[k].reshape(-1)
        for idx in sorted(set(int(i) for i in rs.randint(0, flat.numel(), 4))):
            vals = []
            for sgn in (1.0, -1.0):
                wp = dict(w)
                t = w[k].clone()
                t.reshape(-1)[idx] += sgn * h
                wp[k] = t
                with torch.no_grad():
                    vals.append(float(loss(wp)))
            fd = (vals[0] - vals[1]) / (2 * h)
            g = float(grads[k].reshape(-1)[idx])
            # central differences in float64: truncation O(h^2), rounding ~ 1e-16 |loss| / h = 1e-10 |loss|
            assert abs(fd - g) <= 1e-6 * max(1.0, float(grads[k].abs().max())) + 1e-5 * abs(g), (tag, k, idx, fd, g)
    # the last layer's residual output feeds nothing: its gradient is exactly zero (or absent)
    last = 'res_%d/W' % thp.num_layers
    lw = w[last].clone().requires_grad_(True)
    wl = dict(w)
    wl.update(leaves)
    wl[last] = lw
    g = torch.autograd.grad(loss(wl), [lw], allow_unused=True)[0]
    assert g is None or float(g.abs().max()) == 0
