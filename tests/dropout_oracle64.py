"""Float64 restatement of the teacher's TRAINING forward (wavenet/wavenet.py:204-239, 276-278): distill_oracle64.teacher_ff
with tf.layers.dropout(training=True) inserted where the reference inserts it, under the masks of the numpy twin
nsynth_wavenet_amd.train.dropout_keep instead of TensorFlow's random stream.  A kept element is
v / float32(1 - rate) (TF1's nn.dropout divides by the float32 keep probability), a dropped one is 0.

  dropout_inputs  site 0 on l and site 1 on s, both after s = skip_start(l) was computed from the undropped l
  dropout_all     site 0 on l before skip_start, site i on the output of residual layer i (1-based); the last layer's output
                  is read by nothing, so its mask changes no value
"""
import numpy as np
import torch

import distill_oracle64 as D
from nsynth_wavenet_amd.train import dropout_keep

MODES = ('dropout_inputs', 'dropout_all')


def _drop(v, seed, site, rate):
    B, T, C = v.shape
    keep = torch.as_tensor(dropout_keep(seed, site, B, C, T, rate).astype(np.float64), device=v.device)
    return v * keep / float(np.float32(1.0 - rate))


def teacher_ff(x, enc, w, hp, dropout, masks=None, pre=None):
    """distill_oracle64.teacher_ff (same arguments) with dropout = (mode, seed, rate)"""
    mode, seed, rate = dropout
    assert mode in MODES, mode
    relu = (lambda v, k: torch.relu(v)) if masks is None else (lambda v, k: v * masks[k])
    x = x[..., None]
    l = D._conv(D._delay(x, 1), w, 'conv_start')
    if mode == 'dropout_all':
        l = _drop(l, seed, 0, rate)
    s = D._conv(l, w, 'skip_start')
    if mode == 'dropout_inputs':
        l = _drop(l, seed, 0, rate)
        s = _drop(s, seed, 1, rate)
    for i in range(hp.num_layers):
        d = D._cond(D._conv(l, w, 'dilated_conv_%d' % (i + 1), 2 ** (i % hp.num_stages)),
                    D._conv(enc, w, 'mel_cond_%d' % (i + 1)))
        m = d.shape[2] // 2
        g = torch.sigmoid(d[..., :m]) * torch.tanh(d[..., m:])
        l = l + D._conv(g, w, 'res_%d' % (i + 1))
        s = s + D._conv(g, w, 'skip_%d' % (i + 1))
        if mode == 'dropout_all':
            l = _drop(l, seed, i + 1, rate)
    if pre is not None:
        pre['s'] = s.detach()
    s = relu(s, 's')
    h1 = D._cond(D._conv(s, w, 'out1'), D._conv(enc, w, 'mel_cond_out1'))
    if pre is not None:
        pre['h1'] = h1.detach()
    return D._conv(relu(h1, 'h1'), w, 'out2')
