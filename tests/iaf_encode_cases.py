"""The models and inputs of the IAF-encode tests (tests/test_iaf_inverse_oracle.py on the CPU, tests/test_gpu_iaf_encode.py
on the GPU), all with synth_weights(init='tf', seed=1234).  With init='unit' the inverse is chaotic in float32 (errors of
order 1), so no accuracy test uses it.

  S  the STUDENT dict of tests/test_gpu_train_cli.py: 5 layers, 3 stages, width 64 / deconv_width 64 (the generic fp32 kernels)
  P  parallel_wavenet.json with num_stages = 7, num_iaf_layers = [7, 8]: the MFMA path, dilations wrap, T off the 256 tile
  G  parallel_wavenet_gauss.json with the same two keys
"""
import functools

import numpy as np

from conftest import load_json
from oracle import wavenet_np as wn
import iaf_inverse_oracle64 as inv
from test_gpu_train_cli import STUDENT

# name -> (model, batch, frames); T = iaf_length(frames): 200, 400, 384, 576, 384
CASES = {'S200': ('S', 2, 1), 'S400': ('S', 2, 2), 'P384': ('P', 2, 2), 'P576': ('P', 1, 3), 'G384': ('G', 2, 2)}


def model_config(model):
    if model == 'S':
        return dict(STUDENT)
    cfg = dict(load_json('parallel_wavenet.json' if model == 'P' else 'parallel_wavenet_gauss.json'))
    cfg.update(num_stages=7, num_iaf_layers=[7, 8])
    return cfg


@functools.lru_cache(maxsize=None)
def _model(model, init):
    hp = wn.HP(model_config(model))
    return hp, wn.synth_weights(hp, 'student', seed=1234, init=init)


def case_model(name, init='tf'):
    """(hp, weights) of the case's model"""
    return _model(CASES[name][0], init)


def case_inputs(name):
    """mel [B,F,80] from RandomState(5).uniform, z0 [B,T] logistic or normal from RandomState(6); float64"""
    model, B, F = CASES[name]
    hp, _ = case_model(name)
    mel = np.random.RandomState(5).uniform(size=(B, F, 80))
    z0 = inv.latent_draw(hp.get('loss_type', 'logistic'), (B, wn.iaf_length(F, hp)), seed=6)
    return mel, z0
