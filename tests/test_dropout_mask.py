"""CPU tests of the dropout mask's numpy twin: nsynth_wavenet_amd.train.dropout_keep, the counter hash
keep(seed, site, b, c, t) = word t % 4 of Philox4x32-10(key = seed, counter = (t // 4, c, site, b)) >= thr, and
dropout_step_seed.  tests/test_gpu_teacher_dropout.py holds the device function to these bits.

Statistical checks: N = 2^20 elements per check, every share within 5 sigma with sigma = sqrt(rate (1 - rate) / N) -- the keep
share's own deviation, and for the agreement shares no more than theirs (rate^2 + (1 - rate)^2 is never closer to 0 or 1 than
the rate is), so the bar is the stricter of the two readings."""
import json
import os

import numpy as np
import pytest

from nsynth_wavenet_amd.train import dropout_keep, dropout_step_seed, dropout_threshold

SEED = 0x1234567887654321
B, C, T = 4, 512, 512
N = B * C * T
RATES = [0.5, 0.3, 0.05]


def test_same_arguments_same_bits():
    a = dropout_keep(SEED, 3, 2, 64, 260, 0.3)
    b = dropout_keep(SEED, 3, 2, 64, 260, 0.3)
    assert a.dtype == np.bool_ and a.shape == (2, 260, 64)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, dropout_keep(SEED + 1, 3, 2, 64, 260, 0.3))
    assert not np.array_equal(a, dropout_keep(SEED + 2 ** 32, 3, 2, 64, 260, 0.3)), 'the high seed word is part of the key'
    assert not np.array_equal(a, dropout_keep(SEED, 4, 2, 64, 260, 0.3))


def test_bits_do_not_depend_on_the_extent():
    small = dropout_keep(SEED, 1, 2, 64, 201, 0.5)
    for shape in [(3, 64, 201), (2, 128, 201), (2, 64, 460), (5, 192, 1027)]:
        big = dropout_keep(SEED, 1, shape[0], shape[1], shape[2], 0.5)
        assert np.array_equal(big[:2, :201, :64], small), shape


def test_rate_zero_keeps_everything():
    assert dropout_threshold(0.0) == 0
    assert dropout_keep(SEED, 0, 3, 64, 260, 0.0).all()
    assert dropout_threshold(1.0 - 2.0 ** -40) == 2 ** 32 - 1
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError):
            dropout_keep(SEED, 0, 1, 8, 8, bad)


def test_a_smaller_rate_keeps_a_superset():
    lo, hi = dropout_keep(SEED, 2, 1, 64, 256, 0.05), dropout_keep(SEED, 2, 1, 64, 256, 0.5)
    assert not (hi & ~lo).any()


@pytest.mark.parametrize('rate', RATES)
def test_statistics(rate):
    assert N == 2 ** 20
    sigma = np.sqrt(rate * (1.0 - rate) / N)
    agree = rate ** 2 + (1.0 - rate) ** 2
    base = dropout_keep(SEED, 0, B + 1, C + 1, T + 1, rate)
    k = base[:B, :T, :C]
    share = k.mean()
    print('rate {}: keep share {:.6f} (expected {:.6f}, {:+.2f} sigma)'.format(rate, share, 1 - rate, (share - (1 - rate)) / sigma))
    assert abs(share - (1.0 - rate)) <= 5 * sigma
    others = {'site 0 / 1': dropout_keep(SEED, 1, B, C, T, rate),
              'seed / seed + 1': dropout_keep(SEED + 1, 0, B, C, T, rate),
              'b / b + 1': base[1:, :T, :C],
              't / t + 1': base[:B, 1:, :C],
              'c / c + 1': base[:B, :T, 1:]}
    for name, o in others.items():
        assert o.shape == k.shape
        a = (o == k).mean()
        print('rate {}: agreement {} {:.6f} (expected {:.6f}, {:+.2f} sigma)'.format(rate, name, a, agree, (a - agree) / sigma))
        assert abs(a - agree) <= 5 * sigma, name


@pytest.mark.parametrize('base', [0, 0xFEDCBA9876543210])
def test_step_seeds_are_distinct(base):
    seeds = [dropout_step_seed(base, k) for k in range(10 ** 4 + 1)]
    assert seeds[0] == base and all(0 <= s < 2 ** 64 for s in seeds)
    assert len(set(seeds)) == len(seeds)
    assert dropout_step_seed(dropout_step_seed(base, 7), 0) == dropout_step_seed(base, 7)


def test_loss_and_weight_grads_refuses_a_config_without_dropout():
    """the refusal comes before the engine is touched: the engine here is a stand-in"""
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'config_jsons', 'wavenet_mol.json')
    with open(path) as f:
        cfgd = json.load(f)
    assert cfgd.get('dropout_inputs') is True
    cfgd.pop('dropout_inputs')
    net = Wavenet(cfgd, engine=object())
    with pytest.raises(ValueError, match='neither dropout_inputs nor dropout_all'):
        net.loss_and_weight_grads({'wav': None, 'mel': None}, dropout_seed=1)
    with_key = Wavenet(dict(cfgd, dropout_all=True), engine=object())
    assert with_key.dropout_rate == 0.05
    assert Wavenet(dict(cfgd, dropout_inputs=True), engine=object()).dropout_rate == 0.5
    assert Wavenet(dict(cfgd, dropout_inputs=True, dropout_rate=0.3), engine=object()).dropout_rate == 0.3
