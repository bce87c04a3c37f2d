"""CPU checks of the float64 autograd oracle of the student's weight gradients (tests/student_grad_oracle64.py): its values
against oracle.torch_ref.StudentRef in float64, its gradients against central differences, its variable list against
weights.expected_variables."""
import re

import numpy as np
import pytest
import torch

import student_grad_oracle64 as S
from nsynth_wavenet_amd import weights as wts
from oracle import wavenet_np as O
from oracle.torch_ref import StudentRef

CASES = {'shared': S.case_config(8, 16, 3, [2, 3], True, 'logistic'),
         'private': S.case_config(8, 16, 3, [4, 1], False, 'gauss')}
B, F, T = 2, 3, 24


def _case(tag):
    cfgd = CASES[tag]
    hp = O.HP(cfgd)
    w = O.synth_weights(hp, 'student', seed=31, init='unit')
    mel, noise, cot = S.case_inputs(B, F, T, seed=5)
    return hp, w, mel, noise, cot


@pytest.mark.parametrize('tag', sorted(CASES))
def test_values_equal_student_ref(tag):
    hp, w, mel, noise, cot = _case(tag)
    ref = StudentRef(w, hp, dtype=torch.float64).feed_forward(mel, noise)
    got = S.StudentGrad64(w, hp).grads(mel, noise, *cot)
    for k in ('x', 'mean_tot', 'scale_tot'):
        assert np.abs(got['values'][k] - ref[k]).max() <= 1e-10, k
    assert S.clamps_inactive(got['aux']) and S.near_tie_fraction(got['aux']) == 0.0
    n_stacks = 1 if tag == 'shared' else len(hp.num_iaf_layers)
    assert got['d_encoding'].shape == (n_stacks, B, F * 8, hp.deconv_width)


@pytest.mark.parametrize('tag', sorted(CASES))
def test_gradients_match_central_differences(tag):
    hp, w, mel, noise, cot = _case(tag)
    orc = S.StudentGrad64(w, hp)
    g = orc.grads(mel, noise, *cot)['grads']
    rs = np.random.RandomState(9)
    kinds = {}
    for n in orc.names:                              # one variable of each kind: the last flow's, its last layer's
        kinds[re.sub(r'^iaf_\d+/|_\d+(?=/)', '', n)] = n
    assert len(kinds) == 16, sorted(kinds)
    eps = 1e-6
    for n in sorted(kinds.values()):
        a = np.asarray(w[n], np.float64)
        idx = tuple(int(rs.randint(s)) for s in a.shape)
        vals = []
        for sgn in (+1, -1):
            p = a.copy()
            p[idx] += sgn * eps
            vals.append(orc.surrogate(mel, noise, cot, {n: p}))
        fd = (vals[0] - vals[1]) / (2 * eps)
        scale = max(np.abs(g[n]).max(), 1e-12)
        assert abs(fd - g[n][idx]) <= 1e-6 * scale + 1e-7, (n, idx, fd, g[n][idx])


def test_d_encoding_matches_central_differences():
    """the cotangent of the conditioning: one element inside the centre crop, and exact zeros outside a shorter crop"""
    hp, w, mel, noise, cot = _case('private')
    orc = S.StudentGrad64(w, hp)
    Ts = 16                                          # 24 encoded columns, 16 samples: a centre crop of 4 on each side
    noise, cot = noise[:, :Ts], [c[:, :Ts] for c in cot]
    r = orc.grads(mel, noise, *cot)
    d = r['d_encoding']
    assert np.all(d[:, :, :4] == 0) and np.all(d[:, :, 20:] == 0) and np.abs(d[:, :, 4:20]).min() > 0
    encs = orc.encodings(mel)
    s, b, t, c = 1, 1, 9, 3
    vals = []
    for sgn in (+1, -1):
        e2 = [e.clone() for e in encs]
        e2[s][b, c, t] += sgn * 1e-6
        with torch.no_grad():
            out, _ = orc.forward(noise, e2)
        vals.append(float(sum((out[k] * torch.as_tensor(v, dtype=torch.float64)).sum()
                              for k, v in zip(('x', 'mean_tot', 'scale_tot'), cot))))
    fd = (vals[0] - vals[1]) / 2e-6
    assert abs(fd - d[s, b, t, c]) <= 1e-6 * np.abs(d).max() + 1e-7


@pytest.mark.parametrize('cfgd', [S.S1, S.S2] + sorted(CASES.values(), key=str), ids=['S1', 'S2', 'a', 'b'])
def test_variable_list(cfgd):
    hp = O.HP(cfgd)
    want = [n for n, _ in wts.expected_variables(hp, 'student') if 'trans_conv' not in n]
    assert S.variable_names(hp) == want
    w = O.synth_weights(hp, 'student', seed=1, init='tf')
    assert set(want) | {n for n in w if 'trans_conv' in n} == set(w)
