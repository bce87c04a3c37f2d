"""tests/iaf_nll_grad_oracle64.py held to its own claims (CPU, float64), on the init='tf' models of
tests/iaf_encode_cases.py at z0 = case_inputs(name)[1] and x = the float64 forward of z0 (so encode(x) = z0):

  * the implicit gradient against central differences that RE-SOLVE the inverse, as directional derivatives in x, in the
    flows' variables and in the encoding, at 1e-4 relative.  Measured: x 4e-11 .. 7e-11 (h = 1e-6; 1e-5 already crosses ReLU
    kinks on S200: 9e-5), variables 7e-10 .. 8e-10 (h = 1e-7; 1e-6 crosses kinks: 1e-3), encoding 2e-10 .. 1e-9 (h = 1e-6);
  * near_tie_fraction <= 1e-4 and clamps_inactive on all five cases (what the GPU tests' bar presupposes);
  * the Jacobi update max |lam' - lam| / max |lam'| is <= 1e-9 within 16 sweeps (measured: from the 6th or 7th on);
  * a right-hand side that is non-zero at one t0 gives lam[t > t0] == 0 and lam[t0] = q[t0] / S[t0]."""
import numpy as np
import pytest
import torch

import iaf_inverse_oracle64 as inv
import iaf_nll_grad_oracle64 as N
import student_grad_oracle64 as S
from iaf_encode_cases import CASES, case_inputs, case_model

_SOLVED = {}


def solved(name):
    """per case, once: the graph at z0, x = its float64 forward, a dense cotangent and the oracle's gradients for it"""
    if name not in _SOLVED:
        hp, w = case_model(name)
        mel, z0 = case_inputs(name)
        G = N.NllGrad64(w, hp, mel, z0)
        c = N.dense_cotangent(z0.shape)
        _SOLVED[name] = (hp, w, mel, z0, G, G.values()['x'], c, G.grads(c, n_sweeps=24))
    return _SOLVED[name]


def _rel(label, fd, an):
    e = abs(fd - an) / abs(an)
    print('{}: central difference {:.10g}, oracle {:.10g}, relative error {:.2e}'.format(label, fd, an, e))
    return e


@pytest.mark.parametrize('name', ['S200', 'P384', 'G384'])
def test_implicit_gradient_against_central_differences(name):
    hp, w, mel, z0, G, x, c, g = solved(name)
    assert np.abs(inv.forward(mel, z0, w, hp, np.float64)['x'] - x).max() <= 1e-13       # the two float64 forwards agree
    rs = np.random.RandomState(3)
    v = rs.standard_normal(z0.shape)
    h = 1e-6
    fd = (N.value(mel, x + h * v, c, w, hp, z0) - N.value(mel, x - h * v, c, w, hp, z0)) / (2 * h)
    ex = _rel('{} <lam, v>'.format(name), fd, float((g['lam'] * v).sum()))
    d = {n: rs.standard_normal(np.shape(w[n])) for n in G.ora.names}
    h = 1e-7
    wp, wm = dict(w), dict(w)
    for n in d:
        wp[n] = np.asarray(w[n], np.float64) + h * d[n]
        wm[n] = np.asarray(w[n], np.float64) - h * d[n]
    fd = (N.value(mel, x, c, wp, hp, z0) - N.value(mel, x, c, wm, hp, z0)) / (2 * h)
    ew = _rel('{} <d theta, d>'.format(name), fd, float(sum((g['grads'][n] * d[n]).sum() for n in d)))
    encs = [e.detach() for e in G.encs]
    de = [torch.as_tensor(rs.standard_normal(tuple(e.shape))) for e in encs]
    h = 1e-6
    fd = (N.value_on_encodings(G.ora, [e + h * q for e, q in zip(encs, de)], x, c, z0) -
          N.value_on_encodings(G.ora, [e - h * q for e, q in zip(encs, de)], x, c, z0)) / (2 * h)
    ee = _rel('{} <d encoding, d>'.format(name), fd,
              float(sum((g['d_encoding'][s] * de[s].transpose(1, 2).numpy()).sum() for s in range(len(encs)))))
    assert ex <= 1e-4 and ew <= 1e-4 and ee <= 1e-4, (name, ex, ew, ee)


@pytest.mark.parametrize('name', sorted(CASES))
def test_cases_are_clear_of_ties_and_clamps(name):
    G = solved(name)[4]
    f = S.near_tie_fraction(G.aux)
    print('{}: near_tie_fraction {:.2e}'.format(name, f))
    assert f <= 1e-4
    assert S.clamps_inactive(G.aux)


@pytest.mark.parametrize('name', sorted(CASES))
def test_jacobi_update_falls_below_1e_9_within_16_sweeps(name):
    upd = solved(name)[7]['updates']
    print('{}: relative update per sweep {}'.format(name, ' '.join('{:.1e}'.format(u) for u in upd[:16])))
    assert upd[0] == 1.0                        # from zero the first sweep is all update
    assert upd[15] <= 1e-9 and min(upd[:16]) <= 1e-9


@pytest.mark.parametrize('name', ['S200', 'P384'])
def test_the_solve_is_upper_triangular(name):
    """A^T is upper triangular with diagonal S: the future of t0 stays exactly zero and lam[t0] = q[t0] / S[t0]"""
    _, _, _, z0, G, _, _, _ = solved(name)
    B, T = z0.shape
    S_ = G.S.numpy()
    for t0 in (0, T // 2 + 1, T - 2):
        q = np.zeros((B, T))
        q[:, t0] = np.random.RandomState(t0).standard_normal(B) + 2.0
        lam, _ = G.solve(q, np.zeros((B, T)), n_sweeps=8)
        lam = lam.numpy()
        assert np.all(lam[:, t0 + 1:] == 0), (name, t0)
        assert np.abs(lam[:, t0] - q[:, t0] / S_[:, t0]).max() <= 4 * np.finfo(np.float64).eps * np.abs(lam[:, t0]).max()
        if t0 > 0:
            assert np.abs(lam[:, :t0]).max() > 0
