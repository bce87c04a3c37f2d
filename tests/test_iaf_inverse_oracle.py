"""tests/iaf_inverse_oracle64.py held to its own claims (CPU): the prefix property of the sweeps, convergence in at most T
sweeps, and the float64 round trip z0 -> x -> z0, on the models tests/test_gpu_iaf_encode.py runs."""
import numpy as np
import pytest

import iaf_inverse_oracle64 as inv
from iaf_encode_cases import CASES, case_inputs, case_model


@pytest.fixture(scope='module')
def solved():
    """per case: the float64 forward of z0 and the float64 sweeps on it, every iterate kept -- computed once"""
    out = {}
    for name in CASES:
        hp, w = case_model(name)
        mel, z0 = case_inputs(name)
        x = inv.forward(mel, z0, w, hp, np.float64)['x']
        trace = []
        r = inv.inverse(mel, x, w, hp, np.float64, trace=trace)
        out[name] = (z0, x, r, trace)
    return out


@pytest.mark.parametrize('name', sorted(CASES))
def test_float64_round_trip(solved, name):
    """x = forward64(z0); the sweeps return z0 to 1e-12 or better (measured: 2e-15 .. 4e-14), bitwise converged in <= T sweeps"""
    z0, x, r, _ = solved[name]
    T = x.shape[1]
    err = float(np.abs(r['z'] - z0).max())
    print('{}: T = {}, {} sweeps, max |z - z0| = {:.3g}, max |z0| = {:.3g}'.format(name, T, r['sweeps'], err, np.abs(z0).max()))
    assert r['converged'] and r['sweeps'] <= T
    assert err <= 1e-12


@pytest.mark.parametrize('name', sorted(CASES))
def test_prefix_property(solved, name):
    """sweep k changes nothing before index k - 1 (its input was exact on [0, k - 1)), and z[:, :k] is final after it"""
    _, _, r, trace = solved[name]
    zero = np.zeros_like(trace[0])
    for k in range(1, len(trace) + 1):
        before = trace[k - 2] if k >= 2 else zero
        assert before[:, :k - 1].tobytes() == trace[k - 1][:, :k - 1].tobytes(), (name, k)
        assert trace[k - 1][:, :k].tobytes() == r['z'][:, :k].tobytes(), (name, k)


def test_float32_sweeps_are_the_yardstick():
    """the float32 loop on the float64 x: converged in <= T sweeps, and within 1e-4 max|z| of z0 (the admissibility bar of the
    GPU test's cases; measured 6.5e-7 .. 1.6e-6 at max|z| 3.7 .. 10)"""
    for name in sorted(CASES):
        hp, w = case_model(name)
        mel, z0 = case_inputs(name)
        x = inv.forward(mel, z0, w, hp, np.float64)['x'].astype(np.float32)
        r = inv.inverse(mel, x, w, hp, np.float32)
        err = float(np.abs(r['z'].astype(np.float64) - z0).max())
        print('{}: float32 sweeps {}, max |z32 - z0| = {:.3g}, max |z0| = {:.3g}, scale_tot in [{:.3g}, {:.3g}]'.format(
            name, r['sweeps'], err, np.abs(z0).max(), r['scale_tot'].min(), r['scale_tot'].max()))
        assert r['converged'] and r['sweeps'] <= x.shape[1]
        assert r['z'].dtype == np.float32
        assert err <= 1e-4 * np.abs(z0).max()


def test_max_sweeps_and_restart():
    """max_sweeps = k stops after k sweeps; started from the converged z one sweep confirms it"""
    hp, w = case_model('S200')
    mel, z0 = case_inputs('S200')
    x = inv.forward(mel, z0, w, hp, np.float64)['x']
    full = inv.inverse(mel, x, w, hp, np.float64)
    part = inv.inverse(mel, x, w, hp, np.float64, max_sweeps=3)
    assert part['sweeps'] == 3 and not part['converged']
    assert part['z'][:, :3].tobytes() == full['z'][:, :3].tobytes()
    again = inv.inverse(mel, x, w, hp, np.float64, z_init=full['z'])
    assert again['sweeps'] == 1 and again['converged']


def test_log_density_is_the_forward_density():
    """log f integrates to one (trapezoid on a wide grid) and the change of variables holds: a latent shifted by dz moves x by
    scale dz, so p_x(x) = f(z) / scale"""
    g = np.linspace(-40.0, 40.0, 400001)
    for lt in ('logistic', 'gauss'):
        p = np.exp(inv.log_density(g, np.zeros_like(g), lt))
        assert abs(float(np.sum(0.5 * (p[1:] + p[:-1]) * np.diff(g))) - 1.0) < 1e-9
        ls = np.log(0.3)
        assert np.allclose(inv.log_density(g, ls * np.ones_like(g), lt), inv.log_density(g, np.zeros_like(g), lt) - ls,
                           rtol=0, atol=1e-12)
