"""Engine.iaf_encode / wn_iaf_encode and the latent log-likelihood on the GPU against the CPU inverse of
tests/iaf_inverse_oracle64.py, on the models of tests/iaf_encode_cases.py (init='tf').

The round-trip bar is not a constant: per case the float32 oracle sweeps give the yardstick, max |z32 - z64|, the engine gets
4 x that (it sums in another order, and model P / G in the split-fp16 form), and a case is admissible only while the
yardstick stays below 1e-4 max|z|.  Measured on MI355X (yardstick | engine error | max|z| | engine sweeps):
    S200  1.10e-6 | 9.5e-7  | 6.32 | 11         P384  1.47e-6 | 7.9e-7  | 6.32 | 150
    S400  1.31e-6 | 9.1e-7  | 10.0 | 17         P576  1.11e-6 | 1.02e-6 | 6.32 | 224
    G384  6.1e-7  | 5.9e-7  | 3.69 | 151
Identity 2 peaks at 0.45-0.50 of its bound on every case.  log_prob error | its bound d + e_ls: S200 7.0e-7 | 1.12e-6,
S400 6.4e-7 | 1.08e-6, P384 7.1e-7 | 1.14e-6, P576 8.6e-7 | 1.29e-6, G384 1.65e-6 | 2.39e-6.  tol = 1e-6 stops after 5-6
sweeps (S400, P576, G384).  The init='unit' stress case converged in 194 sweeps with nothing clamped.
"""
import ctypes

import numpy as np
import pytest

import iaf_inverse_oracle64 as inv
from iaf_encode_cases import CASES, case_inputs, case_model, model_config

pytestmark = pytest.mark.gpu
U = 2.0 ** -24

_ENGINES, _SOLVED = {}, {}


def _np(t):
    return t.detach().cpu().numpy()


def _engine(model, init='tf'):
    """one engine per (model, init) for the module"""
    from nsynth_wavenet_amd.engine import Engine
    from iaf_encode_cases import _model
    if (model, init) not in _ENGINES:
        _ENGINES[(model, init)] = Engine(model_config(model)).load_weights(_model(model, init)[1])
    return _ENGINES[(model, init)]


@pytest.fixture(scope='module', autouse=True)
def _close_engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()
    _SOLVED.clear()


def _solved(name):
    """Per case, once: the engine's x for z0, its encode, the float64 inverse of that x (sweeps started at z0: the fixed point
    is unique, the start only shortens the loop) and the float32 oracle sweeps from zero, the yardstick."""
    if name in _SOLVED:
        return _SOLVED[name]
    hp, w = case_model(name)
    mel, z0 = case_inputs(name)
    eng = _engine(CASES[name][0])
    z0f = z0.astype(np.float32)
    x = eng.iaf_generate(mel, noise=z0f, want=('x',))['x']
    r = eng.iaf_encode(x, mel, want=('z', 'mean_tot', 'scale_tot', 'log_prob'))
    xn = _np(x)
    r64 = inv.inverse(mel, xn, w, hp, np.float64, z_init=z0f)
    r32 = inv.inverse(mel, xn, w, hp, np.float32)
    assert r64['converged'] and r32['converged']
    s = {'eng': eng, 'mel': mel, 'z0': z0f, 'x': x, 'r': r, 'z': _np(r['z']), 'r64': r64, 'hp': hp,
         'yard': float(np.abs(r32['z'].astype(np.float64) - r64['z']).max()), 'zmax': float(np.abs(r64['z']).max())}
    s['err'] = float(np.abs(s['z'].astype(np.float64) - r64['z']).max())
    _SOLVED[name] = s
    return s


def _identity(eng, mel, r, x):
    """identity 2: generating from the encode's z, in the form the encode reports, gives x back to four roundings"""
    g = eng.iaf_generate(mel, noise=r['z'], want=('x', 'mean_tot'), form=r['form'])
    xg, m, xn = _np(g['x']).astype(np.float64), _np(g['mean_tot']).astype(np.float64), _np(x).astype(np.float64)
    bound = 4 * U * (np.abs(xn) + np.abs(m))
    excess = np.abs(xg - xn) - bound
    print('identity: max |x_gen - x| = {:.3g}, max of (error / bound) = {:.3g}'.format(
        np.abs(xg - xn).max(), (np.abs(xg - xn) / np.maximum(bound, 1e-300)).max()))
    assert (excess <= 0).all(), float(excess.max())


@pytest.mark.parametrize('name', sorted(CASES))
def test_round_trip(name):
    s = _solved(name)
    r, T = s['r'], s['z'].shape[1]
    print('{}: yardstick {:.3g}, engine error {:.3g}, max|z| {:.3g}, sweeps {}, form {}'.format(
        name, s['yard'], s['err'], s['zmax'], r['sweeps'], r['form']))
    assert s['yard'] <= 1e-4 * s['zmax'], 'case not admissible'
    assert bool(r['converged'].all()) and r['clamped'] == 0 and r['sweeps'] <= T
    assert (_np(r['front']) == T).all()
    assert s['err'] <= 4 * s['yard']


@pytest.mark.parametrize('name', sorted(CASES))
def test_fixed_point_identity(name):
    s = _solved(name)
    _identity(s['eng'], s['mel'], s['r'], s['x'])


def test_fixed_point_identity_on_foreign_audio():
    """an x the student did not produce: 0.3 sin + 0.05 noise on model S"""
    import torch
    hp, w = case_model('S200')
    mel, _ = case_inputs('S200')
    eng = _engine('S')
    T = eng.iaf_length(mel.shape[1])
    t = np.arange(T)
    x = (0.3 * np.sin(2 * np.pi * t / 37.0)[None, :] + 0.05 * np.random.RandomState(7).standard_normal((2, T))).astype(np.float32)
    r = eng.iaf_encode(x, mel)
    assert bool(r['converged'].all()) and r['clamped'] == 0 and r['sweeps'] <= T
    _identity(eng, mel, r, torch.as_tensor(x))
    r64 = inv.inverse(mel, x, w, hp, np.float64)
    r32 = inv.inverse(mel, x, w, hp, np.float32)
    yard = float(np.abs(r32['z'] - r64['z']).max())
    err = float(np.abs(_np(r['z']) - r64['z']).max())
    print('foreign audio: yardstick {:.3g}, engine error {:.3g}, max|z| {:.3g}'.format(yard, err, np.abs(r64['z']).max()))
    assert err <= 4 * yard


@pytest.mark.parametrize('name', ['S200', 'P384'])
def test_prefix_and_restart(name):
    s = _solved(name)
    eng, T = s['eng'], s['z'].shape[1]
    for k in (1, 3, 8):
        p = eng.iaf_encode(s['x'], s['mel'], max_sweeps=k)
        assert p['sweeps'] == k
        assert _np(p['z'])[:, :k].tobytes() == s['z'][:, :k].tobytes(), k
        assert (_np(p['front']) >= k - 1).all(), (k, _np(p['front']))
    again = eng.iaf_encode(s['x'], s['mel'], z_init=s['r']['z'])
    assert again['sweeps'] == 1 and bool(again['converged'].all())
    assert _np(again['z']).tobytes() == s['z'].tobytes()
    # the sweeps of one encode do not depend on how they are cut into C calls
    one = eng.iaf_encode(s['x'], s['mel'], check_every=1)
    assert one['sweeps'] == s['r']['sweeps'] and _np(one['z']).tobytes() == s['z'].tobytes()


@pytest.mark.parametrize('name', ['S400', 'P576', 'G384'])
def test_stopping_on_tol(name):
    s = _solved(name)
    r = s['eng'].iaf_encode(s['x'], s['mel'], tol=1e-6)
    print('{}: tol 1e-6 stops after {} sweeps, bitwise after {}'.format(name, r['sweeps'], s['r']['sweeps']))
    assert bool(r['converged'].all()) and r['sweeps'] <= s['r']['sweeps']
    assert np.abs(_np(r['z']) - s['z']).max() <= 1e-4 * s['zmax']


@pytest.mark.parametrize('name', sorted(CASES))
def test_log_likelihood(name):
    s = _solved(name)
    r, r64 = s['r'], s['r64']
    lt = s['hp'].get('loss_type', 'logistic')
    want = inv.log_density(r64['z'], r64['log_scale_tot'], lt)
    e_ls = float(np.abs(np.log(_np(r['scale_tot']).astype(np.float64)) - r64['log_scale_tot']).max())
    d = s['err'] * (s['zmax'] if lt == 'gauss' else 1.0)
    lp = _np(r['log_prob']).astype(np.float64)
    err = float(np.abs(lp - want).max())
    print('{}: log_prob error {:.3g}, bound d + e_ls = {:.3g} + {:.3g}, mean log p = {:.6f}'.format(name, err, d, e_ls, want.mean()))
    assert err <= d + e_ls
    sums = _np(r['log_prob_sums'])
    assert sums.dtype == np.float64
    # a float64 sum of T values in another order: T rounding steps of the running sum at most
    assert np.abs(sums - lp.sum(axis=1)).max() <= lp.shape[1] * 2.0 ** -52 * np.abs(lp).sum(axis=1).max()
    # the model-level call: the same numbers, the loss their mean
    from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet
    if name == 'S200':
        pw = ParallelWavenet(model_config('S')).load_weights(case_model(name)[1])
        out = pw.log_prob({'wav': s['x'], 'mel': s['mel']})
        assert _np(out['log_probs']).tobytes() == _np(r['log_prob']).tobytes()
        assert abs(float(out['loss']) + lp.mean()) <= 1e-12 * max(1.0, abs(lp.mean()))
        enc = pw.encode({'x': s['x'], 'mel': s['mel']})
        assert _np(enc['z']).tobytes() == s['z'].tobytes() and enc['sweeps'] == r['sweeps']
        assert np.abs(_np(enc['log_scale_tot']) - np.log(_np(r['scale_tot']).astype(np.float64))).max() <= 4 * U * 2
        pw.engine.close()


def test_stress_unit_init():
    """init='unit' weights make the inverse chaotic in float32: no accuracy claim, only that the call comes back within T
    sweeps with a finite z and says what happened"""
    mel, z0 = case_inputs('S200')
    eng = _engine('S', 'unit')
    x = eng.iaf_generate(mel, noise=z0.astype(np.float32), want=('x',))['x']
    T = x.shape[1]
    r = eng.iaf_encode(x, mel, want=('z', 'mean_tot', 'scale_tot'))
    z = _np(r['z'])
    print('unit init: sweeps {}, converged {}, clamped {}, max|z| {:.3g}'.format(r['sweeps'], _np(r['converged']), r['clamped'],
                                                                                 np.abs(z).max()))
    assert r['sweeps'] <= T and np.isfinite(z).all() and np.abs(z).max() <= 64.0
    if bool(r['converged'].all()) and r['clamped'] == 0:
        _identity(eng, mel, r, x)
    else:
        assert r['clamped'] > 0 or not bool(r['converged'].all())


def test_refusals_by_name():
    import torch
    from nsynth_wavenet_amd.engine import Engine
    from nsynth_wavenet_amd import _lib
    from conftest import load_json
    s = _solved('S200')
    eng, x, mel = s['eng'], s['x'], s['mel']
    with pytest.raises(ValueError, match='n_sweeps must be >= 1'):
        eng.iaf_encode(x, mel, max_sweeps=0)
    with pytest.raises(ValueError, match='z_max must be > 0'):
        eng.iaf_encode(x, mel, z_max=0.0)
    with pytest.raises(ValueError, match='tol must be >= 0'):
        eng.iaf_encode(x, mel, tol=-1.0)
    # the C call itself: a short workspace, a null pointer
    B, F, T = 2, 1, x.shape[1]
    lib, h = eng.lib, eng._h
    need = lib.wn_iaf_encode_workspace_bytes(h, _lib.FORM_DEFAULT, B, F)
    assert need > lib.wn_iaf_workspace_bytes_form(h, _lib.FORM_DEFAULT, B, F) > 0
    ws = torch.empty(need, dtype=torch.uint8, device=eng.device)
    meld, z = eng._dev(mel), torch.zeros_like(x)
    meta = torch.zeros(B + 4, dtype=torch.int32, device=eng.device)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(xp, wsb, n=1):
        return lib.wn_iaf_encode(h, _lib.FORM_DEFAULT, P(meld), B, F, xp, P(z), n, 64.0, 0.0, 1, None, None, P(meta),
                                 ctypes.c_void_p(meta.data_ptr() + 4 * B), P(ws), wsb, None)
    assert call(P(x), need - 1) == -12 and b'workspace' in lib.wn_last_error(h)
    assert call(None, need) == -22 and b'null' in lib.wn_last_error(h)
    assert call(P(x), need, n=0) == -22 and b'n_sweeps' in lib.wn_last_error(h)
    torch.cuda.synchronize()
    assert not z.any(), 'a refused call wrote z'
    # a teacher, and a mu-law student
    teacher = Engine(load_json('wavenet_mol.json'))
    assert teacher.lib.wn_iaf_encode_workspace_bytes(teacher._h, _lib.FORM_DEFAULT, B, F) == 0
    with pytest.raises(ValueError, match='not a ParallelWavenet student'):
        teacher.iaf_encode(x, mel)
    teacher.close()
    mu = Engine(dict(model_config('S'), use_mu_law=True))
    assert mu.lib.wn_iaf_encode_workspace_bytes(mu._h, _lib.FORM_DEFAULT, B, F) == 0
    with pytest.raises(ValueError, match='mu-law'):
        mu.iaf_encode(x, mel)
    mu.close()


@pytest.mark.parametrize('name', ['S200', 'P384'])
def test_generate_is_untouched_and_buffers_do_not_matter(name):
    """iaf_generate before and after an encode on the same handle: the same bits.  The encode's workspace and iterate
    pre-filled with 0x00 and with 0xFF: the same z bits."""
    mel, z0 = case_inputs(name)
    eng = _engine(CASES[name][0])
    want = ('wav', 'x', 'mean_tot', 'scale_tot')
    before = eng.iaf_generate(mel, seed=11, want=want)
    x = before['x']
    zs = []
    for fill in (0x00, 0xFF):
        eng.iaf_encode(x, mel, max_sweeps=1)                 # the workspace exists
        eng._enc_ws.fill_(fill)
        if eng._ws is not None:
            eng._ws[64:].fill_(fill)                         # (its first 64 bytes are the generate calls' range words)
        zs.append(_np(eng.iaf_encode(x, mel)['z']))
    assert zs[0].tobytes() == zs[1].tobytes()
    after = eng.iaf_generate(mel, seed=11, want=want)
    for k in want:
        assert _np(before[k]).tobytes() == _np(after[k]).tobytes(), k
