"""wn_iaf_latent_log_prob_grad and wn_iaf_adjoint (csrc/wn_iaf_nll.hip) behind Engine.iaf_latent_log_prob_grad
and Engine.iaf_adjoint, against tests/iaf_nll_grad_oracle64.py (held to central differences by
tests/test_iaf_nll_grad_oracle.py) on the init='tf' models of tests/iaf_encode_cases.py.

The bar of every gradient is the project's: max |g - g64| <= TOL max |g64| (TOL of tests/test_gpu_distill_grad.py), per row
for lam.  The tapes are written at z = float32(z0), which is where the oracle stands as well."""
import ctypes

import numpy as np
import pytest

import iaf_nll_grad_oracle64 as N
from iaf_encode_cases import CASES, model_config
from test_gpu_distill_grad import TOL

pytestmark = pytest.mark.gpu
U = 2.0 ** -24

_ENGINES, _TAPES = {}, {}


def _np(t):
    return t.detach().cpu().numpy()


def _new_engine(model):
    from nsynth_wavenet_amd.engine import Engine
    from iaf_encode_cases import _model
    return Engine(model_config(model)).load_weights(_model(model, 'tf')[1])


def _engine(model):
    if model not in _ENGINES:
        _ENGINES[model] = _new_engine(model)
    return _ENGINES[model]


@pytest.fixture(scope='module', autouse=True)
def _close_engines():
    yield
    _TAPES.clear()
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def _taped(name):
    """per case, once: (engine, oracle case, the tape forward's outputs at z, the tape)"""
    if name not in _TAPES:
        o = N.case_oracle(name)
        eng = _engine(CASES[name][0])
        ff, tape = eng.iaf_forward_train_tape(o['mel'], noise=o['z'])
        _TAPES[name] = (eng, o, ff, tape)
    return _TAPES[name]


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


# ---- the cotangent kernel ----
@pytest.mark.parametrize('model', ['S', 'G'])
@pytest.mark.parametrize('shape', [(1, 1), (3, 37), (2, 1025), (4, 256)])      # the last one takes the 16-byte path
def test_cotangents_within_one_rounding(model, shape):
    """both loss types, d_log_prob null and dense; z holds 0, +-11.5 and +-40; every element within one float32 rounding of
    the float64 value (and of the smallest normal where that underflows)"""
    import torch
    eng = _engine(model)
    gauss = model == 'G'
    rs = np.random.RandomState(shape[1])
    n = shape[0] * shape[1]
    z = (4.0 * rs.standard_normal(n)).astype(np.float32)
    special = np.array([0.0, 11.5, -11.5, 40.0, -40.0], np.float32)
    z[:min(n, 5)] = special[:min(n, 5)]
    z = z.reshape(shape)
    s = np.exp(rs.uniform(-9.0, 7.0, shape)).astype(np.float32)
    dense = rs.standard_normal(shape).astype(np.float32)
    for c32 in (None, dense):
        g, d = eng.iaf_latent_log_prob_grad(z, s, c32)
        c = -1.0 / n if c32 is None else c32.astype(np.float64)
        z64 = z.astype(np.float64)
        g64 = c * (-z64 if gauss else -np.tanh(0.5 * z64))
        d64 = -c / s.astype(np.float64)
        for label, got, ref in (('g_z', g, g64), ('d_scale_tot', d, d64)):
            got = _np(got).astype(np.float64)
            assert got.shape == shape
            err = np.abs(got - ref) / np.maximum(np.abs(ref), 2.0 ** -126)
            print('{} {} {} {}: max error {:.3g} roundings'.format(model, shape, 'null' if c32 is None else 'dense', label,
                                                                  err.max() / U))
            assert err.max() <= U, (label, float(err.max() / U))
    assert not torch.isnan(g).any()


def test_cotangent_refusals():
    import torch
    eng = _engine('S')
    lib, h = eng.lib, eng._h
    a = torch.zeros(8, dtype=torch.float32, device='cuda')
    p = ctypes.c_void_p(a.data_ptr())
    for args in ((None, p, 1, 8, None, p, p), (p, None, 1, 8, None, p, p), (p, p, 1, 8, None, None, p), (p, p, 1, 8, None, p, None)):
        assert lib.wn_iaf_latent_log_prob_grad(h, *args, None) == -22
        assert b'null z/scale_tot/g_z/d_scale_tot' in lib.wn_last_error(h)
    assert lib.wn_iaf_latent_log_prob_grad(h, p, p, 0, 8, None, p, p, None) == -22
    assert b'B and T must be >= 1' in lib.wn_last_error(h)
    assert lib.wn_iaf_latent_log_prob_grad(None, p, p, 1, 8, None, p, p, None) == -22


# ---- the adjoint with z given ----
@pytest.mark.parametrize('name', sorted(CASES))
def test_adjoint_matches_the_oracle(name):
    """dense random d_log_prob; after 16 sweeps lam is within the bar of the oracle's, row by row"""
    eng, o, ff, tape = _taped(name)
    ref = o['dense']
    g_z, d_s = eng.iaf_latent_log_prob_grad(o['z'], ff['scale_tot'], o['c'].astype(np.float32))
    r = eng.iaf_adjoint(tape, g_z, d_s, max_sweeps=16, tol=0.0)
    assert r['sweeps'] == 16 and r['replaced'] == 0
    lam = _np(r['lam']).astype(np.float64)
    assert lam.shape == ref['lam'].shape and np.isfinite(lam).all()
    e = np.abs(lam - ref['lam']).max(axis=1) / np.abs(ref['lam']).max(axis=1)
    res = _np(r['resid']).astype(np.float64)
    print('ADJ {} per row max |lam - lam64| / max |lam64| = {}; last update / max |lam| = {}'.format(
        name, ' '.join('{:.2e}'.format(v) for v in e), ' '.join('{:.2e}'.format(v) for v in res[:, 0] / res[:, 1])))
    assert np.abs(res[:, 1] - np.abs(lam).max(axis=1)).max() == 0          # resid[:, 1] is max |lam| of the row
    assert e.max() <= TOL, (name, e)


@pytest.mark.parametrize('name', ['S200', 'P384'])
def test_triangular_property(name):
    """a right-hand side that is non-zero at one t0: lam[t > t0] is exactly 0 and lam[t0] is q / S -- one rounding after one
    sweep; after 16, lam' = lam + ((q - lam S) / S) has the rounding of lam S and its own, two in all.  A zero row of the
    right-hand side gives an exactly zero row."""
    import torch
    eng, o, ff, tape = _taped(name)
    B, T = o['z'].shape
    S = _np(ff['scale_tot']).astype(np.float64)
    zero = np.zeros((B, T), np.float32)
    for t0 in (0, T // 2 + 1, T - 2):
        q = zero.copy()
        q[-1, t0] = 1.75 + t0 / 1024.0            # row 0 of a batch of two stays zero
        want = q[-1, t0] / S[-1, t0]
        for sweeps, roundings in ((1, 1), (16, 2)):
            r = eng.iaf_adjoint(tape, q, zero, max_sweeps=sweeps, tol=0.0)
            lam = _np(r['lam'])
            assert np.all(lam[:, t0 + 1:] == 0), (t0, sweeps, 'the future leaks into lam')
            assert abs(lam[-1, t0] - want) <= roundings * U * abs(want) * (1 + 2 * U), (t0, sweeps, lam[-1, t0], want)
            if B > 1:
                assert int((_bits(r['lam'][0]) & 0x7fffffff != 0).sum()) == 0, 'a zero row must stay exactly zero'
            if sweeps > 1 and t0 > 0:
                assert np.abs(lam[-1, :t0]).max() > 0


# ---- robustness ----
def _raw(eng, shape, tape, tape_bytes, g_z, d_s, lam, n_sweeps, tol, resid, counts, ws, ws_bytes):
    """wn_iaf_adjoint itself on the caller's buffers (None: a null pointer) -> (return code, message)"""
    import torch
    B, F, T = shape
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rc = eng.lib.wn_iaf_adjoint(eng._h, p(tape), tape_bytes, p(g_z), None, p(d_s), B, F, T, p(lam), n_sweeps, tol, p(resid),
                                p(counts), p(ws), ws_bytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, eng.lib.wn_last_error(eng._h).decode() if rc else ''


def test_workspace_contents_guards_and_repeats():
    """workspaces pre-filled with 0x00 and with 0xFF give the same bits; the floats behind lam and resid stay untouched; a
    repeated call is bit-identical; iaf_backward_input / _weights return the bits of calls made before any adjoint call"""
    import torch
    o = N.case_oracle('S200')
    eng = _new_engine('S')                      # an engine no adjoint call has touched
    try:
        ff, tape = eng.iaf_forward_train_tape(o['mel'], noise=o['z'])
        B, T = o['z'].shape
        F = o['mel'].shape[1]
        g_z, d_s = eng.iaf_latent_log_prob_grad(o['z'], ff['scale_tot'], o['c'].astype(np.float32))
        cot = [torch.as_tensor(v, device='cuda') for v in (-o['dense']['lam'].astype(np.float32), np.zeros((B, T), np.float32))] + [d_s]
        before_in = eng.iaf_backward_input(tape, *cot)
        before_w = eng.iaf_backward_weights(tape, *cot)
        nb = int(eng.lib.wn_iaf_adjoint_workspace_bytes(eng._h, B, F, T))
        assert nb > int(eng.lib.wn_iaf_backward_input_workspace_bytes(eng._h, B, F, T)) > 0
        GUARD = 64
        runs = []
        for fill in (0x00, 0xFF, 0xFF):
            ws = torch.full((nb,), fill, dtype=torch.uint8, device='cuda')
            lam = torch.zeros(B * T + GUARD, dtype=torch.float32, device='cuda')
            resid = torch.zeros(2 * B + GUARD, dtype=torch.float32, device='cuda')
            lam[B * T:] = 12345.0
            resid[2 * B:] = 12345.0
            counts = torch.full((4,), -1, dtype=torch.int32, device='cuda')
            rc, msg = _raw(eng, (B, F, T), tape, tape.numel(), g_z, d_s, lam, 6, 0.0, resid, counts, ws, nb)
            assert rc == 0, msg
            torch.cuda.synchronize()
            assert bool((lam[B * T:] == 12345.0).all()) and bool((resid[2 * B:] == 12345.0).all())
            assert counts.tolist() == [0, B, 0, 0]
            runs.append((lam[:B * T].clone(), resid[:2 * B].clone()))
        for lam, resid in runs[1:]:
            assert torch.equal(_bits(lam), _bits(runs[0][0])) and torch.equal(_bits(resid), _bits(runs[0][1]))
        after_in = eng.iaf_backward_input(tape, *cot)
        after_w = eng.iaf_backward_weights(tape, *cot)
        assert torch.equal(_bits(after_in['d_noise']), _bits(before_in['d_noise']))
        assert torch.equal(_bits(after_in['d_encoding']), _bits(before_in['d_encoding']))
        assert torch.equal(_bits(after_w['flat_grads']), _bits(before_w['flat_grads']))
        assert torch.equal(_bits(after_w['d_encoding']), _bits(before_w['d_encoding']))
    finally:
        eng.close()


@pytest.mark.parametrize('name', ['S400', 'P384'])
def test_result_does_not_depend_on_check_every(name):
    """check_every 1 and 8 stop after the same sweep with the same bits; sweeps enqueued past the stop change nothing"""
    import torch
    eng, o, ff, tape = _taped(name)
    g_z, d_s = eng.iaf_latent_log_prob_grad(o['z'], ff['scale_tot'], None)
    a = eng.iaf_adjoint(tape, g_z, d_s, check_every=1)
    b = eng.iaf_adjoint(tape, g_z, d_s, check_every=8)
    print('{}: {} sweeps at the default tol {:g}'.format(name, a['sweeps'], eng.ADJOINT_TOL))
    assert bool(a['converged'].all()) and bool(b['converged'].all())
    assert a['sweeps'] == b['sweeps'] and 1 < a['sweeps'] < 16
    assert torch.equal(_bits(a['lam']), _bits(b['lam'])) and torch.equal(_bits(a['resid']), _bits(b['resid']))
    e = np.abs(_np(a['lam']).astype(np.float64) - o['loss']['lam']).max() / np.abs(o['loss']['lam']).max()
    print('{}: at the default tol max |lam - lam64| / max |lam64| = {:.2e}'.format(name, e))
    assert e <= TOL


# ---- refusals ----
def test_refusals():
    """by message; the size query returns 0 for a handle or a shape the call refuses"""
    import os
    import torch
    import distill_oracle64 as D
    from oracle import wavenet_np as O
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    eng, o, ff, tape = _taped('S200')
    B, T = o['z'].shape
    F = o['mel'].shape[1]
    dev = lambda a: torch.as_tensor(np.asarray(a, np.float32), device='cuda')
    g_z, d_s = dev(o['dense']['g_z']), dev(o['dense']['d_S'])
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_distill.npz')
    te_cfg, te_seed, te_init = D.golden_case(np.load(gold), 'mol')[1]
    te = Wavenet(te_cfg).load_weights(O.synth_weights(O.HP(te_cfg), 'teacher', seed=te_seed, init=te_init))
    try:
        assert int(te.engine.lib.wn_iaf_adjoint_workspace_bytes(te.engine._h, B, F, T)) == 0
        with pytest.raises(ValueError, match='wn_iaf_adjoint: handle is not a ParallelWavenet student'):
            te.engine.iaf_adjoint(tape, g_z, d_s, n_frames=F)
    finally:
        te.engine.close()
    with pytest.raises(ValueError, match='wn_iaf_adjoint: the tape was not written by wn_iaf_forward_train_tape of this handle'):
        eng.iaf_adjoint(tape.clone(), g_z, d_s, n_frames=F)
    other = _new_engine('S')
    try:
        with pytest.raises(ValueError, match='wn_iaf_adjoint: the tape was not written by wn_iaf_forward_train_tape of this handle'):
            other.iaf_adjoint(tape, g_z, d_s, n_frames=F)
        with pytest.raises(ValueError, match='pass n_frames'):
            other.iaf_adjoint(tape, g_z, d_s)
    finally:
        other.close()
    with pytest.raises(ValueError, match='the tape holds B = 2, T = 200, not B = 1, T = 200'):
        eng.iaf_adjoint(tape, g_z[:1], d_s[:1], n_frames=F)
    with pytest.raises(ValueError, match='the tape holds F = 1 mel frames, not 2'):
        eng.iaf_adjoint(tape, g_z, d_s, n_frames=F + 1)
    md = 2 ** (o['hp'].num_stages - 1)
    with pytest.raises(ValueError, match='wn_iaf_adjoint: length 199 is not a multiple of the largest dilation'):
        eng.iaf_adjoint(tape, g_z[:, :T - 1], d_s[:, :T - 1], n_frames=F)
    with pytest.raises(ValueError, match='the tape holds B = 2, T = 200, not B = 2, T = {}'.format(T - md)):
        eng.iaf_adjoint(tape, g_z[:, :T - md], d_s[:, :T - md], n_frames=F)
    assert int(eng.lib.wn_iaf_adjoint_workspace_bytes(eng._h, B, F, T - 1)) == 0
    assert int(eng.lib.wn_iaf_adjoint_workspace_bytes(eng._h, 0, F, T)) == 0
    assert int(eng.lib.wn_iaf_adjoint_workspace_bytes(eng._h, B, F, T * 100)) == 0         # more samples than the frames give
    with pytest.raises(ValueError, match='wn_iaf_adjoint: n_sweeps must be >= 1, got 0'):
        eng.iaf_adjoint(tape, g_z, d_s, max_sweeps=0)
    with pytest.raises(ValueError, match='wn_iaf_adjoint: tol must be >= 0, got -1'):
        eng.iaf_adjoint(tape, g_z, d_s, tol=-1.0)
    with pytest.raises(ValueError, match='wn_iaf_adjoint: tol must be >= 0, got nan'):
        eng.iaf_adjoint(tape, g_z, d_s, tol=float('nan'))
    nb = int(eng.lib.wn_iaf_adjoint_workspace_bytes(eng._h, B, F, T))
    ws = torch.zeros(nb, dtype=torch.uint8, device='cuda')
    lam = torch.zeros((B, T), dtype=torch.float32, device='cuda')
    resid = torch.zeros((B, 2), dtype=torch.float32, device='cuda')
    counts = torch.zeros(4, dtype=torch.int32, device='cuda')
    rc, msg = _raw(eng, (B, F, T), tape, tape.numel(), g_z, d_s, lam, 1, 0.0, resid, counts, ws, nb - 1)
    assert rc == -12 and 'wn_iaf_adjoint: workspace {} < {} bytes'.format(nb - 1, nb) in msg
    full = dict(tape=tape, g_z=g_z, d_s=d_s, lam=lam, resid=resid, counts=counts, ws=ws)
    for missing in sorted(full):
        a = dict(full, **{missing: None})
        rc, msg = _raw(eng, (B, F, T), a['tape'], tape.numel(), a['g_z'], a['d_s'], a['lam'], 1, 0.0, a['resid'], a['counts'],
                       a['ws'], nb)
        assert rc == -22 and 'wn_iaf_adjoint: null tape/g_z/d_scale_tot/lam/resid/counts/workspace' in msg, (missing, msg)
    r = eng.iaf_adjoint(tape, g_z, d_s, max_sweeps=2)              # and the tape is still good
    assert r['sweeps'] == 2
    torch.cuda.synchronize()
