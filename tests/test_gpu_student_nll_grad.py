"""The gradient of the student's log-likelihood through the public API: ParallelWavenet.nll_and_weight_grads,
log_prob under autograd and train.StudentMleTrainer, against tests/iaf_nll_grad_oracle64.py (held to central differences by
tests/test_iaf_nll_grad_oracle.py) on S200, P384 and G384 of tests/iaf_encode_cases.py (init='tf').

x is float32 of the oracle's float64 forward at z = float32(z0), so the engine's encode lands within float32 of where the
oracle stands.  The bar: max |g - g64| <= TOL max |g64| per tensor (TOL of tests/test_gpu_distill_grad.py)."""
import math

import numpy as np
import pytest

import deconv_grad_oracle64 as DG
import iaf_nll_grad_oracle64 as N
import student_grad_oracle64 as S
from iaf_encode_cases import CASES, model_config
from test_gpu_distill_grad import TOL

pytestmark = pytest.mark.gpu
NAMES = ['S200', 'P384', 'G384']

_PW, _RUNS = {}, {}


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    import torch
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _new_pw(model, weights=None):
    from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet
    from iaf_encode_cases import _model
    return ParallelWavenet(model_config(model)).load_weights(_model(model, 'tf')[1] if weights is None else weights)


def _pw(model):
    """one student WITHOUT a teacher per model for the module"""
    if model not in _PW:
        _PW[model] = _new_pw(model)
    return _PW[model]


@pytest.fixture(scope='module', autouse=True)
def _close():
    yield
    _RUNS.clear()
    for p in _PW.values():
        p.engine.close()
    _PW.clear()


def _run(name):
    """per case, once: (student, oracle case, mel and x on the device, nll_and_weight_grads with the encode run to tol = 0)"""
    import torch
    if name not in _RUNS:
        o = N.case_oracle(name)
        pw = _pw(CASES[name][0])
        mel = torch.as_tensor(o['mel'].astype(np.float32)).cuda()
        x = torch.as_tensor(o['x'].astype(np.float32)).cuda()
        _RUNS[name] = (pw, o, mel, x, pw.nll_and_weight_grads({'mel': mel, 'wav': x}, encode_tol=0.0))
    return _RUNS[name]


def _err(label, got, ref):
    g = _np(got).astype(np.float64).reshape(ref.shape)
    assert np.isfinite(g).all(), label
    e = np.abs(g - ref).max() / np.abs(ref).max()
    print('{} max |g - g64| / max |g64| = {:.2e} (max |g64| {:.3e})'.format(label, e, np.abs(ref).max()))
    return e


@pytest.mark.parametrize('name', NAMES)
def test_nll_and_weight_grads(name):
    import torch
    pw, o, mel, x, out = _run(name)
    eng, ref = pw.engine, o['loss']
    assert set(out) == {'loss', 'log_probs', 'grads', 'flat_grads', 'flat_upsampler_grads', 'd_encoding', 'd_wav', 'sweeps',
                        'adjoint_sweeps', 'converged'}
    assert bool(out['converged'].all())
    print('NLL {}: loss {:.6f}, {} encode sweeps, {} adjoint sweeps'.format(name, float(out['loss']), out['sweeps'],
                                                                           out['adjoint_sweeps']))
    plain = pw.log_prob({'mel': mel, 'wav': x}, tol=0.0)
    assert torch.equal(_bits(plain['loss']), _bits(out['loss'])) and torch.equal(_bits(plain['log_probs']), _bits(out['log_probs']))
    lp64 = o['G'].log_prob()
    assert abs(float(out['loss']) + lp64.mean()) <= 1e-5 * max(1.0, abs(lp64.mean()))
    errs = {k: _err('NLL {} {}'.format(name, k), out['grads'][k], ref['grads'][k]) for k in o['G'].ora.names}
    errs['d_wav'] = _err('NLL {} d_wav'.format(name), out['d_wav'], ref['lam'])
    for s in range(ref['d_encoding'].shape[0]):
        errs['d_encoding[{}]'.format(s)] = _err('NLL {} d_encoding[{}]'.format(name, s), out['d_encoding'][s], ref['d_encoding'][s])
    hp = o['hp']
    dc = hp.deconv_config
    assert sorted(out['flat_upsampler_grads']) == sorted(S.stack_scopes(hp))
    for s, scope in enumerate(S.stack_scopes(hp)):
        up64 = DG.grads(torch.as_tensor(o['mel']), DG.weights64(o['w'], len(dc), scope), dc, 'leaky_relu',
                        torch.as_tensor(ref['d_encoding'][s]), scope)
        for k, v in up64.items():
            errs[k] = _err('NLL {} {}'.format(name, k), out['grads'][k], v.numpy())
    bad = {k: e for k, e in errs.items() if not e <= TOL}
    assert not bad, bad
    # d_encoding is iaf_backward_weights' on the tape at the encode's z, with the cotangents (-lam, 0, d_S)
    z = pw.encode({'mel': mel, 'wav': x}, tol=0.0)['z']
    ff, tape = eng.iaf_forward_train_tape(mel, noise=z)
    c = torch.full(tuple(z.shape), -1.0 / z.numel(), dtype=torch.float64, device=z.device).to(torch.float32)
    _, d_s = eng.iaf_latent_log_prob_grad(z, ff['scale_tot'], c)
    again = eng.iaf_backward_weights(tape, -out['d_wav'], torch.zeros_like(z), d_s)
    assert torch.equal(out['d_encoding'], again['d_encoding'])
    assert torch.equal(_bits(out['flat_grads']), _bits(again['flat_grads']))


def test_wav_is_cropped_like_power_loss_and_a_short_one_refused():
    import torch
    pw, o, mel, x, out = _run('S200')
    T = x.shape[1]
    pad = torch.cat([torch.full((x.shape[0], 3), 9.0, device='cuda'), x, torch.full((x.shape[0], 4), -9.0, device='cuda')], 1)
    got = pw.nll_and_weight_grads({'mel': mel, 'wav': pad}, encode_tol=0.0, upsampler=False)       # 7 to drop, 3 on the left
    assert torch.equal(_bits(got['loss']), _bits(out['loss'])) and torch.equal(_bits(got['d_wav']), _bits(out['d_wav']))
    assert 'flat_upsampler_grads' not in got
    with pytest.raises(ValueError, match=r'nll_and_weight_grads: wav must be \[B, >= {}\]'.format(T)):
        pw.nll_and_weight_grads({'mel': mel, 'wav': x[:, :T - 1]})


@pytest.mark.parametrize('name', ['S200', 'G384'])
def test_log_prob_with_grad(name):
    """the values are the bits of the no-grad call, which are iaf_encode's; wav.grad is d_wav, mel.grad the summed
    deconv_backward_input calls on d_encoding"""
    import torch
    pw, o, mel, x, out = _run(name)
    eng = pw.engine
    plain = pw.log_prob({'mel': mel, 'wav': x}, tol=0.0)
    enc = eng.iaf_encode(x, mel, tol=0.0, want=('z', 'log_prob'))
    assert torch.equal(_bits(plain['log_probs']), _bits(enc['log_prob']))
    assert torch.equal(_bits(plain['loss']), _bits(-(enc['log_prob_sums'].sum() / enc['log_prob'].numel())))
    wav, m = x.clone().requires_grad_(True), mel.clone().requires_grad_(True)
    r = pw.log_prob({'mel': m, 'wav': wav}, tol=0.0)
    assert r['loss'].requires_grad and r['log_probs'].requires_grad
    assert torch.equal(_bits(r['loss']), _bits(plain['loss'])) and torch.equal(_bits(r['log_probs']), _bits(plain['log_probs']))
    r['loss'].backward()
    assert torch.equal(_bits(wav.grad), _bits(out['d_wav']))
    d_mel = None
    for s, (e, scope) in enumerate(pw._input_grad_stacks()):
        g = e.deconv_backward_input(mel, out['d_encoding'][s], scope)
        d_mel = g if d_mel is None else d_mel + g
    assert torch.equal(_bits(m.grad), _bits(d_mel)) and float(m.grad.abs().max()) > 0
    # one input alone, and through log_probs instead of the loss: a dense cotangent against the oracle
    wav2 = x.clone().requires_grad_(True)
    r2 = pw.log_prob({'mel': mel, 'wav': wav2}, tol=0.0)
    (r2['log_probs'] * torch.as_tensor(o['c'].astype(np.float32)).cuda()).sum().backward()
    assert _err('log_prob {} wav.grad, dense cotangent'.format(name), wav2.grad, o['dense']['lam']) <= TOL
    with torch.no_grad():
        r3 = pw.log_prob({'mel': m, 'wav': wav}, tol=0.0)
    assert not r3['loss'].requires_grad


def test_descent_through_the_public_api():
    """nll_and_weight_grads, then load_weights(w - eps g) on a fresh student lowers log_prob's 'loss'.  eps is chosen on the
    float64 oracle alone (its own decrease, with the inverse re-solved, at least 1e-3 and within 5 % of eps |g|^2); the
    engine's decrease must be within 10 % of the oracle's.  The step is taken on the kernels ('/W') of every flow: with the
    biases in the step no eps meets both conditions on the oracle -- out2_scale/biases moves every log scale at once, and at
    eps |g|^2 = 1e-3 the curvature already takes 12 % of the decrease (S200 and S400 alike).  Every variable's gradient,
    biases included, is held to the oracle by test_nll_and_weight_grads."""
    pw, o, mel, x, out = _run('S200')
    hp, w = o['hp'], o['w']
    names = [k for k in o['G'].ora.names if k.endswith('/W')]
    assert len(names) == len(o['G'].ora.names) // 2
    g64 = o['loss']['grads']
    n = o['z'].size
    c = np.full(o['z'].shape, -1.0 / n)
    z64 = o['z'].astype(np.float64)
    L0 = N.value(o['mel'], o['x'], c, w, hp, z64)
    gg = float(sum((g64[k] ** 2).sum() for k in names))
    eps, dec64 = None, None
    for e in [2.0 ** -j for j in range(-6, 24)]:
        stepped = dict(w)
        stepped.update({k: np.asarray(w[k], np.float64) - e * g64[k] for k in names})
        try:
            dec = L0 - N.value(o['mel'], o['x'], c, stepped, hp, z64)
        except AssertionError:                  # the inverse did not converge under so large a step
            continue
        if dec >= 1e-3 and abs(dec - e * gg) <= 0.05 * e * gg:
            eps, dec64 = e, dec
            break
    assert eps is not None, 'no step on the oracle is both large enough and in the linear regime'
    new = dict(w)
    for k in names:
        new[k] = (np.asarray(w[k], np.float64) - eps * out['grads'][k].double().cpu().numpy()).astype(np.float32)
    pw2 = _new_pw('S', new)
    try:
        after = pw2.log_prob({'mel': mel, 'wav': x}, tol=0.0)
    finally:
        pw2.engine.close()
    dec = float(out['loss']) - float(after['loss'])
    print('descent: eps {:.3e}, |g|^2 {:.4e}, oracle loss {:.6f} decrease {:.4e}; engine loss {:.6f} decrease {:.4e}'.format(
        eps, gg, L0, dec64, float(out['loss']), dec))
    assert dec > 0
    assert abs(dec - dec64) <= 0.10 * dec64, (dec, dec64)


def _flat(table, size, w):
    flat = np.zeros(size, np.float32)
    for name, off, shape in table:
        a = np.asarray(w[name], np.float32).reshape(-1)
        flat[off:off + a.size] = a
    return flat


def test_student_mle_trainer_step():
    """a student with teacher=None is accepted; step() equals nll_and_weight_grads + adam_ema_step + iaf_set_weights done by
    hand, bit for bit; after three steps on one batch the loss has dropped"""
    import torch
    from nsynth_wavenet_amd import engine as E, train
    o = N.case_oracle('S200')
    w = o['w']
    mel = torch.as_tensor(o['mel'].astype(np.float32)).cuda()
    x = torch.as_tensor(o['x'].astype(np.float32)).cuda()
    batch = {'mel': mel, 'wav': x}
    a, b = _new_pw('S'), _new_pw('S')
    try:
        assert a.teacher is None
        lr = 1e-3
        tr = train.StudentMleTrainer(a, w, lr=lr)
        assert tr.upsampler and tr.scopes == ['iaf_share']
        first = tr.step(batch)
        assert set(first) == {'loss', 'log_probs', 'grad_norm', 'sweeps', 'adjoint_sweeps', 'converged'}
        # by hand on the twin
        eng = b.engine
        out = b.nll_and_weight_grads(batch, upsampler=True, encode_tol=1e-5)
        scopes = eng.iaf_stack_scopes()
        tables = [eng.iaf_grad_table()] + [eng.deconv_grad_table(s) for s in scopes]
        sizes = [eng.iaf_grad_floats()] + [eng.deconv_grad_floats(s) for s in scopes]
        p = [torch.from_numpy(_flat(t, n, w)).cuda() for t, n in zip(tables, sizes)]
        m, v, ema = [torch.zeros_like(q) for q in p], [torch.zeros_like(q) for q in p], [q.clone() for q in p]
        flats = [out['flat_grads']] + [out['flat_upsampler_grads'][s] for s in scopes]
        sumsq = torch.zeros(1, dtype=torch.float64, device='cuda')
        for i, g in enumerate(flats):
            E.grad_sumsq(g, sumsq, accumulate=i > 0)
        lr_t = float(np.float32(lr * math.sqrt(1.0 - 0.999) / (1.0 - 0.9)))
        for q, g, mm, vv, ee in zip(p, flats, m, v, ema):
            E.adam_ema_step(q, g, mm, vv, ee, lr_t, 0.9, 0.999, 1e-8, min(0.9999, 1.0 / 10.0), sumsq=None, clip_norm=1.0)
        eng.iaf_set_weights(p[0], dict(zip(scopes, p[1:])))
        assert torch.equal(_bits(first['loss']), _bits(out['loss'])) and torch.equal(_bits(first['log_probs']), _bits(out['log_probs']))
        assert torch.equal(_bits(first['grad_norm']), _bits(sumsq.sqrt()[0]))
        assert (first['sweeps'], first['adjoint_sweeps']) == (out['sweeps'], out['adjoint_sweeps'])
        for i in range(len(p)):
            assert torch.equal(_bits(tr.p[i]), _bits(p[i])) and torch.equal(_bits(tr.ema[i]), _bits(ema[i])), i
        la, lb = a.log_prob(batch, tol=1e-5), b.log_prob(batch, tol=1e-5)
        assert torch.equal(_bits(la['log_probs']), _bits(lb['log_probs']))
        losses = [float(first['loss'])] + [float(tr.step(batch)['loss']) for _ in range(2)]
        losses.append(float(a.log_prob(batch, tol=1e-5)['loss']))
        print('MLE: loss before steps 1, 2, 3 and after: {}'.format(' '.join('{:.6f}'.format(v) for v in losses)))
        assert tr.global_step == 3 and losses[3] < losses[0]
    finally:
        a.engine.close()
        b.engine.close()
