"""GPU tests of the teacher's differentiable loss: wn_teacher_log_prob_grad (csrc/wn_teacher.hip), the gradient
of the scoring kernel, and the public path over it -- Engine.teacher_log_prob_grad, distill_autograd.TeacherLogProb,
Wavenet.calculate_loss and Wavenet.feed_forward with tensors that require grad -- against the float64 torch restatement of the
reference's loss (tests/teacher_nll_oracle64.py, pinned by tests/test_teacher_nll_oracle.py) and of its teacher
(tests/distill_oracle64.py)."""
import ctypes
import json
import os

import numpy as np
import pytest

import distill_oracle64 as D
import teacher_nll_oracle64 as N

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_distill.npz')

# Bounds on max |g_engine - g_oracle| / max |g_oracle| per output tensor.  NOT YET MEASURED on an MI355X: until
# the figures these tests print are recorded here and the bounds set to four times the largest, they come from the arithmetic:
# the kernel chains about ten float32 operations per output, each exp / log within 2 ulp on arguments of magnitude up to 20
# (logit spread, logistic arguments), i.e. 20 * 2^-23 = 2.4e-6 per step and about 1e-5 in the worst chain, times four.  The
# chain adds the input VJP's split-fp16 GEMMs, measured at 1.2e-6 on this small teacher.
TOL_KERNEL = 4e-5
TOL_CHAIN = 4e-5


@pytest.fixture(scope='module')
def R():
    return np.load(GOLD)


def _small_cfg(R, loss, mu=False, mol_mix=10):
    """the small teacher of tests/test_gpu_distill_grad.py (width 128, skip 64, gate 128, 7 layers, 3 stages) with another head"""
    c = dict(json.loads(str(R['mol/te_cfg_json'])), loss_type=loss, use_mu_law=mu)
    if loss == 'mol':
        c['mol_mix'] = mol_mix
    else:
        c.pop('mol_mix', None)
    return c


def _wavenet(cfgd, weights=True):
    from oracle import wavenet_np as O
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    net = Wavenet(cfgd)
    return net.load_weights(O.synth_weights(O.HP(cfgd), 'teacher', seed=1234, init='unit')) if weights else net


@pytest.fixture(scope='module')
def nets(R):
    """one Wavenet per kernel case, built on first use; the 65 536-class head stays without weights (scoring reads none, and
    its out2 kernel alone would be 4 M values)"""
    made = {}

    def get(tag):
        if tag not in made:
            loss, mu, M, _, _ = N.KERNEL_CASES[tag]
            made[tag] = _wavenet(_small_cfg(R, loss, mu, M), weights=tag != 'ce_16bit')
        return made[tag]
    yield get
    for net in made.values():
        net.engine.close()


def _err(got, ref):
    """max |got - ref| / max |ref|"""
    return float((got.detach().double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def _cuda(*arrays):
    import torch
    return [torch.as_tensor(a).cuda() for a in arrays]


@pytest.mark.parametrize('tag', sorted(N.KERNEL_CASES))
def test_gradient_kernel_matches_oracle(nets, tag):
    """B = 2, T = 37 (74 waves: the last block holds two) with a random d_log_prob; every element is compared."""
    import torch
    loss, mu = N.KERNEL_CASES[tag][:2]
    par, wav, g = N.kernel_case(tag)
    r = N.tie_report(tag, par, wav)
    assert r['mass_in_band'] == 0 and r['target_near_threshold'] == 0 and r['scale_near_tie'] == 0, r
    eng = nets(tag).engine
    P, X, G = _cuda(par, wav, g)
    d_out, d_wav = eng.teacher_log_prob_grad(P, X, G)
    lp, rp, rx = N.grads(par, wav, g, loss, mu)
    assert float((eng.teacher_log_prob(P, X).double().cpu() - lp).abs().max()) <= 1e-4
    e_out = _err(d_out, rp)
    print('{}: d_out_params error / max |g| = {:.2e} (max |g| {:.3e})'.format(tag, e_out, float(rp.abs().max())))
    if mu or loss == 'ce':
        assert float(rx.abs().max()) == 0 and float(d_wav.abs().max()) == 0          # exactly zero, every element written
        e_wav = 0.0
    else:
        e_wav = _err(d_wav, rx)
        print('{}: d_wav error / max |g| = {:.2e} (max |g| {:.3e})'.format(tag, e_wav, float(rx.abs().max())))
    d_out2, none = eng.teacher_log_prob_grad(P, X, G, want_wav=False)
    assert none is None and torch.equal(d_out2, d_out)
    assert bool(torch.isfinite(d_out).all())
    assert e_out <= TOL_KERNEL and e_wav <= TOL_KERNEL, (tag, e_out, e_wav)


@pytest.mark.parametrize('tag', sorted(N.KERNEL_CASES))
def test_gradient_kernel_is_deterministic(nets, tag):
    import torch
    eng = nets(tag).engine
    P, X, G = _cuda(*N.kernel_case(tag))
    a, b = eng.teacher_log_prob_grad(P, X, G), eng.teacher_log_prob_grad(P, X, G)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize('tag', ['mol10', 'gauss', 'ce_mulaw'])
def test_calculate_loss_is_differentiable_and_the_same_bits(nets, tag):
    """Wavenet.calculate_loss on out_params that require grad: the values of the no-grad call, and d loss / d out_params (and
    d loss / d wav through the target) of the oracle's -mean.  Fails before this change: the result had no grad_fn."""
    import torch
    loss, mu, _, B, T = N.KERNEL_CASES[tag]
    par, wav, _ = N.kernel_case(tag)
    net = nets(tag)
    P, X = _cuda(par, wav)
    plain = net.calculate_loss({'out_params': P, 'wav': X})
    assert not plain['loss'].requires_grad
    Pg, Xg = P.clone().requires_grad_(True), X.clone().requires_grad_(True)
    graded = net.calculate_loss({'out_params': Pg, 'wav': Xg})
    assert graded['loss'].requires_grad and graded['log_probs'].grad_fn is not None
    assert set(graded) == set(plain)
    for k in plain:
        assert torch.equal(plain[k], graded[k].detach()), k
    with torch.no_grad():
        assert not net.calculate_loss({'out_params': Pg, 'wav': Xg})['loss'].requires_grad
    graded['loss'].backward()
    _, rp, rx = N.grads(par, wav, np.full([B, T], -1.0 / (B * T)), loss, mu)
    e = _err(Pg.grad, rp)
    print('calculate_loss {}: d out_params error / max |g| = {:.2e}'.format(tag, e))
    assert e <= TOL_KERNEL
    if mu or loss == 'ce':
        assert float(Xg.grad.abs().max()) == 0
    else:
        assert _err(Xg.grad, rx) <= TOL_KERNEL


@pytest.mark.parametrize('tag', ['mol', 'gauss'])
def test_loss_backpropagates_to_the_audio_through_both_paths(R, tag):
    """The frozen teacher as a likelihood critic: calculate_loss(feed_forward({'wav': x, 'mel': mel}))['loss'].backward() sums
    the gradient through the network input (the engine's input VJP) and the one through the target into x.grad."""
    import torch
    hp_st, (cfgd, seed, init), _, mel = D.golden_case(R, tag)
    net = _wavenet(cfgd)
    B, T = 1, 256
    rs = np.random.RandomState(11)
    x = np.clip(0.5 * np.sin(0.05 * np.arange(T))[None] + 0.1 * rs.standard_normal([B, T]), -0.95, 0.95).astype(np.float32)
    mel = mel['mel'][:1, :2]                                       # 2 frames of 200 samples: the conditioning is cropped to T
    xg = torch.as_tensor(x).cuda().requires_grad_(True)
    melg = torch.as_tensor(mel).cuda()
    ff = net.feed_forward({'wav': xg, 'mel': melg})
    assert ff['out_params'].grad_fn is not None and ff['wav'] is not None
    res = net.calculate_loss(ff)
    res['loss'].backward()
    with torch.no_grad():
        plain = net.calculate_loss(net.feed_forward({'wav': xg, 'mel': melg}))
    assert torch.equal(plain['loss'], res['loss'].detach()) and torch.equal(plain['log_probs'], res['log_probs'].detach())
    # float64 oracle; near-tie ReLU derivatives from the engine's tape, as in tests/test_gpu_distill_grad.py
    thp, w = D.teacher_weights(cfgd, seed, init)
    enc = D.teacher_enc(mel, cfgd, seed, init)
    x64 = torch.as_tensor(x.astype(np.float64)).requires_grad_(True)
    pre = {}
    D.teacher_ff(x64.detach(), enc, w, thp, pre=pre)
    _, tape = net.engine.teacher_forward_tape(xg.detach(), melg)
    masks, nflip = D.relu_masks(pre, D.tape_pre(tape, B, T, cfgd['skip_width']))
    assert nflip <= 16
    out64 = D.teacher_ff(x64, enc, w, thp, masks=masks)
    L = -N.teacher_log_prob(out64, x64, tag, False).mean()
    L.backward()
    _, _, target_part = N.grads(out64.detach().numpy(), x, np.full([B, T], -1.0 / (B * T)), tag, False)
    assert float(target_part.abs().max()) > 0 and float((x64.grad - target_part).abs().max()) > 0     # both paths carry gradient
    e = _err(xg.grad, x64.grad)
    print('chain {}: loss {:.6f} (oracle {:.6f}), x.grad error / max |g| = {:.2e}; max |g| {:.3e}, target path {:.3e}, {} ReLU '
          'derivatives from the tape'.format(tag, float(res['loss']), float(L), e, float(x64.grad.abs().max()),
                                             float(target_part.abs().max()), nflip))
    assert e <= TOL_CHAIN, (tag, e)
    net.engine.close()


def test_invalid_calls_are_refused(R, nets, student_cfg):
    import torch
    from nsynth_wavenet_amd.engine import Engine
    from nsynth_wavenet_amd._lib import ERRNAMES
    par, wav, g = N.kernel_case('mol10')
    P, X, G = _cuda(par, wav, g)
    eng = nets('mol10').engine

    def refused(fn, text):
        with pytest.raises(ValueError) as e:
            fn()
        assert text in str(e.value), str(e.value)
    st = Engine(student_cfg)
    refused(lambda: st.teacher_log_prob_grad(P, X, G), 'not a Wavenet teacher')
    st.close()
    refused(lambda: eng.teacher_log_prob_grad(P[..., :29].contiguous(), X, G), 'out_params must be [B,T,30]')
    refused(lambda: eng.teacher_log_prob_grad(P, X[:, :-1].contiguous(), G), 'out_params must be [B,T,30]')
    refused(lambda: eng.teacher_log_prob_grad(P, X, G[:1]), 'd_log_prob must be [B,T]')
    # the C call itself: sizes below 1, null pointers, a null handle
    d_out = torch.full_like(P, 7.0)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
    call = lambda h, p, x, B, T, gg, do: eng.lib.wn_teacher_log_prob_grad(h, ptr(p), ptr(x), B, T, ptr(gg), ptr(do), ptr(None),
                                                                          eng._stream())
    for args in ((eng._h, P, X, 0, 37, G, d_out), (eng._h, P, X, 2, 0, G, d_out), (eng._h, None, X, 2, 37, G, d_out),
                 (eng._h, P, None, 2, 37, G, d_out), (eng._h, P, X, 2, 37, None, d_out), (eng._h, P, X, 2, 37, G, None),
                 (ctypes.c_void_p(0), P, X, 2, 37, G, d_out)):
        assert ERRNAMES[call(*args)] == 'WN_EINVAL'
        assert b'wn_teacher_log_prob_grad' in eng.lib.wn_last_error(eng._h)
    torch.cuda.synchronize()
    assert float((d_out - 7.0).abs().max()) == 0                   # nothing was launched
    # a mu-law teacher has no input VJP: feed_forward with a wav that requires grad surfaces the engine's refusal
    mu = _wavenet(_small_cfg(R, 'mol', True, 3), weights=False)
    mel = torch.as_tensor(R['mol/in_mel'][:1, :2]).cuda()
    refused(lambda: mu.feed_forward({'wav': torch.zeros(1, 256).cuda().requires_grad_(True), 'mel': mel}), 'mu-law')
    mu.engine.close()
