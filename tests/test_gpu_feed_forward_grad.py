"""ParallelWavenet.feed_forward differentiated in its inputs: dag.IafFeedForward = the tape forward, then
Engine.iaf_backward_input and one Engine.deconv_backward_input per deconv stack.  mel.grad and noise.grad of a fixed linear
functional of x, mean_tot and scale_tot against the composed float64 oracle input_grad_oracle64.feed_forward_grads (held to
central differences by tests/test_input_grad_oracle.py) at the project's bar (TOL of tests/test_gpu_distill_grad.py), on a
shared stack (S1) and on private stacks (S2).

Ties (tests/input_grad_oracle64.py): the mel rows' hidden pre-activations are clear of zero in every stack, and at the last
layer's near ties -- at most 0.1 % of its elements -- the oracle takes the sign the engine's forward took, read from
Engine.deconv.  Both are asserted before the comparison."""
import numpy as np
import pytest

import deconv_grad_oracle64 as DG
import input_grad_cases as C
import input_grad_oracle64 as IG
import student_grad_oracle64 as S
from test_gpu_distill_grad import TOL

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope='module')
def students():
    from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet
    made = {}

    def get(tag):
        if tag not in made:
            hp, w, ora, mel, seeds, noise, cot = C.ff_inputs(tag)
            pw = ParallelWavenet(C.IAF_CFG[C.FF_CASES[tag][0]]).load_weights(w)
            made[tag] = (pw, ora, mel, seeds, noise, cot)
        return made[tag]
    yield get
    for v in made.values():
        v[0].engine.close()


def _functional(ff, cot):
    import torch
    return sum((ff[k].double() * torch.as_tensor(c).cuda().double()).sum() for k, c in zip(('x', 'mean_tot', 'scale_tot'), cot))


def _engine_signs(pw, ora, mel):
    """{scope: sign of the last pre-activation [B,Cd,TE]}: the oracle's, and at its near ties the engine's own"""
    import torch
    pos, n_near, n_flip = {}, 0, 0
    for p, zs in IG.stacks_pre(ora, mel).items():
        assert sum(int(DG.near(z).sum()) for z in zs[:-1]) == 0, 'a hidden pre-activation is a near tie'
        near = DG.near(zs[-1])
        assert int(near.sum()) <= DG.MAX_ZEROED * near.numel()
        dev = (pw.engine.deconv(mel, scope=p).double().cpu() > 0).transpose(1, 2)
        pos[p] = torch.where(near, dev, zs[-1] > 0)
        n_near += int(near.sum())
        n_flip += int((pos[p] != (zs[-1] > 0)).sum())
    return pos, n_near, n_flip


@pytest.mark.parametrize('tag', sorted(C.FF_CASES))
def test_mel_and_noise_gradients_match_the_composed_oracle(students, tag):
    import torch
    pw, ora, mel, seeds, noise, cot = students(tag)
    pos, n_near, n_flip = _engine_signs(pw, ora, mel)
    print('FF-GRAD {}: mel seeds {}, {} last-layer near ties, {} signs from the engine'.format(tag, seeds, n_near, n_flip))
    ref = IG.feed_forward_grads(ora, mel, noise, cot, pos=pos)
    aux = ora.grads(mel, noise, *cot)['aux']
    assert S.near_tie_fraction(aux) <= 1e-4 and S.clamps_inactive(aux)
    M = torch.as_tensor(mel).cuda().requires_grad_()
    Z = torch.as_tensor(noise).cuda().requires_grad_()
    ff = pw.feed_forward({'mel': M}, noise=Z)
    assert sorted(ff) == ['log_scale_tot', 'mean_tot', 'rand_input', 'scale_tot', 'x']
    assert ff['x'].requires_grad and not ff['rand_input'].requires_grad and torch.equal(ff['rand_input'], Z.detach())
    # the values are the tape forward's, bit for bit
    tf, _ = pw.engine.iaf_forward_train_tape(mel, noise=noise)
    for k in ('x', 'mean_tot', 'scale_tot'):
        assert torch.equal(ff[k].detach(), tf[k]), k
    _functional(ff, cot).backward()
    worst = {}
    for name, got, want in (('mel.grad', M.grad, ref['d_mel']), ('noise.grad', Z.grad, ref['d_noise'])):
        assert got is not None and tuple(got.shape) == want.shape and bool(torch.isfinite(got).all()), name
        worst[name] = np.abs(_np(got).astype(np.float64) - want).max() / np.abs(want).max()
        print('FF-GRAD {} {:10s} max |g - g64| / max |g64| = {:.2e} (max |g64| {:.3e})'.format(tag, name, worst[name], np.abs(want).max()))
    assert all(e <= TOL for e in worst.values()), (tag, worst)
    # mel alone, noise alone: the same bits, and no gradient for the other
    M2 = torch.as_tensor(mel).cuda().requires_grad_()
    _functional(pw.feed_forward({'mel': M2}, noise=noise), cot).backward()
    assert torch.equal(M2.grad, M.grad)
    Z2 = torch.as_tensor(noise).cuda().requires_grad_()
    _functional(pw.feed_forward({'mel': mel}, noise=Z2), cot).backward()
    assert torch.equal(Z2.grad, Z.grad)


def test_the_plain_path_is_iaf_generate_as_before(students):
    """under torch.no_grad(), or with inputs that do not require grad: the bits of Engine.iaf_generate"""
    import torch
    pw, ora, mel, seeds, noise, cot = students('S1')
    gen = pw.engine.iaf_generate(mel, noise=noise, want=('x', 'mean_tot', 'scale_tot', 'rand_input'))
    M = torch.as_tensor(mel).cuda().requires_grad_()
    Z = torch.as_tensor(noise).cuda().requires_grad_()
    with torch.no_grad():
        a = pw.feed_forward({'mel': M}, noise=Z)
    b = pw.feed_forward({'mel': M.detach()}, noise=Z.detach())
    c = pw.feed_forward({'mel': mel}, noise=noise)
    for out in (a, b, c):
        assert not out['x'].requires_grad
        for k in gen:
            assert torch.equal(out[k], gen[k]), k
        assert torch.equal(out['log_scale_tot'], torch.log(gen['scale_tot']))
    # a drawn noise: the device generator's under `seed`, on both paths, and no gradient for it
    drawn = pw.feed_forward({'mel': M}, seed=7)
    assert drawn['x'].requires_grad and not drawn['rand_input'].requires_grad
    assert torch.equal(drawn['rand_input'], pw.feed_forward({'mel': mel}, seed=7)['rand_input'])


def test_directional_finite_difference_through_the_engine(students):
    """(f(mel + e v) - f(mel - e v)) / 2e against <mel.grad, v>, f the functional through the engine's own tape forward; within
    1e-2 relative, as tests/test_gpu_distill_grad.py's directional check"""
    import torch
    pw, ora, mel, seeds, noise, cot = students('S1')
    M = torch.as_tensor(mel).cuda().requires_grad_()
    _functional(pw.feed_forward({'mel': M}, noise=noise), cot).backward()
    v = torch.as_tensor(np.random.RandomState(21).standard_normal(mel.shape)).cuda()
    v = v / v.norm()
    dd = float((M.grad.double() * v).sum())
    eps = 3e-3 * float(M.detach().abs().max())

    def f(sign):
        m = (M.detach().double() + sign * eps * v).float()
        out, _ = pw.engine.iaf_forward_train_tape(m, noise=noise)
        return float(_functional(out, cot))
    fd = (f(1) - f(-1)) / (2 * eps)
    print('FF-GRAD directional S1: fd {:.6e} grad {:.6e}'.format(fd, dd))
    assert abs(fd - dd) <= 1e-2 * abs(dd), (fd, dd)


def test_power_loss_reaches_mel(students):
    """the README's use: mel.requires_grad_(), feed_forward, power_loss(...).backward(), mel.grad"""
    import torch
    pw, ora, mel, seeds, noise, cot = students('S1')
    M = torch.as_tensor(mel).cuda().requires_grad_()
    ff = pw.feed_forward({'mel': M}, noise=noise)
    target = torch.as_tensor(np.random.RandomState(3).uniform(-0.5, 0.5, noise.shape).astype(np.float32)).cuda()
    loss = pw.power_loss({'x': ff['x'], 'wav': target})['power_loss']
    loss.backward()
    assert M.grad is not None and bool(torch.isfinite(M.grad).all()) and float(M.grad.abs().max()) > 0
    assert int((M.grad != 0).sum()) > 0.9 * M.grad.numel()


def test_a_teacher_owned_stack_is_differentiated_under_the_teachers_handle():
    """use_teacher_deconv: the student conditions on the teacher's upsampler ('iaf_share/trans_conv_*' holds the teacher's
    'trans_conv_*').  With a teacher object, d mel comes from the teacher's handle (scope ''); without one, from the student's
    own copy -- the same variables through the same kernels, so the same bits; and noise.grad does not depend on which."""
    import torch
    import deconv_bwd_geometries as BG
    from oracle import wavenet_np as O
    from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    cfgd = dict(S.S1, use_share_deconv=False, use_teacher_deconv=True)
    w = O.synth_weights(O.HP(cfgd), 'student', seed=C.IAF_SEED, init='unit')
    te_cfg = dict(BG.teacher_cfg('base'), deconv_config=S.DECONV, upsample_act='leaky_relu')
    te_w = O.synth_weights(O.HP(te_cfg), 'teacher', seed=3, init='unit')
    for k in list(te_w):
        if k.startswith('trans_conv_'):
            assert te_w[k].shape == w['iaf_share/' + k].shape
            te_w[k] = w['iaf_share/' + k]
    te = Wavenet(te_cfg).load_weights(te_w)
    with_te, alone = ParallelWavenet(cfgd, teacher=te).load_weights(w), ParallelWavenet(cfgd).load_weights(w)
    try:
        assert with_te._input_grad_stacks() == [(te.engine, '')] and alone._input_grad_stacks() == [(alone.engine, 'iaf_share')]
        B, F, T = 2, 25, 200
        mel, noise, cot = S.case_inputs(B, F, T, seed=C.IAF_SEED + 100)
        grads = []
        for pw in (with_te, alone):
            M = torch.as_tensor(mel).cuda().requires_grad_()
            Z = torch.as_tensor(noise).cuda().requires_grad_()
            _functional(pw.feed_forward({'mel': M}, noise=Z), cot).backward()
            assert float(M.grad.abs().max()) > 0 and bool(torch.isfinite(M.grad).all())
            grads.append((M.grad, Z.grad))
        assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    finally:
        for e in (with_te.engine, alone.engine, te.engine):
            e.close()


def test_refusals_surface_as_they_are():
    """the tape forward's: a mu-law student, a weight-norm student, a width that is no multiple of 64"""
    import torch
    from nsynth_wavenet_amd import config as cfg, weights as wts
    from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet
    mel = torch.rand(1, 4, 80, device='cuda').requires_grad_()
    for change, msg in ((dict(use_mu_law=True), 'mu-law student'), (dict(use_weight_norm=True), 'weight-norm student'),
                        (dict(width=32), 'multiples of 64')):
        cfgd = dict(S.S1, **change)
        pw = ParallelWavenet(cfgd).load_weights(wts.synthetic_weights(cfg.load_hparams(cfgd), 'student', seed=1))
        try:
            with pytest.raises(ValueError, match=msg):
                pw.feed_forward({'mel': mel}, seed=1)
            with torch.no_grad():
                pw.feed_forward({'mel': mel}, seed=1)           # the plain path still serves them
        finally:
            pw.engine.close()
