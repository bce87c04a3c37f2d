"""GPU tests of the distillation-loss gradients: ParallelWavenet.calculate_loss and its terms differentiated
with respect to the student's x, mean_tot and scale_tot -- the teacher's tape forward and input VJP (csrc/wn_teacher_bwd.hip)
and the loss gradients (csrc/wn_distill.hip) -- against the float64 torch restatement of the reference's graph
(tests/distill_oracle64.py, pinned to tests/golden/ref_distill.npz by tests/test_distill_grad_oracle.py)."""
import json
import os
import threading

import numpy as np
import pytest

import distill_oracle64 as D
from conftest import load_json

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_distill.npz')
TOL = 1e-4          # max-abs error of a gradient, relative to its largest magnitude


@pytest.fixture(scope='module')
def R():
    return np.load(GOLD)


def _teacher(cfgd, seed=1234, init='unit'):
    from oracle import wavenet_np as O
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    return Wavenet(cfgd).load_weights(O.synth_weights(O.HP(cfgd), 'teacher', seed=seed, init=init))


@pytest.fixture(scope='module')
def teachers(R):
    return {tag: _teacher(*D.golden_case(R, tag)[1]) for tag in ('mol', 'gauss')}


def _err(got, ref):
    """max |got - ref| / max |ref|"""
    import torch
    got = torch.zeros_like(ref) if got is None else got.detach().double().to(ref.device)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


class _Case(object):
    """one golden case: the GPU inputs (float32, requiring grad) and the float64 oracle on the same values"""

    def __init__(self, R, tag, wav='wav_long'):
        import torch
        self.hp, (cfgd, seed, init), inp, mel = D.golden_case(R, tag)
        self.tag = tag
        self.mel = {k: torch.as_tensor(v).cuda() for k, v in mel.items()}
        self.wav = {k: torch.as_tensor(R['{}/in_{}'.format(tag, k)]).cuda() for k in ('wav_long', 'wav_eq', 'wav_short')}
        self.v32 = {k: torch.as_tensor(R['{}/in_{}'.format(tag, k)]).cuda() for k in ('x', 'mean_tot', 'scale_tot')}
        self.rl = [torch.as_tensor(v).cuda() for v in D.golden_rl(R)]
        self.thp, self.w = D.teacher_weights(cfgd, seed, init)
        self.enc = {k: D.teacher_enc(v, cfgd, seed, init) for k, v in mel.items()}
        self.S = int(R['S'])

    def gpu_inputs(self):
        return {k: v.clone().requires_grad_(True) for k, v in self.v32.items()}

    def ff(self, g, wav='wav_long'):
        d = dict(g)
        d.update({'mel': self.mel['mel'], 'mel_rand': self.mel['mel_rand'], 'wav': self.wav[wav]})
        return d

    def oracle(self, term, wav='wav_long'):
        """the float64 oracle's value and gradients (x, mean_tot, scale_tot) of one term"""
        import torch
        v = {k: t.detach().cpu().double().requires_grad_(True) for k, t in self.v32.items()}
        rl = [r.cpu().double() for r in self.rl]
        te = lambda m: D.teacher_ff(v['x'], self.enc[m], self.w, self.thp)
        if term == 'loss':
            ff = dict(v, wav=self.wav[wav].cpu().double())
            L = D.calculate_loss(self.hp, te('mel'), te('mel_rand') if self.tag == 'mol' else None, ff, rl[0], rl[1])['loss']
        elif term == 'kl':
            L = D.kl_logistic(te('mel'), v['mean_tot'], v['scale_tot'], rl[0])['kl_loss']
        elif term == 'contrastive':
            L = -D.kl_logistic(te('mel_rand'), v['mean_tot'], v['scale_tot'], rl[1])['kl_loss']
        elif term == 'gauss':
            L = D.kl_gauss(te('mel'), v['mean_tot'], v['scale_tot'])['kl_loss']
        else:
            L = D.power_loss(v['x'], self.wav[wav].cpu().double())
        L.backward()
        return float(L.detach()), {k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in v.items()}


def _check_grads(g, ref, what):
    errs = {k: _err(g[k].grad, ref[k]) for k in ref if float(ref[k].abs().max()) > 0}
    print('{}: max-abs error / max |g| = {}'.format(what, ', '.join('{} {:.2e}'.format(k, e) for k, e in errs.items())))
    for k, e in errs.items():
        assert e <= TOL, (what, k, e)
    for k in ref:
        if float(ref[k].abs().max()) == 0:
            assert g[k].grad is None or float(g[k].grad.abs().max()) == 0, (what, k)


@pytest.mark.parametrize('tag', ['mol', 'gauss'])
def test_calculate_loss_gradient_matches_oracle(R, teachers, tag):
    """VJP parity of the whole calculate_loss with every hparams factor (kl + power + contrastive for mol)."""
    from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet
    c = _Case(R, tag)
    pw = ParallelWavenet(c.hp, teacher=teachers[tag])
    g = c.gpu_inputs()
    kw = {'noise': c.rl[0], 'cl_noise': c.rl[1]} if tag == 'mol' else {}
    losses = pw.calculate_loss(c.ff(g), **kw)
    if tag == 'mol':
        assert {'kl_loss', 'power_loss', 'contrastive_loss', 'loss'} <= set(losses)
    losses['loss'].backward()
    val, ref = c.oracle('loss')
    assert abs(float(losses['loss'].detach()) - val) <= 1e-5 * max(1.0, abs(val))
    _check_grads(g, ref, 'calculate_loss ' + tag)
    pw.engine.close()


@pytest.mark.parametrize('term', ['kl', 'contrastive', 'gauss', 'power_wav_eq', 'power_wav_long', 'power_wav_short'])
def test_each_term_gradient_matches_oracle(R, teachers, term):
    from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet
    tag = 'gauss' if term == 'gauss' else 'mol'
    c = _Case(R, tag)
    pw = ParallelWavenet(c.hp, teacher=teachers[tag])
    g = c.gpu_inputs()
    if term == 'kl':
        L = pw.kl_loss_logistic(c.ff(g), c.S, noise=c.rl[0])['kl_loss']
    elif term == 'contrastive':
        L = pw.contrastive_loss(c.ff(g), c.S, noise=c.rl[1])['contrastive_loss']
    elif term == 'gauss':
        L = pw.kl_loss_gauss(c.ff(g))['kl_loss']
    else:
        wav = term[6:]
        L = pw.power_loss({'x': g['x'], 'wav': c.wav[wav]})['power_loss']
    L.backward()
    val, ref = c.oracle(term[:5] if term.startswith('power') else term, wav=term[6:] if term.startswith('power') else 'wav_long')
    assert abs(float(L.detach()) - val) <= 1e-5 * max(1.0, abs(val)), (float(L.detach()), val)
    _check_grads(g, ref, term)
    pw.engine.close()


def test_full_width_teacher_gradient_matches_oracle():
    """wavenet_mol.json (width 512, 30 layers) at T = 2048: kl_loss_logistic's gradients against the float64 oracle (run on
    the device in float64)."""
    import torch
    from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet
    te_cfg = load_json('wavenet_mol.json')
    teacher = _teacher(te_cfg, seed=1234, init='tf')
    st_cfg = load_json('parallel_wavenet.json')
    pw = ParallelWavenet(st_cfg, teacher=teacher)
    B, F, T, S = 1, 11, 2048, 8
    rs = np.random.RandomState(9)
    mel = torch.as_tensor(rs.uniform(0, 1, [B, F, 80]).astype(np.float32)).cuda()
    x = torch.as_tensor(np.clip(0.2 * rs.standard_normal([B, T]), -1.2, 1.2).astype(np.float32)).cuda()
    mean = x + torch.as_tensor(0.01 * rs.standard_normal([B, T]).astype(np.float32)).cuda()
    scale = torch.as_tensor(np.exp(rs.uniform(-7, -2, [B, T])).astype(np.float32)).cuda()
    u = rs.uniform(1e-5, 1 - 1e-5, [B, S, T])
    rl = torch.as_tensor((np.log(u) - np.log(1 - u)).astype(np.float32)).cuda()
    g = {k: v.clone().requires_grad_(True) for k, v in (('x', x), ('mean_tot', mean), ('scale_tot', scale))}
    L = pw.kl_loss_logistic(dict(g, mel=mel), S, noise=rl)['kl_loss']
    L.backward()
    thp, w = D.teacher_weights(te_cfg, 1234, 'tf', device='cuda')
    enc = D.teacher_enc(mel.cpu().numpy(), te_cfg, 1234, 'tf', device='cuda')
    v = {k: t.detach().double().requires_grad_(True) for k, t in (('x', x), ('mean_tot', mean), ('scale_tot', scale))}
    # Of the 2 x 2048 x 256 pre-ReLU values a few lie within 1e-4 of their maximum from the kink, where the engine's float32
    # forward may fall on the other side: there the oracle takes the engine's ReLU derivative (read from its tape).
    pre = {}
    D.teacher_ff(v['x'].detach(), enc, w, thp, pre=pre)
    _, tape = teacher.engine.teacher_forward_tape(x, mel)
    masks, nflip = D.relu_masks(pre, D.tape_pre(tape, B, T, te_cfg['skip_width']))
    print('full width: {} near-tie ReLU derivatives taken from the engine'.format(nflip))
    assert nflip <= 16
    Lr = D.kl_logistic(D.teacher_ff(v['x'], enc, w, thp, masks=masks), v['mean_tot'], v['scale_tot'], rl.double())['kl_loss']
    Lr.backward()
    assert abs(float(L.detach()) - float(Lr.detach())) <= 1e-5 * max(1.0, abs(float(Lr.detach())))
    _check_grads(g, {k: t.grad for k, t in v.items()}, 'full width T=2048')
    pw.engine.close()
    teacher.engine.close()


def test_tape_forward_and_grad_path_are_bit_identical(R, teachers):
    import torch
    from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet
    c = _Case(R, 'mol')
    eng = teachers['mol'].engine
    a = eng.teacher_forward(c.v32['x'], c.mel['mel'])
    b, tape = eng.teacher_forward_tape(c.v32['x'], c.mel['mel'])
    assert torch.equal(a, b)
    assert tape.numel() == eng.teacher_tape_bytes(2, 512)
    for tag in ('mol', 'gauss'):
        c = _Case(R, tag)
        pw = ParallelWavenet(c.hp, teacher=teachers[tag])
        kw = {'noise': c.rl[0], 'cl_noise': c.rl[1]} if tag == 'mol' else {}
        with torch.no_grad():
            plain = pw.calculate_loss(c.ff(c.v32), **kw)
        graded = pw.calculate_loss(c.ff(c.gpu_inputs()), **kw)
        assert graded['loss'].requires_grad
        for k in plain:
            assert torch.equal(plain[k], graded[k].detach()), (tag, k)
        pw.engine.close()


def test_backward_is_repeatable_and_device_draws_match_injected(R, teachers):
    import torch
    from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet
    c = _Case(R, 'mol')
    pw = ParallelWavenet(c.hp, teacher=teachers['mol'])

    def grads(**kw):
        g = c.gpu_inputs()
        pw.calculate_loss(c.ff(g), **kw)['loss'].backward()
        return {k: t.grad.clone() for k, t in g.items()}
    g1, g2 = grads(seed=5), grads(seed=5)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    eng = teachers['mol'].engine
    te = eng.teacher_forward(c.v32['x'], c.mel['mel'])
    nz = eng.distill_mol_xent(te, c.v32['mean_tot'], c.v32['scale_tot'], c.S, seed=5, want_noise=True)['noise']
    te_r = eng.teacher_forward(c.v32['x'], c.mel['mel_rand'])
    cl_seed = (5 + 0x9E3779B97F4A7C15) % (1 << 64)
    nz_cl = eng.distill_mol_xent(te_r, c.v32['mean_tot'], c.v32['scale_tot'], c.S, seed=cl_seed, want_noise=True)['noise']
    g3 = grads(noise=nz, cl_noise=nz_cl)
    for k in g1:
        assert torch.equal(g1[k], g3[k]), k
    g4 = grads(seed=6)
    assert not torch.equal(g1['mean_tot'], g4['mean_tot'])
    pw.engine.close()


def test_two_threads_on_one_teacher_handle(R, teachers):
    import torch
    c = _Case(R, 'mol')
    eng = teachers['mol'].engine
    rs = np.random.RandomState(3)
    gout = torch.as_tensor(rs.standard_normal([2, 512, 30]).astype(np.float32)).cuda()
    fac = torch.tensor([1e-3, -2e-3], dtype=torch.float64).cuda()

    def run(e, seed):
        out, tape = e.teacher_forward_tape(c.v32['x'], c.mel['mel'])
        dw = e.teacher_backward_input(tape, gout)
        gr = e.distill_mol_xent_grad(out, c.v32['mean_tot'], c.v32['scale_tot'], 16, fac, seed=seed)
        return [dw] + list(gr)
    serial = {s: run(eng, s) for s in (11, 12)}
    torch.cuda.synchronize()
    got, errs = {}, []

    def work(seed):
        try:
            f = eng.fork()
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                rr = [run(f, seed) for _ in range(4)]
            st.synchronize()
            got[seed] = rr
        except Exception as e:                                     # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=work, args=(s,)) for s in (11, 12)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for s in (11, 12):
        for rr in got[s]:
            for a, b in zip(rr, serial[s]):
                assert torch.equal(a, b)


def _expect_refusal(fn, text):
    with pytest.raises((ValueError, RuntimeError)) as e:
        fn()
    assert text in str(e.value), str(e.value)


def test_invalid_gradient_calls_are_refused(R, teachers, student_cfg):
    import torch
    from nsynth_wavenet_amd.engine import Engine
    c = _Case(R, 'mol')
    mol, gauss = teachers['mol'].engine, teachers['gauss'].engine
    x, mel = c.v32['x'], c.mel['mel']
    mean, scale = c.v32['mean_tot'], c.v32['scale_tot']
    fac = torch.ones(2, dtype=torch.float64).cuda()
    out, tape = mol.teacher_forward_tape(x, mel)
    gout = torch.ones_like(out)
    _expect_refusal(lambda: gauss.distill_mol_xent_grad(out, mean, scale, 4, fac), 'loss_type is not mol')
    _expect_refusal(lambda: mol.distill_gauss_kl_grad(out[..., :2].contiguous(), mean, scale, fac), 'loss_type is not gauss')
    _expect_refusal(lambda: mol.distill_mol_xent_grad(out, mean, scale, 0, fac), 'num_samples')
    # a tape of another handle of the same shape, a tape of another shape, a truncated tape
    other = _teacher(*D.golden_case(R, 'mol')[1]).engine
    _expect_refusal(lambda: other.teacher_backward_input(tape, gout), 'not written by')
    _, tape1 = mol.teacher_forward_tape(x[:1], mel[:1])
    _expect_refusal(lambda: mol.teacher_backward_input(tape1, gout), 'cannot hold')
    _expect_refusal(lambda: mol.teacher_backward_input(tape, gout[:1].contiguous()), 'holds B = 2')
    _expect_refusal(lambda: mol.teacher_backward_input(tape[:1024], gout), 'cannot hold')
    other.close()
    st = Engine(student_cfg)
    _expect_refusal(lambda: st.teacher_backward_input(tape, gout), 'student handle')
    _expect_refusal(lambda: st.distill_mol_xent_grad(out, mean, scale, 4, fac), 'student handle')
    st.close()
    mu = Engine(dict(json.loads(str(R['mol/te_cfg_json'])), use_mu_law=True))
    _expect_refusal(lambda: mu.teacher_forward_tape(x, mel), 'mu-law')
    _expect_refusal(lambda: mu.distill_mol_xent_grad(out, mean, scale, 4, fac), 'mu-law')
    mu.close()


@pytest.mark.parametrize('tag,keys', [('mol', ('x',)), ('gauss', ('x', 'mean_tot', 'scale_tot'))])
def test_directional_derivative_in_the_engines_arithmetic(R, teachers, tag, keys):
    """(L(p + eps v) - L(p - eps v)) / 2 eps against <grad L, v> for the whole calculate_loss, fixed draws, v half along the
    gradient and half random.  (With the MoL teacher's sharp components -- scales down to e^-7 -- and eight fixed draws,
    L is smooth in mean_tot / scale_tot only on steps far below float32 resolution of L, so those two are held to the oracle
    alone, above.)"""
    import torch
    from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet
    c = _Case(R, tag)
    pw = ParallelWavenet(c.hp, teacher=teachers[tag])
    kw = {'noise': c.rl[0], 'cl_noise': c.rl[1]} if tag == 'mol' else {}
    g = c.gpu_inputs()
    pw.calculate_loss(c.ff(g), **kw)['loss'].backward()
    rs = np.random.RandomState(4)
    for k in keys:
        gk = g[k].grad.double()
        r = torch.as_tensor(rs.standard_normal(c.v32[k].shape)).cuda()
        v = gk / gk.norm() + r / r.norm()
        v = v / v.norm()
        eps = 3e-3 * float(c.v32[k].abs().max())
        dd = float((gk * v).sum())

        def L(sign):
            p = dict(c.v32)
            p[k] = (c.v32[k].double() + sign * eps * v).float()
            with torch.no_grad():
                return float(pw.calculate_loss(c.ff(p), **kw)['loss'])
        fd = (L(1) - L(-1)) / (2 * eps)
        print('directional {} {}: fd {:.6e} grad {:.6e}'.format(tag, k, fd, dd))
        assert abs(fd - dd) <= 1e-2 * abs(dd), (k, fd, dd)
    pw.engine.close()


def test_pytorch_student_trains_through_calculate_loss(R, teachers):
    """A tiny PyTorch student -- affine maps of fixed logistic noise z to mean_tot and log scale_tot, x = z scale + mean --
    takes SGD steps through calculate_loss(...).backward(); its parameter gradients match the float64 oracle's."""
    import torch
    from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet
    c = _Case(R, 'mol')
    pw = ParallelWavenet(c.hp, teacher=teachers['mol'])
    B, T = c.v32['x'].shape
    z = c.rl[0][:, 0].clone()
    params = [torch.tensor(v, dtype=torch.float32, device='cuda', requires_grad=True) for v in (0.05, 0.0, 0.3, -4.0)]

    def student(p, z):
        mean = p[0] * z + p[1]
        scale = torch.exp(p[2] * z + p[3])
        return {'x': z * scale + mean, 'mean_tot': mean, 'scale_tot': scale}
    losses = []
    for step in range(3):
        ff = dict(student(params, z), mel=c.mel['mel'], mel_rand=c.mel['mel_rand'], wav=c.wav['wav_long'])
        loss = pw.calculate_loss(ff, noise=c.rl[0], cl_noise=c.rl[1])['loss']
        for p in params:
            p.grad = None
        loss.backward()
        got = torch.stack([p.grad for p in params]).double().cpu()
        p64 = [p.detach().double().cpu().requires_grad_(True) for p in params]
        s64 = student(p64, z.double().cpu())
        te = lambda m: D.teacher_ff(s64['x'], c.enc[m], c.w, c.thp)
        ref_loss = D.calculate_loss(c.hp, te('mel'), te('mel_rand'), dict(s64, wav=c.wav['wav_long'].double().cpu()),
                                    c.rl[0].double().cpu(), c.rl[1].double().cpu())['loss']
        ref = torch.stack(torch.autograd.grad(ref_loss, p64))
        e = float((got - ref).abs().max()) / float(ref.abs().max())
        print('student step {}: loss {:.6f}, parameter-gradient error / max |g| = {:.2e}'.format(step, float(loss.detach()), e))
        assert e <= TOL, (step, e)
        losses.append(float(loss.detach()))
        with torch.no_grad():
            for p in params:
                p -= 1e-3 * p.grad
    assert np.all(np.isfinite(losses))
    pw.engine.close()
