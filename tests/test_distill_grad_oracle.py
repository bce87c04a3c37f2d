"""The float64 torch restatement of the teacher and the distillation losses (tests/distill_oracle64.py) that the GPU gradient
tests compare with: it reproduces the losses the reference's own code stored in tests/golden/ref_distill.npz to float64
rounding (so its torch.autograd gradient is the gradient of the reference's graph), central finite differences confirm that
gradient on single coordinates, edge branches included, and the library exports the gradient calls.  CPU only."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import distill_oracle64 as D

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_distill.npz')


@pytest.fixture(scope='module')
def R():
    return np.load(GOLD)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def _teacher_out(R, tag, mel_key, x):
    cfgd, seed, init = json.loads(str(R[tag + '/te_cfg_json'])), int(R[tag + '/te_seed']), str(R[tag + '/te_init'])
    hp, w = D.teacher_weights(cfgd, seed, init)
    enc = D.teacher_enc(R['{}/in_{}'.format(tag, mel_key)], cfgd, seed, init)
    return D.teacher_ff(x, enc, w, hp)


def test_teacher_matches_the_numpy_oracle(R):
    from oracle import wavenet_np as O
    x = torch.as_tensor(R['mol/in_x'].astype(np.float64))
    got = _teacher_out(R, 'mol', 'mel', x).numpy()
    cfgd = json.loads(str(R['mol/te_cfg_json']))
    hp = O.HP(cfgd)
    w = O.synth_weights(hp, 'teacher', seed=int(R['mol/te_seed']), init=str(R['mol/te_init']))
    enc = O.deconv_stack(R['mol/in_mel'].astype(np.float64), w, hp, '', np.float64)
    want = O.teacher_feed_forward(R['mol/in_x'].astype(np.float64), enc, w, hp, np.float64)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize('tag', ['mol', 'gauss'])
def test_reproduces_the_references_losses(R, tag):
    hp, _, inp, _ = D.golden_case(R, tag)
    x = inp['x']
    te, te_rand = _teacher_out(R, tag, 'mel', x), _teacher_out(R, tag, 'mel_rand', x)
    rl_kl, rl_cl = (torch.as_tensor(v) for v in D.golden_rl(R, np.float64))
    ff = {'x': x, 'mean_tot': inp['mean_tot'], 'scale_tot': inp['scale_tot'], 'wav': inp['wav_long']}
    got = D.calculate_loss(hp, te, te_rand, ff, rl_kl, rl_cl, log_scale=inp['log_scale_tot'])
    want = [k[len(tag) + 6:] for k in R.files if k.startswith(tag + '/full_') and R[k].ndim == 0]
    assert sorted(got) == sorted(want)
    for k in want:                                     # the teacher in float64, summed in another order than the reference's
        assert _rel(float(got[k]), R['{}/full_{}'.format(tag, k)]) < 1e-8, k
    for case in ('eq', 'long', 'short'):
        pl = D.power_loss(x, inp['wav_' + case])
        assert _rel(float(pl), R['{}/parts_power_loss_{}'.format(tag, case)]) < 1e-10
    if tag == 'mol':
        te32 = torch.as_tensor(R['mol/in_te_out_f32'].astype(np.float64))
        d = D.kl_logistic(te32, inp['mean_tot'], inp['scale_tot'], rl_kl, inp['log_scale_tot'])
        assert _rel(d['H_bl'].numpy(), R['mol/parts_H_bl']) < 1e-9
        for k in ('kl_loss', 'H_Ps', 'H_Ps_Pt'):
            assert _rel(float(d[k]), R['mol/parts_' + k]) < 1e-10, k
    else:
        te32 = torch.as_tensor(R['gauss/in_te_out_f32'].astype(np.float64))
        d = D.kl_gauss(te32, inp['mean_tot'], inp['scale_tot'], inp['log_scale_tot'])
        assert _rel(float(d['kl_loss']), R['gauss/parts_kl_loss']) < 1e-10


def _fd_check(f, t, coords, eps, rel=False):
    """autograd of the scalar f(t) against central differences at the given flat coordinates (step eps, or eps |t_i|)"""
    t = t.clone().requires_grad_(True)
    f(t).backward()
    g = t.grad.reshape(-1)
    for i in coords:
        h = eps * abs(float(t.detach().reshape(-1)[i])) if rel else eps
        tp, tm = t.detach().clone().reshape(-1), t.detach().clone().reshape(-1)
        tp[i] += h
        tm[i] -= h
        fd = (float(f(tp.reshape(t.shape))) - float(f(tm.reshape(t.shape)))) / (2 * h)
        assert abs(fd - float(g[i])) <= 1e-6 * max(1.0, abs(fd)) + 1e-9, (i, fd, float(g[i]))
    return g


def test_finite_differences_mol(R):
    hp, _, inp, _ = D.golden_case(R, 'mol')
    rl = torch.as_tensor(D.golden_rl(R, np.float64)[0])
    x, mean, scale, wav = inp['x'], inp['mean_tot'].clone(), inp['scale_tot'].clone(), inp['wav_long']
    B, T = x.shape
    # edge branches: draws below min_thres and above max_thres at two rows, and a mass below the 1e-12 floor
    mean[0, 5], scale[0, 5] = -1.0, 1e-3
    mean[1, 7], scale[1, 7] = 1.0, 1e-3
    te = _teacher_out(R, 'mol', 'mel', x).detach()
    with torch.no_grad():
        xs = rl * scale[:, None] + mean[:, None]
        assert (xs < -1 + 1 / 65536.).any() and (xs > 1 - 1 / 65536.).any()
    kl = lambda m=mean, s=scale, t=te: D.kl_logistic(t, m, s, rl)['kl_loss']
    _fd_check(lambda m: kl(m=m), mean, [5, T + 7, 100, 3], 1e-7)
    _fd_check(lambda s: kl(s=s), scale, [5, T + 7, 100, 3], 1e-6, rel=True)
    # teacher parameters: a log scale clamped at -7 (zero gradient), one inside, a mean and a logit
    te2 = te.clone()
    te2[0, 9, 20] = -9.0
    g = _fd_check(lambda t: kl(t=t), te2, [9 * 30 + 20, 11 * 30 + 21, 11 * 30 + 12, 11 * 30 + 2], 1e-7)
    assert float(g[9 * 30 + 20]) == 0.0
    # x through the teacher and the power loss (centre-trimmed against the longer wav)
    cfgd, seed, init = json.loads(str(R['mol/te_cfg_json'])), int(R['mol/te_seed']), str(R['mol/te_init'])
    thp, w = D.teacher_weights(cfgd, seed, init)
    enc = D.teacher_enc(R['mol/in_mel'], cfgd, seed, init)
    _fd_check(lambda xx: D.kl_logistic(D.teacher_ff(xx, enc, w, thp), mean, scale, rl)['kl_loss'], x, [17, T + 300], 1e-6)
    _fd_check(lambda xx: D.power_loss(xx, wav), x, [0, 250, T + 511], 1e-6)


def test_finite_differences_gauss(R):
    _, _, inp, _ = D.golden_case(R, 'gauss')
    te = torch.as_tensor(R['gauss/in_te_out_f32'].astype(np.float64))
    te[0, 3, 1] = -8.0
    mean, scale = inp['mean_tot'], inp['scale_tot']
    g = _fd_check(lambda t: D.kl_gauss(t, mean, scale)['kl_loss'], te, [3 * 2 + 1, 4 * 2 + 1, 4 * 2], 1e-7)
    assert float(g[7]) == 0.0
    _fd_check(lambda m: D.kl_gauss(te, m, scale)['kl_loss'], mean, [0, 600], 1e-7)
    _fd_check(lambda s: D.kl_gauss(te, mean, s)['kl_loss'], scale, [0, 600], 1e-6, rel=True)


def test_product_form_of_the_bin_mass_is_the_difference_form():
    """mol_log_probs(stable=True) forms the mass of a bin as sigma(a) sigma(-b) (1 - e^-(a-b)), which is the reference's
    sigma(a) - sigma(b) without its cancellation: in float64 the difference is off by about 1e-16 / mass.  On random interior
    inputs the two agree -- the mass itself, log p of every draw and the autograd gradients of their sum -- to 1e-6 relative
    wherever every component that carries a mixture weight above 1e-3 has a mass above 1e-8 (there the difference form is good
    to 1e-8; a lighter component, whose mass is at least the 1e-12 floor, adds at most its weight times 1e-4: 1e-7)."""
    B, T, S, M = 2, 130, 21, 10
    rs = np.random.RandomState(21)
    u = rs.uniform(1e-5, 1 - 1e-5, [B, S, T])
    rl = torch.as_tensor(np.log(u) - np.log(1 - u))
    te0 = np.concatenate([rs.standard_normal([B, T, M]), rs.uniform(-0.8, 0.8, [B, T, M]), rs.uniform(-6.5, -2, [B, T, M])], -1)
    k = rs.randint(0, M, [B, T])
    near = np.take_along_axis(te0[..., M:2 * M], k[..., None], -1)[..., 0]
    mean0 = np.clip(near + 0.01 * rs.standard_normal([B, T]), -0.9, 0.9)
    scale0 = np.minimum(np.exp(rs.uniform(-7, -3, [B, T])), (0.98 - np.abs(mean0)) / 12)       # every draw inside the thresholds
    with torch.no_grad():
        par = torch.as_tensor(te0)[:, None]
        x = rl * torch.as_tensor(scale0)[:, None] + torch.as_tensor(mean0)[:, None]
        assert float(x.abs().max()) < 0.99
        inv = torch.exp(-par[..., 2 * M:])
        c = x[..., None] - par[..., M:2 * M]
        a, b = inv * (c + 1.0 / D.Q), inv * (c - 1.0 / D.Q)
        diff = torch.sigmoid(a) - torch.sigmoid(b)
        prod = torch.sigmoid(a) * torch.sigmoid(-b) * (-torch.expm1(-(2.0 / D.Q) * inv))
        sc = torch.log_softmax(par[..., :M], -1) + torch.log(prod.clamp(min=1e-12))
        w = torch.softmax(sc, -1)
        keep = ((prod > 1e-8) | (w <= 1e-3)).all(-1)                     # [B,S,T]
        dom = torch.gather(prod, -1, sc.argmax(-1, keepdim=True))[..., 0]
        e_mass = float(((diff - prod).abs() / prod)[prod > 1e-8].max())
    n_low = int(((dom > 1e-13) & (dom < 1e-8)).sum())
    assert int(keep.sum()) >= 0.5 * keep.numel() and n_low >= 1

    def run(stable):
        v = [torch.as_tensor(t).requires_grad_(True) for t in (te0, mean0, scale0)]
        xx = rl * v[2][:, None] + v[1][:, None]
        lp = D.mol_log_probs(v[0][:, None].expand(-1, S, -1, -1), xx, stable)
        (lp * keep).sum().backward()
        return lp.detach(), [t.grad for t in v]
    lp_d, g_d = run(False)
    lp_p, g_p = run(True)
    e_val = float(((lp_d - lp_p).abs() / lp_p.abs().clamp(min=1.0))[keep].max())
    e_grad = [float((p - q).abs().max()) / float(p.abs().max()) for p, q in zip(g_p, g_d)]
    print('difference form against product form in float64: {} of {} draws kept ({} with a dominant mass in (1e-13, 1e-8)); '
          'mass {:.2e} relative where it is above 1e-8, log p {:.2e}, gradients (out_params, mean_tot, scale_tot) {:.2e} {:.2e} '
          '{:.2e} of their largest magnitude'.format(int(keep.sum()), keep.numel(), n_low, e_mass, e_val, *e_grad))
    assert e_mass <= 1e-6 and e_val <= 1e-6 and max(e_grad) <= 1e-6
    # and with the option off nothing changed: the pinned golden comparison above runs the difference form
    assert torch.equal(D.mol_log_probs(torch.as_tensor(te0), torch.as_tensor(mean0)), D.mol_log_probs(
        torch.as_tensor(te0), torch.as_tensor(mean0), stable=False))


def test_library_exports_the_gradient_calls():
    from nsynth_wavenet_amd import _lib
    new = ['wn_teacher_tape_bytes', 'wn_teacher_forward_tape', 'wn_teacher_backward_workspace_bytes',
           'wn_teacher_backward_input', 'wn_distill_mol_xent_grad', 'wn_distill_gauss_kl_grad',
           'wn_power_loss_grad_workspace_bytes', 'wn_power_loss_grad']
    assert set(new) <= set(_lib.SYMBOLS)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in new:
        assert hasattr(lib, s), s
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'wnhip.h')).read()
    for s in new:
        assert 'WN_API' in header and s + '(' in header, s
