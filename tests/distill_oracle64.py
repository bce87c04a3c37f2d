"""Float64 PyTorch restatement of the teacher's Wavenet.feed_forward (wavenet/wavenet.py:180-291) and of the distillation
losses (wavenet/parallel_wavenet.py:361-512, loss_func.py:22-75) -- the reference's graph, written so that torch.autograd
gives the gradient TensorFlow's autodiff gives for it: the MoL mass as the difference of two sigmoids, tf.maximum as
clamp (the gradient passes at the tie), tf.where as torch.where, relu, and |STFT| with a zero gradient at 0.
tests/test_distill_grad_oracle.py pins it to tests/golden/ref_distill.npz; the GPU gradient tests compare with it."""
import json

import numpy as np
import torch
import torch.nn.functional as Fn

PRIORITY_FREQ = 384
Q = 65536


def teacher_weights(cfgd, seed, init, device='cpu'):
    """the teacher's synthetic weights (oracle.wavenet_np.synth_weights) as float64 tensors, and its hparams"""
    from oracle import wavenet_np as O
    hp = O.HP(cfgd)
    w = O.synth_weights(hp, 'teacher', seed=seed, init=init)
    return hp, {k: torch.as_tensor(np.asarray(v, np.float64), device=device) for k, v in w.items()}


def teacher_enc(mel, cfgd, seed, init, device='cpu'):
    """the teacher's upsampled conditioning [B,TE,Cd] in float64 (no gradient flows to mel)"""
    from oracle import wavenet_np as O
    hp = O.HP(cfgd)
    w = O.synth_weights(hp, 'teacher', seed=seed, init=init)
    return torch.as_tensor(O.deconv_stack(np.asarray(mel, np.float64), w, hp, '', np.float64), device=device)


def _delay(x, n):
    if n == 0:
        return x
    if n >= x.shape[1]:
        return torch.zeros_like(x)
    return Fn.pad(x[:, :-n], (0, 0, n, 0))


def _conv(x, w, scope, dilation=1):
    """causal dilated conv (masked.py:160-232): y[t] = b + sum_k x[t - (K-1-k) d] @ W[0,k]"""
    W, b = w[scope + '/W'], w[scope + '/biases']
    K = W.shape[1]
    y = b
    for k in range(K):
        y = y + _delay(x, (K - 1 - k) * dilation) @ W[0, k]
    return y


def _cond(x, c):
    left = (c.shape[1] - x.shape[1]) // 2
    return x + c[:, left:left + x.shape[1]]


def teacher_ff(x, enc, w, hp, masks=None, pre=None):
    """out_params [B,T,out_width] of the raw audio x [B,T] (no mu-law).  masks: {'s', 'h1'} [B,T,skip] 0/1 tensors that
    replace the two ReLUs' derivatives (relu(v) = v * mask, see relu_masks); pre: a dict that receives the two pre-ReLU
    tensors."""
    relu = (lambda v, k: torch.relu(v)) if masks is None else (lambda v, k: v * masks[k])
    x = x[..., None]
    l = _conv(_delay(x, 1), w, 'conv_start')
    s = _conv(l, w, 'skip_start')
    for i in range(hp.num_layers):
        d = _cond(_conv(l, w, 'dilated_conv_%d' % (i + 1), 2 ** (i % hp.num_stages)),
                  _conv(enc, w, 'mel_cond_%d' % (i + 1)))
        m = d.shape[2] // 2
        g = torch.sigmoid(d[..., :m]) * torch.tanh(d[..., m:])
        l = l + _conv(g, w, 'res_%d' % (i + 1))
        s = s + _conv(g, w, 'skip_%d' % (i + 1))
    if pre is not None:
        pre['s'] = s.detach()
    s = relu(s, 's')
    h1 = _cond(_conv(s, w, 'out1'), _conv(enc, w, 'mel_cond_out1'))
    if pre is not None:
        pre['h1'] = h1.detach()
    return _conv(relu(h1, 'h1'), w, 'out2')


def tape_pre(tape, B, T, S):
    """the engine's pre-ReLU skip sum and out1 rows [B,T,S] from a tape of Engine.teacher_forward_tape (header of 256 bytes,
    then both as float32 in the accumulator layout [B][t/16][S/16][lane = 16 ((c % 16) // 4) + t % 16][c % 4])"""
    Tp = (T + 255) // 256 * 256
    f = tape[256:256 + 2 * B * S * Tp * 4].view(torch.float32).reshape(2, B, Tp // 16, S // 16, 4, 16, 4)
    # [k][b][tb][rb][q][n][r] -> [k][b][tb n][rb q r]
    v = f.permute(0, 1, 2, 5, 3, 4, 6).reshape(2, B, Tp, S)[:, :, :T]
    return {'s': v[0], 'h1': v[1]}


def relu_masks(pre64, pre_dev, rel=1e-4):
    """ReLU derivatives for the oracle: its own sign, except where its float64 pre-activation lies within rel * max of 0 --
    there a float32 evaluation may land on the other side of the kink, and the engine's sign (pre_dev) is taken.
    Returns (masks, number of such near-tie elements whose sign differs)."""
    m, nflip = {}, 0
    for k in ('s', 'h1'):
        p, d = pre64[k], pre_dev[k].to(pre64[k].device, torch.float64)
        near = p.abs() < rel * float(p.abs().max())
        nflip += int(((p > 0) != (d > 0))[near].sum())
        m[k] = torch.where(near, d > 0, p > 0).to(torch.float64)
    return m, nflip


def _softplus(v):
    return Fn.softplus(v, beta=1, threshold=50)


def mol_log_probs(par, x, stable=False):
    """loss_func.py:22-63: par [...,3M], x [...] -> log p [...].  stable: the bin mass as the product
    sigma(a) sigma(-b) (1 - e^-(a-b)) with a - b = 2 inv_s / Q taken directly -- the same function as the reference's
    difference of two sigmoids, which in float64 loses about 1e-16 / mass of relative accuracy where both are near 1."""
    M = par.shape[-1] // 3
    lg, mean, ls = par[..., :M], par[..., M:2 * M], torch.clamp(par[..., 2 * M:], min=-7.0)
    inv = torch.exp(-ls)
    x = x[..., None]
    c = x - mean
    plus, mn = inv * (c + 1.0 / Q), inv * (c - 1.0 / Q)
    if stable:
        delta = torch.sigmoid(plus) * torch.sigmoid(-mn) * (-torch.expm1(-(2.0 / Q) * inv))
    else:
        delta = torch.sigmoid(plus) - torch.sigmoid(mn)
    max_thres, min_thres = (Q - 1 - 0.5) / (Q / 2.) - 1.0, 0.5 / (Q / 2.) - 1.0
    xe = x.expand_as(plus)
    lp = torch.where(xe < min_thres, plus - _softplus(plus),
                     torch.where(xe > max_thres, -_softplus(mn), torch.log(torch.clamp(delta, min=1e-12))))
    return torch.logsumexp(lp + torch.log_softmax(lg, dim=-1), dim=-1)


def kl_logistic(te, mean, scale, rl, log_scale=None, stable=False):
    """kl_loss_logistic (parallel_wavenet.py:361-402) on the draws rl [B,S,T]; H_Ps from log_scale when given (the
    reference's input), else from log(scale) (the mirror's); stable as in mol_log_probs"""
    S = rl.shape[1]
    x = rl * scale[:, None, :] + mean[:, None, :]
    lp = mol_log_probs(te[:, None].expand(-1, S, -1, -1), x, stable)
    hb = -lp.mean(dim=1)
    H_Ps = (torch.log(scale) if log_scale is None else log_scale).mean() + 2
    H_Ps_Pt = hb.mean()
    return {'kl_loss': H_Ps_Pt - H_Ps, 'H_Ps': H_Ps, 'H_Ps_Pt': H_Ps_Pt, 'H_bl': hb}


def kl_gauss(te, mean_q, scale_q, log_scale_q=None):
    """kl_loss_gauss (parallel_wavenet.py:404-429)"""
    mean_p, log_scale_p = te[..., 0], torch.clamp(te[..., 1], min=-7.0)
    scale_p = torch.exp(log_scale_p)
    lq = torch.log(scale_q) if log_scale_q is None else log_scale_q
    kl_bl = log_scale_p - lq + (scale_q ** 2 - scale_p ** 2 + (mean_p - mean_q) ** 2) / (2 * scale_p ** 2)
    return {'kl_loss': kl_bl.mean() + 4.0 * ((log_scale_p - lq) ** 2).mean(), 'kl_bl': kl_bl}


def stft_mag(y):
    """tf.contrib.signal.stft(frame_length=800, frame_step=200, fft_length=2048, pad_end=True), magnitude"""
    L = y.shape[1]
    nf = -(-L // 200)
    y = Fn.pad(y, (0, (nf - 1) * 200 + 800 - L))
    n = torch.arange(800, dtype=torch.float64, device=y.device)
    w = 0.5 - 0.5 * torch.cos(2 * np.pi * n / 800)
    frames = y.unfold(1, 800, 200) * w
    return torch.abs(torch.fft.rfft(frames, n=2048, dim=-1))


def _trim(x, n):
    left = n // 2
    return x[:, left:left + x.shape[1] - n]


def power_loss(pred, orig):
    lp, lo = pred.shape[1], orig.shape[1]
    if lp > lo:
        pred = _trim(pred, lp - lo)
    elif lo > lp:
        orig = _trim(orig, lo - lp)
    d = (stft_mag(orig) - stft_mag(pred)) ** 2
    return 0.5 * d.mean() + 0.5 * d[:, :, :PRIORITY_FREQ].mean()


def calculate_loss(hp, te, te_rand, ff, rl_kl=None, rl_cl=None, log_scale=None, stable=False):
    """parallel_wavenet.py:492-512: te / te_rand are the teacher's out_params on x under mel / mel_rand"""
    plf = hp['power_loss_factor']
    if hp.get('loss_type', 'logistic') == 'logistic':
        d = kl_logistic(te, ff['mean_tot'], ff['scale_tot'], rl_kl, log_scale, stable)
        d.pop('H_bl')
        clf = hp.get('contrastive_loss_factor', 0.0)
    else:
        d = {'kl_loss': kl_gauss(te, ff['mean_tot'], ff['scale_tot'], log_scale)['kl_loss']}
        clf = 0.0
    loss = d['kl_loss']
    if plf > 0:
        d['power_loss'] = power_loss(ff['x'], ff['wav'])
        loss = loss + plf * d['power_loss']
    if clf > 0:
        d['contrastive_loss'] = -kl_logistic(te_rand, ff['mean_tot'], ff['scale_tot'], rl_cl, log_scale, stable)['kl_loss']
        loss = loss + clf * d['contrastive_loss']
    d['loss'] = loss
    return d


def golden_rl(R, dtype=np.float32):
    """the reference's logistic draws of tests/golden/ref_distill.npz as [B,S,T] (kl, contrastive): float32 as the GPU
    tests inject them, float64 as the reference's graph forms them"""
    B, T = R['mol/in_x'].shape
    S = int(R['S'])
    u = np.random.RandomState(int(R['mol/u_seed'])).uniform(1e-5, 1 - 1e-5, [2, B * S, T]).astype(np.float32)
    u = u.astype(np.float64)
    return [(np.log(v) - np.log(1.0 - v)).astype(dtype).reshape(B, S, T) for v in u]


def golden_case(R, tag, device='cpu'):
    """(student hparams, teacher (cfg, seed, init), float64 inputs) of one golden case"""
    te = (json.loads(str(R[tag + '/te_cfg_json'])), int(R[tag + '/te_seed']), str(R[tag + '/te_init']))
    inp = {k: torch.as_tensor(R['{}/in_{}'.format(tag, k)].astype(np.float64), device=device)
           for k in ('x', 'mean_tot', 'scale_tot', 'log_scale_tot', 'wav_long', 'wav_eq', 'wav_short')}
    mel = {k: R['{}/in_{}'.format(tag, k)] for k in ('mel', 'mel_rand')}
    return json.loads(str(R[tag + '/st_cfg_json'])), te, inp, mel
