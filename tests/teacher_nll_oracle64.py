"""Float64 PyTorch restatement of the teacher's scoring -- the per-sample term of Wavenet.calculate_loss (wavenet/wavenet.py:
293-316): loss_func.mol_log_probs (loss_func.py:22-63, the class count Q a parameter), gauss_log_prob (:66-75,104-119) and the
sparse softmax cross entropy of ce_loss (:128-133), on the targets of Wavenet.encode_signal (wavenet.py:157-178) -- written as
distill_oracle64.py is, so that torch.autograd gives the gradient TensorFlow's autodiff gives for the reference's graph: the MoL
mass as the difference of two sigmoids, tf.maximum as clamp (the gradient passes at the tie), tf.where as torch.where, and
floor (mu-law, the class index) with a zero gradient.  tests/test_teacher_nll_oracle.py pins it to oracle.wavenet_np and to
finite differences; tests/test_gpu_teacher_nll_grad.py compares the HIP gradient kernel with it.
Also the inputs of those GPU tests (kernel_case) and the conditions that keep them away from every tie (tie_report), so that
the CPU suite checks the seeds before a GPU sees them."""
import numpy as np
import torch

from distill_oracle64 import _softplus


def quant_chann(use_mu_law):
    return 256 if use_mu_law else 65536


def mu_law_value(wav):
    """utils.py:72-87 before the floor: sign(x) log(1 + 255 |x|) / log(256) * 128, in (-128, 128)"""
    return torch.sign(wav) * torch.log(1.0 + 255.0 * torch.abs(wav)) / float(np.log(256.0)) * 128.0


def encode_targets(wav, use_mu_law):
    """wavenet.py:157-178: (real_targets [B,T], cate_targets [B,T] int64).  Without mu-law the real target is the audio itself
    (and carries its graph); with it, and for the class index, floor() cuts the graph as TensorFlow's does."""
    q = quant_chann(use_mu_law)
    if use_mu_law:
        xq = torch.floor(mu_law_value(wav))
        return xq / (q / 2.), xq.detach().long() + q // 2
    return wav, torch.floor(wav.detach() * (q / 2.)).long() + q // 2


def mol_log_probs(par, x, Q):
    """loss_func.py:22-63 with quant_chann = Q: par [...,3M], x [...] -> log p [...]"""
    M = par.shape[-1] // 3
    lg, mean, ls = par[..., :M], par[..., M:2 * M], torch.clamp(par[..., 2 * M:], min=-7.0)
    inv = torch.exp(-ls)
    x = x[..., None]
    c = x - mean
    plus, mn = inv * (c + 1.0 / Q), inv * (c - 1.0 / Q)
    delta = torch.sigmoid(plus) - torch.sigmoid(mn)
    max_thres, min_thres = (Q - 1 - 0.5) / (Q / 2.) - 1.0, 0.5 / (Q / 2.) - 1.0
    xe = x.expand_as(plus)
    lp = torch.where(xe < min_thres, plus - _softplus(plus),
                     torch.where(xe > max_thres, -_softplus(mn), torch.log(torch.clamp(delta, min=1e-12))))
    return torch.logsumexp(lp + torch.log_softmax(lg, dim=-1), dim=-1)


def gauss_log_prob(par, x):
    """loss_func.py:66-75,104-119: Normal(mean, exp(max(p, -7))).log_prob(x)"""
    ls = torch.clamp(par[..., 1], min=-7.0)
    z = (x - par[..., 0]) * torch.exp(-ls)
    return -0.5 * z * z - ls - 0.5 * float(np.log(2.0 * np.pi))


def ce_log_prob(par, cate):
    """loss_func.py:128-133: minus the sparse softmax cross entropy per sample"""
    return torch.gather(torch.log_softmax(par, dim=-1), -1, cate[..., None])[..., 0]


def teacher_log_prob(par, wav, loss_type, use_mu_law):
    """log-likelihood [B,T] of the raw audio wav [B,T] under out_params par [B,T,ow]; Wavenet.calculate_loss's 'loss' is minus
    its mean"""
    real, cate = encode_targets(wav, use_mu_law)
    if loss_type == 'mol':
        return mol_log_probs(par, real, quant_chann(use_mu_law))
    if loss_type == 'gauss':
        return gauss_log_prob(par, real)
    if loss_type == 'ce':
        return ce_log_prob(par, cate)
    raise ValueError(loss_type)


def grads(par, wav, g, loss_type, use_mu_law):
    """float64 (log_prob, d par, d wav) of sum(g * log_prob) at the given (float32 or float64) values; d wav is zero where
    autograd finds no path (quantised targets)"""
    p = torch.as_tensor(np.asarray(par, np.float64)).requires_grad_(True)
    x = torch.as_tensor(np.asarray(wav, np.float64)).requires_grad_(True)
    lp = teacher_log_prob(p, x, loss_type, use_mu_law)
    (lp * torch.as_tensor(np.asarray(g, np.float64))).sum().backward()
    return lp.detach(), p.grad, (x.grad if x.grad is not None else torch.zeros_like(x))


# ---- inputs of the GPU kernel tests: every edge the gradient kernel has, and nothing within reach of a tie ----
KERNEL_CASES = {
    # tag: (loss_type, use_mu_law, mol_mix, B, T)
    'mol10': ('mol', False, 10, 2, 37),
    'mol3_mulaw': ('mol', True, 3, 2, 37),
    'gauss': ('gauss', False, 0, 2, 37),
    'ce_mulaw': ('ce', True, 0, 2, 37),
    'ce_16bit': ('ce', False, 0, 1, 5),
}


def _inv_mu_law(k):
    from oracle import wavenet_np as O
    return O.inv_mu_law(np.asarray(k, np.int64), dtype=np.float64).astype(np.float32)


def kernel_case(tag, seed=20):
    """float32 (out_params [B,T,ow], wav [B,T], d_log_prob [B,T]) of one kernel case.
    Targets sit in the lowest and the highest bin at the first two samples and the last one (the tail wave of the last
    block); mu-law and class targets are bin centres (inv_mu_law of integers, (k + 0.5) / 32768).  MoL log-scales are drawn
    from [-6.5, -3], a tenth of them below -7 and one exactly -7; the means are placed a logistic argument a in [-4, 4] from
    the target (a bin mass of at least 1e-5, which float64 resolves to 1e-11 as a difference of sigmoids), except for a few
    components at a = -500 with a narrow scale: a mass far below the 1e-12 floor.  Logits span +-20."""
    loss, mu, M, B, T = KERNEL_CASES[tag]
    rs = np.random.RandomState(seed + sorted(KERNEL_CASES).index(tag))
    Q = quant_chann(mu)
    if mu:
        k = rs.randint(-128, 128, [B, T])
        k[k == 0] = 1                                   # inv_mu_law(0) is 0 itself (utils.py:121), a bin edge, not a centre
        k[0, 0], k[0, 1], k[-1, -1] = -128, 127, -128
        wav = _inv_mu_law(k)
        xt = k / 128.0
    elif loss == 'ce':
        k = rs.randint(-32768, 32768, [B, T])
        k[0, 0], k[0, 1], k[-1, -1] = -32768, 32767, 32767
        wav = ((k + 0.5) / 32768.0).astype(np.float32)
        xt = wav.astype(np.float64)
    else:
        wav = rs.uniform(-0.9, 0.9, [B, T]).astype(np.float32)
        wav[0, 0], wav[0, 1], wav[-1, -1] = -1.0, 1.0 - 2.0 / Q, -1.0
        xt = wav.astype(np.float64)
    g = rs.standard_normal([B, T]).astype(np.float32)
    if loss == 'ce':
        par = rs.uniform(-20, 20, [B, T, Q])
    elif loss == 'gauss':
        ls = rs.uniform(-6.5, -1.0, [B, T])
        low = rs.uniform(size=[B, T]) < 0.1
        ls[low] = rs.uniform(-9.0, -7.5, int(low.sum()))
        ls[1, 3] = -7.0
        z = rs.uniform(-5, 5, [B, T])
        par = np.stack([xt - z * np.exp(np.maximum(ls, -7.0)), ls], axis=-1)
    else:
        lg = rs.uniform(-20, 20, [B, T, M])
        ls = rs.uniform(-6.5, -3.0, [B, T, M])
        low = rs.uniform(size=[B, T, M]) < 0.1
        ls[low] = rs.uniform(-9.0, -7.5, int(low.sum()))
        ls[1, 3, 1] = -7.0
        a = rs.uniform(-4, 4, [B, T, M])
        far = np.zeros([B, T, M], bool)
        far[0, 5, 0] = far[1, 7, M - 1] = far[0, 0, 1] = far[-1, -1, 0] = True    # interior and edge-bin samples
        ls[far], a[far] = -6.9, -500.0
        mean = xt[..., None] - a * np.exp(np.maximum(ls, -7.0))
        par = np.concatenate([lg, mean, ls], axis=-1)
    return par.astype(np.float32), wav, g


def tie_report(tag, par, wav):
    """what the GPU test asserts about a case's inputs, evaluated in float64: {'mass_in_band': MoL component masses in
    [1e-13, 1e-11], 'target_near_threshold': targets within 1e-6 of an edge-bin threshold (mol) / of a class boundary (the
    continuous value before floor(), in target units: mu-law and ce), 'scale_near_tie': raw log-scales within 1e-6 of -7 that
    are not exactly -7, 'scale_at_tie': exactly -7, 'scale_below': below -7, 'mass_below_floor', 'low_bin', 'high_bin'}"""
    loss, mu, M, B, T = KERNEL_CASES[tag]
    Q = quant_chann(mu)
    p, x = torch.as_tensor(np.asarray(par, np.float64)), torch.as_tensor(np.asarray(wav, np.float64))
    r = dict.fromkeys(('mass_in_band', 'target_near_threshold', 'scale_near_tie', 'scale_at_tie', 'scale_below',
                       'mass_below_floor', 'low_bin', 'high_bin'), 0)
    real, cate = encode_targets(x, mu)
    near = torch.zeros_like(x, dtype=torch.bool)
    if mu or loss == 'ce':
        v = mu_law_value(x) if mu else x * (Q / 2.)               # floor(v) is the class; v / (Q / 2) the target
        near |= (v - torch.round(v)).abs() / (Q / 2.) <= 1e-6
    if loss == 'ce':
        r['low_bin'], r['high_bin'] = int((cate == 0).sum()), int((cate == Q - 1).sum())
    else:
        raw = p[..., 2 * M:] if loss == 'mol' else p[..., 1]
        r['scale_at_tie'] = int((raw == -7.0).sum())
        r['scale_near_tie'] = int((((raw + 7.0).abs() <= 1e-6) & (raw != -7.0)).sum())
        r['scale_below'] = int((raw < -7.0).sum())
    if loss == 'mol':
        max_thres, min_thres = (Q - 1 - 0.5) / (Q / 2.) - 1.0, 0.5 / (Q / 2.) - 1.0
        near |= ((real - min_thres).abs() <= 1e-6) | ((real - max_thres).abs() <= 1e-6)
        r['low_bin'], r['high_bin'] = int((real < min_thres).sum()), int((real > max_thres).sum())
        inv = torch.exp(-torch.clamp(p[..., 2 * M:], min=-7.0))
        c = real[..., None] - p[..., M:2 * M]
        mass = torch.sigmoid(inv * (c + 1.0 / Q)) - torch.sigmoid(inv * (c - 1.0 / Q))
        r['mass_in_band'] = int(((mass >= 1e-13) & (mass <= 1e-11)).sum())
        r['mass_below_floor'] = int((mass < 1e-13).sum())
    r['target_near_threshold'] = int(near.sum())
    return r
