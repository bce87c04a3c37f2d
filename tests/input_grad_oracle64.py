"""Float64 oracles of the input gradients (TEST INFRASTRUCTURE): d mel through a deconv stack, d noise
through the student's flows, and the two composed -- ParallelWavenet.feed_forward differentiated in mel and noise.  Built on
tests/deconv_grad_oracle64.py and tests/student_grad_oracle64.py, which stay as they are; tests/test_input_grad_oracle.py
holds every gradient here to float64 central differences on the CPU.

Ties.  d mel of a stack alone goes by the rules of deconv_grad_oracle64 (pick_rows seeds, mask_last on the cotangent).  In
the composed gradient the cotangent of the encoding is the student's and cannot be masked, so the rule is that of
test_gpu_deconv_backward_geometries.test_public_chain_on_three_layers: mel rows whose hidden pre-activations are clear of
zero (pick_rows_stacks), and at the last layer's near ties -- at most MAX_ZEROED of its elements -- the oracle takes the sign
the engine's forward took (feed_forward_grads' `pos`)."""
import numpy as np
import torch
import torch.nn.functional as F

import deconv_grad_oracle64 as DG
import student_grad_oracle64 as S
from oracle.torch_ref import EXP_7, EXP_M9, conv1d

DT = torch.float64


# ---- d mel of one stack ----
def stack_d_mel(mel, w, deconv_config, act, g, prefix=''):
    """d sum(enc * g) / d mel [B,F,n_mel] in float64: deconv_grad_oracle64.stack_ff with mel as the leaf"""
    leaf = torch.as_tensor(np.asarray(mel), dtype=DT).clone().requires_grad_(True)
    _, enc = DG.stack_ff(leaf, w, deconv_config, act, prefix)
    return torch.autograd.grad((enc * torch.as_tensor(g, dtype=DT)).sum(), leaf)[0]


def stack_value(mel, w, deconv_config, act, g, prefix=''):
    """the functional stack_d_mel differentiates, as a float"""
    with torch.no_grad():
        _, enc = DG.stack_ff(torch.as_tensor(np.asarray(mel), dtype=DT), w, deconv_config, act, prefix)
        return float((enc * torch.as_tensor(g, dtype=DT)).sum())


# ---- d noise of the student ----
def student_forward(ora, noise, encs, w=None):
    """StudentGrad64.forward restated with `noise` a float64 TENSOR that stays in the graph (the method wraps it with
    np.asarray, which cuts it): x, mean_tot, scale_tot [B,T].  encs: [n_stacks] of [B,Cd,TE] tensors."""
    hp, w = ora.hp, (ora.w if w is None else w)
    T = noise.shape[1]
    c = lambda v, scope, d=1: conv1d(v, w[scope + '/W'], w[scope + '/biases'], d)
    x = noise[:, None, :]
    mean_tot, scale_tot = torch.zeros_like(x), torch.ones_like(x)
    for k, L in enumerate(hp.num_iaf_layers):
        p = 'iaf_{:d}'.format(k + 1)
        e = encs[0] if S.is_shared(hp) else encs[k]
        left = (e.shape[2] - T) // 2
        ec = e[:, :, left:left + T]
        l = c(F.pad(x, (1, 0))[:, :, :-1], p + '/start_conv')
        for i in range(L):
            d = c(l, '{}/dilated_conv_{:d}'.format(p, i + 1), 2 ** (i % hp.num_stages))
            d = d + c(ec, '{}/mel_cond_{:d}'.format(p, i + 1))
            m = d.shape[1] // 2
            l = l + c(torch.sigmoid(d[:, :m]) * torch.tanh(d[:, m:]), '{}/res_{:d}'.format(p, i + 1))
        r = torch.relu(c(torch.relu(l), p + '/out1') + c(ec, p + '/mel_cond_out1'))
        scale = torch.clamp(F.softplus(c(r, p + '/out2_scale')), EXP_M9, EXP_7)
        mean = c(r, p + '/out2_mean')
        x = x * scale + mean
        mean_tot = mean + mean_tot * scale
        scale_tot = scale_tot * scale
    scale_tot = torch.clamp(scale_tot, max=EXP_7)[:, 0]
    mean_tot = mean_tot[:, 0]
    return {'x': noise * scale_tot + mean_tot, 'mean_tot': mean_tot, 'scale_tot': scale_tot}


def functional(out, cot):
    """sum(x d_x + mean_tot d_mean_tot + scale_tot d_scale_tot)"""
    return sum((out[k] * torch.as_tensor(np.asarray(c), dtype=DT)).sum() for k, c in zip(('x', 'mean_tot', 'scale_tot'), cot))


def student_input_grads(ora, mel, noise, cot):
    """{'values', 'd_noise' [B,T], 'd_encoding' [n_stacks,B,TE,Cd]} with the noise and the encodings as leaves"""
    z = torch.as_tensor(np.asarray(noise), dtype=DT).clone().requires_grad_(True)
    encs = [e.clone().requires_grad_(True) for e in ora.encodings(mel)]
    out = student_forward(ora, z, encs)
    g = torch.autograd.grad(functional(out, cot), [z] + encs)
    return {'values': {k: v.detach().numpy() for k, v in out.items()}, 'd_noise': g[0].numpy(),
            'd_encoding': np.stack([gi.transpose(1, 2).numpy() for gi in g[1:]])}


def student_value(ora, mel, noise, cot):
    with torch.no_grad():
        return float(functional(student_forward(ora, torch.as_tensor(np.asarray(noise), dtype=DT), ora.encodings(mel)), cot))


# ---- the two composed: feed_forward in mel and noise ----
def stacks_pre(ora, mel):
    """{scope: [pre-activation z_j [B,C,T_j]]} of every stack of the student, float64"""
    hp = ora.hp
    with torch.no_grad():
        return {p: DG.stack_ff(mel, DG.weights64(ora.w, len(hp.deconv_config), p), hp.deconv_config, 'leaky_relu', p)[0]
                for p in S.stack_scopes(hp)}


def pick_rows_stacks(ora, B, F, n_mel=80, first=DG.FIRST_SEED):
    """deconv_grad_oracle64.pick_rows for EVERY stack of the student at once: (mel, seeds), row i the first seed from `first`
    upward (after row i - 1's) whose hidden pre-activations have no near tie in any stack"""
    hp = ora.hp
    ws = [(p, DG.weights64(ora.w, len(hp.deconv_config), p)) for p in S.stack_scopes(hp)]
    rows, seeds, seed = [], [], first
    while len(rows) < B:
        assert seed < first + DG.SEARCH_LIMIT, 'no seed without a hidden near tie'
        cand = list(range(seed, seed + DG.BATCH))
        mels = np.stack([DG._mel_row(s, F, n_mel) for s in cand])
        ties = np.sum([DG.hidden_ties(mels, w, hp.deconv_config, p, 'leaky_relu') for p, w in ws], axis=0)
        clear = [i for i, n in enumerate(ties) if n == 0]
        if not clear:
            seed += DG.BATCH
            continue
        rows.append(mels[clear[0]])
        seeds.append(cand[clear[0]])
        seed = cand[clear[0]] + 1
    return np.stack(rows), tuple(seeds)


def _stack_graph(mel, w, dc, prefix, pos_last):
    """stack_ff under leaky_relu, the last layer's sign given (pos_last [B,C,TE] bool, or None: its own): enc [B,Cd,TE]"""
    h = mel.transpose(1, 2)
    for j, (fl, s) in enumerate(dc):
        W, b = w['{}/trans_conv_{:d}/kernel'.format(prefix, j + 1)], w['{}/trans_conv_{:d}/bias'.format(prefix, j + 1)]
        z = F.conv_transpose1d(h, W[0].permute(2, 1, 0).contiguous(), b, stride=s, padding=(fl - s) // 2)
        if pos_last is not None and j == len(dc) - 1:
            h = z * torch.where(pos_last, torch.tensor(1.0, dtype=DT), torch.tensor(0.4, dtype=DT))     # 0.4 in float64
        else:
            h = F.leaky_relu(z, 0.4)
    return h


def feed_forward_grads(ora, mel, noise, cot, pos=None):
    """The functional of feed_forward's x, mean_tot, scale_tot with mel and noise as leaves, every stack in the graph.
    pos: None, or {scope: bool [B,Cd,TE]} -- the sign of each stack's last pre-activation (see the module docstring)
    -> {'values', 'd_mel' [B,F,n_mel], 'd_noise' [B,T], 'value': the functional}"""
    hp = ora.hp
    m = torch.as_tensor(np.asarray(mel), dtype=DT).clone().requires_grad_(True)
    z = torch.as_tensor(np.asarray(noise), dtype=DT).clone().requires_grad_(True)
    encs = [_stack_graph(m, ora.w, hp.deconv_config, p, None if pos is None else pos[p]) for p in S.stack_scopes(hp)]
    out = student_forward(ora, z, encs)
    L = functional(out, cot)
    g = torch.autograd.grad(L, [m, z])
    return {'values': {k: v.detach().numpy() for k, v in out.items()}, 'd_mel': g[0].numpy(), 'd_noise': g[1].numpy(),
            'value': float(L.detach())}
