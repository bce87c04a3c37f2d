"""float64 torch restatement of oracle.torch_ref.StudentRef.feed_forward WITH autograd (TEST INFRASTRUCTURE): the oracle of the
student's weight gradients.  Built from torch.clamp and F.softplus on torch_ref's conv primitives, so that
autograd's conventions are the project's: a clamp passes the gradient at the tie and none beyond it, a ReLU at exactly 0
passes none.  Shared / teacher-owned and private deconv stacks.  tests/test_student_grad_oracle.py holds its values to
StudentRef(dtype=float64) and its gradients to central differences."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.torch_ref import EXP_7, EXP_M9, conv1d, trans_conv1d

DT = torch.float64


def is_shared(hp):
    return bool(hp.get('use_share_deconv', False) or hp.get('use_teacher_deconv', False))


def stack_scopes(hp):
    """the deconv stacks in the order of d_encoding's leading axis"""
    return ['iaf_share'] if is_shared(hp) else ['iaf_{:d}'.format(k + 1) for k in range(len(hp.num_iaf_layers))]


def variable_names(hp):
    """every variable of every flow, upsampler excluded, in the order weights.expected_variables lists them"""
    out = []
    for k, L in enumerate(hp.num_iaf_layers):
        p = 'iaf_{:d}/'.format(k + 1)
        scopes = ['start_conv']
        for i in range(L):
            scopes += ['dilated_conv_{:d}'.format(i + 1), 'mel_cond_{:d}'.format(i + 1), 'res_{:d}'.format(i + 1)]
        scopes += ['out1', 'mel_cond_out1', 'out2_mean', 'out2_scale']
        for s in scopes:
            out += [p + s + '/W', p + s + '/biases']
    return out


class StudentGrad64(object):
    def __init__(self, weights, hp):
        assert not hp.get('use_weight_norm', False) and hp.get('upsample_act', 'tanh') == 'leaky_relu'
        self.hp = hp
        self.w = {k: torch.as_tensor(np.asarray(v), dtype=DT) for k, v in weights.items()}
        self.names = variable_names(hp)

    def encodings(self, mel):
        """[n_stacks] of enc [B, Cd, F frame_shift] (the upsampler's own variables are not differentiated here)"""
        h0 = torch.as_tensor(np.asarray(mel), dtype=DT).transpose(1, 2)
        out = []
        with torch.no_grad():
            for prefix in stack_scopes(self.hp):
                h = h0
                for j, (fl, s) in enumerate(self.hp.deconv_config):
                    sc = '{}/trans_conv_{:d}'.format(prefix, j + 1)
                    h = trans_conv1d(h, self.w[sc + '/kernel'], self.w[sc + '/bias'], s)
                out.append(h)
        return out

    def forward(self, noise, encs, w=None):
        """StudentRef.feed_forward on given encodings and variables -> x, mean_tot, scale_tot [B,T] and what the tests
        assert on: 'scales' (per flow, clamped), 'softplus' (per flow, before the clamp), 'scale_prod' (before the e^7
        clamp), 'pre_relu' (every pre-ReLU tensor)."""
        hp, w = self.hp, (self.w if w is None else w)
        x0 = torch.as_tensor(np.asarray(noise), dtype=DT)
        T = x0.shape[1]
        c = lambda v, scope, d=1: conv1d(v, w[scope + '/W'], w[scope + '/biases'], d)
        x = x0[:, None, :]
        mean_tot, scale_tot = torch.zeros_like(x), torch.ones_like(x)
        aux = {'scales': [], 'softplus': [], 'pre_relu': []}
        for k, L in enumerate(hp.num_iaf_layers):
            p = 'iaf_{:d}'.format(k + 1)
            e = encs[0] if is_shared(hp) else encs[k]
            left = (e.shape[2] - T) // 2
            ec = e[:, :, left:left + T]
            l = c(F.pad(x, (1, 0))[:, :, :-1], p + '/start_conv')
            for i in range(L):
                d = c(l, '{}/dilated_conv_{:d}'.format(p, i + 1), 2 ** (i % hp.num_stages))
                d = d + c(ec, '{}/mel_cond_{:d}'.format(p, i + 1))
                m = d.shape[1] // 2
                l = l + c(torch.sigmoid(d[:, :m]) * torch.tanh(d[:, m:]), '{}/res_{:d}'.format(p, i + 1))
            h1 = c(torch.relu(l), p + '/out1') + c(ec, p + '/mel_cond_out1')
            aux['pre_relu'] += [l, h1]
            r = torch.relu(h1)
            mean = c(r, p + '/out2_mean')
            sp = F.softplus(c(r, p + '/out2_scale'))
            scale = torch.clamp(sp, EXP_M9, EXP_7)
            aux['softplus'].append(sp)
            aux['scales'].append(scale)
            x = x * scale + mean
            mean_tot = mean + mean_tot * scale
            scale_tot = scale_tot * scale
        aux['scale_prod'] = scale_tot[:, 0]
        scale_tot = torch.clamp(scale_tot, max=EXP_7)[:, 0]
        mean_tot = mean_tot[:, 0]
        return {'x': x0 * scale_tot + mean_tot, 'mean_tot': mean_tot, 'scale_tot': scale_tot}, aux

    def grads(self, mel, noise, d_x, d_mean_tot, d_scale_tot):
        """The cotangents are those of the three returned tensors as INDEPENDENT outputs; x's dependence on the other two is
        part of the graph.  -> {'values': {x, mean_tot, scale_tot}, 'grads': {tf name: ndarray in the TF shape},
        'd_encoding': [n_stacks, B, F frame_shift, Cd], 'aux': forward()'s}"""
        w = dict(self.w)
        for n in self.names:
            w[n] = self.w[n].clone().requires_grad_(True)
        encs = [e.clone().requires_grad_(True) for e in self.encodings(mel)]
        out, aux = self.forward(noise, encs, w)
        cot = [torch.as_tensor(np.asarray(v), dtype=DT) for v in (d_x, d_mean_tot, d_scale_tot)]
        # x = noise scale_tot + mean_tot is formed inside forward(): the surrogate below differentiates it with the rest
        L = (out['x'] * cot[0]).sum() + (out['mean_tot'] * cot[1]).sum() + (out['scale_tot'] * cot[2]).sum()
        leaves = [w[n] for n in self.names] + encs
        g = torch.autograd.grad(L, leaves, allow_unused=True)
        g = [torch.zeros_like(v) if gi is None else gi for gi, v in zip(g, leaves)]
        nv = len(self.names)
        return {'values': {k: v.detach().numpy() for k, v in out.items()},
                'grads': {n: g[i].numpy() for i, n in enumerate(self.names)},
                'd_encoding': np.stack([gi.transpose(1, 2).numpy() for gi in g[nv:]]),
                'aux': {k: ([t.detach().numpy() for t in v] if isinstance(v, list) else v.detach().numpy())
                        for k, v in aux.items()}}

    def surrogate(self, mel, noise, cot, w=None):
        """the fixed linear functional of (x, mean_tot, scale_tot) grads() differentiates, as a float"""
        ww = None
        if w is not None:
            ww = dict(self.w)
            ww.update({k: torch.as_tensor(np.asarray(v), dtype=DT) for k, v in w.items()})
        with torch.no_grad():
            out, _ = self.forward(noise, self.encodings(mel), ww)
            return float(sum((out[k] * torch.as_tensor(np.asarray(c), dtype=DT)).sum()
                             for k, c in zip(('x', 'mean_tot', 'scale_tot'), cot)))


def near_tie_fraction(aux, eps=1e-6):
    """share of the ReLU mask elements whose pre-ReLU value lies within eps of 0"""
    n = sum(v.size for v in aux['pre_relu'])
    return sum(int((np.abs(v) < eps).sum()) for v in aux['pre_relu']) / float(n)


def clamps_inactive(aux, rel=1e-6):
    """no per-flow scale and no scale_tot within rel (relative) of a clamp bound, and none beyond one"""
    ok = True
    for sp in aux['softplus']:
        ok = ok and bool(np.all(sp > EXP_M9 * (1 + rel))) and bool(np.all(sp < EXP_7 * (1 - rel)))
    return ok and bool(np.all(aux['scale_prod'] < EXP_7 * (1 - rel)))


# ---- the models and inputs the tests share ----
DECONV = [[8, 2], [12, 4]]          # frame_shift 8


def case_config(width, deconv_width, num_stages, num_iaf_layers, shared, loss_type):
    return {'deconv_config': DECONV, 'deconv_width': deconv_width, 'filter_length': 3, 'loss_type': loss_type,
            'num_iaf_layers': list(num_iaf_layers), 'num_stages': num_stages, 'upsample_act': 'leaky_relu',
            'use_mu_law': False, 'use_resize_conv': False, 'use_share_deconv': bool(shared), 'use_teacher_deconv': False,
            'use_weight_norm': False, 'wave_length': 7680, 'width': width}


S1 = case_config(64, 64, 3, [2, 3], True, 'logistic')        # half-tile guard, wrapped dilation cycle, ragged tiles
S2 = case_config(128, 128, 10, [10, 1], False, 'gauss')      # two m-tiles, unguarded BGATE, private stacks


def case_inputs(B, F, T, seed, n_mel=80):
    """mel, logistic noise and dense cotangents of x, mean_tot, scale_tot"""
    rs = np.random.RandomState(seed)
    mel = rs.uniform(0, 1, [B, F, n_mel]).astype(np.float32)
    u = rs.uniform(1e-5, 1 - 1e-5, [B, T])
    noise = (np.log(u) - np.log1p(-u)).astype(np.float32)
    cot = [rs.standard_normal([B, T]).astype(np.float32) for _ in range(3)]
    return mel, noise, cot
