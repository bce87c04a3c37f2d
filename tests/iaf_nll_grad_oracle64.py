"""Float64 oracle of the gradient of the student's log-likelihood (TEST INFRASTRUCTURE), built on
student_grad_oracle64.StudentGrad64 and input_grad_oracle64.student_forward, which stay as they are.

For a cotangent c [B,T] of log p(x[t]) = log f(z[t]) - log S[t], z = encode(x), with x^ = z S + M the forward at z:
    g_z = c (log f)'(z)        d_S = -c / S
    A^T lam = g_z + (dS/dz)^T d_S,   A = d x^ / d z   (lower triangular with diagonal S)
    d / d x = lam;   d / d theta, d / d encoding = the VJP of (x^, S) with the cotangents (-lam, d_S)
The solve is the Jacobi sweep the engine runs, lam <- lam + (g_z + r) / S with r = VJP_z(-lam, d_S), in float64.
tests/test_iaf_nll_grad_oracle.py holds the result to central differences that re-solve the inverse.  A helper, not a test
module."""
import numpy as np
import torch

import iaf_inverse_oracle64 as inv
import input_grad_oracle64 as IG
import student_grad_oracle64 as S

DT = torch.float64


def dlogf(z, loss_type):
    """(log f)'(z): -tanh(z / 2) for Logistic(0,1), -z for Normal(0,1)"""
    return -z if loss_type == 'gauss' else -torch.tanh(0.5 * z)


class NllGrad64(object):
    """The forward graph at one (weights, mel, z), kept for any number of VJPs."""

    def __init__(self, weights, hp, mel, z):
        self.hp, self.loss_type = hp, hp.get('loss_type', 'logistic')
        self.ora = ora = S.StudentGrad64(weights, hp)
        self.z = torch.as_tensor(np.asarray(z), dtype=DT).clone().requires_grad_(True)
        self.w = dict(ora.w)
        for n in ora.names:
            self.w[n] = ora.w[n].clone().requires_grad_(True)
        self.encs = [e.clone().requires_grad_(True) for e in ora.encodings(mel)]
        self.out = IG.student_forward(ora, self.z, self.encs, self.w)
        self.S = self.out['scale_tot'].detach()
        with torch.no_grad():
            self.aux = {k: ([t.numpy() for t in v] if isinstance(v, list) else v.numpy())
                        for k, v in ora.forward(np.asarray(z), [e.detach() for e in self.encs])[1].items()}

    def values(self):
        return {k: v.detach().numpy() for k, v in self.out.items()}

    def log_prob(self):
        return inv.log_density(self.z.detach().numpy(), np.log(self.S.numpy()), self.loss_type)

    def vjp(self, d_x, d_S, wrt):
        g = torch.autograd.grad((self.out['x'] * d_x).sum() + (self.out['scale_tot'] * d_S).sum(), wrt, retain_graph=True,
                                allow_unused=True)
        return [torch.zeros_like(v) if gi is None else gi for gi, v in zip(g, wrt)]

    def cotangents(self, c):
        """(g_z, d_S) as float64 tensors; c None: -1 / (B T)"""
        z = self.z.detach()
        c = torch.full_like(z, -1.0 / z.numel()) if c is None else torch.as_tensor(np.asarray(c), dtype=DT)
        return c * dlogf(z, self.loss_type), -c / self.S

    def solve(self, g_z, d_S, n_sweeps=24, lam0=None):
        """n_sweeps Jacobi sweeps from lam0 (zeros) -> (lam, [max |lam' - lam| / max |lam'| of every sweep])"""
        g_z, d_S = (torch.as_tensor(np.asarray(v), dtype=DT) for v in (g_z, d_S))
        lam = torch.zeros_like(g_z) if lam0 is None else torch.as_tensor(np.asarray(lam0), dtype=DT).clone()
        upd = []
        for _ in range(n_sweeps):
            r = self.vjp(-lam, d_S, [self.z])[0]
            new = lam + (g_z + r) / self.S
            m = float(new.abs().max())
            upd.append(float((new - lam).abs().max()) / m if m > 0 else 0.0)
            lam = new
        return lam, upd

    def grads(self, c, n_sweeps=24):
        """{'lam' [B,T], 'grads': {tf name: ndarray}, 'd_encoding' [n_stacks,B,TE,Cd], 'updates', 'g_z', 'd_S'}"""
        g_z, d_S = self.cotangents(c)
        lam, upd = self.solve(g_z, d_S, n_sweeps)
        names = self.ora.names
        g = self.vjp(-lam, d_S, [self.w[n] for n in names] + self.encs)
        return {'lam': lam.numpy(), 'grads': {n: g[i].numpy() for i, n in enumerate(names)},
                'd_encoding': np.stack([gi.transpose(1, 2).numpy() for gi in g[len(names):]]), 'updates': upd,
                'g_z': g_z.numpy(), 'd_S': d_S.numpy()}


def value(mel, x, c, weights, hp, z_init):
    """sum(c log p(x)) with the inverse re-solved by iaf_inverse_oracle64.inverse in float64 from z_init"""
    r = inv.inverse(mel, x, weights, hp, np.float64, z_init=z_init)
    assert r['converged']
    return float((np.asarray(c, np.float64) * inv.log_density(r['z'], r['log_scale_tot'], hp.get('loss_type', 'logistic'))).sum())


def value_on_encodings(ora, encs, x, c, z_init, max_sweeps=None):
    """the same functional on GIVEN encodings (iaf_inverse_oracle64 starts from mel): the sweeps of the inverse on
    input_grad_oracle64.student_forward, until a sweep moves no bit"""
    x = torch.as_tensor(np.asarray(x), dtype=DT)
    z = torch.as_tensor(np.asarray(z_init), dtype=DT).clone()
    with torch.no_grad():
        for _ in range(x.shape[1] if max_sweeps is None else max_sweeps):
            o = IG.student_forward(ora, z, encs)
            zn = (x - o['mean_tot']) / o['scale_tot']
            same = bool(torch.equal(zn, z))
            z = zn
            if same:
                break
        assert same
        lp = inv.log_density(z.numpy(), np.log(o['scale_tot'].numpy()), ora.hp.get('loss_type', 'logistic'))
    return float((np.asarray(c, np.float64) * lp).sum())


def dense_cotangent(shape, seed=11):
    """a dense d_log_prob, float32 values held in float64"""
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32).astype(np.float64)


_CASES = {}


def case_oracle(name):
    """Per case of tests/iaf_encode_cases.py, once (the GPU test modules share it): the graph at z = float32(z0), a dense
    cotangent c and the loss's own, -1 / (B T), with the oracle's gradients for both.
    -> {'hp', 'w', 'mel', 'z' (float32), 'G', 'x' (float64 forward of z), 'c', 'dense': grads(c), 'loss': grads(None)}"""
    from iaf_encode_cases import case_inputs, case_model
    if name not in _CASES:
        hp, w = case_model(name)
        mel, z0 = case_inputs(name)
        z = z0.astype(np.float32)
        G = NllGrad64(w, hp, mel, z.astype(np.float64))
        c = dense_cotangent(z.shape)
        _CASES[name] = {'hp': hp, 'w': w, 'mel': mel, 'z': z, 'G': G, 'x': G.values()['x'], 'c': c, 'dense': G.grads(c),
                        'loss': G.grads(None)}
    return _CASES[name]
