"""Teacher-NLL gradient benchmark: one JSON line.

    python scripts/bench_teacher_nll_grad.py [--batch 1] [--length 7680] [--steps 200] [--no-torch]

For the four heads -- mol (wavenet_mol.json), gauss (wavenet_gauss.json), ce-256 (wavenet_ce.json) and ce-65536 (the same
without mu-law) -- at B utterances of T samples: milliseconds per call of the gradient kernel (wn_teacher_log_prob_grad) and
of the forward scoring kernel (wn_teacher_log_prob), each issued back to back on one stream into preallocated outputs and
timed with device events (so a small head shows the launch rate, not only the kernel); a float32 torch-autograd composition
of the same loss (forward plus backward) on the GPU; their ratios; and, for ce-65536, the achieved share of the HBM peak for
two reads and one write of the logits.  The scoring calls read no weights, so the handles stay without them.
Every GPU step of a caller should run under its own time limit (`timeout -k 10 ...`).
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nsynth_wavenet_amd import config as cfgmod  # noqa: E402
from nsynth_wavenet_amd.engine import Engine  # noqa: E402

HBM_PEAK_TBS = 8.0                    # MI355X HBM3E; about 6.3 TB/s is achievable by a streaming kernel


def load(name, **over):
    with open(os.path.join(ROOT, 'config_jsons', name)) as f:
        return dict(json.load(f), **over)


def timed(fn, steps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def torch_log_prob(par, wav, loss, mu):
    """float32 torch composition of the scoring (the reference's formulas, loss_func.py:22-63,66-75,128-133)"""
    Q = 256 if mu else 65536
    if mu:
        xq = torch.floor(torch.sign(wav) * torch.log1p(255.0 * wav.abs()) / float(np.log(256.0)) * 128.0)
        real, cate = xq / 128.0, xq.long() + 128
    else:
        real, cate = wav, torch.floor(wav * (Q / 2.)).long() + Q // 2
    if loss == 'ce':
        return -Fn.cross_entropy(par.reshape(-1, Q), cate.clamp(0, Q - 1).reshape(-1), reduction='none').reshape(wav.shape)
    if loss == 'gauss':
        ls = torch.clamp(par[..., 1], min=-7.0)
        z = (real - par[..., 0]) * torch.exp(-ls)
        return -0.5 * z * z - ls - 0.9189385332046727
    M = par.shape[-1] // 3
    lg, mean, ls = par[..., :M], par[..., M:2 * M], torch.clamp(par[..., 2 * M:], min=-7.0)
    inv = torch.exp(-ls)
    c = real[..., None] - mean
    plus, mn = inv * (c + 1 / Q), inv * (c - 1 / Q)
    xe = real[..., None].expand_as(plus)
    lp = torch.where(xe < 0.5 / (Q / 2) - 1, plus - Fn.softplus(plus),
                     torch.where(xe > (Q - 1.5) / (Q / 2) - 1, -Fn.softplus(mn),
                                 torch.log(torch.clamp(torch.sigmoid(plus) - torch.sigmoid(mn), min=1e-12))))
    return torch.logsumexp(lp + torch.log_softmax(lg, dim=-1), dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1)
    ap.add_argument('--length', type=int, default=7680)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--no-torch', action='store_true')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    B, T = a.batch, a.length
    heads = [('mol', load('wavenet_mol.json')), ('gauss', load('wavenet_gauss.json')), ('ce256', load('wavenet_ce.json')),
             ('ce65536', load('wavenet_ce.json', use_mu_law=False))]
    res = {'metric': 'teacher_nll_grad_ms', 'B': B, 'T': T, 'per_head': {}}
    for name, cfgd in heads:
        eng = Engine(cfgd, kind='teacher')
        loss, mu = cfgd['loss_type'], bool(cfgd['use_mu_law'])
        ow = cfgmod.teacher_out_width(eng.hp)
        gen = torch.Generator(device='cuda').manual_seed(1)
        par = torch.randn(B, T, ow, device='cuda', generator=gen)
        nls = {'mol': ow // 3, 'gauss': 1}.get(loss, 0)
        if nls:
            par[..., ow - nls:] -= 4.0                               # log-scales around -4
        wav = (torch.rand(B, T, device='cuda', generator=gen) * 1.8 - 0.9)
        g = torch.full((B, T), -1.0 / (B * T), device='cuda')
        steps = max(10, a.steps // 10) if ow == 65536 else a.steps
        lp, d_out, d_wav = torch.empty_like(wav), torch.empty_like(par), torch.empty_like(wav)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        st = eng._stream()

        def fwd():
            eng._check(eng.lib.wn_teacher_log_prob(eng._h, p(par), p(wav), B, T, p(lp), st))

        def grad():
            eng._check(eng.lib.wn_teacher_log_prob_grad(eng._h, p(par), p(wav), B, T, p(g), p(d_out), p(d_wav), st))
        r = {'out_width': ow, 'steps': steps}
        r['forward_ms'] = timed(fwd, steps)
        r['grad_ms'] = timed(grad, steps)
        r['grad_over_forward'] = r['grad_ms'] / r['forward_ms']
        if ow == 65536:
            nbytes = 3.0 * B * T * ow * 4
            r['grad_tb_per_s'] = nbytes / (r['grad_ms'] * 1e-3) / 1e12
            r['grad_frac_hbm_peak'] = r['grad_tb_per_s'] / HBM_PEAK_TBS
            r['forward_tb_per_s'] = 2.0 * B * T * ow * 4 / (r['forward_ms'] * 1e-3) / 1e12
        if not a.no_torch:
            pg = par.clone().requires_grad_(True)
            xg = wav.clone().requires_grad_(not mu and loss != 'ce')

            def tstep():
                pg.grad = None
                xg.grad = None
                (torch_log_prob(pg, xg, loss, mu) * g).sum().backward()
            with torch.no_grad():
                r['torch_f32_forward_ms'] = timed(lambda: torch_log_prob(par, wav, loss, mu), max(5, steps // 4))
            r['torch_f32_fwd_bwd_ms'] = timed(tstep, max(5, steps // 4))
            r['torch_fwd_bwd_over_forward_plus_grad'] = r['torch_f32_fwd_bwd_ms'] / (r['forward_ms'] + r['grad_ms'])
            del pg, xg
        res['per_head'][name] = {k: (round(v, 5) if isinstance(v, float) else v) for k, v in r.items()}
        del par, d_out
        eng.close()
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == '__main__':
    t0 = time.time()
    main()
    sys.stderr.write('bench_teacher_nll_grad: {:.1f} s\n'.format(time.time() - t0))
