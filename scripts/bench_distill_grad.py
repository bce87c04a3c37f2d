"""Distillation-gradient benchmark: one JSON line.

    python scripts/bench_distill_grad.py [--shapes 1x384,8x39] [--samples 100] [--steps 5] [--no-torch]

parallel_wavenet.json student hparams with the wavenet_mol.json teacher (synthetic weights); shapes BxF: B utterances of F
mel frames (1x384: one 4.8 s utterance, T = 76 800; 8x39: the training shape, eight 7 680-sample clips).  Per shape: ms per
call of the teacher forward, the forward with tape, the input VJP, each gradient kernel (MoL cross entropy with device
draws, Gauss KL on a [B,T,2] tensor, power loss), the no-grad calculate_loss and the differentiable calculate_loss forward
plus backward; the tape bytes; the VJP's executed fp16-MFMA rate in the teacher forward's terms (three
MFMAs per split-fp16 product, every GEMM at its padded row count over the padded columns); the ratios of the targets; and,
beside them, a float32 PyTorch-autograd composition of the same teacher and losses on the GPU at the largest length that
fits, with its peak memory.  Every GPU step of a caller should run under its own time limit (`timeout -k 10 ...`).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import wavenet_np as O  # noqa: E402
from nsynth_wavenet_amd import config as cfgmod  # noqa: E402
from nsynth_wavenet_amd import engine as E  # noqa: E402
from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet  # noqa: E402
from nsynth_wavenet_amd.wavenet.wavenet import Wavenet  # noqa: E402

FP16_PEAK_PFLOPS = 2.5               # MI355X dense fp16 MFMA


def load(name):
    with open(os.path.join(ROOT, 'config_jsons', name)) as f:
        return json.load(f)


def timed(fn, steps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def vjp_flops_per_column(c):
    """executed fp16-MFMA flops of the input VJP per (padded) column: 3 MFMAs x 2 M K per GEMM"""
    W, S, G = c['width'], c['skip_width'], 2 * c['width'] if c.get('double_gate_width') else c['width']
    H, L = G // 2, c['num_layers']
    ow = 3 * c['mol_mix']
    kp = (ow + 31) // 32 * 32
    per_layer = H * (W + S) + W * 3 * G
    return 3 * 2 * (L * per_layer + S * kp + S * S + W * S)


# ---- float32 torch-autograd composition of the teacher and the losses (the comparison the issue asks for) ----
def torch_teacher(x, enc, w, hp):
    def delay(v, n):
        return v if n == 0 else Fn.pad(v[:, :-n], (0, 0, n, 0))

    def conv(v, scope, d=1):
        W, b = w[scope + '/W'], w[scope + '/biases']
        y = b
        for k in range(W.shape[1]):
            y = y + delay(v, (W.shape[1] - 1 - k) * d) @ W[0, k]
        return y

    def cond(v, c):
        left = (c.shape[1] - v.shape[1]) // 2
        return v + c[:, left:left + v.shape[1]]
    l = conv(delay(x[..., None], 1), 'conv_start')
    s = conv(l, 'skip_start')
    for i in range(hp.num_layers):
        d = cond(conv(l, 'dilated_conv_%d' % (i + 1), 2 ** (i % hp.num_stages)), conv(enc, 'mel_cond_%d' % (i + 1)))
        m = d.shape[2] // 2
        g = torch.sigmoid(d[..., :m]) * torch.tanh(d[..., m:])
        l = l + conv(g, 'res_%d' % (i + 1))
        s = s + conv(g, 'skip_%d' % (i + 1))
    s = torch.relu(cond(conv(torch.relu(s), 'out1'), conv(enc, 'mel_cond_out1')))
    return conv(s, 'out2')


def torch_kl(te, mean, scale, S, Q=65536.0):
    B, T, W = te.shape
    M = W // 3
    u = torch.rand(B, S, T, device=te.device) * (1 - 2e-5) + 1e-5
    x = (torch.log(u) - torch.log(1 - u)) * scale[:, None] + mean[:, None]
    p = te[:, None]
    lg, mu, ls = p[..., :M], p[..., M:2 * M], torch.clamp(p[..., 2 * M:], min=-7.0)
    inv = torch.exp(-ls)
    c = x[..., None] - mu
    plus, mn = inv * (c + 1 / Q), inv * (c - 1 / Q)
    xe = x[..., None].expand_as(plus)
    lp = torch.where(xe < 0.5 / (Q / 2) - 1, plus - Fn.softplus(plus),
                     torch.where(xe > (Q - 1.5) / (Q / 2) - 1, -Fn.softplus(mn),
                                 torch.log(torch.clamp(torch.sigmoid(plus) - torch.sigmoid(mn), min=1e-12))))
    hb = -torch.logsumexp(lp + torch.log_softmax(lg, dim=-1), dim=-1).mean(dim=1)
    return hb.mean() - (torch.log(scale).mean() + 2)


def torch_power(pred, orig):
    def mag(y):
        L = y.shape[1]
        nf = -(-L // 200)
        y = Fn.pad(y, (0, (nf - 1) * 200 + 800 - L))
        w = torch.hann_window(800, periodic=True, device=y.device)
        return torch.abs(torch.fft.rfft(y.unfold(1, 800, 200) * w, n=2048, dim=-1))
    d = (mag(orig) - mag(pred)) ** 2
    return 0.5 * d.mean() + 0.5 * d[:, :, :384].mean()


def torch_composition(te_cfg, B, F, S, steps):
    """float32 autograd of kl + power + contrastive through the teacher at the largest F (halving) that fits"""
    hp = O.HP(te_cfg)
    wn = O.synth_weights(hp, 'teacher', seed=1234, init='tf')
    w = {k: torch.as_tensor(np.asarray(v, np.float32)).cuda() for k, v in wn.items()}
    while F >= 3:
        try:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            rs = np.random.RandomState(0)
            T = F * 200 // 512 * 512
            mel = rs.uniform(0, 1, [B, F, 80])
            enc = torch.as_tensor(O.deconv_stack(mel, wn, hp, '', np.float32).astype(np.float32)).cuda()
            x = torch.as_tensor((0.3 * rs.standard_normal([B, T])).astype(np.float32)).cuda().requires_grad_(True)
            mean = (x.detach() + 0.01).requires_grad_(True)
            scale = torch.full((B, T), 1e-3, device='cuda', requires_grad=True)
            wav = x.detach() * 0.9

            def step():
                te = torch_teacher(x, enc, w, hp)
                te_r = torch_teacher(x, enc.flip(1), w, hp)
                L = torch_kl(te, mean, scale, S) + torch_power(x, wav) - 0.3 * torch_kl(te_r, mean, scale, S)
                L.backward()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            ms = timed(step, steps)
            return {'B': B, 'F': F, 'T': T, 'S': S, 'ms': round(ms, 3),
                    'peak_gb': round((torch.cuda.max_memory_allocated() - base) / 1e9, 3)}
        except torch.cuda.OutOfMemoryError:
            F //= 2
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='1x384,8x39')
    ap.add_argument('--samples', type=int, default=100)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--no-torch', action='store_true')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    st_cfg = dict(load('parallel_wavenet.json'), num_samples=a.samples, power_loss_factor=1.0, contrastive_loss_factor=0.3)
    te_cfg = load('wavenet_mol.json')
    teacher = Wavenet(te_cfg).load_weights(O.synth_weights(O.HP(te_cfg), 'teacher', seed=1234, init='tf'))
    pw = ParallelWavenet(st_cfg, teacher=teacher).load_weights(O.synth_weights(O.HP(st_cfg), 'student', seed=1234, init='tf'))
    gauss_teacher = Wavenet(load('wavenet_gauss.json'))          # the Gauss KL kernels need only the handle's shape
    te = teacher.engine
    res = {'metric': 'distill_grad_ms', 'S': a.samples, 'per_shape': {}}
    for shape in a.shapes.split(','):
        B, F = (int(v) for v in shape.split('x'))
        rs = np.random.RandomState(B)
        mel = torch.as_tensor(rs.uniform(0, 1, [B, F, 80]).astype(np.float32)).cuda()
        mel_rand = torch.as_tensor(rs.uniform(0, 1, [B, F, 80]).astype(np.float32)).cuda()
        T = cfgmod.iaf_length(pw.hparams, F)
        ff = pw.feed_forward({'mel': mel}, seed=1)
        ff.update(mel=mel, mel_rand=mel_rand,
                  wav=torch.as_tensor(np.clip(0.3 * rs.standard_normal([B, T + 400]), -1, 1).astype(np.float32)).cuda())
        x, mean, scale = ff['x'], ff['mean_tot'], ff['scale_tot']
        out, tape = te.teacher_forward_tape(x, mel)
        gout = torch.randn_like(out) * 1e-6
        fac = torch.tensor([1.0 / (B * T), -1.0 / (B * T)], dtype=torch.float64, device='cuda')
        g2 = torch.stack([mean, torch.log(scale)], dim=-1).contiguous()
        wav = ff['wav'][:, 200:200 + T]
        r = {'T': T, 'tape_bytes': te.teacher_tape_bytes(B, T)}
        r['teacher_forward_ms'] = timed(lambda: te.teacher_forward(x, mel), a.steps)
        r['forward_tape_ms'] = timed(lambda: te.teacher_forward_tape(x, mel), a.steps)
        r['input_vjp_ms'] = timed(lambda: te.teacher_backward_input(tape, gout), a.steps)
        r['mol_xent_grad_ms'] = timed(lambda: te.distill_mol_xent_grad(out, mean, scale, a.samples, fac, seed=2), a.steps)
        r['gauss_kl_grad_ms'] = timed(lambda: gauss_teacher.engine.distill_gauss_kl_grad(g2, mean, scale, fac), a.steps)
        r['power_loss_grad_ms'] = timed(lambda: E.power_loss_grad(x, wav, fac), a.steps)
        r['calculate_loss_ms'] = timed(lambda: pw.calculate_loss(ff, seed=3), max(2, a.steps // 2))
        xg, mg, sg = (v.detach().clone().requires_grad_(True) for v in (x, mean, scale))
        ffg = dict(ff, x=xg, mean_tot=mg, scale_tot=sg)
        r['calculate_loss_fwd_bwd_ms'] = timed(lambda: pw.calculate_loss(ffg, seed=3)['loss'].backward(), max(2, a.steps // 2))
        Tp = (T + 255) // 256 * 256
        flops = vjp_flops_per_column(te_cfg) * B * Tp
        r['vjp_pflops'] = flops / (r['input_vjp_ms'] * 1e-3) / 1e15
        r['vjp_frac_fp16_peak'] = r['vjp_pflops'] / FP16_PEAK_PFLOPS
        r['forward_tape_over_forward'] = r['forward_tape_ms'] / r['teacher_forward_ms']          # target <= 1.10
        r['vjp_over_forward'] = r['input_vjp_ms'] / r['teacher_forward_ms']                      # target <= 1.25
        r['fwd_bwd_over_calculate_loss'] = r['calculate_loss_fwd_bwd_ms'] / r['calculate_loss_ms']   # target <= 2.5
        del tape, out
        torch.cuda.empty_cache()
        if not a.no_torch:
            r['torch_autograd_f32'] = torch_composition(te_cfg, B, F, a.samples, 2)
        res['per_shape'][shape] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
    print(json.dumps(res))


if __name__ == '__main__':
    t0 = time.time()
    main()
    sys.stderr.write('bench_distill_grad: {:.1f} s\n'.format(time.time() - t0))
