"""Teacher weight-gradient benchmark: one JSON line.

    python scripts/bench_teacher_wgrad.py [--steps 5] [--no-torch] [--shapes 1x76800,8x7680]

On wavenet_mol.json with synthetic weights, at 1 x 76 800 and 8 x 7 680 samples: milliseconds per call of the training-tape
forward (wn_teacher_forward_train_tape), of the plain-tape forward and the input VJP (wn_teacher_forward_tape,
wn_teacher_backward_input -- the yardsticks, timed in the same run on the same build), of the full reverse pass with weight
gradients (wn_teacher_backward_weights, with and without d_encoding and d_wav), the tape and workspace bytes, and a
float32 torch-autograd composition of the same loss (forward plus backward to every weight) on the GPU.
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

from nsynth_wavenet_amd import weights as wts  # noqa: E402
from nsynth_wavenet_amd.engine import Engine  # noqa: E402


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


def torch_teacher(x, enc, w, hp):
    """float32 torch composition of Wavenet.feed_forward on channel-major tensors (one conv call per masked.conv1d)"""
    def conv(h, scope, dilation=1):
        W = w[scope + '/W']
        K = W.shape[1]
        if K > 1:
            h = Fn.pad(h, ((K - 1) * dilation, 0))
        return Fn.conv1d(h, W[0].permute(2, 1, 0), w[scope + '/biases'], dilation=dilation)
    T = x.shape[1]
    left = (enc.shape[2] - T) // 2
    ec = enc[:, :, left:left + T]
    l = conv(Fn.pad(x[:, None, :], (1, 0))[:, :, :-1], 'conv_start')
    s = conv(l, 'skip_start')
    for i in range(hp.num_layers):
        d = conv(l, 'dilated_conv_%d' % (i + 1), 2 ** (i % hp.num_stages)) + conv(ec, 'mel_cond_%d' % (i + 1))
        m = d.shape[1] // 2
        g = torch.sigmoid(d[:, :m]) * torch.tanh(d[:, m:])
        l = l + conv(g, 'res_%d' % (i + 1))
        s = s + conv(g, 'skip_%d' % (i + 1))
    h1 = conv(torch.relu(s), 'out1') + conv(ec, 'mel_cond_out1')
    return conv(torch.relu(h1), 'out2').transpose(1, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--shapes', default='1x76800,8x7680')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    with open(os.path.join(ROOT, 'config_jsons', 'wavenet_mol.json')) as f:
        cfgd = json.load(f)
    eng = Engine(cfgd, kind='teacher')
    w = wts.synthetic_weights(eng.hp, 'teacher', seed=1, init='unit')
    eng.load_weights(w)
    lib, h = eng.lib, eng._h
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    res = {'metric': 'teacher_wgrad_ms', 'config': 'wavenet_mol.json', 'steps': a.steps, 'shapes': {}}
    for shp in a.shapes.split(','):
        B, T = [int(v) for v in shp.split('x')]
        F = -(-T // eng.frame_shift)
        gen = torch.Generator(device='cuda').manual_seed(1)
        wav = torch.rand(B, T, device='cuda', generator=gen) * 1.8 - 0.9
        mel = torch.rand(B, F, 80, device='cuda', generator=gen)
        ow = 3 * cfgd['mol_mix']
        out = torch.empty(B, T, ow, device='cuda')
        g = torch.randn(B, T, ow, device='cuda', generator=gen)
        st = eng._stream()
        n_ws = int(lib.wn_teacher_workspace_bytes(h, B, F, T))
        n_tape = int(lib.wn_teacher_tape_bytes(h, B, T))
        n_ttape = int(lib.wn_teacher_train_tape_bytes(h, B, F, T))
        n_bws = int(lib.wn_teacher_backward_workspace_bytes(h, B, T))
        n_wws = int(lib.wn_teacher_backward_weights_workspace_bytes(h, B, F, T))
        n_g = int(lib.wn_teacher_grad_floats(h))
        ws = torch.empty(n_ws, dtype=torch.uint8, device='cuda')
        tape = torch.empty(n_ttape, dtype=torch.uint8, device='cuda')       # serves as the plain tape too
        bws = torch.empty(n_wws, dtype=torch.uint8, device='cuda')
        flat = torch.empty(n_g, device='cuda')
        dwav = torch.empty(B, T, device='cuda')
        denc = torch.empty(B, F * eng.frame_shift, cfgd['deconv_width'], device='cuda')
        r = {'B': B, 'T': T, 'tape_bytes': n_tape, 'train_tape_bytes': n_ttape, 'train_tape_bytes_per_sample': n_ttape / (B * T),
             'forward_ws_bytes': n_ws, 'backward_input_ws_bytes': n_bws, 'backward_weights_ws_bytes': n_wws, 'grad_floats': n_g}

        def fwd():
            eng._check(lib.wn_teacher_forward(h, p(wav), p(mel), B, F, T, p(out), p(ws), n_ws, st))

        def fwd_tape():
            eng._check(lib.wn_teacher_forward_tape(h, p(wav), p(mel), B, F, T, p(out), p(tape), n_tape, p(ws), n_ws, st))

        def fwd_train():
            eng._check(lib.wn_teacher_forward_train_tape(h, p(wav), p(mel), B, F, T, p(out), p(tape), n_ttape, p(ws), n_ws, st))

        def bwd_in():
            eng._check(lib.wn_teacher_backward_input(h, p(tape), n_ttape, p(g), B, T, p(dwav), p(bws), n_wws, st))

        def bwd_w():
            eng._check(lib.wn_teacher_backward_weights(h, p(tape), n_ttape, p(g), B, F, T, p(flat), n_g, None, None, p(bws), n_wws, st))

        def bwd_all():
            eng._check(lib.wn_teacher_backward_weights(h, p(tape), n_ttape, p(g), B, F, T, p(flat), n_g, p(denc), p(dwav), p(bws),
                                                       n_wws, st))
        r['forward_ms'] = timed(fwd, a.steps)
        r['forward_tape_ms'] = timed(fwd_tape, a.steps)
        r['forward_train_tape_ms'] = timed(fwd_train, a.steps)          # last: the tape the reverse passes below read
        r['backward_input_ms'] = timed(bwd_in, a.steps)
        r['backward_weights_ms'] = timed(bwd_w, a.steps)
        r['backward_weights_denc_dwav_ms'] = timed(bwd_all, a.steps)
        r['train_tape_over_tape_forward'] = r['forward_train_tape_ms'] / r['forward_tape_ms']
        r['backward_weights_over_backward_input'] = r['backward_weights_ms'] / r['backward_input_ms']
        r['backward_weights_over_tape_forward'] = r['backward_weights_ms'] / r['forward_tape_ms']
        del ws, tape, bws
        torch.cuda.empty_cache()
        if not a.no_torch:
            tw = {k: torch.as_tensor(v, device='cuda').requires_grad_('trans_conv' not in k) for k, v in w.items()}

            def tstep():
                for v in tw.values():
                    v.grad = None
                (torch_teacher(wav, enc, tw, eng.hp) * g).sum().backward()
            try:
                enc = eng.deconv(mel).transpose(1, 2).contiguous()      # [B,Cd,TE]
                r['torch_f32_fwd_bwd_ms'] = timed(tstep, max(1, a.steps // 2))
                r['torch_over_train_forward_plus_backward_weights'] = r['torch_f32_fwd_bwd_ms'] / (
                    r['forward_train_tape_ms'] + r['backward_weights_ms'])
            except RuntimeError as e:                                    # out of memory at the long shape: reported, not hidden
                r['torch_f32_fwd_bwd_ms'] = None
                r['torch_error'] = str(e).split('\n')[0][:200]
            del tw
            torch.cuda.empty_cache()
        res['shapes'][shp] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
    eng.close()
    print(json.dumps(res))


if __name__ == '__main__':
    t0 = time.time()
    main()
    sys.stderr.write('bench_teacher_wgrad: {:.1f} s\n'.format(time.time() - t0))
