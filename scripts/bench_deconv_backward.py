"""Upsampler-backward benchmark: one JSON line.

    python scripts/bench_deconv_backward.py [--steps 20] [--rounds 5] [--shapes 1x76800,8x7680]

On wavenet_mol.json with synthetic weights, at 1 x 76 800 and 8 x 7 680 samples (F = 384 and 8 x 39 mel frames), in one run
on one build, milliseconds per call of
  * wn_deconv_backward alone (the gradients of trans_conv_j/kernel and /bias from a cotangent of the encoding),
  * wn_teacher_backward_weights with d_encoding, for scale,
  * the float32 torch-autograd route over conv_transpose1d (forward plus backward to the same variables): the yardstick,
  * Wavenet.loss_and_weight_grads with and without upsampler=True (what the flag adds).
Every candidate is warmed up at the shape, then timed in `rounds` windows of `steps` calls between device events, the
candidates alternating inside a round; the median over the rounds is reported with the smallest and largest window.
Every GPU step of a caller should run under its own time limit (`timeout -k 10 ...`).
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nsynth_wavenet_amd import weights as wts  # noqa: E402
from nsynth_wavenet_amd.wavenet.wavenet import Wavenet  # noqa: E402


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def measure(cands, steps, rounds):
    """{name: {'ms': median, 'min_ms', 'max_ms'}}: warm-up, then `rounds` rounds in which the candidates take turns"""
    for fn, _ in cands.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in cands}
    for _ in range(rounds):
        for k, (fn, div) in cands.items():
            got[k].append(window(fn, max(1, steps // div)))
    out = {}
    for k, v in got.items():
        v = sorted(v)
        out[k] = {'ms': round(v[len(v) // 2], 4), 'min_ms': round(v[0], 4), 'max_ms': round(v[-1], 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--shapes', default='1x76800,8x7680')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    with open(os.path.join(ROOT, 'config_jsons', 'wavenet_mol.json')) as f:
        cfgd = json.load(f)
    net = Wavenet(cfgd)
    eng = net.engine
    w = wts.synthetic_weights(eng.hp, 'teacher', seed=1, init='unit')
    net.load_weights(w)
    lib, h = eng.lib, eng._h
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    dc = cfgd['deconv_config']
    assert cfgd['upsample_act'] == 'leaky_relu'
    res = {'metric': 'deconv_backward_ms', 'config': 'wavenet_mol.json', 'steps': a.steps, 'rounds': a.rounds, 'shapes': {}}
    for shp in a.shapes.split(','):
        B, T = [int(v) for v in shp.split('x')]
        F = -(-T // eng.frame_shift)
        gen = torch.Generator(device='cuda').manual_seed(1)
        wav = torch.rand(B, T, device='cuda', generator=gen) * 1.8 - 0.9
        mel = torch.rand(B, F, 80, device='cuda', generator=gen)
        ow = 3 * cfgd['mol_mix']
        out = torch.empty(B, T, ow, device='cuda')
        g = torch.randn(B, T, ow, device='cuda', generator=gen)
        genc = torch.randn(B, F * eng.frame_shift, cfgd['deconv_width'], device='cuda', generator=gen)
        st = eng._stream()
        n_ws = int(lib.wn_teacher_workspace_bytes(h, B, F, T))
        n_ttape = int(lib.wn_teacher_train_tape_bytes(h, B, F, T))
        n_wws = int(lib.wn_teacher_backward_weights_workspace_bytes(h, B, F, T))
        n_g = int(lib.wn_teacher_grad_floats(h))
        n_dws = int(lib.wn_deconv_backward_workspace_bytes(h, b'', B, F))
        n_dg = int(lib.wn_deconv_grad_floats(h, b''))
        ws = torch.empty(n_ws, dtype=torch.uint8, device='cuda')
        tape = torch.empty(n_ttape, dtype=torch.uint8, device='cuda')
        bws = torch.empty(n_wws, dtype=torch.uint8, device='cuda')
        dws = torch.empty(n_dws, dtype=torch.uint8, device='cuda')
        flat = torch.empty(n_g, device='cuda')
        dflat = torch.empty(n_dg, device='cuda')
        denc = torch.empty(B, F * eng.frame_shift, cfgd['deconv_width'], device='cuda')
        eng._check(lib.wn_teacher_forward_train_tape(h, p(wav), p(mel), B, F, T, p(out), p(tape), n_ttape, p(ws), n_ws, st))
        tw = {k: torch.as_tensor(v, device='cuda').requires_grad_(True) for k, v in w.items() if 'trans_conv' in k}
        mel_cm = mel.transpose(1, 2).contiguous()
        genc_cm = genc.transpose(1, 2).contiguous()

        def deconv_bwd():
            eng._check(lib.wn_deconv_backward(h, b'', p(mel), p(genc), B, F, p(dflat), n_dg, p(dws), n_dws, st))

        def teacher_bwd():
            eng._check(lib.wn_teacher_backward_weights(h, p(tape), n_ttape, p(g), B, F, T, p(flat), n_g, p(denc), None, p(bws),
                                                       n_wws, st))

        def torch_route():
            for v in tw.values():
                v.grad = None
            x = mel_cm
            for j, (fl, s) in enumerate(dc):
                W = tw['trans_conv_%d/kernel' % (j + 1)]
                x = Fn.leaky_relu(Fn.conv_transpose1d(x, W[0].permute(2, 1, 0), tw['trans_conv_%d/bias' % (j + 1)], stride=s,
                                                      padding=(fl - s) // 2), 0.4)
            (x * genc_cm).sum().backward()
        inputs = {'wav': wav, 'mel': mel}
        r = {'B': B, 'T': T, 'F': F, 'workspace_bytes': n_dws, 'grad_floats': n_dg}
        r.update(measure({'deconv_backward': (deconv_bwd, 1), 'teacher_backward_weights_denc': (teacher_bwd, 4),
                          'torch_f32_conv_transpose1d_fwd_bwd': (torch_route, 1)}, a.steps, a.rounds))
        r.update(measure({'loss_and_weight_grads': (lambda: net.loss_and_weight_grads(inputs), 4),
                          'loss_and_weight_grads_upsampler': (lambda: net.loss_and_weight_grads(inputs, upsampler=True), 4)},
                         a.steps, a.rounds))
        r['deconv_backward_over_torch'] = round(r['deconv_backward']['ms'] / r['torch_f32_conv_transpose1d_fwd_bwd']['ms'], 4)
        r['upsampler_flag_adds_ms'] = round(r['loss_and_weight_grads_upsampler']['ms'] - r['loss_and_weight_grads']['ms'], 4)
        # same inputs, both routes.  The float32 torch forward and the engine's split-fp16 forward do not agree on the sign of
        # every near-zero pre-activation at this size, and no tie is excluded here (the tests do that, on a float64 oracle):
        # reported are the sign disagreements of the stack's output, and per gradient the largest and the rms difference
        deconv_bwd()
        torch_route()
        torch.cuda.synchronize()
        with torch.no_grad():
            x = mel_cm
            for j, (fl, s) in enumerate(dc):
                x = Fn.leaky_relu(Fn.conv_transpose1d(x, tw['trans_conv_%d/kernel' % (j + 1)][0].permute(2, 1, 0),
                                                      tw['trans_conv_%d/bias' % (j + 1)], stride=s, padding=(fl - s) // 2), 0.4)
            r['output_sign_disagreements_with_torch_f32'] = int(((x > 0) != (eng.deconv(mel).transpose(1, 2) > 0)).sum())
        diff = {}
        for name, off, shape in eng.deconv_grad_table():
            n = 1
            for d in shape:
                n *= d
            a_, b_ = dflat[off:off + n].view(shape), tw[name].grad
            diff[name] = {'max_over_max': float((a_ - b_).abs().max() / b_.abs().max()),
                          'rms_over_rms': float((a_ - b_).pow(2).mean().sqrt() / b_.pow(2).mean().sqrt())}
        r['difference_to_torch_f32'] = diff
        res['shapes'][shp] = r
        del ws, tape, bws, dws, tw
        torch.cuda.empty_cache()
    eng.close()
    print(json.dumps(res))


if __name__ == '__main__':
    t0 = time.time()
    main()
    sys.stderr.write('bench_deconv_backward: {:.1f} s\n'.format(time.time() - t0))
