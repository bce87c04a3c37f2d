"""Student weight-gradient benchmark: one JSON line.

    python scripts/bench_student_grad.py [--steps 5] [--no-torch] [--shapes 1x76800,8x7680]

On parallel_wavenet.json with synthetic weights, at 1 x 76 800 and 8 x 7 680 samples: milliseconds per call, from device events
on preallocated buffers, of iaf_generate (wn_iaf_generate: the first yardstick), of the training-tape forward
(wn_iaf_forward_train_tape), of the reverse pass (wn_iaf_backward_weights, with and without d_encoding), the tape and
workspace bytes, and a float32 torch-autograd composition of the same student (forward plus backward to every variable of
the flows and to the encoding) on the GPU in the same run: the second yardstick.
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
from nsynth_wavenet_amd.engine import Engine  # noqa: E402

EXP_M9, EXP_7 = 1.2340980408667956e-4, 1096.6331584284585


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


def torch_student(noise, enc, w, hp):
    """float32 torch composition of ParallelWavenet.feed_forward on channel-major tensors (one conv call per masked.conv1d);
    enc [B,Cd,TE] is the shared stack's"""
    def conv(h, scope, dilation=1):
        W = w[scope + '/W']
        K = W.shape[1]
        if K > 1:
            h = Fn.pad(h, ((K - 1) * dilation, 0))
        return Fn.conv1d(h, W[0].permute(2, 1, 0), w[scope + '/biases'], dilation=dilation)
    T = noise.shape[1]
    left = (enc.shape[2] - T) // 2
    ec = enc[:, :, left:left + T]
    x = noise[:, None, :]
    mean_tot, scale_tot = torch.zeros_like(x), torch.ones_like(x)
    for k, L in enumerate(hp.num_iaf_layers):
        p = 'iaf_%d/' % (k + 1)
        l = conv(Fn.pad(x, (1, 0))[:, :, :-1], p + 'start_conv')
        for i in range(L):
            d = conv(l, p + 'dilated_conv_%d' % (i + 1), 2 ** (i % hp.num_stages)) + conv(ec, p + 'mel_cond_%d' % (i + 1))
            m = d.shape[1] // 2
            l = l + conv(torch.sigmoid(d[:, :m]) * torch.tanh(d[:, m:]), p + 'res_%d' % (i + 1))
        h1 = torch.relu(conv(torch.relu(l), p + 'out1') + conv(ec, p + 'mel_cond_out1'))
        mean = conv(h1, p + 'out2_mean')
        scale = torch.clamp(Fn.softplus(conv(h1, p + 'out2_scale')), EXP_M9, EXP_7)
        x = x * scale + mean
        mean_tot = mean + mean_tot * scale
        scale_tot = scale_tot * scale
    scale_tot = torch.clamp(scale_tot, max=EXP_7)[:, 0]
    mean_tot = mean_tot[:, 0]
    return noise * scale_tot + mean_tot, mean_tot, scale_tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--shapes', default='1x76800,8x7680')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    with open(os.path.join(ROOT, 'config_jsons', 'parallel_wavenet.json')) as f:
        cfgd = json.load(f)
    eng = Engine(cfgd, kind='student')
    w = wts.synthetic_weights(eng.hp, 'student', seed=1, init='tf')
    eng.load_weights(w)
    lib, h = eng.lib, eng._h
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    res = {'metric': 'student_grad_ms', 'config': 'parallel_wavenet.json', 'steps': a.steps, 'shapes': {}}
    for shp in a.shapes.split(','):
        B, T = [int(v) for v in shp.split('x')]
        F = -(-T // eng.frame_shift)
        if eng.iaf_length(F) != T:
            raise SystemExit('{}: {} samples are not the length of {} frames ({})'.format(shp, T, F, eng.iaf_length(F)))
        gen = torch.Generator(device='cuda').manual_seed(1)
        mel = torch.rand(B, F, 80, device='cuda', generator=gen)
        u = torch.rand(B, T, device='cuda', generator=gen) * (1 - 2e-5) + 1e-5
        noise = torch.log(u) - torch.log1p(-u)
        cot = [torch.randn(B, T, device='cuda', generator=gen) for _ in range(3)]
        st = eng._stream()
        n_gws = int(lib.wn_workspace_bytes(h, B, F))
        n_tape = int(lib.wn_iaf_train_tape_bytes(h, B, F, T))
        n_ws = int(lib.wn_iaf_train_workspace_bytes(h, B, F, T))
        n_bws = int(lib.wn_iaf_backward_weights_workspace_bytes(h, B, F, T))
        n_g = int(lib.wn_iaf_grad_floats(h))
        gws = eng._workspace(n_gws)
        tape = torch.empty(n_tape, dtype=torch.uint8, device='cuda')
        ws = torch.empty(n_ws, dtype=torch.uint8, device='cuda')
        bws = torch.empty(n_bws, dtype=torch.uint8, device='cuda')
        flat = torch.empty(n_g, device='cuda')
        out = [torch.empty(B, T, device='cuda') for _ in range(4)]
        denc = torch.empty(eng.iaf_n_stacks(), B, F * eng.frame_shift, cfgd['deconv_width'], device='cuda')
        r = {'B': B, 'T': T, 'train_tape_bytes': n_tape, 'train_tape_bytes_per_sample': n_tape / (B * T),
             'generate_ws_bytes': n_gws, 'forward_ws_bytes': n_ws, 'backward_weights_ws_bytes': n_bws, 'grad_floats': n_g}

        def generate():
            eng._check(lib.wn_iaf_generate(h, p(mel), B, F, p(noise), ctypes.c_uint64(0), p(out[3]), None, p(out[0]), p(out[1]),
                                           p(out[2]), None, p(gws), gws.numel(), st))

        def fwd_train():
            eng._check(lib.wn_iaf_forward_train_tape(h, p(noise), p(mel), B, F, T, p(out[0]), p(out[1]), p(out[2]), p(tape), n_tape,
                                                     p(ws), n_ws, st))

        def bwd(d):
            eng._check(lib.wn_iaf_backward_weights(h, p(tape), n_tape, p(cot[0]), p(cot[1]), p(cot[2]), B, F, T, p(flat), n_g, p(d),
                                                   p(bws), n_bws, st))
        r['iaf_generate_ms'] = timed(generate, a.steps)
        r['forward_train_tape_ms'] = timed(fwd_train, a.steps)
        r['backward_weights_ms'] = timed(lambda: bwd(None), a.steps)
        r['backward_weights_denc_ms'] = timed(lambda: bwd(denc), a.steps)
        r['train_forward_over_generate'] = r['forward_train_tape_ms'] / r['iaf_generate_ms']
        r['backward_weights_denc_over_generate'] = r['backward_weights_denc_ms'] / r['iaf_generate_ms']
        del tape, ws, bws
        torch.cuda.empty_cache()
        if not a.no_torch:
            tw = {k: torch.as_tensor(v, device='cuda').requires_grad_('trans_conv' not in k) for k, v in w.items()}

            def tstep():
                for v in tw.values():
                    v.grad = None
                enc.grad = None
                x, m, s = torch_student(noise, enc, tw, eng.hp)
                ((x * cot[0]).sum() + (m * cot[1]).sum() + (s * cot[2]).sum()).backward()
            try:
                enc = eng.deconv(mel, 'iaf_share').transpose(1, 2).contiguous().requires_grad_(True)      # [B,Cd,TE]
                r['torch_f32_fwd_bwd_ms'] = timed(tstep, max(1, a.steps // 2))
                r['torch_over_train_forward_plus_backward_weights_denc'] = r['torch_f32_fwd_bwd_ms'] / (
                    r['forward_train_tape_ms'] + r['backward_weights_denc_ms'])
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
    sys.stderr.write('bench_student_grad: {:.1f} s\n'.format(time.time() - t0))
