"""Input-gradient benchmark: one JSON line.

    python scripts/bench_input_grad.py [--steps 10] [--rounds 3] [--shapes 1x76800,8x7680]

On parallel_wavenet.json with synthetic weights, at 1 x 76 800 and 8 x 7 680 samples: milliseconds per call, from device events
on preallocated buffers, of wn_deconv_backward_input (d mel of the shared stack from a cotangent of its encoding), of
wn_iaf_backward_input (d noise and d encoding, no weight products) and, in the same run, of wn_iaf_backward_weights with
d_encoding -- the reverse pass it shares its body with.  Each figure is the median of `rounds` timings of `steps` calls; the
workspace bytes of the three calls go with them.  Nothing is asserted on time.
Every GPU step of a caller should run under its own time limit (`timeout -k 10 ...`).
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nsynth_wavenet_amd import weights as wts  # noqa: E402
from nsynth_wavenet_amd.engine import Engine  # noqa: E402


def timed(fn, steps, rounds):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / steps)
    ms.sort()
    return {'ms': round(ms[len(ms) // 2], 4), 'min_ms': round(ms[0], 4), 'max_ms': round(ms[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--shapes', default='1x76800,8x7680')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    with open(os.path.join(ROOT, 'config_jsons', 'parallel_wavenet.json')) as f:
        cfgd = json.load(f)
    eng = Engine(cfgd, kind='student')
    eng.load_weights(wts.synthetic_weights(eng.hp, 'student', seed=1, init='tf'))
    lib, h = eng.lib, eng._h
    scope = eng.iaf_stack_scopes()[0].encode()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    res = {'metric': 'input_grad_ms', 'config': 'parallel_wavenet.json', 'steps': a.steps, 'rounds': a.rounds, 'shapes': {}}
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
        n_tape = int(lib.wn_iaf_train_tape_bytes(h, B, F, T))
        n_ws = int(lib.wn_iaf_train_workspace_bytes(h, B, F, T))
        n_iws = int(lib.wn_iaf_backward_input_workspace_bytes(h, B, F, T))
        n_bws = int(lib.wn_iaf_backward_weights_workspace_bytes(h, B, F, T))
        n_dws = int(lib.wn_deconv_backward_input_workspace_bytes(h, scope, B, F))
        n_g = int(lib.wn_iaf_grad_floats(h))
        tape = torch.empty(n_tape, dtype=torch.uint8, device='cuda')
        ws = torch.empty(max(n_ws, n_iws, n_bws, n_dws), dtype=torch.uint8, device='cuda')
        flat = torch.empty(n_g, device='cuda')
        out = [torch.empty(B, T, device='cuda') for _ in range(3)]
        dnoise = torch.empty(B, T, device='cuda')
        dmel = torch.empty(B, F, 80, device='cuda')
        denc = torch.empty(eng.iaf_n_stacks(), B, F * eng.frame_shift, cfgd['deconv_width'], device='cuda')
        eng._check(lib.wn_iaf_forward_train_tape(h, p(noise), p(mel), B, F, T, p(out[0]), p(out[1]), p(out[2]), p(tape), n_tape,
                                                 p(ws), n_ws, st))

        def bwd_input():
            eng._check(lib.wn_iaf_backward_input(h, p(tape), n_tape, p(cot[0]), p(cot[1]), p(cot[2]), B, F, T, p(dnoise), p(denc),
                                                 p(ws), n_iws, st))

        def bwd_weights():
            eng._check(lib.wn_iaf_backward_weights(h, p(tape), n_tape, p(cot[0]), p(cot[1]), p(cot[2]), B, F, T, p(flat), n_g,
                                                   p(denc), p(ws), n_bws, st))

        def deconv_input():
            eng._check(lib.wn_deconv_backward_input(h, scope, p(mel), p(denc[0]), B, F, p(dmel), p(ws), n_dws, st))
        r = {'B': B, 'T': T, 'iaf_backward_input_ws_bytes': n_iws, 'iaf_backward_weights_ws_bytes': n_bws,
             'deconv_backward_input_ws_bytes': n_dws}
        r['iaf_backward_weights'] = timed(bwd_weights, a.steps, a.rounds)
        r['iaf_backward_input'] = timed(bwd_input, a.steps, a.rounds)
        r['deconv_backward_input'] = timed(deconv_input, a.steps, a.rounds)
        r['iaf_backward_input_over_weights'] = round(r['iaf_backward_input']['ms'] / r['iaf_backward_weights']['ms'], 4)
        res['shapes'][shp] = r
        del tape, ws
        torch.cuda.empty_cache()
    eng.close()
    print(json.dumps(res))


if __name__ == '__main__':
    t0 = time.time()
    main()
    sys.stderr.write('bench_input_grad: {:.1f} s\n'.format(time.time() - t0))
