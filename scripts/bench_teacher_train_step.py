"""Teacher training-step benchmark: one JSON line.

    python scripts/bench_teacher_train_step.py [--steps 8] [--rounds 5] [--shapes 1x76800,8x7680]

On wavenet_mol.json with synthetic weights, at 1 x 76 800 and 8 x 7 680 samples, in one run on one build, milliseconds of
  * train.TeacherTrainer.step, and its three parts: the gradient calls (Wavenet.loss_and_weight_grads with the upsampler),
    the optimiser kernels (wn_grad_sumsq and wn_adam_ema_step on both buffers) and wn_teacher_set_weights (its stream
    synchronisation included);
  * the update (optimiser kernels + wn_teacher_set_weights) as one candidate, beside wn_teacher_backward_weights alone: a
    step should stay gradient-bound, so the update has to be the cheaper of the two;
  * the host route for one step: gradients to the host, a numpy update, Wavenet(hparams).load_weights(new).
Every candidate is warmed up at the shape, then timed in `rounds` windows between device events (the events also span the
host's share of a window), the candidates alternating inside a round; the median over the rounds is reported with the
smallest and largest window.  Every GPU step of a caller should run under its own time limit (`timeout -k 10 ...`).
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
from nsynth_wavenet_amd.train import TeacherTrainer  # noqa: E402
from nsynth_wavenet_amd.wavenet.wavenet import Wavenet  # noqa: E402


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def measure(cands, rounds):
    """cands: {name: (fn, calls per window, warm-up calls)} -> {name: {'ms': median, 'min_ms', 'max_ms'}}"""
    for fn, _, warm in cands.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in cands}
    for _ in range(rounds):
        for k, (fn, steps, _) in cands.items():
            got[k].append(window(fn, steps))
    out = {}
    for k, v in got.items():
        v = sorted(v)
        out[k] = {'ms': round(v[len(v) // 2], 4), 'min_ms': round(v[0], 4), 'max_ms': round(v[-1], 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=8)
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
    lr = 1e-9                      # the timing does not depend on it; the weights stay where the forward is well behaved
    tr = TeacherTrainer(net, w, lr=lr, clip_norm=1.0)
    lib, h = eng.lib, eng._h
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    res = {'metric': 'teacher_train_step_ms', 'config': 'wavenet_mol.json', 'steps': a.steps, 'rounds': a.rounds,
           'param_floats': [int(b.numel()) for b in tr.p], 'shapes': {}}
    host = {'net': Wavenet(cfgd).load_weights(w), 'w': dict(w)}
    for shp in a.shapes.split(','):
        B, T = [int(v) for v in shp.split('x')]
        F = -(-T // eng.frame_shift)
        gen = torch.Generator(device='cuda').manual_seed(1)
        wav = torch.rand(B, T, device='cuda', generator=gen) * 1.8 - 0.9
        mel = torch.rand(B, F, 80, device='cuda', generator=gen)
        inputs = {'wav': wav, 'mel': mel}
        ow = 3 * cfgd['mol_mix']
        st = eng._stream()
        n_ws = int(lib.wn_teacher_workspace_bytes(h, B, F, T))
        n_ttape = int(lib.wn_teacher_train_tape_bytes(h, B, F, T))
        n_wws = int(lib.wn_teacher_backward_weights_workspace_bytes(h, B, F, T))
        n_g = int(lib.wn_teacher_grad_floats(h))
        ws = torch.empty(n_ws, dtype=torch.uint8, device='cuda')
        tape = torch.empty(n_ttape, dtype=torch.uint8, device='cuda')
        bws = torch.empty(n_wws, dtype=torch.uint8, device='cuda')
        flat = torch.empty(n_g, device='cuda')
        out = torch.empty(B, T, ow, device='cuda')
        g = torch.randn(B, T, ow, device='cuda', generator=gen) / (B * T)
        denc = torch.empty(B, F * eng.frame_shift, cfgd['deconv_width'], device='cuda')
        _, flats = tr._grads(inputs)
        flats = [f.clone() for f in flats]
        state = {'tape_ok': False}

        def teacher_bwd():
            if not state['tape_ok']:          # a re-pack since the tape was written: the handle refuses it, write it again
                eng._check(lib.wn_teacher_forward_train_tape(h, p(wav), p(mel), B, F, T, p(out), p(tape), n_ttape, p(ws), n_ws, st))
                state['tape_ok'] = True
            eng._check(lib.wn_teacher_backward_weights(h, p(tape), n_ttape, p(g), B, F, T, p(flat), n_g, p(denc), None, p(bws),
                                                       n_wws, st))

        def optimiser():
            tr._update(flats)

        def set_weights():
            tr._repack(tr.p)
            state['tape_ok'] = False

        def update():
            optimiser()
            set_weights()

        def step():
            tr.step(inputs)
            state['tape_ok'] = False

        def host_route():
            o = host['net'].loss_and_weight_grads(inputs, upsampler=True)
            new = {k: host['w'][k] - lr * o['grads'][k].cpu().numpy() for k in host['w']}
            nxt = Wavenet(cfgd).load_weights(new)
            host['net'].engine.close()
            host['net'], host['w'] = nxt, new

        r = {'B': B, 'T': T, 'F': F}
        # the reverse pass needs a tape of the weights in force, so it is measured before the candidates that re-pack
        teacher_bwd()
        r.update(measure({'teacher_backward_weights': (teacher_bwd, a.steps, 2)}, a.rounds))
        r.update(measure({'gradient_calls': (lambda: tr._grads(inputs), a.steps, 2),
                          'optimiser_kernels': (optimiser, a.steps, 2),
                          'teacher_set_weights': (set_weights, a.steps, 2),
                          'update': (update, a.steps, 2),
                          'trainer_step': (step, a.steps, 2),
                          'host_route_step': (host_route, 1, 1)}, a.rounds))
        r['update_over_teacher_backward_weights'] = round(r['update']['ms'] / r['teacher_backward_weights']['ms'], 4)
        hr, ts = r['host_route_step'], r['trainer_step']
        r['host_route_over_trainer_step'] = {'ratio': round(hr['ms'] / ts['ms'], 2), 'min': round(hr['min_ms'] / ts['max_ms'], 2),
                                             'max': round(hr['max_ms'] / ts['min_ms'], 2)}
        res['shapes'][shp] = r
        del ws, tape, bws
        torch.cuda.empty_cache()
    host['net'].engine.close()
    eng.close()
    print(json.dumps(res))


if __name__ == '__main__':
    t0 = time.time()
    main()
    sys.stderr.write('bench_teacher_train_step: {:.1f} s\n'.format(time.time() - t0))
