"""Student training-step benchmark: one JSON line.

    python scripts/bench_student_train_step.py [--steps 5] [--rounds 5] [--shapes 1x76800,8x7680]

On parallel_wavenet.json under a wavenet_mol.json teacher, both with synthetic weights, at 1 x 76 800 and 8 x 7 680 samples,
in one run on one build, milliseconds of
  * wn_iaf_backward_weights with d_encoding: the yardstick;
  * train.StudentTrainer.step, and its three parts: the gradient calls (ParallelWavenet.loss_and_weight_grads with the
    upsampler: tape forward, the losses and their backward through the frozen teacher, the student's reverse pass, the
    stack's), the optimiser kernels (wn_grad_sumsq and wn_adam_ema_step on every buffer) and wn_iaf_set_weights (its
    stream synchronisation included), with the number of kernels one wn_iaf_set_weights launches (counted by the profiler
    in a call outside the timed windows; null where the profiler gives no kernel events);
  * the update (optimiser kernels + wn_iaf_set_weights) as one candidate: it should stay below the yardstick;
  * the host route for one step: gradients to the host, a numpy update, ParallelWavenet(hparams).load_weights(new).
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_teacher_train_step import measure  # noqa: E402
from nsynth_wavenet_amd import weights as wts  # noqa: E402
from nsynth_wavenet_amd.train import StudentTrainer  # noqa: E402
from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet  # noqa: E402
from nsynth_wavenet_amd.wavenet.wavenet import Wavenet  # noqa: E402

LOSS_HPARAMS = {'num_samples': 100, 'power_loss_factor': 1.0, 'contrastive_loss_factor': 0.3}


def count_kernels(fn):
    """device kernels one call of fn launches, by the profiler; None where it reports none"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')]
        names = [n for n in names if 'memcpy' not in n.lower() and 'memset' not in n.lower()]
        return len(names) or None
    except Exception as e:                       # reported, not hidden
        sys.stderr.write('count_kernels: {}\n'.format(str(e).split('\n')[0][:200]))
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--shapes', default='1x76800,8x7680')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    with open(os.path.join(ROOT, 'config_jsons', 'parallel_wavenet.json')) as f:
        cfgd = dict(json.load(f), **LOSS_HPARAMS)
    with open(os.path.join(ROOT, 'config_jsons', 'wavenet_mol.json')) as f:
        te_cfg = json.load(f)
    te = Wavenet(te_cfg)
    te.load_weights(wts.synthetic_weights(te.engine.hp, 'teacher', seed=1, init='unit'))
    pw = ParallelWavenet(cfgd, teacher=te)
    eng = pw.engine
    w = wts.synthetic_weights(eng.hp, 'student', seed=1, init='tf')
    pw.load_weights(w)
    lr = 1e-9                      # the timing does not depend on it; the weights stay where the forward is well behaved
    tr = StudentTrainer(pw, w, lr=lr, clip_norm=1.0)
    lib, h = eng.lib, eng._h
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    res = {'metric': 'student_train_step_ms', 'config': 'parallel_wavenet.json', 'teacher': 'wavenet_mol.json', 'steps': a.steps,
           'rounds': a.rounds, 'param_floats': [int(b.numel()) for b in tr.p], 'shapes': {}}
    host = {'net': ParallelWavenet(cfgd, teacher=te).load_weights(w), 'w': dict(w)}
    for shp in a.shapes.split(','):
        B, T = [int(v) for v in shp.split('x')]
        F = -(-T // eng.frame_shift)
        if eng.iaf_length(F) != T:
            raise SystemExit('{}: {} samples are not the length of {} frames ({})'.format(shp, T, F, eng.iaf_length(F)))
        gen = torch.Generator(device='cuda').manual_seed(1)
        mel = torch.rand(B, F, 80, device='cuda', generator=gen)
        inputs = {'mel': mel, 'mel_rand': torch.rand(B, F, 80, device='cuda', generator=gen),
                  'wav': torch.rand(B, T, device='cuda', generator=gen) * 1.8 - 0.9}
        u = torch.rand(B, T, device='cuda', generator=gen) * (1 - 2e-5) + 1e-5
        noise = torch.log(u) - torch.log1p(-u)
        cot = [torch.randn(B, T, device='cuda', generator=gen) / (B * T) for _ in range(3)]
        st = eng._stream()
        n_tape = int(lib.wn_iaf_train_tape_bytes(h, B, F, T))
        n_ws = int(lib.wn_iaf_train_workspace_bytes(h, B, F, T))
        n_bws = int(lib.wn_iaf_backward_weights_workspace_bytes(h, B, F, T))
        n_g = int(lib.wn_iaf_grad_floats(h))
        tape = torch.empty(n_tape, dtype=torch.uint8, device='cuda')
        ws = torch.empty(n_ws, dtype=torch.uint8, device='cuda')
        bws = torch.empty(n_bws, dtype=torch.uint8, device='cuda')
        flat = torch.empty(n_g, device='cuda')
        out = [torch.empty(B, T, device='cuda') for _ in range(3)]
        denc = torch.empty(eng.iaf_n_stacks(), B, F * eng.frame_shift, cfgd['deconv_width'], device='cuda')
        state = {'tape_ok': False}

        def grads():
            return pw.loss_and_weight_grads(inputs, seed=1, noise=noise, upsampler=True)
        o = grads()
        flats = [o['flat_grads'].clone()] + [o['flat_upsampler_grads'][s].clone() for s in tr.scopes]
        del o

        def student_bwd():
            if not state['tape_ok']:          # a re-pack since the tape was written: the handle refuses it, write it again
                eng._check(lib.wn_iaf_forward_train_tape(h, p(noise), p(mel), B, F, T, p(out[0]), p(out[1]), p(out[2]), p(tape),
                                                         n_tape, p(ws), n_ws, st))
                state['tape_ok'] = True
            eng._check(lib.wn_iaf_backward_weights(h, p(tape), n_tape, p(cot[0]), p(cot[1]), p(cot[2]), B, F, T, p(flat), n_g,
                                                   p(denc), p(bws), n_bws, st))

        def optimiser():
            tr._update(flats)

        def set_weights():
            tr._repack(tr.p)
            state['tape_ok'] = False

        def update():
            optimiser()
            set_weights()

        def step():
            tr.step(inputs, noise=noise)
            state['tape_ok'] = False

        def host_route():
            g = host['net'].loss_and_weight_grads(inputs, seed=1, noise=noise, upsampler=True)['grads']
            new = {k: host['w'][k] - lr * g[k].cpu().numpy().reshape(host['w'][k].shape) for k in host['w']}
            nxt = ParallelWavenet(cfgd, teacher=te).load_weights(new)
            host['net'].engine.close()
            host['net'], host['w'] = nxt, new

        r = {'B': B, 'T': T, 'F': F}
        # the reverse pass needs a tape of the weights in force, so it is measured before the candidates that re-pack
        student_bwd()
        r.update(measure({'iaf_backward_weights_denc': (student_bwd, a.steps, 2)}, a.rounds))
        r.update(measure({'gradient_calls': (grads, a.steps, 2),
                          'optimiser_kernels': (optimiser, a.steps, 2),
                          'iaf_set_weights': (set_weights, a.steps, 2),
                          'update': (update, a.steps, 2),
                          'trainer_step': (step, a.steps, 2),
                          'host_route_step': (host_route, 1, 1)}, a.rounds))
        r['iaf_set_weights']['kernel_launches'] = count_kernels(set_weights)
        r['update_over_iaf_backward_weights_denc'] = round(r['update']['ms'] / r['iaf_backward_weights_denc']['ms'], 4)
        hr, ts = r['host_route_step'], r['trainer_step']
        r['host_route_over_trainer_step'] = {'ratio': round(hr['ms'] / ts['ms'], 2), 'min': round(hr['min_ms'] / ts['max_ms'], 2),
                                             'max': round(hr['max_ms'] / ts['min_ms'], 2)}
        res['shapes'][shp] = r
        del ws, tape, bws
        torch.cuda.empty_cache()
    host['net'].engine.close()
    eng.close()
    te.engine.close()
    print(json.dumps(res))


if __name__ == '__main__':
    t0 = time.time()
    main()
    sys.stderr.write('bench_student_train_step: {:.1f} s\n'.format(time.time() - t0))
