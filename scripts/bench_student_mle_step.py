"""Maximum-likelihood training-step benchmark: one JSON line.

    python scripts/bench_student_mle_step.py [--steps 3] [--rounds 3] [--shapes 1x76800,8x7680] [--trace 12]

On parallel_wavenet.json with synthetic weights (init='tf'), at 1 x 76 800 and 8 x 7 680 samples, in one run on one build,
milliseconds of
  * train.StudentMleTrainer.step on a student WITHOUT a teacher, and its parts on the same batch: the encode
    (Engine.iaf_encode, tol 1e-5, with the log-likelihood), the tape forward at z, the cotangents and the adjoint solve
    (Engine.iaf_adjoint at its default tolerance), and the weights (Engine.iaf_backward_weights with d_encoding plus the
    stack's Engine.deconv_backward);
  * train.StudentTrainer.step of the same student under a wavenet_mol.json teacher, beside it;
with the sweeps the encode and the adjoint took, and the adjoint's relative update max |lam' - lam| / max |lam'| (the
largest over the rows) of each of the first `--trace` sweeps from zero -- the figures DESIGN.md 27.3 takes the default
tolerance from.  The audio is the student's own x for a logistic draw, so the inverse exists and the encode converges as it
does on audio the student models; real audio of an untrained student takes more sweeps.  The learning rate is 1e-9: the
weights stay where the forward is well behaved.  Every candidate is warmed up at the shape, then timed in `rounds` windows
between device events, the candidates alternating inside a round; medians with the smallest and largest window.  Nothing is
asserted on time.  Every GPU step of a caller should run under its own time limit (`timeout -k 10 ...`).
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_teacher_train_step import measure  # noqa: E402
from bench_student_train_step import LOSS_HPARAMS  # noqa: E402
from nsynth_wavenet_amd import weights as wts  # noqa: E402
from nsynth_wavenet_amd.train import StudentMleTrainer, StudentTrainer  # noqa: E402
from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet  # noqa: E402
from nsynth_wavenet_amd.wavenet.wavenet import Wavenet  # noqa: E402


def adjoint_trace(eng, tape, g_z, d_s, n):
    """the relative update of each of n sweeps from zero, the largest over the rows"""
    lam, out = None, []
    for _ in range(n):
        r = eng.iaf_adjoint(tape, g_z, d_s, lam_init=lam, max_sweeps=1, tol=0.0, check_every=1)
        lam = r['lam']
        out.append(float((r['resid'][:, 0] / r['resid'][:, 1]).max()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--shapes', default='1x76800,8x7680')
    ap.add_argument('--trace', type=int, default=12)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    with open(os.path.join(ROOT, 'config_jsons', 'parallel_wavenet.json')) as f:
        cfgd = dict(json.load(f), **LOSS_HPARAMS)
    with open(os.path.join(ROOT, 'config_jsons', 'wavenet_mol.json')) as f:
        te_cfg = json.load(f)
    te = Wavenet(te_cfg)
    te.load_weights(wts.synthetic_weights(te.engine.hp, 'teacher', seed=1, init='unit'))
    pd = ParallelWavenet(cfgd, teacher=te)
    w = wts.synthetic_weights(pd.engine.hp, 'student', seed=1, init='tf')
    pd.load_weights(w)
    pm = ParallelWavenet(cfgd).load_weights(w)
    eng = pm.engine
    lr = 1e-9
    distill = StudentTrainer(pd, w, lr=lr, clip_norm=1.0)
    mle = StudentMleTrainer(pm, w, lr=lr, clip_norm=1.0)
    res = {'metric': 'student_mle_step_ms', 'config': 'parallel_wavenet.json', 'teacher': 'wavenet_mol.json', 'steps': a.steps,
           'rounds': a.rounds, 'encode_tol': mle.encode_tol, 'adjoint_tol': eng.ADJOINT_TOL, 'shapes': {}}
    for shp in a.shapes.split(','):
        B, T = [int(v) for v in shp.split('x')]
        F = -(-T // eng.frame_shift)
        if eng.iaf_length(F) != T:
            raise SystemExit('{}: {} samples are not the length of {} frames ({})'.format(shp, T, F, eng.iaf_length(F)))
        gen = torch.Generator(device='cuda').manual_seed(1)
        mel = torch.rand(B, F, 80, device='cuda', generator=gen)
        u = torch.rand(B, T, device='cuda', generator=gen) * (1 - 2e-5) + 1e-5
        noise = torch.log(u) - torch.log1p(-u)
        wav = eng.iaf_generate(mel, noise=noise, want=('x',))['x']
        batch = {'mel': mel, 'wav': wav}
        dbatch = dict(batch, mel_rand=torch.rand(B, F, 80, device='cuda', generator=gen))
        state = {}

        def encode():
            state['enc'] = eng.iaf_encode(wav, mel, want=('z', 'log_prob'), tol=mle.encode_tol)

        def tape_forward():
            state['ff'], state['tape'] = eng.iaf_forward_train_tape(mel, noise=state['enc']['z'])

        def adjoint():
            state['cot'] = eng.iaf_latent_log_prob_grad(state['enc']['z'], state['ff']['scale_tot'])
            state['adj'] = eng.iaf_adjoint(state['tape'], *state['cot'])

        def weights():
            lam = state['adj']['lam']
            r = eng.iaf_backward_weights(state['tape'], -lam, torch.zeros_like(lam), state['cot'][1])
            for s, scope in enumerate(eng.iaf_stack_scopes()):
                eng.deconv_backward(mel, r['d_encoding'][s], scope)

        def mle_step():
            state['step'] = mle.step(batch)
            state.pop('tape', None)                # the re-pack has outdated it

        def distill_step():
            distill.step(dbatch, noise=noise)

        encode(); tape_forward(); adjoint()
        r = {'B': B, 'T': T, 'F': F, 'encode_sweeps': state['enc']['sweeps'], 'adjoint_sweeps': state['adj']['sweeps'],
             'adjoint_converged': bool(state['adj']['converged'].all()),
             'adjoint_relative_updates': [float('{:.3e}'.format(v)) for v in adjoint_trace(eng, state['tape'], *state['cot'], a.trace)]}
        # the parts need a tape of the weights in force: they are measured before the candidates that re-pack
        r.update(measure({'encode': (encode, a.steps, 1), 'tape_forward': (tape_forward, a.steps, 1),
                          'adjoint': (adjoint, a.steps, 1), 'weights': (weights, a.steps, 1)}, a.rounds))
        r.update(measure({'mle_trainer_step': (mle_step, a.steps, 1), 'student_trainer_step': (distill_step, a.steps, 1)}, a.rounds))
        r['step_sweeps'] = [state['step']['sweeps'], state['step']['adjoint_sweeps']]
        r['mle_over_student_trainer_step'] = round(r['mle_trainer_step']['ms'] / r['student_trainer_step']['ms'], 3)
        r['adjoint_share_of_mle_step'] = round(r['adjoint']['ms'] / r['mle_trainer_step']['ms'], 3)
        res['shapes'][shp] = r
        state.clear()
        torch.cuda.empty_cache()
    eng.close()
    pd.engine.close()
    te.engine.close()
    print(json.dumps(res))


if __name__ == '__main__':
    t0 = time.time()
    main()
    sys.stderr.write('bench_student_mle_step: {:.1f} s\n'.format(time.time() - t0))
