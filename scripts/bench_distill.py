"""Distillation-loss benchmark (csrc/wn_distill.hip, ParallelWavenet.calculate_loss): one JSON line.

    python scripts/bench_distill.py [--batches 1,8] [--frames 384] [--samples 100] [--steps 10]

parallel_wavenet.json student with the wavenet_mol.json teacher (synthetic weights), F frames of mel per utterance
(T = 76 800 samples at F = 384), num_samples S.  Per batch size B: ms per call of the student forward, the teacher forward,
each new kernel (MoL cross entropy with device draws, Gauss KL on a [B,T,2] tensor, power loss) and the whole
calculate_loss (two teacher forwards, two cross entropies, the power loss); the MoL kernel's rate as a fraction of the
transcendental issue rate of the SIMDs (one wave instruction per 8 cycles per SIMD, MI355X_MICROARCH.md; the kernel's
transcendental-class instructions per draw counted from its formula: 2 exp + 2 rcp + 1 log per component, M exp + 1 log for
the mixture, 2 log for a drawn logistic); and, beside them, a torch-on-GPU composition of the reference's formulas
(tf_repeat of the teacher parameters, mol_log_probs on the [B*S,T,3M] copy) at the largest S that fits, with its peak
memory.  Every GPU step of a caller should run under its own time limit (`timeout -k 10 ...`), as the rest of the project's
scripts do.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import wavenet_np as O  # noqa: E402
from nsynth_wavenet_amd import config as cfgmod  # noqa: E402
from nsynth_wavenet_amd.engine import power_loss  # noqa: E402
from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet  # noqa: E402
from nsynth_wavenet_amd.wavenet.wavenet import Wavenet  # noqa: E402

CU, SIMD_PER_CU, WAVE = 256, 4, 64
TRANS_CYCLES = 8.0                   # issue cycles of one wave-wide v_exp / v_log / v_rcp
SCLK_GHZ = 2.4                       # peak engine clock the fraction is taken against


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


def torch_composition(out, mean, scale, S, Q=65536.0):
    """the reference's kl_loss_logistic cross entropy as written, in torch on the GPU (float32, like its graph)"""
    B, T, W = out.shape
    M = W // 3
    te = out.repeat_interleave(S, dim=0)                         # utils.tf_repeat(te_mol, [S, 1, 1])
    u = torch.rand(B * S, T, device=out.device) * (1 - 2e-5) + 1e-5
    rl = torch.log(u) - torch.log(1 - u)
    x = rl * scale.repeat_interleave(S, dim=0) + mean.repeat_interleave(S, dim=0)
    lg, mu, ls = te[..., :M], te[..., M:2 * M], torch.clamp(te[..., 2 * M:], min=-7.0)
    inv = torch.exp(-ls)
    c = x[..., None] - mu
    plus, mn = inv * (c + 1 / Q), inv * (c - 1 / Q)
    delta = torch.sigmoid(plus) - torch.sigmoid(mn)
    xe = x[..., None]
    lp = torch.where(xe < 0.5 / (Q / 2) - 1, plus - torch.nn.functional.softplus(plus),
                     torch.where(xe > (Q - 1.5) / (Q / 2) - 1, -torch.nn.functional.softplus(mn),
                                 torch.log(torch.clamp(delta, min=1e-12))))
    lp = lp + torch.log_softmax(lg, dim=-1)
    return -torch.logsumexp(lp, dim=-1).reshape(B, S, T).mean(dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,8')
    ap.add_argument('--frames', type=int, default=384)
    ap.add_argument('--samples', type=int, default=100)
    ap.add_argument('--steps', type=int, default=10)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    st_cfg = dict(load('parallel_wavenet.json'), num_samples=a.samples, power_loss_factor=1.0, contrastive_loss_factor=0.3)
    te_cfg = load('wavenet_mol.json')
    teacher = Wavenet(te_cfg).load_weights(O.synth_weights(O.HP(te_cfg), 'teacher', seed=1234, init='tf'))
    pw = ParallelWavenet(st_cfg, teacher=teacher).load_weights(O.synth_weights(O.HP(st_cfg), 'student', seed=1234, init='tf'))
    gauss_teacher = Wavenet(load('wavenet_gauss.json'))          # the Gauss KL kernel needs only the handle's shape
    M = te_cfg['mol_mix']
    ghz = SCLK_GHZ
    res = {'metric': 'distill_ms', 'S': a.samples, 'F': a.frames, 'sclk_ghz': ghz, 'per_batch': {}}
    for B in [int(b) for b in a.batches.split(',')]:
        rs = np.random.RandomState(B)
        mel = torch.as_tensor(rs.uniform(0, 1, [B, a.frames, 80]).astype(np.float32)).cuda()
        mel_rand = torch.as_tensor(rs.uniform(0, 1, [B, a.frames, 80]).astype(np.float32)).cuda()
        T = cfgmod.iaf_length(pw.hparams, a.frames)
        ff = pw.feed_forward({'mel': mel}, seed=1)
        ff.update(mel=mel, mel_rand=mel_rand,
                  wav=torch.as_tensor(np.clip(0.3 * rs.standard_normal([B, T + 400]), -1, 1).astype(np.float32)).cuda())
        te_eng = teacher.engine
        out = te_eng.teacher_forward(ff['x'], mel)
        g_out = torch.stack([ff['mean_tot'], torch.log(ff['scale_tot'])], dim=-1).contiguous()
        r = {}
        r['student_forward_ms'] = timed(lambda: pw.feed_forward({'mel': mel}, seed=1), a.steps)
        r['teacher_forward_ms'] = timed(lambda: te_eng.teacher_forward(ff['x'], mel), a.steps)
        r['mol_xent_ms'] = timed(lambda: te_eng.distill_mol_xent(out, ff['mean_tot'], ff['scale_tot'], a.samples, seed=2),
                                 a.steps)
        r['gauss_kl_ms'] = timed(lambda: gauss_teacher.engine.distill_gauss_kl(g_out, ff['mean_tot'], ff['scale_tot']),
                                 a.steps)
        r['power_loss_ms'] = timed(lambda: power_loss(ff['x'], ff['wav']), a.steps)
        r['calculate_loss_ms'] = timed(lambda: pw.calculate_loss(ff, seed=3), max(2, a.steps // 2))
        r['calculate_loss_over_forwards'] = r['calculate_loss_ms'] / (r['student_forward_ms'] + r['teacher_forward_ms'])
        trans_per_draw = 5 * M + M + 1 + 2
        peak = CU * SIMD_PER_CU * WAVE / TRANS_CYCLES * ghz * 1e9          # lane-transcendentals per second
        r['mol_trans_per_draw'] = trans_per_draw
        r['mol_frac_trans_issue'] = B * T * a.samples * trans_per_draw / (r['mol_xent_ms'] * 1e-3) / peak
        # the reference's composition at the largest S that fits (halving from S)
        s = a.samples
        while s >= 1:
            try:
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                ms = timed(lambda: torch_composition(out, ff['mean_tot'], ff['scale_tot'], s), 2)
                r['torch_composition'] = {'S': s, 'ms': ms, 'ms_per_draw_scaled_to_S': ms * a.samples / s,
                                          'peak_gb': (torch.cuda.max_memory_allocated() - base) / 1e9}
                break
            except torch.cuda.OutOfMemoryError:
                s //= 2
        torch.cuda.empty_cache()
        res['per_batch'][str(B)] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
    print(json.dumps(res))


if __name__ == '__main__':
    t0 = time.time()
    main()
    sys.stderr.write('bench_distill: {:.1f} s\n'.format(time.time() - t0))
