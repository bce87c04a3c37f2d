"""IAF encode benchmark: one JSON line.

    python scripts/bench_iaf_encode.py [--rounds 5] [--max-sweeps N]

parallel_wavenet.json (4 flows, 60 layers) with synthetic init='tf' weights at 1 x 76 800 and 8 x 7 680 samples; x is the
student's own sample (Engine.iaf_generate under a seed).  Per shape, in one run on one build:
  * sweeps of Engine.iaf_encode from zero until no bit moves (tol = 0) and until no sample moves by more than 1e-6 / 1e-5,
    with check_every = 64 and capped at --max-sweeps (default T, where the inverse is exact; 'converged' says whether the
    stop condition was met first), the wall time of each encode in ms (read-backs included) and its largest |z - noise|
    against the noise x was drawn with;
  * the largest |z - noise| after 4, 8, ... 128 sweeps from zero;
  * ms per sweep after the first: (an encode of 1 + 32 sweeps - an encode of 1 sweep) / 32, each as one C call between device
    events, median of `rounds`;
  * ms of Engine.iaf_generate at the same shape, the same way (check_range off: no host synchronisation inside the window).
Nothing gates on these numbers.  Every GPU step of a caller should run under its own time limit (`timeout -k 10 ...`).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nsynth_wavenet_amd import weights as wts  # noqa: E402
from nsynth_wavenet_amd.engine import Engine  # noqa: E402

EXTRA = 32


def timed(fn, rounds):
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--max-sweeps', type=int, default=0, help='0: T')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    with open(os.path.join(ROOT, 'config_jsons', 'parallel_wavenet.json')) as f:
        cfgd = json.load(f)
    eng = Engine(cfgd, device='cuda:0')
    eng.load_weights(wts.synthetic_weights(eng.hp, 'student', seed=1234, init='tf'))
    rs = np.random.RandomState(0)
    res = {'metric': 'iaf_encode', 'config': 'parallel_wavenet.json', 'init': 'tf', 'rounds': a.rounds,
           'max_sweeps': a.max_sweeps, 'shapes': {}}
    for name, B, F in (('1x76800', 1, 384), ('8x7680', 8, 39)):
        mel = torch.as_tensor(rs.uniform(0, 1, [B, F, 80]).astype(np.float32)).to(eng.device)
        T = eng.iaf_length(F)
        g = eng.iaf_generate(mel, seed=1, want=('x', 'rand_input'))
        x, noise = g['x'], g['rand_input']
        cap = min(a.max_sweeps, T) if a.max_sweeps > 0 else T
        out = {'batch': B, 'samples_per_row': T}
        for key, tol in (('bitwise', 0.0), ('tol_1e-6', 1e-6), ('tol_1e-5', 1e-5)):
            eng.iaf_encode(x, mel, max_sweeps=1)                      # warm-up at the shape
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = eng.iaf_encode(x, mel, tol=tol, max_sweeps=cap, check_every=64)
            torch.cuda.synchronize()
            out[key] = {'sweeps': r['sweeps'], 'converged': bool(r['converged'].all()), 'clamped': r['clamped'],
                        'total_ms': (time.perf_counter() - t0) * 1e3, 'form': r['form'],
                        'max_abs_z_minus_noise': float((r['z'] - noise).abs().max()),
                        'min_front': int(r['front'].min())}
        out['max_abs_z_minus_noise_after'] = {
            str(k): float((eng.iaf_encode(x, mel, max_sweeps=k)['z'] - noise).abs().max()) for k in (4, 8, 16, 32, 64, 128)}
        one = timed(lambda: eng.iaf_encode(x, mel, max_sweeps=1, check_every=1), a.rounds)
        many = timed(lambda: eng.iaf_encode(x, mel, max_sweeps=1 + EXTRA, check_every=1 + EXTRA), a.rounds)
        out['first_sweep_ms'] = one
        out['ms_per_sweep_after_first'] = (many - one) / EXTRA
        eng.iaf_generate(mel, seed=1, check_range=False)
        out['iaf_generate_ms'] = timed(lambda: eng.iaf_generate(mel, seed=1, check_range=False), a.rounds)
        out['range_fallbacks'] = eng.range_fallbacks
        res['shapes'][name] = out
    eng.check_range()
    eng.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
