"""Windowed generation benchmark: one JSON line.

    python scripts/bench_iaf_stream.py [--rounds 5] [--calls 3]

parallel_wavenet.json with synthetic weights at B = 1, in one run on one build:
  * Engine.iaf_generate_long of 60 s and of 600 s of audio (default plan: windows of 384 frames, eight rows per call) and the
    one-shot Engine.iaf_generate at 4.8 s and at 8 x 4.8 s, in M samples/s, every candidate warmed up at its shape and then
    timed in `rounds` windows of `calls` calls between device events, the candidates alternating inside a round (median,
    smallest and largest window); outputs are preallocated for the long calls, check_range is off on both sides (no host
    synchronisation inside a window);
  * for each plan the MODEL ratio (kept + recomputed samples) / kept samples beside the MEASURED ratio: time per kept
    sample over the 8 x 4.8 s one-shot's time per sample;
  * a stream (Engine.iaf_stream) fed 30 s of mel in pushes of 10, 50 and 200 frames: host time from push() to its samples on
    the host's side of a stream synchronise, over the pushes that returned samples (median, largest), and audio seconds per
    second of the whole run (x real time).
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

from nsynth_wavenet_amd import config as C  # noqa: E402
from nsynth_wavenet_amd import weights as wts  # noqa: E402
from nsynth_wavenet_amd.engine import Engine  # noqa: E402

RATE = 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    with open(os.path.join(ROOT, 'config_jsons', 'parallel_wavenet.json')) as f:
        cfgd = json.load(f)
    eng = Engine(cfgd, device='cuda:0')
    eng.load_weights(wts.synthetic_weights(eng.hp, 'student', seed=1234, init='tf'))
    fs = eng.frame_shift
    rs = np.random.RandomState(0)

    def mel(B, F):
        return torch.as_tensor(rs.uniform(0, 1, [B, F, 80]).astype(np.float32)).to(eng.device)

    cands, plans = {}, {}
    for name, B, F in (('one_shot_4.8s', 1, 384), ('one_shot_8x4.8s', 8, 384)):
        m = mel(B, F)
        cands[name] = (B * eng.iaf_length(F), lambda m=m: eng.iaf_generate(m, seed=1, check_range=False))
    for name, secs in (('long_60s', 60), ('long_600s', 600)):
        F = secs * RATE // fs
        m = mel(1, F)
        out = eng._window_outputs(1, eng.iaf_length(F), ('wav',))
        Fw, plan = C.iaf_plan_windows(eng.hp, F)
        plans[name] = {'frames': F, 'window_frames': Fw, 'rows': len(plan),
                       'model_ratio': len(plan) * eng.iaf_length(Fw) / float(eng.iaf_length(F))}
        cands[name] = (eng.iaf_length(F), lambda m=m, out=out: eng.iaf_generate_long(m, seed=1, check_range=False, out=out))
    for n, fn in cands.values():                                   # warm-up at every shape
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cands}
    for _ in range(a.rounds):
        for k, (n, fn) in cands.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _c in range(a.calls):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.calls)
    eng.check_range()
    res = {'metric': 'iaf_windowed_generation', 'config': 'parallel_wavenet.json', 'batch': 1, 'rounds': a.rounds,
           'calls_per_window': a.calls, 'candidates': {}}
    for k, (n, fn) in cands.items():
        med = statistics.median(ms[k])
        res['candidates'][k] = {'samples': n, 'ms': med, 'ms_min': min(ms[k]), 'ms_max': max(ms[k]),
                                'msamples_per_s': n / med / 1e3}
    base = res['candidates']['one_shot_8x4.8s']
    for k, p in plans.items():
        c = res['candidates'][k]
        p['measured_ratio'] = (c['ms'] / c['samples']) / (base['ms'] / base['samples'])
        c['plan'] = p

    # the stream: 30 s of mel in pushes of n frames
    F = 30 * RATE // fs
    m = mel(1, F)
    res['stream'] = {'frames': F, 'window_frames': C.iaf_window_grid(eng.hp, C.iaf_default_window_frames(eng.hp), 0)[0]}
    for n in (10, 50, 200):
        for timed in (False, True):                                # one untimed pass warms the shapes up
            st = eng.iaf_stream(batch=1, seed=1)
            lat, got = [], 0
            torch.cuda.synchronize()
            t_all = time.perf_counter()
            for at in range(0, F, n):
                t0 = time.perf_counter()
                o = st.push(m[:, at:at + n])['wav']
                torch.cuda.current_stream().synchronize()
                if o.shape[1]:
                    lat.append((time.perf_counter() - t0) * 1e3)
                got += int(o.shape[1])
            got += int(st.finish()['wav'].shape[1])
            torch.cuda.synchronize()
            t_all = time.perf_counter() - t_all
        res['stream']['push_{}'.format(n)] = {'pushes_with_samples': len(lat), 'push_to_samples_ms_median': statistics.median(lat),
                                              'push_to_samples_ms_max': max(lat), 'samples': got,
                                              'x_real_time': got / float(RATE) / t_all}
    eng.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
