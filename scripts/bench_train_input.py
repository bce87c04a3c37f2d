"""Training-input benchmark: one JSON line.

    python scripts/bench_train_input.py [--steps 8] [--rounds 7] [--batches 4,8] [--pool_seconds 600]

At wave_length 7680 (39 frames) on wavenet_mol.json with synthetic weights and a pool of noise utterances of 1 to 4 s, for
B = 4 and 8, in one run on one build, milliseconds of
  * device_batch: train.DeviceDataset.batch (one launch of wn_train_batch; no mel_rand), and with mel_rand;
  * host_batch_upload: DeviceDataset.host_batch (numpy picks and slices, the float64 host featuriser) plus the upload of
    wav and mel;
  * step_premade: train.TeacherTrainer.step on tensors already on the device -- the step as it was before the dataset
    existed;
  * step_device_batch: the same step fed by ds.batch(k, B), k advancing;
  * step_host_batch: the same step fed by host_batch(k, B) and the upload.
Every candidate is warmed up at the shape, then timed in `rounds` windows of `steps` calls between device events (the events
also span the host's share of a window), the candidates alternating inside a round; the median over the rounds is reported
with the smallest and largest window.  step_device_minus_premade is the difference of the two medians, with the spread of the
per-round differences (the two windows of a round are neighbours in time).  host_syncs_in_device_batch is 0 when ds.batch
runs under torch.cuda.set_sync_debug_mode('error'), which raises on a synchronising torch call (the allocations and views
around the C call; wn_train_batch itself enqueues one kernel and returns), else the message.
Every GPU step of a caller should run under its own time limit (`timeout -k 10 ...`).
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

from nsynth_wavenet_amd import weights as wts  # noqa: E402
from nsynth_wavenet_amd.train import DeviceDataset, TeacherTrainer  # noqa: E402
from nsynth_wavenet_amd.wavenet.wavenet import Wavenet  # noqa: E402

WAVE_LENGTH = 7680


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def measure(cands, rounds):
    """cands: {name: (fn, calls per window, warm-up calls)} -> ({name: {'ms': median, 'min_ms', 'max_ms'}}, the windows)"""
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
        s = sorted(v)
        out[k] = {'ms': round(s[len(s) // 2], 4), 'min_ms': round(s[0], 4), 'max_ms': round(s[-1], 4)}
    return out, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--batches', default='4,8')
    ap.add_argument('--pool_seconds', type=float, default=600.0)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    with open(os.path.join(ROOT, 'config_jsons', 'wavenet_mol.json')) as f:
        cfgd = json.load(f)
    net = Wavenet(cfgd)
    w = wts.synthetic_weights(net.engine.hp, 'teacher', seed=1, init='unit')
    net.load_weights(w)
    tr = TeacherTrainer(net, w, lr=1e-9, clip_norm=1.0)       # the timing does not depend on the rate; the weights stay put
    rs = np.random.RandomState(0)
    utts, total = [], 0
    while total < a.pool_seconds * 16000:
        n = int(rs.randint(16000, 64001))
        utts.append(rs.uniform(-0.5, 0.5, n).astype(np.float32))
        total += n
    ds = DeviceDataset(utts, WAVE_LENGTH, seed=0)
    res = {'metric': 'train_input_ms', 'config': 'wavenet_mol.json', 'wave_length': WAVE_LENGTH, 'frames': ds.frames,
           'pool_utterances': len(utts), 'pool_samples': total, 'steps': a.steps, 'rounds': a.rounds, 'batches': {}}
    for B in [int(v) for v in a.batches.split(',')]:
        k = {'dev': 0, 'host': 0}

        def device_batch(mel_rand=False):
            k['dev'] += 1
            return ds.batch(k['dev'], B, mel_rand=mel_rand)

        def host_batch_upload():
            k['host'] += 1
            h = ds.host_batch(k['host'], B)
            return {'wav': torch.from_numpy(h['wav']).cuda(), 'mel': torch.from_numpy(h['mel']).cuda()}

        premade = {key: v.clone() for key, v in ds.batch(0, B).items()}
        # the device route must not make the host wait: torch raises on a synchronising call in this mode
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            device_batch()
            device_batch(True)
            syncs = 0
        except RuntimeError as e:
            syncs = str(e)
        finally:
            torch.cuda.set_sync_debug_mode('default')
        r = {'B': B, 'host_syncs_in_device_batch': syncs}
        m, _ = measure({'device_batch': (device_batch, 4 * a.steps, 4),
                        'device_batch_mel_rand': (lambda: device_batch(True), 4 * a.steps, 4),
                        'host_batch_upload': (host_batch_upload, 2, 1)}, a.rounds)
        r.update(m)
        m, got = measure({'step_premade': (lambda: tr.step(premade), a.steps, 2),
                          'step_device_batch': (lambda: tr.step(device_batch()), a.steps, 2),
                          'step_host_batch': (lambda: tr.step(host_batch_upload()), 2, 1)}, a.rounds)
        r.update(m)
        diffs = sorted(d - p for d, p in zip(got['step_device_batch'], got['step_premade']))
        r['step_device_minus_premade'] = {'ms': round(m['step_device_batch']['ms'] - m['step_premade']['ms'], 4),
                                          'round_min_ms': round(diffs[0], 4), 'round_median_ms': round(diffs[len(diffs) // 2], 4),
                                          'round_max_ms': round(diffs[-1], 4)}
        res['batches'][str(B)] = r
    net.engine.close()
    print(json.dumps(res))


if __name__ == '__main__':
    t0 = time.time()
    main()
    sys.stderr.write('bench_train_input: {:.1f} s\n'.format(time.time() - t0))
