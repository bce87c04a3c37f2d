"""Sharded / data-parallel teacher training-step benchmark: one JSON line.

    python scripts/bench_train_dp.py [--steps 4] [--rounds 3] [--worlds 2,4,8]

On wavenet_mol.json with synthetic weights, B = 8 rows of 7 680 samples, milliseconds per train.TeacherTrainer.step of
  * one process, one shard: the unsharded step, measured in the same run;
  * one process, micro_batch = 1: eight shards in sequence -- the price of sharding alone -- with the combine timed on its
    own between device events;
  * W ranks (each of --worlds that the machine has GPUs for), micro_batch = 1: the step, and the row exchange (the
    all-gather of 8 rows) and the combine on their own, as rank 0 sees them.
The two one-process candidates alternate inside a round; every candidate is warmed up first, and the median over the rounds
is reported with the smallest and largest window.  Without a rendezvous in the environment the script launches its own
ranks under torch.distributed.run, each launch in its own session and under its own time limit; a caller should still run
the script under a limit of its own.
"""
import argparse
import json
import os
import signal
import socket
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nsynth_wavenet_amd import dist as wdist  # noqa: E402
from nsynth_wavenet_amd import weights as wts  # noqa: E402
from nsynth_wavenet_amd.train import TeacherTrainer  # noqa: E402
from nsynth_wavenet_amd.wavenet.wavenet import Wavenet  # noqa: E402

B, T = 8, 7680
RANKS_TIMEOUT = 420


def stats(v):
    v = sorted(v)
    return {'ms': round(v[len(v) // 2], 4), 'min_ms': round(v[0], 4), 'max_ms': round(v[-1], 4)}


def setup(data_parallel):
    with open(os.path.join(ROOT, 'config_jsons', 'wavenet_mol.json')) as f:
        cfgd = json.load(f)
    net = Wavenet(cfgd)
    w = wts.synthetic_weights(net.engine.hp, 'teacher', seed=1, init='unit')
    net.load_weights(w)
    tr = TeacherTrainer(net, w, lr=1e-9, clip_norm=1.0, data_parallel=data_parallel)     # the timing does not depend on lr
    gen = torch.Generator(device='cuda').manual_seed(1)
    F = -(-T // net.engine.frame_shift)
    inputs = {'wav': torch.rand(B, T, device='cuda', generator=gen) * 1.8 - 0.9, 'mel': torch.rand(B, F, 80, device='cuda', generator=gen)}
    return tr, inputs


def window(tr, inputs, micro, steps, parts):
    """ms per step over `steps` steps between device events; with `parts` also the exchange and the combine of every step"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    evs = []
    a.record()
    for _ in range(steps):
        tr.step(inputs, micro_batch=micro)
        if parts:
            evs.append(tr.last_events)
    b.record()
    b.synchronize()
    out = {'step': a.elapsed_time(b) / steps}
    if parts:
        out['exchange'] = sum(e[0].elapsed_time(e[1]) for e in evs) / steps
        out['combine'] = sum(e[1].elapsed_time(e[2]) for e in evs) / steps
    return out


def one_process(a):
    torch.cuda.set_device(0)
    tr, inputs = setup(False)
    tr.record_events = True
    cands = {'one_shard': None, 'micro_batch_1': 1}
    for micro in cands.values():
        window(tr, inputs, micro, 2, False)
    got = {k: [] for k in cands}
    for _ in range(a.rounds):
        for k, micro in cands.items():
            got[k].append(window(tr, inputs, micro, a.steps, micro is not None))
    res = {'one_shard': stats([g['step'] for g in got['one_shard']]), 'micro_batch_1': stats([g['step'] for g in got['micro_batch_1']])}
    res['micro_batch_1']['combine'] = stats([g['combine'] for g in got['micro_batch_1']])
    res['row_floats'], res['row_bytes_all_shards'] = tr.row_floats, 4 * tr.row_floats * B
    return res


def rank_main(a):
    rank, world, local = wdist.init_process_group()
    torch.cuda.set_device(local)
    tr, inputs = setup(True)
    tr.record_events = True
    window(tr, inputs, 1, 2, False)
    got = [window(tr, inputs, 1, a.steps, True) for _ in range(a.rounds)]
    if rank == 0:
        print(json.dumps({'world': world, 'step': stats([g['step'] for g in got]), 'exchange': stats([g['exchange'] for g in got]),
                          'combine': stats([g['combine'] for g in got])}), flush=True)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch(world, argv):
    """`world` ranks of this script under torch.distributed.run, in their own session; rank 0's JSON line"""
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world), '--master-addr', '127.0.0.1',
           '--master-port', str(free_port()), os.path.abspath(__file__)] + argv
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')      # dmabuf IPC: what RCCL needs on this driver (bench.py)
    env.setdefault('OMP_NUM_THREADS', '8')
    p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, err = p.communicate(timeout=RANKS_TIMEOUT)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        p.communicate()
        return {'world': world, 'error': 'no result in {} s'.format(RANKS_TIMEOUT)}
    if p.returncode != 0:
        return {'world': world, 'error': 'exit {}: {}'.format(p.returncode, err[-500:])}
    lines = [ln for ln in out.splitlines() if ln.startswith('{')]
    return json.loads(lines[-1]) if lines else {'world': world, 'error': 'no JSON line'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--worlds', default='2,4,8')
    a = ap.parse_args()
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        return rank_main(a)
    res = {'metric': 'teacher_train_step_dp_ms', 'config': 'wavenet_mol.json', 'batch': '{}x{}'.format(B, T), 'steps': a.steps,
           'rounds': a.rounds, 'gpus': torch.cuda.device_count()}
    res.update(one_process(a))
    res['ranks'] = {}
    for world in [int(v) for v in a.worlds.split(',') if v]:
        if world > res['gpus'] or B % world:
            res['ranks'][str(world)] = {'skipped': 'needs {} GPUs, the machine has {}'.format(world, res['gpus'])}
            continue
        r = launch(world, ['--steps', str(a.steps), '--rounds', str(a.rounds)])
        res['ranks'][str(world)] = r
        if 'error' in r:                 # after a failed launch nothing more is started on the GPUs
            break
    print(json.dumps(res))


if __name__ == '__main__':
    main()
