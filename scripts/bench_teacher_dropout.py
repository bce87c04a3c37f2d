"""What dropout costs a teacher training step: one JSON line.

    python scripts/bench_teacher_dropout.py [--parent-tree DIR] [--steps 8] [--rounds 5] [--passes 2] [--shapes 1x76800,8x7680]

Milliseconds per train.TeacherTrainer.step on wavenet_mol.json with synthetic weights, at 1 x 76 800 and 8 x 7 680 samples, for
  parent          the step of another build of the package -- DIR holds a checkout of the parent commit with its library built
                  (python -m nsynth_wavenet_amd.build there); left out without --parent-tree;
  off             this tree, dropout off: the same launches as the parent's;
  dropout_inputs  this tree, TeacherTrainer(dropout=True) on the shipped config (rate 0.5);
  dropout_all     the same with the config's key swapped for dropout_all (rate 0.05).
Every candidate runs in a process of its own (two builds of the package cannot share one), warmed up at each shape and timed
in `rounds` windows of `steps` steps between device events; the candidates alternate over `passes` passes, so that drift of
the machine shows up as spread between the passes of one candidate and not as a difference between candidates.  Reported per
candidate and shape: the median window, the smallest and the largest over all passes.  The callers' time limits apply to the
children too: each runs under --child-timeout seconds and a failed child ends the run.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    sys.path.insert(0, a.tree)
    import torch
    from nsynth_wavenet_amd import weights as wts
    from nsynth_wavenet_amd.train import TeacherTrainer
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    torch.cuda.set_device(0)
    with open(os.path.join(ROOT, 'config_jsons', 'wavenet_mol.json')) as f:
        cfgd = json.load(f)
    kw = {}
    if a.child in ('dropout_inputs', 'dropout_all'):
        cfgd.pop('dropout_inputs', None)
        cfgd[a.child] = True
        kw = {'dropout': True, 'dropout_seed': 1}
    net = Wavenet(cfgd)
    w = wts.synthetic_weights(net.engine.hp, 'teacher', seed=1, init='unit')
    net.load_weights(w)
    tr = TeacherTrainer(net, w, lr=1e-9, clip_norm=1.0, **kw)     # the timing does not depend on the rate
    out = {}
    for shp in a.shapes.split(','):
        B, T = [int(v) for v in shp.split('x')]
        F = -(-T // net.engine.frame_shift)
        gen = torch.Generator(device='cuda').manual_seed(1)
        inputs = {'wav': torch.rand(B, T, device='cuda', generator=gen) * 1.8 - 0.9,
                  'mel': torch.rand(B, F, 80, device='cuda', generator=gen)}
        for _ in range(2):
            tr.step(inputs)
        torch.cuda.synchronize()
        wins = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                tr.step(inputs)
            e1.record()
            e1.synchronize()
            wins.append(e0.elapsed_time(e1) / a.steps)
        out[shp] = wins
        del inputs
        torch.cuda.empty_cache()
    net.engine.close()
    print('RESULT ' + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--passes', type=int, default=2)
    ap.add_argument('--shapes', default='1x76800,8x7680')
    ap.add_argument('--child-timeout', type=int, default=180)
    ap.add_argument('--child', default=None)
    ap.add_argument('--tree', default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cands = ([('parent', os.path.abspath(a.parent_tree))] if a.parent_tree else []) + \
        [('off', ROOT), ('dropout_inputs', ROOT), ('dropout_all', ROOT)]
    wins = {name: {} for name, _ in cands}
    for _ in range(a.passes):
        for name, tree in cands:
            cmd = [sys.executable, os.path.abspath(__file__), '--child', name, '--tree', tree, '--steps', str(a.steps),
                   '--rounds', str(a.rounds), '--shapes', a.shapes]
            env = dict(os.environ)
            env.pop('WN_LIB_PATH', None)                  # every tree loads its own library
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout, env=env)
            line = [l for l in p.stdout.splitlines() if l.startswith('RESULT ')]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit('bench_teacher_dropout: the {} child failed ({})'.format(name, p.returncode))
            for shp, v in json.loads(line[-1][7:]).items():
                wins[name].setdefault(shp, []).extend(v)
    res = {'metric': 'teacher_train_step_dropout_ms', 'config': 'wavenet_mol.json', 'steps': a.steps, 'rounds': a.rounds,
           'passes': a.passes, 'shapes': {}}
    for shp in a.shapes.split(','):
        r = {}
        for name, _ in cands:
            v = sorted(wins[name][shp])
            r[name] = {'ms': round(v[len(v) // 2], 3), 'min_ms': round(v[0], 3), 'max_ms': round(v[-1], 3)}
        base = r['off']['ms']
        for name in ('dropout_inputs', 'dropout_all'):
            r[name]['over_off_percent'] = round(100.0 * (r[name]['ms'] / base - 1.0), 2)
        res['shapes'][shp] = r
    print(json.dumps(res))


if __name__ == '__main__':
    main()
