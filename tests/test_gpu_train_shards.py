"""GPU tests of the sharded training step (nsynth_wavenet_amd/train.py).  step(batch, micro_batch=m) of the
three trainers has the bits of the loop written out here -- one public gradient call per shard under train.shard_seed, the
numpy twin of the combine on host copies, then the optimiser kernels and the re-pack as they were; the combined gradient
is the full-batch gradient within the project's bar; micro_batch=None and micro_batch=B are the unsharded step; and a
command-line run on two ranks has the bits of the same command line in one process.

Models: TEACHER and STUDENT of tests/test_gpu_train_cli.py (width 64, wave_length 1600 = 9 frames, the student's 1800
samples), the four utterances of its tfrecord, B = 4.  Every child process has its own time limit, runs in its own session,
is run once, and its whole process group is killed if the limit passes."""
import json
import math
import os
import signal
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_train_cli import STUDENT, TEACHER, _continue_from, _logged, _same_tensors, _tensors

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300
SEED, B, WAVE = 0, 4, 1600
LR = {0: 1e-3, 2: 5e-4}
SCALARS = ('loss', 'kl_loss', 'H_Ps', 'H_Ps_Pt', 'power_loss', 'contrastive_loss')


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach().contiguous().view(torch.int64)


def _child(argv, nproc=1, port=None):
    """one child (or one torch.distributed.run of nproc ranks), once, in its own session: its stdout.  A non-zero exit fails
    the test with its stderr; at the time limit the whole process group is killed."""
    cmd = [sys.executable]
    if nproc > 1:
        cmd += ['-m', 'torch.distributed.run', '--nproc-per-node', str(nproc), '--master-addr', '127.0.0.1', '--master-port', str(port)]
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    if nproc > 1:
        env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')      # as bench.py launches its ranks
    p = subprocess.Popen(cmd + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT, env=env, start_new_session=True)
    try:
        out, err = p.communicate(timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        p.communicate()
        pytest.fail('{} did not finish in {} s'.format(' '.join(argv[:1]), CHILD_TIMEOUT))
    finally:
        try:
            os.killpg(p.pid, signal.SIGKILL)          # no rank outlives its launcher
        except ProcessLookupError:
            pass
    assert p.returncode == 0, '{} exited with {}:\n{}'.format(' '.join(argv), p.returncode, err[-4000:])
    return out


@pytest.fixture(scope='module')
def work(tmp_path_factory):
    from nsynth_wavenet_amd.auxilaries import reader
    d = tmp_path_factory.mktemp('train_shards')
    rs = np.random.RandomState(7)
    utts = []
    for i, n in enumerate((1600, 2100, 4000, 1601)):
        t = np.arange(n) / 16000.0
        utts.append(('utt{}'.format(i), (0.3 * np.sin(2 * np.pi * (220.0 * (i + 1)) * t) + 0.05 * rs.standard_normal(n)).astype(np.float32)))
    reader.write_tfrecord(str(d / 'train.tfrecord'), utts)
    for name, cfg in (('teacher.json', TEACHER), ('student.json', STUDENT)):
        (d / name).write_text(json.dumps(cfg))
    return d


@pytest.fixture(scope='module')
def ds(work):
    from nsynth_wavenet_amd import train
    return train.DeviceDataset.from_tfrecord(str(work / 'train.tfrecord'), WAVE, seed=SEED)


@pytest.fixture(scope='module')
def weights():
    """the initial weights of both models: computed once, never written to (the trainers copy them)"""
    from nsynth_wavenet_amd import weights as wts
    from nsynth_wavenet_amd.config import load_hparams
    return {kind: wts.synthetic_weights(load_hparams(cfg), kind, seed=SEED, init='tf')
            for kind, cfg in (('teacher', TEACHER), ('student', STUDENT))}


def _update_by_hand(ref, grads, k):
    """step k (k completed before it) of the optimiser on the reference trainer's buffers, by the kernels as they were:
    grad_sumsq chained, adam_ema_step per buffer with the schedule and the decay of DESIGN.md 16, the re-pack.  Returns the
    global norm."""
    from nsynth_wavenet_amd import engine as E, train
    t = k + 1
    lr_t = float(np.float32(train.scheduled_lr(LR, k) * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)))
    sumsq = torch.zeros(1, dtype=torch.float64, device='cuda')
    for i, g in enumerate(grads):
        E.grad_sumsq(g, sumsq, accumulate=i > 0)
    for p, g, m, v, e in zip(ref.p, grads, ref.m, ref.v, ref.ema):
        E.adam_ema_step(p, g, m, v, e, lr_t, 0.9, 0.999, 1e-8, min(0.9999, (1.0 + k) / (10.0 + k)), sumsq=None, clip_norm=1.0)
    ref._repack(ref.p)
    return sumsq.sqrt()[0]


def _check_against_the_written_out_loop(tr, ref, batches, m, shard_call):
    """tr.step(batch, micro_batch=m) against: per shard j the public call `shard_call(rows, k, j)` -> (dict, flat gradients),
    combine_np over the host copies in shard order, _update_by_hand"""
    from nsynth_wavenet_amd import train
    S = B // m
    for k, batch in enumerate(batches):
        got = tr.step(batch, micro_batch=m)
        per = []
        for j in range(S):
            rows = {key: batch[key][j * m:(j + 1) * m] for key in ('wav', 'mel', 'mel_rand') if key in batch}
            out, flats = shard_call(rows, k, j)
            per.append(([f.cpu().numpy() for f in flats], {key: np.float32(out[key].float().cpu().numpy()) for key in SCALARS if key in out},
                        out.get('log_probs')))
        grads = [torch.from_numpy(train.combine_np([p[0][i] for p in per])).cuda() for i in range(len(ref.p))]
        norm = _update_by_hand(ref, grads, k)
        keys = [key for key in SCALARS if key in per[0][1]]
        assert keys and keys[0] == 'loss' and set(keys) == set(key for key in SCALARS if key in got)
        for key in keys:
            want = train.combine_np([np.asarray(p[1][key]).reshape(1) for p in per])[0]
            print('step', k, 'm', m, key, float(got[key]), float(want))
            assert np.isfinite(want) and got[key].dtype == torch.float32
            assert np.float32(got[key].cpu().numpy()).tobytes() == np.float32(want).tobytes(), (k, key)
        assert torch.equal(_bits(got['grad_norm']), _bits(norm)), k
        assert got['rows'].tolist() == list(range(B))
        if per[0][2] is not None:
            assert torch.equal(_bits(got['log_probs']), _bits(torch.cat([p[2] for p in per])))
        for name in ('p', 'm', 'v', 'ema'):
            for i, (a, b) in enumerate(zip(getattr(tr, name), getattr(ref, name))):
                assert torch.equal(_bits(a), _bits(b)), (k, name, i)
    assert tr.global_step == len(batches)


@pytest.mark.parametrize('m', [1, 2])
def test_teacher_sharded_step_equals_the_written_out_loop(ds, weights, m):
    from nsynth_wavenet_amd import train
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    w = weights['teacher']
    a, b = Wavenet(TEACHER).load_weights(w), Wavenet(TEACHER).load_weights(w)
    try:
        tr = train.TeacherTrainer(a, w, lr=LR, dropout=True, dropout_seed=SEED + 5)
        ref = train.TeacherTrainer(b, w, lr=LR, dropout=True, dropout_seed=SEED + 5)

        def shard_call(rows, k, j):
            out = b.loss_and_weight_grads(rows, upsampler=True,
                                          dropout_seed=train.shard_seed(train.dropout_step_seed(SEED + 5, k), j))
            return out, [out['flat_grads'], out['flat_upsampler_grads']]
        _check_against_the_written_out_loop(tr, ref, [ds.batch(k, B) for k in range(3)], m, shard_call)
    finally:
        a.engine.close()
        b.engine.close()


@pytest.fixture(scope='module')
def frozen_teacher(weights):
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    te = Wavenet(TEACHER).load_weights(weights['teacher'])
    yield te
    te.engine.close()


@pytest.mark.parametrize('m', [1, 2])
def test_distilled_student_sharded_step_equals_the_written_out_loop(ds, weights, frozen_teacher, m):
    from nsynth_wavenet_amd import train
    from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet
    w = weights['student']
    a = ParallelWavenet(STUDENT, teacher=frozen_teacher).load_weights(w)
    b = ParallelWavenet(STUDENT, teacher=frozen_teacher).load_weights(w)
    try:
        tr = train.StudentTrainer(a, w, lr=LR, seed=SEED + 11)
        ref = train.StudentTrainer(b, w, lr=LR, seed=SEED + 11)
        scopes = b.engine.iaf_stack_scopes()

        def shard_call(rows, k, j):
            out = b.loss_and_weight_grads(rows, seed=train.shard_seed(SEED + 11 + k, j), upsampler=True)
            return out, [out['flat_grads']] + [out['flat_upsampler_grads'][s] for s in scopes]
        _check_against_the_written_out_loop(tr, ref, [ds.batch(k, B, mel_rand=True) for k in range(3)], m, shard_call)
    finally:
        a.engine.close()
        b.engine.close()


def _mle_batches(ds, n):
    """n batches for the MLE student: real-audio-like rows of the student's own length (1800 samples for the 9 frames of
    'mel'; the crops of the dataset have 1600), a tone in noise per row"""
    T = 1800
    rs = np.random.RandomState(3)
    t = np.arange(T) / 16000.0
    batches = []
    for k in range(n):
        wav = np.stack([0.3 * np.sin(2 * np.pi * 110.0 * (i + k + 1) * t) + 0.05 * rs.standard_normal(T) for i in range(B)])
        batches.append({'mel': ds.batch(k, B)['mel'], 'wav': torch.from_numpy(wav.astype(np.float32)).cuda()})
    return batches


def test_mle_student_sharded_step_equals_the_written_out_loop(ds, weights):
    """three steps at m = 2, as for the other two trainers: the third is past the change of the schedule"""
    from nsynth_wavenet_amd import train
    from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet
    w = weights['student']
    a, b = ParallelWavenet(STUDENT).load_weights(w), ParallelWavenet(STUDENT).load_weights(w)
    try:
        assert a.engine.iaf_length(9) == 1800
        tr = train.StudentMleTrainer(a, w, lr=LR)
        ref = train.StudentMleTrainer(b, w, lr=LR)
        scopes = b.engine.iaf_stack_scopes()
        calls = []

        def shard_call(rows, k, j):
            out = b.nll_and_weight_grads(rows, upsampler=True, encode_tol=1e-5)
            calls.append(out)
            return out, [out['flat_grads']] + [out['flat_upsampler_grads'][s] for s in scopes]
        _check_against_the_written_out_loop(tr, ref, _mle_batches(ds, 3), 2, shard_call)
        assert len(calls) == 6 and tr.lr_history == [1e-3, 1e-3, 5e-4]
    finally:
        a.engine.close()
        b.engine.close()


def test_mle_sharded_step_merges_its_outputs_and_defers_non_convergence(ds, weights):
    """A converging sharded step: 'sweeps' and 'adjoint_sweeps' are the largest of any shard, 'converged' and 'log_probs'
    cover all rows in shard order.  With max_sweeps=1 neither shard's encode converges: every shard still runs, the step
    raises afterwards naming both, and nothing -- global_step, weights, moments, shadows, the handle -- has changed."""
    from nsynth_wavenet_amd import train
    from nsynth_wavenet_amd.engine import NotConverged
    from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet
    w = weights['student']
    a, b = ParallelWavenet(STUDENT).load_weights(w), ParallelWavenet(STUDENT).load_weights(w)
    try:
        batch = _mle_batches(ds, 1)[0]
        halves = [b.nll_and_weight_grads({k: v[j * 2:j * 2 + 2] for k, v in batch.items()}, upsampler=True, encode_tol=1e-5) for j in range(2)]
        assert all(int(h['sweeps']) > 1 for h in halves)        # so one sweep cannot be enough
        tr = train.StudentMleTrainer(a, w, lr=LR)
        got = tr.step(batch, micro_batch=2)
        assert set(got) == {'loss', 'log_probs', 'rows', 'grad_norm', 'sweeps', 'adjoint_sweeps', 'converged'}
        assert got['sweeps'] == max(h['sweeps'] for h in halves) and got['adjoint_sweeps'] == max(h['adjoint_sweeps'] for h in halves)
        assert got['converged'].dtype == torch.bool and got['converged'].tolist() == [True] * B
        assert torch.equal(got['converged'], torch.cat([h['converged'] for h in halves]))
        assert torch.equal(_bits(got['log_probs']), _bits(torch.cat([h['log_probs'] for h in halves])))
        assert tr.global_step == 1

        short = train.StudentMleTrainer(a, tr.weights(), lr=LR, max_sweeps=1)
        before = {name: [t.clone() for t in getattr(short, name)] for name in ('p', 'm', 'v', 'ema')}
        lp_before = a.log_prob(batch, tol=1e-5)['log_probs']
        ran = []
        shard = short._shard
        short._shard = lambda rows, j, noise=None: (ran.append(j), shard(rows, j, noise))[1]
        with pytest.raises(NotConverged):                      # what one shard on its own raises
            a.nll_and_weight_grads({k: v[:2] for k, v in batch.items()}, upsampler=True, encode_tol=1e-5, max_sweeps=1)
        with pytest.raises(RuntimeError, match=r'StudentMleTrainer.step: 2 of 2 shards did not converge, nothing was updated; '
                                               r'shard 0: .*did not converge in \d+ sweeps; shard 1: .*did not converge in \d+ sweeps'):
            short.step(batch, micro_batch=2)
        assert ran == [0, 1]                                   # the second shard ran although the first had failed
        assert short.global_step == 0 and short.lr_history == []
        for name in ('p', 'm', 'v', 'ema'):
            for x, y in zip(getattr(short, name), before[name]):
                assert torch.equal(_bits(x), _bits(y)), name
        assert torch.equal(_bits(a.log_prob(batch, tol=1e-5)['log_probs']), _bits(lp_before))    # the handle's weights too
    finally:
        a.engine.close()
        b.engine.close()


def test_combined_gradient_is_the_full_batch_gradient_within_the_bar(ds, weights):
    """Dropout off, so that the shards and the full batch evaluate the same function: the combine of the four one-row
    gradients against the parent's full-batch call on the same four rows.  Bars of tests/test_gpu_teacher_geometries.py:
    every tensor within 1e-4 of that tensor's largest magnitude, the loss within 4e-5 max(1, |loss|)."""
    from nsynth_wavenet_amd import engine as E
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    net = Wavenet(TEACHER).load_weights(weights['teacher'])
    try:
        eng = net.engine
        batch = ds.batch(0, B)
        full = net.loss_and_weight_grads(batch, upsampler=True)
        want = [full['flat_grads'].clone(), full['flat_upsampler_grads'].clone()]
        want_loss = float(full['loss'])
        sizes = [g.numel() for g in want]
        rows = torch.zeros(B, sum(sizes) + 1, device='cuda')
        for j in range(B):
            out = net.loss_and_weight_grads({k: batch[k][j:j + 1] for k in ('wav', 'mel')}, upsampler=True)
            rows[j] = torch.cat([out['flat_grads'], out['flat_upsampler_grads'], out['loss'].reshape(1)])
        got = E.grad_combine(rows)
        print('loss: full batch {:.9g}, combined {:.9g}'.format(want_loss, float(got[-1])))
        assert abs(float(got[-1]) - want_loss) <= 4e-5 * max(1.0, abs(want_loss))
        worst = 0.0
        for tab, base, ref in ((eng.teacher_grad_table(), 0, want[0]), (eng.deconv_grad_table(''), sizes[0], want[1])):
            for name, off, shape in tab:
                n = int(np.prod(shape))
                r = ref[off:off + n]
                scale = float(r.abs().max())
                err = float((got[base + off:base + off + n] - r).abs().max())
                assert err <= 1e-4 * scale, (name, err, scale)
                worst = max(worst, err / scale if scale > 0 else 0.0)
        print('combined against full batch: worst tensor error {:.3e} of its largest magnitude'.format(worst))
    finally:
        net.engine.close()


def test_one_shard_is_the_step_as_it_was(ds, weights):
    """micro_batch=None and micro_batch=B against the parent's step written out: one loss_and_weight_grads on the whole
    batch under dropout_step_seed, the optimiser kernels, the re-pack -- no combine, the loss in its own dtype"""
    from nsynth_wavenet_amd import train
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    w = weights['teacher']
    nets = [Wavenet(TEACHER).load_weights(w) for _ in range(3)]
    try:
        trs = [train.TeacherTrainer(n, w, lr=LR, dropout=True, dropout_seed=9) for n in nets]
        for k in range(2):
            batch = ds.batch(k, B)
            none, full = trs[0].step(batch), trs[1].step(batch, micro_batch=B)
            out = nets[2].loss_and_weight_grads(batch, upsampler=True, dropout_seed=train.dropout_step_seed(9, k))
            norm = _update_by_hand(trs[2], [out['flat_grads'], out['flat_upsampler_grads']], k)
            for got in (none, full):
                assert set(got) == {'loss', 'log_probs', 'grad_norm'}
                assert torch.equal(_bits(got['loss']), _bits(out['loss'])) and torch.equal(_bits(got['log_probs']), _bits(out['log_probs']))
                assert torch.equal(_bits(got['grad_norm']), _bits(norm))
            for name in ('p', 'm', 'v', 'ema'):
                for i in range(2):
                    assert torch.equal(_bits(getattr(trs[0], name)[i]), _bits(getattr(trs[2], name)[i])), (k, name, i)
                    assert torch.equal(_bits(getattr(trs[1], name)[i]), _bits(getattr(trs[2], name)[i])), (k, name, i)
        assert all(t._rows is None for t in trs)         # no shard buffer was ever made
    finally:
        for n in nets:
            n.engine.close()


def test_step_refuses_before_anything_is_computed(ds, weights):
    from nsynth_wavenet_amd import train
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    w = weights['teacher']
    net = Wavenet(TEACHER).load_weights(w)
    try:
        tr = train.TeacherTrainer(net, w, lr=LR)
        before = [p.clone() for p in tr.p]
        with pytest.raises(ValueError, match='B = 4 rows does not split into micro-batches of m = 3'):
            tr.step(ds.batch(0, B), micro_batch=3)
        with pytest.raises(ValueError, match='data_parallel=True needs an initialised'):
            train.TeacherTrainer(net, w, lr=LR, data_parallel=True)
        assert tr.global_step == 0 and all(torch.equal(a, b) for a, b in zip(before, tr.p))
    finally:
        net.engine.close()


# ---- two data-parallel ranks on ONE GPU (gloo; the rows cross through the host): everything but RCCL ----
def _dp_worker(rank, port, workdir):
    """python tests/test_gpu_train_shards.py --dp-worker RANK PORT WORKDIR: rank RANK of two, three sharded teacher steps"""
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE='2', LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    from nsynth_wavenet_amd import dist as wdist, train, weights as wts
    from nsynth_wavenet_amd.config import load_hparams
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    wdist.init_process_group('gloo', timeout_s=120)
    torch.cuda.set_device(0)
    w = wts.synthetic_weights(load_hparams(TEACHER), 'teacher', seed=SEED, init='tf')
    net = Wavenet(TEACHER).load_weights(w)
    tr = train.TeacherTrainer(net, w, lr=LR, dropout=True, dropout_seed=SEED + 5, data_parallel=True)
    assert (tr.world, tr.rank) == (2, rank)
    data = train.DeviceDataset.from_tfrecord(os.path.join(workdir, 'train.tfrecord'), WAVE, seed=SEED)
    outs = [tr.step(data.batch(k, B), micro_batch=1) for k in range(3)]
    assert all(o['rows'].tolist() == [2 * rank, 2 * rank + 1] and tuple(o['log_probs'].shape) == (2, WAVE) for o in outs)
    state = {name: [t.cpu() for t in getattr(tr, name)] for name in ('p', 'm', 'v', 'ema')}
    state['loss'] = [o['loss'].cpu() for o in outs]
    state['log_probs'] = [o['log_probs'].cpu() for o in outs]
    torch.save(state, os.path.join(workdir, 'dp_rank{}.pt'.format(rank)))
    prefix = tr.save(os.path.join(workdir, 'dp_ckpt'))
    assert os.path.basename(prefix) == 'model.ckpt-3'
    torch.distributed.barrier()
    assert os.path.exists(prefix + '.index')                       # rank 0's, seen by both
    torch.distributed.destroy_process_group()
    net.engine.close()


def _cli_worker(rank, port, kind, argv):
    """python tests/test_gpu_train_shards.py --cli-worker RANK PORT KIND ARGV...: rank RANK of two of a training command line.
    The worker brings its own process group (gloo) and device (GPU 0), which train_cli then uses as they are."""
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE='2', LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    from nsynth_wavenet_amd import dist as wdist, train_cli
    wdist.init_process_group('gloo', timeout_s=120)
    torch.cuda.set_device(0)
    train_cli.main(kind, argv)
    assert torch.distributed.is_initialized()           # a group train_cli was given is not train_cli's to end
    torch.distributed.destroy_process_group()


def _two_workers(args, port):
    """two ranks of this file's worker `args`, each once, in its own session and under the time limit -> rank 0's stdout"""
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), args[0], str(r), str(port)] + list(args[1:]), env=env, cwd=ROOT,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True) for r in range(2)]
    try:
        done = [p.communicate(timeout=CHILD_TIMEOUT) for p in procs]
    except subprocess.TimeoutExpired:
        pytest.fail('the two ranks did not finish in {} s'.format(CHILD_TIMEOUT))
    finally:
        for p in procs:
            try:
                os.killpg(p.pid, signal.SIGKILL)
            except ProcessLookupError:
                pass
    for p, (_, err) in zip(procs, done):
        assert p.returncode == 0, err[-4000:]
    assert 'step ' not in done[1][0] and 'saved ' not in done[1][0]             # rank 1 neither logs nor saves
    return done[0][0]


def test_two_ranks_on_one_gpu_have_the_bits_of_one_process(work, ds, weights):
    from nsynth_wavenet_amd import train
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    _two_workers(['--dp-worker', str(work)], 27500 + os.getpid() % 2000)
    w = weights['teacher']
    net = Wavenet(TEACHER).load_weights(w)
    try:
        tr = train.TeacherTrainer(net, w, lr=LR, dropout=True, dropout_seed=SEED + 5)
        outs = [tr.step(ds.batch(k, B), micro_batch=1) for k in range(3)]
        ranks = [torch.load(str(work / 'dp_rank{}.pt'.format(r))) for r in range(2)]
        for r, st in enumerate(ranks):
            for name in ('p', 'm', 'v', 'ema'):
                for i, (a, b) in enumerate(zip(getattr(tr, name), st[name])):
                    assert torch.equal(_bits(a.cpu()), _bits(b)), (r, name, i)
            for k in range(3):
                assert torch.equal(_bits(outs[k]['loss'].cpu()), _bits(st['loss'][k])), (r, k)
                assert torch.equal(_bits(outs[k]['log_probs'][2 * r:2 * r + 2].cpu()), _bits(st['log_probs'][k])), (r, k)
        tr.save(str(work / 'dp_one'))
        _same_tensors(_tensors(str(work / 'dp_one' / 'model.ckpt-3')), _tensors(str(work / 'dp_ckpt' / 'model.ckpt-3')), 'two ranks on one GPU')
    finally:
        net.engine.close()


# ---- command line ----
def _teacher_argv(work, log_root):
    return [os.path.join(ROOT, 'train_wavenet.py'), '--config', str(work / 'teacher.json'), '--train_path', str(work / 'train.tfrecord'),
            '--log_root', str(log_root), '--total_batch_size', str(B), '--micro_batch_size', '1', '--num_iters', '4',
            '--save_interval_steps', '2', '--log_every_n_steps', '1', '--seed', str(SEED)]


def _only_run(log_root, prefix):
    runs = os.listdir(str(log_root))
    assert len(runs) == 1 and runs[0].startswith(prefix), runs
    return os.path.join(str(log_root), runs[0])


@pytest.fixture(scope='module')
def teacher_one_process(work):
    out = _child(_teacher_argv(work, work / 'te1'))
    return _only_run(work / 'te1', 'wavenet-'), out


def test_cli_micro_batch_in_one_process_equals_the_trainer(work, ds, weights, teacher_one_process):
    from nsynth_wavenet_amd import train, train_cli
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    logdir, out = teacher_one_process
    w = weights['teacher']
    net = Wavenet(TEACHER).load_weights(w)
    try:
        tr = train.TeacherTrainer(net, w, lr=train_cli.lr_schedule(TEACHER), dropout=True, dropout_seed=SEED)
        losses = [float(tr.step(ds.batch(k, B), micro_batch=1)['loss'].double().cpu()) for k in range(4)]
        got = _logged(out)
        assert sorted(got) == [1, 2, 3, 4] and [got[k] for k in (1, 2, 3, 4)] == losses
        tr.save(os.path.join(logdir, 'manual'))
        _same_tensors(_tensors(os.path.join(logdir, 'model.ckpt-4')), _tensors(os.path.join(logdir, 'manual', 'model.ckpt-4')), 'sharded ckpt-4')
    finally:
        net.engine.close()


def test_cli_two_ranks_on_one_gpu_have_the_bits_of_one_process(work, teacher_one_process):
    """train_cli.main on two ranks that share GPU 0 over a gloo group of the worker's own: rank 0 alone makes the run
    directory, logs and saves; losses and checkpoints are the one-process run's; and the run continues in one process"""
    dir1, out1 = teacher_one_process
    out2 = _two_workers(['--cli-worker', 'teacher'] + _teacher_argv(work, work / 'te2g')[1:], 21500 + os.getpid() % 2000)
    dir2 = _only_run(work / 'te2g', 'wavenet-')
    one, two = _logged(out1), _logged(out2)
    assert sorted(one) == sorted(two) == [1, 2, 3, 4] and one == two
    assert _logged(open(os.path.join(dir2, 'train.log')).read()) == two
    assert out2.count('saved ') == 2
    for n in (2, 4):
        _same_tensors(_tensors(os.path.join(dir1, 'model.ckpt-{}'.format(n))), _tensors(os.path.join(dir2, 'model.ckpt-{}'.format(n))),
                      'teacher ckpt-{}, two ranks on one GPU'.format(n))
    dst = _continue_from(dir2, str(work / 'te2g_resumed'), 2, 4)
    out = _child([os.path.join(ROOT, 'train_wavenet.py'), '--train_path', str(work / 'train.tfrecord'), '--logdir', dst,
                  '--total_batch_size', str(B), '--micro_batch_size', '1', '--num_iters', '4', '--log_every_n_steps', '1', '--seed', str(SEED)])
    second = _logged(out)
    assert sorted(second) == [3, 4] and [second[k] for k in (3, 4)] == [two[k] for k in (3, 4)]
    _same_tensors(_tensors(os.path.join(dir2, 'model.ckpt-4')), _tensors(os.path.join(dst, 'model.ckpt-4')), 'continued in one process')


needs_two_gpus = pytest.mark.skipif(torch.cuda.device_count() < 2, reason='the two-rank runs need two GPUs, this machine has {}'.format(
    torch.cuda.device_count()))


@pytest.fixture(scope='module')
def teacher_two_ranks(work):
    out = _child(_teacher_argv(work, work / 'te2'), nproc=2, port=23500 + os.getpid() % 2000)
    return _only_run(work / 'te2', 'wavenet-'), out


@needs_two_gpus
def test_teacher_on_two_ranks_has_the_bits_of_one_process(teacher_one_process, teacher_two_ranks):
    (dir1, out1), (dir2, out2) = teacher_one_process, teacher_two_ranks
    one, two = _logged(out1), _logged(out2)
    print('one process', one, 'two ranks', two)
    assert sorted(one) == sorted(two) == [1, 2, 3, 4] and one == two              # as printed at %.17g
    assert _logged(open(os.path.join(dir2, 'train.log')).read()) == two            # rank 0 alone wrote the log, once per step
    for n in (2, 4):
        _same_tensors(_tensors(os.path.join(dir1, 'model.ckpt-{}'.format(n))), _tensors(os.path.join(dir2, 'model.ckpt-{}'.format(n))),
                      'teacher ckpt-{} on two ranks'.format(n))


@needs_two_gpus
def test_a_two_rank_run_continues_in_one_process(work, teacher_two_ranks):
    dir2, out2 = teacher_two_ranks
    dst = _continue_from(dir2, str(work / 'te2_resumed'), 2, 4)
    out = _child([os.path.join(ROOT, 'train_wavenet.py'), '--train_path', str(work / 'train.tfrecord'), '--logdir', dst,
                  '--total_batch_size', str(B), '--micro_batch_size', '1', '--num_iters', '4', '--log_every_n_steps', '1', '--seed', str(SEED)])
    first, second = _logged(out2), _logged(out)
    assert sorted(second) == [3, 4] and [second[k] for k in (3, 4)] == [first[k] for k in (3, 4)]
    _same_tensors(_tensors(os.path.join(dir2, 'model.ckpt-4')), _tensors(os.path.join(dst, 'model.ckpt-4')), 'two ranks, continued in one process')


def _student_argv(work, teacher_dir, log_root):
    return [os.path.join(ROOT, 'train_parallel_wavenet.py'), '--config', str(work / 'student.json'), '--train_path', str(work / 'train.tfrecord'),
            '--teacher_dir', teacher_dir, '--total_batch_size', str(B), '--micro_batch_size', '1', '--save_interval_steps', '2',
            '--log_every_n_steps', '1', '--seed', str(SEED), '--log_root', str(log_root)]


@pytest.fixture(scope='module')
def student_one_process(work, teacher_one_process):
    """train_parallel_wavenet.py in one process under the one-process teacher: four steps (the json's num_iters), m = 1"""
    out = _child(_student_argv(work, teacher_one_process[0], work / 'st1'))
    return _only_run(work / 'st1', 'parallel_wavenet-'), out


@pytest.mark.parametrize('same_gpu', [True, pytest.param(False, marks=needs_two_gpus)], ids=['one-gpu-gloo', 'two-gpus'])
def test_student_on_two_ranks_has_the_bits_of_one_process(work, teacher_one_process, student_one_process, same_gpu):
    dir1, out1 = student_one_process
    root = work / ('st2g' if same_gpu else 'st2')
    argv = _student_argv(work, teacher_one_process[0], root)
    if same_gpu:
        out2 = _two_workers(['--cli-worker', 'student'] + argv[1:], 25500 + os.getpid() % 2000)
    else:
        out2 = _child(argv, nproc=2, port=35500 + os.getpid() % 2000)
    dir2 = _only_run(root, 'parallel_wavenet-')
    for key in ('loss', 'kl_loss', 'power_loss', 'contrastive_loss'):
        one, two = _logged(out1, key), _logged(out2, key)
        assert sorted(one) == sorted(two) == [1, 2, 3, 4] and one == two, key
    for n in (2, 4):
        _same_tensors(_tensors(os.path.join(dir1, 'model.ckpt-{}'.format(n))), _tensors(os.path.join(dir2, 'model.ckpt-{}'.format(n))),
                      'student ckpt-{} on two ranks'.format(n))


if __name__ == '__main__':
    if sys.argv[1] == '--dp-worker':
        _dp_worker(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
    else:
        assert sys.argv[1] == '--cli-worker'
        _cli_worker(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5:])
