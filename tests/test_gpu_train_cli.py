"""GPU tests of train_wavenet.py / train_parallel_wavenet.py (nsynth_wavenet_amd/train_cli.py): a run from
the command line has the bits of the same loop written out in Python, a run continued from a checkpoint has the bits of the
uninterrupted one, and the eval loaders read what a run saved.

Models: a MoL teacher of width 64 (double gate: 128 is the narrowest gate the engine takes; geometry B of
tests/test_gpu_teacher_geometries.py with four layers in three stages) and a logistic student of width 64 with flows of 2 and
3 layers in three stages and a shared stack (S1 of tests/test_gpu_student_grad.py, the smallest student the training kernels
are tested at), both with deconv_width 64 and deconv_config [[40, 10], [80, 20]] (frame_shift 200, the featuriser's hop).
wave_length 1600 = 9 frames; the student generates iaf_length(9) = 1800 samples against the 1600 of 'wav' -- the trainers'
'wav' [B, T'] case.  total_batch_size 2; four utterances of a tone in noise, 1600 to 4000 samples, written by
reader.write_tfrecord.  Every child process has its own time limit and is run once."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300
SEED, BATCH, WAVE = 0, 2, 1600
TEACHER = {'deconv_config': [[40, 10], [80, 20]], 'deconv_width': 64, 'double_gate_width': True, 'dropout_inputs': True,
           'filter_length': 3, 'loss_type': 'mol', 'mol_mix': 10, 'num_layers': 4, 'num_stages': 3, 'skip_width': 64,
           'upsample_act': 'leaky_relu', 'use_mu_law': False, 'use_resize_conv': False, 'use_weight_norm': False,
           'wave_length': WAVE, 'width': 64, 'lr_schedule': {'0': 1e-3, '4': 5e-4}}
STUDENT = {'deconv_config': [[40, 10], [80, 20]], 'deconv_width': 64, 'filter_length': 3, 'loss_type': 'logistic',
           'num_iaf_layers': [2, 3], 'num_stages': 3, 'upsample_act': 'leaky_relu', 'use_mu_law': False, 'use_resize_conv': False,
           'use_share_deconv': True, 'use_teacher_deconv': False, 'use_weight_norm': False, 'wave_length': WAVE, 'width': 64,
           'num_samples': 8, 'power_loss_factor': 1.0, 'contrastive_loss_factor': 0.3, 'num_iters': 4}


def _child(script, argv):
    """one child process, once: its stdout; a non-zero exit fails the test with its stderr"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=ROOT)
    assert r.returncode == 0, '{} {} exited with {}:\n{}'.format(script, ' '.join(argv), r.returncode, r.stderr[-4000:])
    return r.stdout


def _logged(text, key='loss'):
    """{step: value} of the 'step N ... key V' lines"""
    return {int(m.group(1)): float(m.group(2)) for m in re.finditer(r'^step (\d+) .*?\b' + key + r' (\S+)', text, re.M)}


def _tensors(prefix):
    from nsynth_wavenet_amd import tf_bundle
    r = tf_bundle.BundleReader(prefix)
    return {k: r.get_tensor(k) for k in r.entries}


def _same_tensors(a, b, what):
    assert sorted(a) == sorted(b), what
    bad = [k for k in sorted(a) if a[k].dtype != b[k].dtype or a[k].tobytes() != b[k].tobytes()]
    assert not bad, (what, bad[:6])


def _continue_from(logdir, dst, step, last):
    """a copy of the run's directory whose `checkpoint` names model.ckpt-<step> and that lacks model.ckpt-<last>"""
    shutil.copytree(logdir, dst)
    for name in os.listdir(dst):
        if name.startswith('model.ckpt-{}.'.format(last)):
            os.remove(os.path.join(dst, name))
    with open(os.path.join(dst, 'checkpoint'), 'wt') as f:
        f.write('model_checkpoint_path: "model.ckpt-{0}"\nall_model_checkpoint_paths: "model.ckpt-{0}"\n'.format(step))
    return dst


@pytest.fixture(scope='module')
def work(tmp_path_factory):
    from nsynth_wavenet_amd.auxilaries import reader
    d = tmp_path_factory.mktemp('train_cli')
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
def teacher_run(work):
    """train_wavenet.py --log_root: six steps, a save every three -> (logdir, stdout)"""
    out = _child('train_wavenet.py', ['--config', str(work / 'teacher.json'), '--train_path', str(work / 'train.tfrecord'),
                                      '--log_root', str(work / 'te_logs'), '--total_batch_size', str(BATCH), '--num_iters', '6',
                                      '--save_interval_steps', '3', '--log_every_n_steps', '1', '--seed', str(SEED)])
    runs = os.listdir(str(work / 'te_logs'))
    assert len(runs) == 1 and runs[0].startswith('wavenet-')
    return str(work / 'te_logs' / runs[0]), out


@pytest.fixture(scope='module')
def teacher_manual(work):
    """the same six steps written out: (trainer, losses, the batch of step 0)"""
    from nsynth_wavenet_amd import train, train_cli, weights as wts
    from nsynth_wavenet_amd.config import load_hparams
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    w = wts.synthetic_weights(load_hparams(TEACHER), 'teacher', seed=SEED, init='tf')
    net = Wavenet(TEACHER).load_weights(w)
    tr = train.TeacherTrainer(net, w, lr=train_cli.lr_schedule(TEACHER), dropout=True, dropout_seed=SEED)
    ds = train.DeviceDataset.from_tfrecord(str(work / 'train.tfrecord'), WAVE, seed=SEED)
    losses = [float(tr.step(ds.batch(k, BATCH))['loss'].double().cpu()) for k in range(6)]
    return tr, losses, ds.batch(0, BATCH)


def test_teacher_cli_equals_the_manual_loop(teacher_run, teacher_manual):
    logdir, out = teacher_run
    tr, losses, _ = teacher_manual
    got = _logged(out)
    print('logged', got, 'manual', losses)
    assert sorted(got) == [1, 2, 3, 4, 5, 6] and all(np.isfinite(losses))
    assert [got[k] for k in range(1, 7)] == losses
    assert _logged(out, 'lr') == {1: 1e-3, 2: 1e-3, 3: 1e-3, 4: 1e-3, 5: 5e-4, 6: 5e-4}
    files = set(os.listdir(logdir))
    for n in (3, 6):
        assert {'model.ckpt-{}.index'.format(n), 'model.ckpt-{}.data-00000-of-00001'.format(n)} <= files
    assert {'teacher.json', 'checkpoint', 'train.log'} <= files
    assert _logged(open(os.path.join(logdir, 'train.log')).read()) == got
    # what the run saved is the manual trainer's state, bit for bit
    tr.save(os.path.join(logdir, 'manual'))
    _same_tensors(_tensors(os.path.join(logdir, 'model.ckpt-6')), _tensors(os.path.join(logdir, 'manual', 'model.ckpt-6')), 'teacher ckpt-6')


def test_teacher_resume_has_the_bits_of_the_uninterrupted_run(work, teacher_run):
    logdir, out = teacher_run
    dst = _continue_from(logdir, str(work / 'te_resumed'), 3, 6)
    out2 = _child('train_wavenet.py', ['--train_path', str(work / 'train.tfrecord'), '--logdir', dst, '--total_batch_size', str(BATCH),
                                       '--num_iters', '6', '--log_every_n_steps', '1', '--seed', str(SEED)])
    first, second = _logged(out), _logged(out2)
    assert sorted(second) == [4, 5, 6]
    assert [second[k] for k in (4, 5, 6)] == [first[k] for k in (4, 5, 6)]
    _same_tensors(_tensors(os.path.join(logdir, 'model.ckpt-6')), _tensors(os.path.join(dst, 'model.ckpt-6')), 'resumed teacher ckpt-6')


def test_eval_loader_reads_the_teacher_logdir(teacher_run, teacher_manual):
    import torch
    from nsynth_wavenet_amd import cli
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    logdir, _ = teacher_run
    tr, _, batch = teacher_manual
    hp, ckpt = cli.resolve_model(logdir)                       # what eval_wavenet.py does with --ckpt_dir
    assert ckpt == os.path.join(logdir, 'model.ckpt-6')
    got = Wavenet(hp).restore(ckpt).feed_forward(batch)['out_params']
    tr.use_ema()
    want = tr.net.feed_forward(batch)['out_params']
    tr.use_weights()
    assert bool(torch.isfinite(want).all()) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(want, tr.net.feed_forward(batch)['out_params'])          # the shadows are not the weights


@pytest.fixture(scope='module')
def student_run(work, teacher_run):
    out = _child('train_parallel_wavenet.py', ['--config', str(work / 'student.json'), '--train_path', str(work / 'train.tfrecord'),
                                               '--teacher_dir', teacher_run[0], '--log_root', str(work / 'st_logs'),
                                               '--total_batch_size', str(BATCH), '--save_interval_steps', '2', '--log_every_n_steps', '1',
                                               '--seed', str(SEED)])
    runs = os.listdir(str(work / 'st_logs'))
    assert len(runs) == 1 and runs[0].startswith('parallel_wavenet-')
    return str(work / 'st_logs' / runs[0]), out


def test_student_cli_resume_and_eval(work, teacher_run, student_run):
    """the teacher's three checks for train_parallel_wavenet.py under that teacher, with mel_rand (contrastive_loss_factor 0.3):
    four steps, a save at two"""
    import torch
    from nsynth_wavenet_amd import cli, train, train_cli, weights as wts
    from nsynth_wavenet_amd.config import load_hparams
    from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    logdir, out = student_run
    te_hp, te_ckpt = cli.resolve_model(teacher_run[0])
    te_w = wts.load_checkpoint(te_ckpt, te_hp, 'teacher')
    teacher = Wavenet(te_hp).load_weights(te_w)
    w = wts.synthetic_weights(load_hparams(STUDENT), 'student', seed=SEED, init='tf')
    fresh = {k: v.copy() for k, v in w.items()}
    done = train_cli.init_from_teacher(w, te_w)
    # a fresh student starts from the teacher's (shadow) upsampler
    assert sorted(done) == ['iaf_share/trans_conv_{}/{}'.format(j, leaf) for j in (1, 2) for leaf in ('bias', 'kernel')]
    for name in done:
        assert np.array_equal(w[name], te_w[name.split('/', 1)[1]]) and w[name].shape == fresh[name].shape
    assert not np.array_equal(w['iaf_share/trans_conv_1/kernel'], fresh['iaf_share/trans_conv_1/kernel'])
    pw = ParallelWavenet(STUDENT, teacher=teacher).load_weights(w)
    tr = train.StudentTrainer(pw, w, lr=train_cli.lr_schedule(STUDENT), seed=SEED)
    ds = train.DeviceDataset.from_tfrecord(str(work / 'train.tfrecord'), WAVE, seed=SEED)
    assert pw.engine.iaf_length(9) == 1800
    manual = []
    for k in range(4):
        o = tr.step(ds.batch(k, BATCH, mel_rand=True))
        manual.append({key: float(o[key].double().cpu()) for key in ('loss', 'kl_loss', 'power_loss', 'contrastive_loss')})
    print('logged', _logged(out), 'manual', manual)
    for key in ('loss', 'kl_loss', 'power_loss', 'contrastive_loss'):
        got = _logged(out, key)
        assert sorted(got) == [1, 2, 3, 4] and [got[k] for k in (1, 2, 3, 4)] == [m[key] for m in manual], key
    assert all(np.isfinite(m['loss']) for m in manual)
    files = set(os.listdir(logdir))
    assert {'model.ckpt-2.index', 'model.ckpt-4.index', 'student.json', 'checkpoint', 'train.log'} <= files
    tr.save(os.path.join(logdir, 'manual'))
    _same_tensors(_tensors(os.path.join(logdir, 'model.ckpt-4')), _tensors(os.path.join(logdir, 'manual', 'model.ckpt-4')), 'student ckpt-4')

    # resume from step 2
    dst = _continue_from(logdir, str(work / 'st_resumed'), 2, 4)
    out2 = _child('train_parallel_wavenet.py', ['--train_path', str(work / 'train.tfrecord'), '--teacher_dir', teacher_run[0],
                                                '--logdir', dst, '--total_batch_size', str(BATCH), '--log_every_n_steps', '1',
                                                '--seed', str(SEED)])
    first, second = _logged(out), _logged(out2)
    assert sorted(second) == [3, 4] and [second[k] for k in (3, 4)] == [first[k] for k in (3, 4)]
    _same_tensors(_tensors(os.path.join(logdir, 'model.ckpt-4')), _tensors(os.path.join(dst, 'model.ckpt-4')), 'resumed student ckpt-4')

    # the eval loader (eval_parallel_wavenet.py --ckpt_dir) on the run's directory: the shadows
    hp, ckpt = cli.resolve_model(logdir)
    assert ckpt == os.path.join(logdir, 'model.ckpt-4')
    mel = ds.batch(0, BATCH)['mel']
    got = ParallelWavenet(hp).restore(ckpt).feed_forward({'mel': mel}, seed=3)
    tr.use_ema()
    want = pw.feed_forward({'mel': mel}, seed=3)
    tr.use_weights()
    for key in ('x', 'mean_tot', 'scale_tot'):
        assert bool(torch.isfinite(want[key]).all()) and torch.equal(got[key].view(torch.int32), want[key].view(torch.int32)), key
