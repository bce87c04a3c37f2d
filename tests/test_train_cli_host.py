"""Host tests of the training CLIs (nsynth_wavenet_amd/train_cli.py) and of the trainers' checkpoints: the
command-line surface, the refusals, the checkpoint's key set and its round trip through a trainer whose buffers are CPU
tensors, and the C ABI of wn_train_batch as declared and as bound."""
import json
import os
import re
from argparse import Namespace

import numpy as np
import pytest

from nsynth_wavenet_amd import _lib, tf_bundle, train, train_cli
from nsynth_wavenet_amd import weights as wts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_FLAGS = ['config', 'train_path', 'logdir', 'log_root', 'total_batch_size', 'log', 'gpu_id']
ADDED = ['num_iters', 'seed', 'save_interval_steps', 'save_interval_secs', 'log_every_n_steps', 'clip_norm']


def test_train_batch_is_declared_and_bound_alike():
    header = open(os.path.join(ROOT, 'include', 'wnhip.h')).read()
    m = re.search(r'^WN_API int wn_train_batch\s*\(([^;]*)\);', header, re.M | re.S)
    assert m, 'wn_train_batch is not declared in include/wnhip.h'
    assert len(m.group(1).split(',')) == 14 == len(_lib.load().wn_train_batch.argtypes)
    assert 'wn_train_batch' in _lib.SYMBOLS
    assert re.search(r'#define WN_ABI_VERSION\s+1\b', header)
    src = open(os.path.join(ROOT, 'nsynth_wavenet_amd', 'build.py')).read()
    assert "'wn_batch.hip'" in src and "'wn_mel.h'" in src


@pytest.mark.parametrize('kind', ['teacher', 'student'])
def test_parsers_take_the_reference_flags_and_the_additions(kind):
    p = train_cli.build_parser(kind)
    dests = sorted({a.dest for a in p._actions if a.dest != 'help'})          # --dropout / --no-dropout share one
    want = REFERENCE_FLAGS + ADDED + (['teacher_dir'] if kind == 'student' else ['dropout'])
    assert dests == sorted(want)
    argv = ['--train_path', 'x.tfrecord'] + (['--teacher_dir', 'te'] if kind == 'student' else [])
    a = p.parse_args(argv)
    # the reference's defaults, and those the additions document
    assert (a.config, a.logdir, a.log_root, a.total_batch_size, a.log, a.gpu_id) == (None, '/tmp/nsynth', '', 4, 'INFO', '0')
    assert (a.num_iters, a.seed, a.save_interval_steps, a.save_interval_secs, a.log_every_n_steps, a.clip_norm) == \
        (None, 0, 0, 3600, 100, None)
    with pytest.raises(SystemExit):
        p.parse_args(argv[2:] if kind == 'teacher' else argv[:2])           # --train_path / --teacher_dir are required
    if kind == 'teacher':
        assert a.dropout is None
        assert p.parse_args(argv + ['--dropout']).dropout is True and p.parse_args(argv + ['--no-dropout']).dropout is False
    else:
        with pytest.raises(SystemExit):
            p.parse_args(argv + ['--dropout'])


def test_refusals(tmp_path):
    with pytest.raises(RuntimeError, match='exactly one GPU.*multi-clone'):
        train_cli.check_gpu_id('0,1')
    with pytest.raises(RuntimeError, match='exactly one GPU'):
        train_cli.check_gpu_id('')
    assert train_cli.check_gpu_id('3') == '3'
    args = train_cli.build_parser('teacher').parse_args(['--train_path', 'x'])
    with pytest.raises(RuntimeError, match='neither by --num_iters nor by the config\'s "num_iters"'):
        train_cli.resolve_num_iters(args, {'width': 64})
    assert train_cli.resolve_num_iters(args, {'num_iters': 7}) == 7
    args.num_iters = 3
    assert train_cli.resolve_num_iters(args, {'num_iters': 7}) == 3
    # --logdir without a json, with two; --log_root without --config
    empty = tmp_path / 'empty'
    empty.mkdir()
    args.logdir = str(empty)
    with pytest.raises(RuntimeError, match=r'--logdir .* exactly one \*\.json config, found 0'):
        train_cli.resolve_run(args, 'teacher')
    for n in ('a.json', 'b.json'):
        (empty / n).write_text('{}')
    with pytest.raises(RuntimeError, match='found 2'):
        train_cli.resolve_run(args, 'teacher')
    args.logdir = str(tmp_path / 'nowhere')
    with pytest.raises(RuntimeError, match='is not a directory'):
        train_cli.resolve_run(args, 'teacher')
    args.log_root = str(tmp_path / 'root')
    with pytest.raises(RuntimeError, match='No config json specified'):
        train_cli.resolve_run(args, 'teacher')


def test_log_root_makes_a_run_directory_with_the_json(tmp_path):
    cfg = tmp_path / 'my_model.json'
    cfg.write_text(json.dumps({'width': 64, 'num_iters': 5}))
    args = train_cli.build_parser('student').parse_args(
        ['--train_path', 'x', '--teacher_dir', 't', '--config', str(cfg), '--log_root', str(tmp_path / 'logs')])
    hp, config_json, logdir, fresh = train_cli.resolve_run(args, 'student', now=0)
    assert fresh and hp == {'width': 64, 'num_iters': 5}
    assert os.path.dirname(logdir) == str(tmp_path / 'logs') and os.path.basename(logdir).startswith('parallel_wavenet-')
    assert os.listdir(logdir) == ['my_model.json'] and config_json == os.path.join(logdir, 'my_model.json')
    # ... and that directory is what --logdir continues from
    args.log_root, args.logdir = '', logdir
    hp2, config_json2, logdir2, fresh2 = train_cli.resolve_run(args, 'student')
    assert (hp2, config_json2, logdir2, fresh2) == (hp, config_json, logdir, False)


def test_lr_schedule():
    assert train_cli.lr_schedule({}) == train_cli.DEFAULT_LR_SCHEDULE
    assert train_cli.DEFAULT_LR_SCHEDULE[0] == 2e-4 and train_cli.DEFAULT_LR_SCHEDULE[90000] == 4e-4 / 3 and \
        list(train_cli.DEFAULT_LR_SCHEDULE) == [0, 90000, 120000, 150000, 180000, 210000, 240000]
    s = train_cli.lr_schedule(json.loads('{"lr_schedule": {"0": 1e-4, "90000": 6e-5}}'))
    assert s == {0: 1e-4, 90000: 6e-5} and all(isinstance(k, int) for k in s)
    assert train_cli.lr_schedule(Namespace(lr_schedule=[[0, 1e-4], [10, 5e-5]])) == {0: 1e-4, 10: 5e-5}
    assert train.scheduled_lr(s, 90000) == 6e-5


def test_init_from_teacher():
    te = {'trans_conv_1/kernel': np.ones((1, 4, 2, 3), np.float32), 'trans_conv_1/bias': np.full(2, 2.0, np.float32),
          'conv_start/W': np.zeros(3, np.float32)}
    st = {'iaf_1/trans_conv_1/kernel': np.zeros((1, 4, 2, 3), np.float32), 'iaf_2/trans_conv_1/kernel': np.zeros((1, 4, 2, 3), np.float32),
          'iaf_1/trans_conv_1/bias': np.zeros(2, np.float32), 'iaf_1/start_conv/W': np.zeros(3, np.float32)}
    done = train_cli.init_from_teacher(st, te)
    assert sorted(done) == ['iaf_1/trans_conv_1/bias', 'iaf_1/trans_conv_1/kernel', 'iaf_2/trans_conv_1/kernel']
    assert st['iaf_2/trans_conv_1/kernel'].min() == 1 and st['iaf_1/trans_conv_1/bias'].tolist() == [2, 2] and not st['iaf_1/start_conv/W'].any()
    with pytest.raises(ValueError, match='shape'):
        train_cli.init_from_teacher({'iaf_share/trans_conv_1/bias': np.zeros(5, np.float32)}, te)


# ---- checkpoints ----
HP = Namespace(deconv_config=[[4, 2]], deconv_width=4, double_gate_width=False, filter_length=3, loss_type='gauss', num_layers=2,
               num_stages=2, skip_width=4, use_mu_law=False, use_weight_norm=False, use_resize_conv=False, width=4)


class _CpuEngine(object):
    device = 'cpu'


def _cpu_trainer(w, frozen_prefix='trans_conv'):
    """a TeacherTrainer whose buffers are CPU tensors: two tables over the trained variables, the rest frozen"""
    tr = object.__new__(train.TeacherTrainer)
    tr.eng = _CpuEngine()
    tr._init_optimiser({0: 1e-3}, 0.9, 0.999, 1e-8, 0.9999, None)
    names = [n for n, _ in wts.expected_variables(HP, 'teacher') if not n.startswith(frozen_prefix)]
    tables, sizes = [], []
    for part in (names[:5], names[5:]):
        tab, off = [], 3                                   # a table need not start at 0 nor be dense
        for n in part:
            tab.append((n, off, tuple(w[n].shape)))
            off += w[n].size + 1
        tables.append(tab)
        sizes.append(off + 2)
    tr._init_buffers(w, tables, sizes)
    tr.repacked = []
    tr._repack = lambda bufs: tr.repacked.append([b.clone() for b in bufs])
    return tr


def _randomise(tr, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    for bufs in (tr.p, tr.m, tr.v, tr.ema):
        for b in bufs:
            b.copy_(torch.randn(b.shape, generator=g))


def test_checkpoint_keys_and_round_trip(tmp_path):
    import torch
    w = wts.synthetic_weights(HP, 'teacher', seed=3, init='unit')
    tr = _cpu_trainer(w)
    _randomise(tr, 1)
    tr.global_step = 12
    prefix = tr.save(str(tmp_path))
    assert prefix == str(tmp_path / 'model.ckpt-12') and tf_bundle.is_bundle(prefix)
    assert wts.latest_checkpoint(str(tmp_path)) == prefix
    assert 'model_checkpoint_path: "model.ckpt-12"' in (tmp_path / 'checkpoint').read_text()
    # the key set: four per trained variable, the plain name of a frozen one, the step and the two powers
    trained = [n for tab in tr.tables for n, _, _ in tab]
    frozen = [n for n, _ in wts.expected_variables(HP, 'teacher') if n.startswith('trans_conv')]
    assert frozen and len(trained) + len(frozen) == len(w)
    want = set(frozen) | {'global_step', 'beta1_power', 'beta2_power'}
    for n in trained:
        want |= {n, n + '/Adam', n + '/Adam_1', n + '/ExponentialMovingAverage'}
    r = tf_bundle.BundleReader(prefix)
    assert set(r.entries) == want
    assert r.get_tensor('global_step').dtype == np.int32 and int(r.get_tensor('global_step')) == 12
    assert r.get_tensor('beta1_power') == np.float32(0.9 ** 12) and r.get_tensor('beta2_power') == np.float32(0.999 ** 12)
    # TF shapes, and the values of each buffer under its key
    host = tr.weights()
    for n in trained:
        assert list(r.entries[n + '/Adam']['shape']) == list(w[n].shape)
        assert np.array_equal(r.get_tensor(n), host[n])
    # the eval loader takes the shadows, and the frozen variables under their plain names
    loaded = wts.load_checkpoint(prefix, HP, 'teacher')
    shadows = tr.weights(ema=True)
    assert sorted(loaded) == sorted(w)
    for n in w:
        assert np.array_equal(loaded[n], shadows[n]), n
    assert not np.array_equal(loaded[trained[0]], host[trained[0]])
    # the weights a run continues from are the plain ones
    plain = train.checkpoint_weights(str(tmp_path), HP, 'teacher')
    for n in w:
        assert np.array_equal(plain[n], host[n]), n

    # restore into another trainer: every buffer bit for bit (the gaps of the tables are not the checkpoint's business)
    tr2 = _cpu_trainer(w)
    _randomise(tr2, 2)
    gaps = [torch.ones_like(b, dtype=torch.bool) for b in tr2.p]
    for tab, gap in zip(tr2.tables, gaps):
        for n, off, shape in tab:
            gap[off:off + int(np.prod(shape))] = False
    tr2.restore(str(tmp_path))
    assert tr2.global_step == 12 and len(tr2.repacked) == 1
    for a, b, in zip((tr.p, tr.m, tr.v, tr.ema), (tr2.p, tr2.m, tr2.v, tr2.ema)):
        for x, y, gap in zip(a, b, gaps):
            assert torch.equal(x[~gap], y[~gap]) and not y[gap].any()
    assert all(torch.equal(x, y) for x, y in zip(tr2.repacked[0], tr2.p))
    assert tr2.restore(prefix).global_step == 12                     # a prefix works like the directory


def test_restore_names_what_is_wrong(tmp_path):
    w = wts.synthetic_weights(HP, 'teacher', seed=3, init='unit')
    tr = _cpu_trainer(w)
    tr.global_step = 2
    prefix = tr.save(str(tmp_path))
    r = tf_bundle.BundleReader(prefix)
    tensors = {k: r.get_tensor(k) for k in r.entries}
    # a missing key
    bad = dict(tensors)
    del bad['out1/W/Adam_1']
    tf_bundle.write_bundle(str(tmp_path / 'lacks'), bad)
    with pytest.raises(KeyError, match='lacks out1/W/Adam_1'):
        _cpu_trainer(w).restore(str(tmp_path / 'lacks'))
    # a shape that disagrees
    bad = dict(tensors)
    bad['out2/biases/ExponentialMovingAverage'] = np.zeros(7, np.float32)
    tf_bundle.write_bundle(str(tmp_path / 'shape'), bad)
    with pytest.raises(ValueError, match=r'out2/biases/ExponentialMovingAverage has shape \[7\]'):
        _cpu_trainer(w).restore(str(tmp_path / 'shape'))
    bad = dict(tensors)
    del bad['global_step']
    tf_bundle.write_bundle(str(tmp_path / 'nostep'), bad)
    with pytest.raises(KeyError, match='lacks global_step'):
        _cpu_trainer(w).restore(str(tmp_path / 'nostep'))
    empty = tmp_path / 'empty'
    empty.mkdir()
    with pytest.raises(ValueError, match='no checkpoint found'):
        _cpu_trainer(w).restore(str(empty))
