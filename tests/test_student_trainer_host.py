"""Host-side tests of the student's training step: the C ABI of wn_iaf_set_weights as declared and as bound,
StudentTrainer's refusals on a stub engine, and the learning-rate / decay bookkeeping the two trainers share."""
import os
import re

import pytest

from nsynth_wavenet_amd import _lib, train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_args(name):
    header = open(os.path.join(ROOT, 'include', 'wnhip.h')).read()
    m = re.search(r'^WN_API [^;(]*?\b' + name + r'\s*\(([^;]*)\);', header, re.M | re.S)
    assert m, name + ' is not declared in include/wnhip.h'
    return [a.strip() for a in m.group(1).split(',')]


def test_set_weights_is_declared_and_bound_alike():
    lib = _lib.load()
    assert 'wn_iaf_set_weights' in _lib.SYMBOLS and 'wn_iaf_set_weights_workspace_bytes' in _lib.SYMBOLS
    for name, nargs in (('wn_iaf_set_weights', 9), ('wn_iaf_set_weights_workspace_bytes', 1)):
        args = _declared_args(name)
        assert len(args) == nargs, args
        assert len(getattr(lib, name).argtypes) == nargs
    assert _declared_args('wn_iaf_set_weights')[3].startswith('const float* const*')
    import ctypes
    assert lib.wn_iaf_set_weights_workspace_bytes.restype is ctypes.c_size_t
    src = open(os.path.join(ROOT, 'nsynth_wavenet_amd', 'build.py')).read()
    assert "'wn_iaf_repack.hip'" in src and "'wn_repack.h'" in src


class _StubEngine(object):
    device = 'cpu'

    def __init__(self, table):
        self.table = table

    def iaf_grad_table(self):
        return self.table

    def iaf_grad_floats(self):
        return 0

    def iaf_stack_scopes(self):
        return []


class _StubStudent(object):
    use_teacher_deconv = False

    def __init__(self, teacher, table):
        self.teacher, self.engine = teacher, _StubEngine(table)


def test_student_trainer_refusals():
    with pytest.raises(ValueError, match='needs a student with a teacher'):
        train.StudentTrainer(_StubStudent(None, [('iaf_1/start_conv/W', 0, (1, 3, 1, 64))]), {})
    with pytest.raises(ValueError, match='no weight gradients on the device'):
        train.StudentTrainer(_StubStudent(object(), []), {})
    with pytest.raises(ValueError, match='needs an entry for step 0'):
        train.StudentTrainer(_StubStudent(object(), []), {}, lr={5: 1e-3})


def test_the_shared_base_keeps_the_teacher_trainer_schedule(monkeypatch):
    """TeacherTrainer._update through the shared base class: scheduled_lr and the decay min(d, (1 + n) / (10 + n)), n = 0..3"""
    import math
    import numpy as np
    assert issubclass(train.TeacherTrainer, train._DeviceTrainer) and issubclass(train.StudentTrainer, train._DeviceTrainer)
    assert train.TeacherTrainer._update is train._DeviceTrainer._update is train.StudentTrainer._update
    assert train.TeacherTrainer.weights is train.StudentTrainer.weights
    seen = []
    monkeypatch.setattr(train, 'grad_sumsq', lambda g, acc, accumulate=False: acc)
    monkeypatch.setattr(train, 'adam_ema_step', lambda p, g, m, v, e, lr_t, b1, b2, eps, decay_t, sumsq=None, clip_norm=1.0:
                        seen.append((lr_t, decay_t, sumsq, clip_norm)))

    class _Sum(object):
        def sqrt(self):
            return [0.0]
    tr = object.__new__(train.TeacherTrainer)
    tr._init_optimiser({0: 1e-3, 2: 5e-4}, 0.9, 0.999, 1e-8, 0.25, None)
    tr.p, tr.m, tr.v, tr.ema = [[0.0]], [[0.0]], [[0.0]], [[0.0]]
    tr.sumsq, tr.global_step, tr.lr_history = _Sum(), 0, []
    for n in range(4):
        tr._update([[0.0]])
        tr.global_step += 1
    lrs = [1e-3, 1e-3, 5e-4, 5e-4]
    assert tr.lr_history == lrs == [train.scheduled_lr({0: 1e-3, 2: 5e-4}, n) for n in range(4)]
    for n, (lr_t, decay_t, sumsq, clip_norm) in enumerate(seen):
        assert decay_t == min(0.25, (1.0 + n) / (10.0 + n))
        assert lr_t == float(np.float32(lrs[n] * math.sqrt(1.0 - 0.999 ** (n + 1)) / (1.0 - 0.9 ** (n + 1))))
        assert sumsq is None and clip_norm == 1.0
    assert [d for _, d, _, _ in seen] == [0.1, 2.0 / 11.0, 0.25, 0.25]
    # the signature did not change
    import inspect
    assert list(inspect.signature(train.TeacherTrainer.__init__).parameters) == \
        ['self', 'wavenet', 'weights', 'lr', 'beta1', 'beta2', 'eps', 'ema_decay', 'clip_norm', 'upsampler', 'dropout', 'dropout_seed']
