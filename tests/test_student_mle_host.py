"""Host-side tests of the student's likelihood gradient: the C ABI of wn_iaf_latent_log_prob_grad,
wn_iaf_adjoint_workspace_bytes and wn_iaf_adjoint as declared and as bound, the source in the build, and StudentMleTrainer's
refusals on a stub engine."""
import ctypes
import inspect
import os
import re

import pytest

from nsynth_wavenet_amd import _lib, build, train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(name):
    header = open(os.path.join(ROOT, 'include', 'wnhip.h')).read()
    m = re.search(r'^WN_API ([^;(]*?)\b' + name + r'\s*\(([^;]*)\);', header, re.M | re.S)
    assert m, name + ' is not declared in include/wnhip.h'
    return m.group(1).strip(), [re.sub(r'\s*/\*.*?\*/', '', ' '.join(a.split())) for a in m.group(2).split(',')]


def test_the_entry_points_are_declared_and_bound_alike():
    lib = _lib.load()
    want = {
        'wn_iaf_latent_log_prob_grad': ('int', ['wn_handle* h', 'const float* z', 'const float* scale_tot', 'int B', 'int64_t T',
                                                'const float* d_log_prob', 'float* g_z', 'float* d_scale_tot', 'void* stream']),
        'wn_iaf_adjoint_workspace_bytes': ('size_t', ['const wn_handle* h', 'int B', 'int F', 'int64_t T']),
        'wn_iaf_adjoint': ('int', ['wn_handle* h', 'const void* tape', 'size_t tape_bytes', 'const float* g_z',
                                   'const float* d_mean_tot', 'const float* d_scale_tot', 'int B', 'int F', 'int64_t T',
                                   'float* lam', 'int n_sweeps', 'float tol', 'float* resid', 'int32_t* counts', 'void* ws',
                                   'size_t ws_bytes', 'void* stream']),
    }
    ctype = {'int': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t, 'float': ctypes.c_float}
    for name, (ret, args) in want.items():
        assert name in _lib.SYMBOLS
        got_ret, got_args = _declared(name)
        assert got_ret == ret and got_args == args, (name, got_ret, got_args)
        bound = getattr(lib, name).argtypes
        assert len(bound) == len(args), name
        for a, b in zip(args, bound):
            t = a.rsplit(' ', 1)[0]
            assert b is (ctypes.c_void_p if t.endswith('*') else ctype[t]), (name, a, b)
    assert lib.wn_iaf_adjoint_workspace_bytes.restype is ctypes.c_size_t
    header = open(os.path.join(ROOT, 'include', 'wnhip.h')).read()
    assert re.search(r'^#define WN_ABI_VERSION 1$', header, re.M)


def test_the_source_is_in_the_build():
    assert 'wn_iaf_nll.hip' in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, 'wn_iaf_nll.hip'))
    assert len(set(build.SOURCES)) == len(build.SOURCES)


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
    use_mu_law = False
    teacher = None

    def __init__(self, table):
        self.engine = _StubEngine(table)


ONE = [('iaf_1/start_conv/W', 0, (1, 3, 1, 64))]


def test_student_mle_trainer_refusals():
    with pytest.raises(ValueError, match='StudentMleTrainer: this model has no weight gradients on the device'):
        train.StudentMleTrainer(_StubStudent([]), {})
    with pytest.raises(ValueError, match='needs an entry for step 0'):
        train.StudentMleTrainer(_StubStudent(ONE), {}, lr={5: 1e-3})
    for kw, msg in (({'encode_tol': -1e-5}, 'encode_tol must be >= 0, got -1e-05'),
                    ({'encode_tol': float('nan')}, 'encode_tol must be >= 0, got nan'),
                    ({'encode_tol': None}, 'encode_tol must be >= 0, got None'),
                    ({'adjoint_tol': -1.0}, 'adjoint_tol must be >= 0, got -1.0'),
                    ({'adjoint_tol': float('nan')}, 'adjoint_tol must be >= 0, got nan'),
                    ({'max_sweeps': 0}, 'max_sweeps must be >= 1, got 0')):
        with pytest.raises(ValueError, match='StudentMleTrainer: ' + re.escape(msg)):
            train.StudentMleTrainer(_StubStudent(ONE), {}, **kw)
    mu = _StubStudent(ONE)
    mu.use_mu_law = True
    with pytest.raises(ValueError, match='StudentMleTrainer: mu-law students are not supported'):
        train.StudentMleTrainer(mu, {})
    with pytest.raises(KeyError):                    # a student WITHOUT a teacher gets as far as its missing weights
        train.StudentMleTrainer(_StubStudent(ONE), {})


def test_step_names_a_missing_input():
    tr = object.__new__(train.StudentMleTrainer)
    with pytest.raises(KeyError, match="inputs lack 'wav'"):
        tr.step({'mel': None})


def test_it_is_student_trainers_machinery_and_student_trainer_is_as_it_was():
    assert issubclass(train.StudentMleTrainer, train.StudentTrainer)
    for name in ('_update', '_repack', 'weights', 'save', 'restore', 'use_ema', 'use_weights', '_init_buffers'):
        assert getattr(train.StudentMleTrainer, name) is getattr(train.StudentTrainer, name), name
    assert train.StudentMleTrainer.step is not train.StudentTrainer.step
    assert list(inspect.signature(train.StudentTrainer.__init__).parameters) == \
        ['self', 'pw', 'weights', 'lr', 'beta1', 'beta2', 'eps', 'ema_decay', 'clip_norm', 'upsampler', 'seed']
    assert list(inspect.signature(train.StudentMleTrainer.__init__).parameters) == \
        ['self', 'pw', 'weights', 'lr', 'beta1', 'beta2', 'eps', 'ema_decay', 'clip_norm', 'upsampler', 'encode_tol',
         'adjoint_tol', 'max_sweeps']
    with pytest.raises(ValueError, match='StudentTrainer needs a student with a teacher'):
        train.StudentTrainer(_StubStudent(ONE), {})
