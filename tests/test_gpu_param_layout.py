"""GPU tests of the parameter layouts a finalized handle keeps: Engine.teacher_grad_table,
iaf_grad_table and deconv_grad_table, with the *_grad_floats calls, on the smallest models the suite builds -- the 'small'
teacher pair of tests/test_gpu_train_step.py and the students S1 (a shared stack) and S2 (private stacks) of
tests/student_grad_oracle64.py.

The tables are held to weights.expected_variables: its names, shapes and order, everything but the trans_conv entries in the
teacher's or the flows' table, each stack's entries in its own; offsets contiguous from 0; the same rows from a second call, from
a fork and after a re-pack.  That the offsets are the ones the kernels write is what the float64 gradient tests and the
bit-exact re-pack tests check."""
import numpy as np
import pytest

import student_grad_oracle64 as S
import test_gpu_student_grad as SG
import test_gpu_train_step as TT

pytestmark = pytest.mark.gpu


def _scopes(eng):
    return eng.iaf_stack_scopes() if eng.kind == 'student' else ['']


def _main(eng):
    return (eng.iaf_grad_table, eng.iaf_grad_floats) if eng.kind == 'student' else (eng.teacher_grad_table, eng.teacher_grad_floats)


def _tables(eng):
    """{which: (table, floats)} of every table the handle has"""
    table, floats = _main(eng)
    out = {'main': (table(), floats())}
    for scope in _scopes(eng):
        out[scope + '/up'] = (eng.deconv_grad_table(scope), eng.deconv_grad_floats(scope))
    return out


def _check(eng):
    """the tables of a finalized engine against weights.expected_variables; returns them"""
    from nsynth_wavenet_amd import weights as wts
    want = [(name, tuple(shape)) for name, shape in wts.expected_variables(eng.hp, eng.kind, eng.n_mel)]
    is_up = lambda name: 'trans_conv_' in name
    got = _tables(eng)
    assert [(n, s) for n, _, s in got['main'][0]] == [(n, s) for n, s in want if not is_up(n)]
    in_stacks = []
    for scope in _scopes(eng):
        prefix = (scope + '/' if scope else '') + 'trans_conv_'
        mine = [(n, s) for n, s in want if n.startswith(prefix)]
        assert mine and [(n, s) for n, _, s in got[scope + '/up'][0]] == mine
        in_stacks += mine
    assert sorted(in_stacks) == sorted((n, s) for n, s in want if is_up(n))
    for which, (table, floats) in got.items():
        at = 0
        for name, off, shape in table:
            assert off == at, (which, name)
            at += int(np.prod(shape))
        assert floats == at > 0, which
    # a second call and a fork: equal rows in a list of the caller's own
    again = _tables(eng)
    fork = eng.fork()
    forked = _tables(fork)
    fork.close()
    for which, (table, floats) in got.items():
        for other in (again, forked):
            assert other[which] == (table, floats) and other[which][0] is not table, which
    mine = _main(eng)[0]()
    mine.clear()
    assert _main(eng)[0]() == got['main'][0]
    return got


def test_teacher_tables():
    pr = TT._Pair(np.load(TT.TS.GOLD), 'small')
    try:
        ea = pr.a.engine
        got = _check(ea)
        assert _check(pr.b.engine) == got
        ea.teacher_set_weights(TT._flat(ea.teacher_grad_table(), pr.w1), TT._flat(ea.deconv_grad_table(''), pr.w1))
        assert _tables(ea) == got
    finally:
        pr.close()


@pytest.mark.parametrize('model', ['S1', 'S2'])
def test_student_tables(model):
    eng = SG._new_engine(SG._cfg(model), SG._weights(model)[1])
    try:
        got = _check(eng)
        assert len(_scopes(eng)) == (1 if model == 'S1' else 2)
        w1 = SG._weights(model, seed=SG.SEED + 1)[1]
        eng.iaf_set_weights(TT._flat(eng.iaf_grad_table(), w1),
                            {scope: TT._flat(eng.deconv_grad_table(scope), w1) for scope in _scopes(eng)})
        assert _tables(eng) == got
    finally:
        eng.close()


def test_a_refused_student_keeps_its_empty_table():
    """S1 with use_weight_norm, as tests/test_gpu_student_grad.py builds it: [] and 0 floats, on a first and a second call"""
    from nsynth_wavenet_amd import config as cfg, weights as wts
    from nsynth_wavenet_amd.engine import Engine
    cfgd = dict(S.S1, use_weight_norm=True)
    eng = Engine(cfgd, kind='student').load_weights(wts.synthetic_weights(cfg.load_hparams(cfgd), 'student', seed=1))
    try:
        for _ in range(2):
            assert eng.iaf_grad_table() == [] and eng.iaf_grad_floats() == 0
            assert int(eng.lib.wn_iaf_grad_count(eng._h)) == 0
    finally:
        eng.close()
