"""The device re-pack of an upsampler stack (wn_repack_deconv_absmax / _plain / _split with tr_deconv_frag_kernel,
tr_deconv_h_kernel and tr_deconv_t_kernel, csrc/wn_train.hip) off the one deconv_config every other test re-packs
(DESIGN.md 25): the nine accepted geometries of tests/deconv_bwd_geometries.py, reached through
Engine.teacher_set_weights(params, up) on the 64-wide teacher handle and Engine.iaf_set_weights(params, {scope: up}) on the
256-wide student handle.

The form is that of tests/test_gpu_train_step.py and tests/test_gpu_student_train_step.py: a handle built from w0 and
re-packed to w1 against a fresh handle loaded from w1, as int32 bit patterns, largest difference 0.  w1 perturbs every
variable and moves every scale of the stack: the first deconv kernel times 2^-3, the last (of two or three) times 8.  A third
set wz is w1 with one deconv kernel all zero (pick_scale's 1): the middle one of 'three', else the first.

Compared: Engine.deconv rows on a default and on a precision='f32' handle (the fp32 fragments and the frame-axis table path),
the G4 consumer (teacher_forward; iaf_generate under injected noise with layer groups on and off) and every tensor of
deconv_backward -- the only reader of the transposed planes tr_deconv_t_kernel writes, 'three's middle layer among them.
Shapes (2, 3) and (1, F_a), the second past one 256-column tile of the forward GEMM; the student's consumer runs where the
shape gives it a sample (T = F hop rounded down to 512 > 0: always at F_a).  Then the flows or the stack alone go back to w0
with up_params=None and the upsampler's outputs stay those of w1; the student with private stacks hands them over one per
call."""
import numpy as np
import pytest

import deconv_bwd_geometries as BG
import test_gpu_deconv_geometries as TF
import test_gpu_student_train_step as ST

pytestmark = pytest.mark.gpu
KINDS = ('teacher', 'student')


def _stack_keys(w):
    return sorted(k for k in w if 'trans_conv_' in k)


def _w1(w0, n_layers, scopes, seed=77):
    rs = np.random.RandomState(seed)
    w1 = {}
    for k in sorted(w0):
        a = np.asarray(w0[k], np.float32)
        w1[k] = (a * (1.0 + 0.05 * rs.standard_normal(a.shape)) + 0.01 * rs.standard_normal(a.shape)).astype(np.float32)
    for s in scopes:
        p = s + '/' if s else ''
        w1[p + 'trans_conv_1/kernel'] = (w1[p + 'trans_conv_1/kernel'] * np.float32(2.0 ** -3)).astype(np.float32)
        if n_layers > 1:
            k = p + 'trans_conv_{:d}/kernel'.format(n_layers)
            w1[k] = (w1[k] * np.float32(8)).astype(np.float32)
    return w1


def _wz(w1, n_layers, scopes):
    wz = dict(w1)
    for s in scopes:
        k = (s + '/' if s else '') + 'trans_conv_{:d}/kernel'.format(2 if n_layers == 3 else 1)
        wz[k] = np.zeros_like(w1[k])
    return wz


def _engine(kind, cfgd, w, precision=None):
    from nsynth_wavenet_amd.engine import Engine
    return Engine(cfgd, precision=precision).load_weights(w)


def _shapes(tag):
    return [(2, 3), (1, BG.f_a(tag))]


def _outputs(eng, kind, tag, backward=True):
    """everything the stack's packs feed, on fixed inputs: {name: device tensor}"""
    import torch
    out = {}
    scopes = eng.iaf_stack_scopes() if kind == 'student' else ['']
    Cd = int(eng.hp.deconv_width)
    for B, F in _shapes(tag):
        sid = 'B{}-F{}'.format(B, F)
        if kind == 'student':
            mel, noise, T = BG.student_inputs(tag, B, F, seed=3)
            if T > 0:
                for groups in (True, False):
                    eng.set_layer_groups(groups)
                    for k, v in eng.iaf_generate(mel, noise, want=TF.OUTS).items():
                        out['iaf_generate/{}/groups{:d}/{}'.format(sid, groups, k)] = v
                eng.set_layer_groups(None)
        else:
            mel, wav = BG.teacher_inputs(tag, B, F, seed=3)
            out['teacher_forward/' + sid] = eng.teacher_forward(wav, mel)
        MEL = torch.as_tensor(mel).cuda()
        g = torch.as_tensor(np.random.RandomState(5 + F).standard_normal([B, F * BG.hop(tag), Cd]).astype(np.float32)).cuda()
        for s in scopes:
            out['deconv/{}/{}'.format(s, sid)] = eng.deconv(MEL, s)
            if backward:
                for k, v in eng.deconv_backward(MEL, g, s)['grads'].items():
                    out['deconv_backward/{}/{}'.format(sid, k)] = v
    assert any(k.startswith('iaf_generate/' if kind == 'student' else 'teacher_forward/') for k in out)
    return {k: v.clone() for k, v in out.items()}


def _set(eng, kind, w, scopes):
    """re-pack the flows / the stack from w, and the upsampler stacks named in `scopes` ([]: none, up_params=None)"""
    if kind == 'student':
        eng.iaf_set_weights(ST._flat(eng.iaf_grad_table(), w), ST._up(eng, w, scopes) if scopes else None)
    else:
        eng.teacher_set_weights(ST._flat(eng.teacher_grad_table(), w), ST._flat(eng.deconv_grad_table(''), w) if scopes else None)


def _moved(before, after, label):
    import torch
    same = [k for k in sorted(after) if not k.startswith('deconv_backward') and torch.equal(before[k], after[k])]
    assert not same, (label, 'the re-pack left these where they were', same)


def _repack_case(kind, tag, label, **extra):
    import torch
    cfgd = BG.cfg_of(kind, tag, **extra)
    n = len(cfgd['deconv_config'])
    w0 = BG.weights(kind, cfgd)
    made = []

    def new(w, precision=None):
        made.append(_engine(kind, cfgd, w, precision))
        return made[-1]
    try:
        a, a32 = new(w0), new(w0, 'f32')
        scopes = a.iaf_stack_scopes() if kind == 'student' else ['']
        w1 = _w1(w0, n, scopes)
        wz = _wz(w1, n, scopes)
        b, b32 = new(w1), new(w1, 'f32')
        before = _outputs(a, kind, tag)
        if len(scopes) > 1:                      # private stacks: one per call
            _set(a, kind, w1, scopes[1:])
            half = dict(w1)
            half.update({k: v for k, v in w0.items() if k.startswith(scopes[0] + '/trans_conv_')})
            ST._assert_same_bits(_outputs(a, kind, tag), _outputs(new(half), kind, tag), label + ' w1, all stacks but the first')
            _set(a, kind, w1, scopes[:1])
        else:
            _set(a, kind, w1, scopes)
        _set(a32, kind, w1, scopes)
        got = _outputs(a, kind, tag)
        ST._assert_same_bits(got, _outputs(b, kind, tag), label + ' w1')
        _moved(before, got, label)
        ST._assert_same_bits(_outputs(a32, kind, tag, backward=False), _outputs(b32, kind, tag, backward=False), label + ' w1 f32')
        # the flows / the stack alone go back to w0: the upsampler stays that of w1
        _set(a, kind, w0, [])
        mixed = dict(w0)
        mixed.update({k: w1[k] for k in _stack_keys(w1)})
        got = _outputs(a, kind, tag)
        ST._assert_same_bits(got, _outputs(new(mixed), kind, tag), label + ' w0 with the upsampler of w1')
        want = _outputs(b, kind, tag)
        for k in got:
            if k.startswith('deconv'):
                assert torch.equal(got[k], want[k]), (label, k)
        # one kernel all zero: the scale of 1
        _set(a, kind, wz, scopes)
        _set(a32, kind, wz, scopes)
        ST._assert_same_bits(_outputs(a, kind, tag), _outputs(new(wz), kind, tag), label + ' wz')
        ST._assert_same_bits(_outputs(a32, kind, tag, backward=False), _outputs(new(wz, 'f32'), kind, tag, backward=False),
                             label + ' wz f32')
    finally:
        for e in made:
            e.close()


@pytest.mark.parametrize('tag', BG.TAGS)
@pytest.mark.parametrize('kind', KINDS)
def test_repack_equals_a_fresh_handle(kind, tag):
    _repack_case(kind, tag, 'DECONV-REPACK-GEO {} {}'.format(kind, tag))


def test_private_stacks_go_over_one_per_call():
    """a student with use_share_deconv off and two flows on taps6: 'iaf_2' in one call, 'iaf_1' in the next"""
    _repack_case('student', 'taps6', 'DECONV-REPACK-GEO student taps6 private stacks', use_share_deconv=False,
                 num_iaf_layers=[10, 10])
