"""GPU tests of the student's training step on the device: the in-place re-pack wn_iaf_set_weights behind
Engine.iaf_set_weights and train.StudentTrainer.  Models and shapes are those of tests/test_gpu_student_grad.py: S1 (generic,
shared stack, width 64: the half-tile res_t), S2 (generic, private stacks, width 128) and the shipped parallel_wavenet.json
(the fp32-fragment and split-fp16 packs of the three launch forms).

The re-pack is held to bit equality with a fresh handle loaded from the same values: every output is compared as int32 words
with largest difference 0.  The optimiser's bars are those of tests/test_gpu_train_step.py (from the number of fp32
roundings): |p - p64| <= 2^-23 |p64| + 2^-20 |u64|, |ema - ema64| <= 2^-22 (|ema64| + |p64|)."""
import ctypes

import numpy as np
import pytest

import adam_oracle64 as A
import student_grad_oracle64 as S
import test_gpu_student_grad as G

pytestmark = pytest.mark.gpu
SHAPES = {'S1': (2, 25, 200), 'S2': (1, 64, 512), 'S3': (1, 6, 1024)}
# the layers whose kernels change scale in w1: (dilated_conv times 8, mel_cond times 2^-6, res all zero), first flow
MOVED = {'S1': (1, 2, 2), 'S2': (3, 5, 7), 'S3': (3, 5, 7)}
FORMS = {'f16x3': 0, 'f32': 1, 'f16x3-fused': 2}      # WN_FORM_F16X3, WN_FORM_F32, WN_FORM_F16X3_FUSED


def _w1(model, w0, seed=77):
    """w0 with a random perturbation everywhere and every kind of scale moved: one dilated_conv times 8, one mel_cond times
    2^-6 in another layer, one res all zero, one out1 times 4, one trans_conv kernel times 2^-3; and one mel_cond times 16,
    so that in one layer the conditioning kernel and not the dilated one decides the split-fp16 gate scale"""
    rs = np.random.RandomState(seed)
    w1 = {}
    for k in sorted(w0):
        a = np.asarray(w0[k], np.float32)
        w1[k] = (a * (1.0 + 0.05 * rs.standard_normal(a.shape)) + 0.01 * rs.standard_normal(a.shape)).astype(np.float32)
    d, c, r = MOVED[model]
    scale = lambda name, f: w1.__setitem__(name, (w1[name] * np.float32(f)).astype(np.float32))
    scale('iaf_1/dilated_conv_{}/W'.format(d), 8.0)
    scale('iaf_1/mel_cond_{}/W'.format(c), 2.0 ** -6)
    w1['iaf_1/res_{}/W'.format(r)] = np.zeros_like(w1['iaf_1/res_{}/W'.format(r)])
    scale('iaf_2/out1/W', 4.0)
    scale('iaf_2/mel_cond_1/W', 16.0)          # a layer whose mel_cond has the larger maximum: the smaller of the two scales is its
    scale(('iaf_2' if model == 'S2' else 'iaf_share') + '/trans_conv_2/kernel', 2.0 ** -3)
    return w1


def _flat(table, w):
    import torch
    name, off, shape = table[-1]
    flat = np.zeros(off + int(np.prod(shape)), np.float32)
    for name, off, shape in table:
        flat[off:off + int(np.prod(shape))] = np.asarray(w[name], np.float32).reshape(-1)
    return torch.as_tensor(flat).cuda()


def _up(eng, w, scopes=None):
    return {s: _flat(eng.deconv_grad_table(s), w) for s in (scopes or eng.iaf_stack_scopes())}


def _generate(eng, form, mel, noise):
    """wn_iaf_generate_form under injected noise: x, mean_tot, scale_tot, wav"""
    import torch
    from nsynth_wavenet_amd.engine import _ptr
    B, F = int(mel.shape[0]), int(mel.shape[1])
    T = eng.iaf_length(F)
    out = [torch.empty((B, T), dtype=torch.float32, device='cuda') for _ in range(4)]
    ws = torch.empty(max(int(eng.lib.wn_iaf_workspace_bytes_form(eng._h, form, B, F)), 256), dtype=torch.uint8, device='cuda')
    eng._check(eng.lib.wn_iaf_generate_form(eng._h, form, _ptr(mel), B, F, _ptr(noise), ctypes.c_uint64(0), _ptr(out[3]), None,
                                            _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), None, _ptr(ws), ws.numel(), eng._stream()))
    return dict(zip(('x', 'mean_tot', 'scale_tot', 'wav'), out))


def _outputs(eng, model):
    """everything the handle's packs feed, on fixed inputs: {name: device tensor}"""
    import torch
    B, F, T = SHAPES[model]
    mel, noise, cot = S.case_inputs(B, F, T, seed=G.SEED + 100)
    MEL, N = torch.as_tensor(mel).cuda(), torch.as_tensor(noise).cuda()
    out = {}
    if model == 'S3':
        for name, form in sorted(FORMS.items()):
            for groups in (True, False):
                eng.set_layer_groups(groups)
                for k, v in _generate(eng, form, MEL, N).items():
                    out['generate/{}/groups{:d}/{}'.format(name, groups, k)] = v
        eng.set_layer_groups(None)
    else:
        for k, v in _generate(eng, -1, MEL, N).items():
            out['generate/' + k] = v
    ff, tape = eng.iaf_forward_train_tape(MEL, noise=N)
    for k in ('x', 'mean_tot', 'scale_tot'):
        out['tape_forward/' + k] = ff[k]
    res = eng.iaf_backward_weights(tape, *cot)
    out['flat_grads'], out['d_encoding'] = res['flat_grads'], res['d_encoding']
    for s, scope in enumerate(eng.iaf_stack_scopes()):
        out['deconv/' + scope] = eng.deconv(MEL, scope)
        out['deconv_backward/' + scope] = eng.deconv_backward(MEL, res['d_encoding'][s], scope)['flat_grads']
    return {k: v.clone() for k, v in out.items()}


def _assert_same_bits(got, want, what):
    import torch
    assert sorted(got) == sorted(want)
    worst = {}
    for k in sorted(want):
        assert bool(torch.isfinite(want[k].double()).all()), (what, k)
        d = int((got[k].view(torch.int32).long() - want[k].view(torch.int32).long()).abs().max())
        if d:
            worst[k] = d
    print('{}: {} outputs, largest difference of the bit patterns {}'.format(what, len(want), max(worst.values()) if worst else 0))
    assert not worst, (what, worst)


@pytest.mark.parametrize('model', ['S1', 'S2', 'S3'])
def test_repack_equals_a_fresh_handle(model):
    """iaf_set_weights(w1) on a handle built from w0 against a fresh handle load_weights(w1); then the flows alone back to
    w0 (up_params=None) against a fresh handle built from w0's flows and w1's stacks.  S2: the stacks go over one per call."""
    import torch
    cfgd = G._cfg(model)
    _, w0 = G._weights(model)
    w1 = _w1(model, w0)
    a, b = G._new_engine(cfgd, w0), G._new_engine(cfgd, w1)
    try:
        before = _outputs(a, model)
        P1 = _flat(a.iaf_grad_table(), w1)
        assert P1.numel() == a.iaf_grad_floats()
        if model == 'S2':                       # one call passes only iaf_2's stack, a second one iaf_1's
            a.iaf_set_weights(P1, _up(a, w1, ['iaf_2']))
            half = dict(w1)
            half.update({k: v for k, v in w0.items() if k.startswith('iaf_1/trans_conv_')})
            c = G._new_engine(cfgd, half)
            _assert_same_bits(_outputs(a, model), _outputs(c, model), model + ' flows and iaf_2 stack')
            c.close()
            a.iaf_set_weights(P1, _up(a, w1, ['iaf_1']))
        else:
            a.iaf_set_weights(P1, _up(a, w1))
        got = _outputs(a, model)
        _assert_same_bits(got, _outputs(b, model), model + ' w1')
        moved = ['tape_forward/x', 'flat_grads', 'd_encoding'] + [k for k in got if k.startswith('deconv')]
        assert not any(torch.equal(before[k], got[k]) for k in moved), 'w1 moves the outputs'
        a.iaf_set_weights(_flat(a.iaf_grad_table(), w0), None)
        mixed = dict(w0)
        mixed.update({k: v for k, v in w1.items() if '/trans_conv_' in k})
        c = G._new_engine(cfgd, mixed)
        _assert_same_bits(_outputs(a, model), _outputs(c, model), model + ' flows back to w0')
        c.close()
    finally:
        a.close()
        b.close()


def test_tapes_written_before_the_repack_are_refused():
    import torch
    B, F, T = SHAPES['S1']
    _, w0 = G._weights('S1')
    eng = G._new_engine(S.S1, w0)
    mel, noise, cot = S.case_inputs(B, F, T, seed=1)
    _, tape = eng.iaf_forward_train_tape(mel, noise=noise)
    eng.iaf_backward_weights(tape, *cot, n_frames=F)                      # accepted before
    eng.iaf_set_weights(_flat(eng.iaf_grad_table(), w0), None)
    with pytest.raises(ValueError, match='was not written by wn_iaf_forward_train_tape of this handle'):
        eng.iaf_backward_weights(tape, *cot, n_frames=F)
    _, tape = eng.iaf_forward_train_tape(mel, noise=noise)               # a new tape works
    eng.iaf_backward_weights(tape, *cot)
    torch.cuda.synchronize()
    eng.close()


def test_refusals():
    """every refusal of the contract by name; the workspace query is 0 for the refused models"""
    import torch
    from oracle import wavenet_np as O
    import distill_oracle64 as D
    from nsynth_wavenet_amd import config as cfg, weights as wts
    from nsynth_wavenet_amd.engine import Engine, _ptr
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    _, w0 = G._weights('S1')
    eng = G._new_engine(S.S1, w0)
    P, U = _flat(eng.iaf_grad_table(), w0), _up(eng, w0)
    nb = int(eng.lib.wn_iaf_set_weights_workspace_bytes(eng._h))
    assert nb >= 256
    with pytest.raises(ValueError, match='params holds'):
        eng.iaf_set_weights(P[:-1].clone(), U)
    with pytest.raises(ValueError, match=r'up_params\[0\] holds'):
        eng.iaf_set_weights(P, {'iaf_share': torch.cat([U['iaf_share'], U['iaf_share'][:1]])})
    ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
    call = lambda ptrs, sizes, n_up, nbytes: eng.lib.wn_iaf_set_weights(eng._h, _ptr(P), P.numel(), ptrs, sizes, n_up, _ptr(ws),
                                                                        nbytes, eng._stream())
    one = (ctypes.c_void_p * 2)(U['iaf_share'].data_ptr(), U['iaf_share'].data_ptr())
    size = (ctypes.c_size_t * 2)(U['iaf_share'].numel(), U['iaf_share'].numel())
    assert call(one, size, 1, nb - 1) == -22 and b'workspace' in eng.lib.wn_last_error(eng._h)
    assert call(one, size, 2, nb) == -22 and b'n_up = 2' in eng.lib.wn_last_error(eng._h)
    assert call(one, size, 1, nb) == 0
    # a teacher handle; wn_teacher_set_weights keeps refusing the student
    te_cfg, te_seed, te_init = D.golden_case(np.load(G.GOLD), 'mol')[1]
    te = Wavenet(te_cfg).load_weights(O.synth_weights(O.HP(te_cfg), 'teacher', seed=te_seed, init=te_init))
    assert int(te.engine.lib.wn_iaf_set_weights_workspace_bytes(te.engine._h)) == 0
    with pytest.raises(ValueError, match='this is a teacher handle'):
        te.engine.iaf_set_weights(P, None)
    with pytest.raises(ValueError, match='student handle'):
        eng.teacher_set_weights(P, None)
    te.engine.close()
    # handles the student's training calls refuse
    for change, msg in ((dict(use_mu_law=True), 'mu-law student'), (dict(use_weight_norm=True), 'weight-norm student'),
                        (dict(width=32), 'multiples of 64')):      # (wn_create itself refuses such a deconv_width: no handle)
        cfgd = dict(S.S1, **change)
        e = Engine(cfgd, kind='student').load_weights(wts.synthetic_weights(cfg.load_hparams(cfgd), 'student', seed=1))
        assert int(e.lib.wn_iaf_set_weights_workspace_bytes(e._h)) == 0 and e.iaf_grad_floats() == 0
        with pytest.raises(ValueError, match=msg):
            e.iaf_set_weights(P, None)
        e.close()
    # not finalized
    e2 = Engine(S.S1, kind='student')
    with pytest.raises(RuntimeError, match='call wn_finalize first'):
        e2.iaf_set_weights(P, None)
    e2.close()
    # resize-conv stacks: the flows alone are accepted, a stack's buffer is not
    cfgd = dict(S.S1, use_resize_conv=True)
    w = wts.synthetic_weights(cfg.load_hparams(cfgd), 'student', seed=1)
    e3 = Engine(cfgd, kind='student').load_weights(w)
    P3 = _flat(e3.iaf_grad_table(), w)
    with pytest.raises(ValueError, match='use_resize_conv'):
        e3.iaf_set_weights(P3, U)
    e3.iaf_set_weights(P3, None)
    with pytest.raises(ValueError, match='no deconv stack with scope'):
        e3.iaf_set_weights(P3, {'iaf_9': U['iaf_share']})
    torch.cuda.synchronize()
    e3.close()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------------------------------------
LR_A, LR_B = 1e-3, 5e-4
SCHEDULE = {0: LR_A, 2: LR_B}
SEED0 = 5


def _batch(B, F, T):
    import torch
    mel, noise, _ = S.case_inputs(B, F, T, seed=G.SEED + 100)
    rs = np.random.RandomState(3)
    inputs = {'mel': torch.as_tensor(mel).cuda(), 'mel_rand': torch.as_tensor(rs.uniform(0, 1, mel.shape).astype(np.float32)).cuda(),
              'wav': torch.as_tensor(rs.uniform(-0.5, 0.5, [B, T]).astype(np.float32)).cuda()}
    return inputs, torch.as_tensor(noise).cuda()


LOSS_KEYS = ('loss', 'kl_loss', 'H_Ps', 'H_Ps_Pt', 'power_loss', 'contrastive_loss')


def _same_losses(a, b, what):
    import torch
    for k in a:
        if k in LOSS_KEYS:
            assert torch.equal(a[k], b[k]), (what, k, float(a[k]), float(b[k]))
    assert torch.equal(a['flat_grads'], b['flat_grads']), what


def test_trainer():
    """StudentTrainer on S1 under the golden small MoL teacher: 3 steps on one batch under the schedule {0: a, 2: b}"""
    import torch
    from nsynth_wavenet_amd.train import StudentTrainer
    from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet
    B, F, T = SHAPES['S1']
    pw, te, w0 = G._teacher_and_student()
    cfgd = dict(S.S1, num_samples=8, power_loss_factor=1.0, contrastive_loss_factor=0.3)      # _teacher_and_student's
    inputs, noise = _batch(B, F, T)
    eng = pw.engine
    first = pw.loss_and_weight_grads(inputs, seed=SEED0, noise=noise, upsampler=True)        # the untrained handle
    flats0 = [first['flat_grads']] + [first['flat_upsampler_grads']['iaf_share']]
    norm64 = float(np.sqrt(sum(float((g.double() ** 2).sum()) for g in flats0)))
    tr = StudentTrainer(pw, w0, lr=SCHEDULE, seed=SEED0)
    assert tr.scopes == ['iaf_share'] and len(tr.p) == 2
    p0 = [p.cpu().numpy().astype(np.float64) for p in tr.p]
    g0 = [g.cpu().numpy() for g in flats0]
    losses, lr_ts = [], []
    at = lambda n: float(n.loss_and_weight_grads(inputs, seed=SEED0, noise=noise, upsampler=False)['loss'])
    for k in range(3):
        if k == 2:
            entry3 = at(pw)                                              # the loss step 3 starts from, at the first step's seed
        out = tr.step(inputs, noise=noise)
        assert sorted(out) == sorted([n for n in first if n in LOSS_KEYS] + ['grad_norm'])
        losses.append(float(out['loss']))
        lr_ts.append(tr.lr_t)
        if k == 0:
            for n in out:
                if n != 'grad_norm':
                    assert torch.equal(out[n], first[n]), n
            gn = float(out['grad_norm'])
            print('grad_norm {:.9e}, float64 norm of the flat gradients {:.9e}'.format(gn, norm64))
            assert abs(gn - norm64) <= 1e-6 * norm64
            f32 = lambda x: float(np.float32(x))
            for p, g, a0, e in zip(tr.p, g0, p0, tr.ema):
                ref = A.adam_ema_step(a0, g, np.zeros_like(a0), np.zeros_like(a0), a0, tr.lr_t, f32(0.9), f32(0.999), f32(1e-8),
                                      f32(A.ema_decay(0.9999, 0)))
                got = p.cpu().numpy().astype(np.float64)
                assert np.all(np.abs(got - ref['p']) <= 2.0 ** -23 * np.abs(ref['p']) + 2.0 ** -20 * np.abs(ref['u']))
                want = 0.1 * a0 + 0.9 * got                           # the shadow after step 1
                assert np.all(np.abs(e.cpu().numpy() - want) <= 2.0 ** -22 * (np.abs(want) + np.abs(got)))
        # a fresh handle loaded from the trainer's weights: the same bits from the next step's call
        fresh = ParallelWavenet(cfgd, teacher=te).load_weights(tr.weights())
        nxt = SEED0 + k + 1
        _same_losses(pw.loss_and_weight_grads(inputs, seed=nxt, noise=noise), fresh.loss_and_weight_grads(inputs, seed=nxt, noise=noise),
                     'after step {}'.format(k + 1))
        fresh.engine.close()
    assert tr.lr_history == [LR_A, LR_A, LR_B]                           # the third step uses rate b
    assert [np.float32(v) for v in lr_ts] == [np.float32(A.lr_t(lr, 0.9, 0.999, t + 1)) for t, lr in enumerate(tr.lr_history)]
    # the loss at a fixed seed and noise: step 3's below step 1's
    after = at(pw)
    print('losses at entry of the steps', losses, '; at the first seed: step 1 {:.6f}, step 3 {:.6f}, after it {:.6f}'.format(
        float(first['loss']), entry3, after))
    assert entry3 < float(first['loss']) and after < float(first['loss'])
    # use_ema() then use_weights() restores the bits
    mel = inputs['mel']
    gen = lambda: {k: v.clone() for k, v in eng.iaf_generate(mel, noise, want=('x', 'mean_tot', 'scale_tot')).items()}
    keep, keep_enc = gen(), eng.deconv(mel, 'iaf_share').clone()
    tr.use_ema()
    fresh = ParallelWavenet(cfgd, teacher=te).load_weights(tr.weights(ema=True))
    ema_out, want = gen(), fresh.engine.iaf_generate(mel, noise, want=('x', 'mean_tot', 'scale_tot'))
    assert all(torch.equal(ema_out[k], want[k]) for k in want) and not torch.equal(ema_out['x'], keep['x'])
    fresh.engine.close()
    tr.use_weights()
    back = gen()
    assert all(torch.equal(back[k], keep[k]) for k in keep) and torch.equal(eng.deconv(mel, 'iaf_share'), keep_enc)
    eng.close()
    # upsampler=False: the stack keeps its bits and its variables come back as given
    pw2 = ParallelWavenet(cfgd, teacher=te).load_weights(w0)
    enc0 = pw2.engine.deconv(mel, 'iaf_share').clone()
    tr2 = StudentTrainer(pw2, w0, lr=LR_A, upsampler=False, seed=SEED0)
    assert tr2.scopes == [] and len(tr2.p) == 1
    out2 = tr2.step(inputs, noise=noise)
    assert torch.equal(out2['loss'], first['loss'])
    assert torch.equal(pw2.engine.deconv(mel, 'iaf_share'), enc0)
    w2 = tr2.weights()
    assert sorted(w2) == sorted(w0)
    same = {n: np.array_equal(w2[n], np.asarray(w0[n], np.float32).reshape(w2[n].shape)) for n in w0}
    assert all(same[n] for n in w0 if '/trans_conv_' in n) and not same['iaf_1/start_conv/W'] and not same['iaf_2/out1/W']
    pw2.engine.close()
    te.engine.close()


def test_trainer_private_stacks():
    """S2 (gauss, one stack per flow) under the golden small Gauss teacher: one step, per-flow stacks in weights()"""
    import torch
    from oracle import wavenet_np as O
    import distill_oracle64 as D
    from nsynth_wavenet_amd.train import StudentTrainer
    from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    B, F, T = SHAPES['S2']
    te_cfg, te_seed, te_init = D.golden_case(np.load(G.GOLD), 'gauss')[1]
    te = Wavenet(te_cfg).load_weights(O.synth_weights(O.HP(te_cfg), 'teacher', seed=te_seed, init=te_init))
    cfgd = dict(S.S2, power_loss_factor=1.0)
    _, w0 = G._weights('S2')
    pw = ParallelWavenet(cfgd, teacher=te).load_weights(w0)
    inputs, noise = _batch(B, F, T)
    tr = StudentTrainer(pw, w0, lr=LR_A, seed=SEED0)
    assert tr.scopes == ['iaf_1', 'iaf_2'] and len(tr.p) == 3
    out = tr.step(inputs, noise=noise)
    assert bool(torch.isfinite(out['loss'])) and float(out['grad_norm']) > 0
    w = tr.weights()
    assert sorted(w) == sorted(w0)
    for scope in tr.scopes:
        n = scope + '/trans_conv_2/kernel'
        assert w[n].shape == np.asarray(w0[n]).shape and not np.array_equal(w[n], w0[n])
    fresh = ParallelWavenet(cfgd, teacher=te).load_weights(w)
    _same_losses(pw.loss_and_weight_grads(inputs, seed=9, noise=noise), fresh.loss_and_weight_grads(inputs, seed=9, noise=noise), 'S2')
    for scope in tr.scopes:
        assert torch.equal(pw.engine.deconv(inputs['mel'], scope), fresh.engine.deconv(inputs['mel'], scope))
    fresh.engine.close()
    pw.engine.close()
    te.engine.close()
