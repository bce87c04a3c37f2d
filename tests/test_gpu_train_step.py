"""GPU tests of the teacher's training step on the device: the optimiser kernels (wn_grad_sumsq,
wn_adam_ema_step), the in-place re-pack wn_teacher_set_weights behind Engine.teacher_set_weights, and train.TeacherTrainer.
The models are the small golden teacher of tests/golden/ref_distill.npz (width 128, skip 64, 7 layers), its copy with
deconv_width 256 (the 'wide' model of tests/test_gpu_deconv_backward.py: phase-group pack and fp32 frame-axis table) and
the small one under Engine(precision='f32').

Optimiser bars (one call against tests/adam_oracle64.py, from the number of fp32 roundings, not tuned): with g' the clipped
gradient and u the applied update,
    |m - m64| <= 2^-22 (|beta1 m| + |(1 - beta1) g'|),    |v - v64| <= 2^-22 (|beta2 v| + |(1 - beta2) g'^2|),
    |p - p64| <= 2^-23 |p64| + 2^-20 |u64|,               |ema - ema64| <= 2^-22 (|ema64| + |p64|).
Measured on MI355X (largest error / bar over all cases): m 0.25, v 0.25, p 0.50, ema 0.26 -- the kernel forms each
element in double and rounds every stored value once.

The re-pack is held to bit equality (torch.equal) with a fresh handle loaded from the same values."""
import json

import numpy as np
import pytest

import adam_oracle64 as A
import distill_oracle64 as D
import test_gpu_deconv_backward as TD
import test_gpu_teacher_shapes as TS

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------
# 1. optimiser arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def _state(n, seed):
    rs = np.random.RandomState(seed)
    p = rs.standard_normal(n).astype(np.float32)
    g = rs.standard_normal(n).astype(np.float32)
    m = (0.1 * rs.standard_normal(n)).astype(np.float32)
    v = (0.05 * rs.standard_normal(n) ** 2).astype(np.float32)
    zero = rs.uniform(size=n) < 0.25
    if n > 1:
        zero[0] = True
    g[zero] = 0.0
    v[zero] = 0.0                                   # exact zeros where the gradient is zero
    ema = (p + 0.01 * rs.standard_normal(n)).astype(np.float32)
    return p, g, m, v, ema


@pytest.mark.parametrize('with_ema', [True, False], ids=['ema', 'noema'])
@pytest.mark.parametrize('clip', [None, 'above', 'below'])
@pytest.mark.parametrize('t', [1, 10000])
@pytest.mark.parametrize('n', [1, 257, 4099])
def test_adam_ema_step_against_the_float64_oracle(n, t, clip, with_ema):
    import torch
    from nsynth_wavenet_amd.engine import adam_ema_step, grad_sumsq
    p, g, m, v, ema = _state(n, 7 * n + t)
    if n == 1:
        g[0], v[0] = np.float32(0.7), np.float32(0.01)      # the one element has a gradient
    f32 = lambda x: float(np.float32(x))
    b1, b2, eps = f32(0.9), f32(0.999), f32(1e-8)
    lr_t = f32(A.lr_t(1e-3, 0.9, 0.999, t))
    dec = f32(A.ema_decay(0.9999, t - 1))
    dev = {k: torch.as_tensor(a.copy()).cuda() for k, a in (('p', p), ('g', g), ('m', m), ('v', v), ('ema', ema))}
    sumsq, clip_norm, ss = None, 1.0, None
    if clip is not None:
        sumsq = grad_sumsq(dev['g'])
        ss = float(sumsq.cpu()[0])
        assert abs(ss - float((g.astype(np.float64) ** 2).sum())) <= n * 2.0 ** -52 * ss
        clip_norm = f32(np.sqrt(ss) * (0.25 if clip == 'above' else 4.0))
    adam_ema_step(dev['p'], dev['g'], dev['m'], dev['v'], dev['ema'] if with_ema else None, lr_t, b1, b2, eps, dec,
                  sumsq=sumsq, clip_norm=clip_norm)
    ref = A.adam_ema_step(p, g, m, v, ema if with_ema else None, lr_t, b1, b2, eps, dec, sumsq=ss if clip else None,
                          clip_norm=clip_norm)
    got = {k: dev[k].cpu().numpy().astype(np.float64) for k in dev}
    assert np.array_equal(got['g'], g.astype(np.float64)), 'the gradient is read only'
    gh = ref['g']
    bars = {'m': 2.0 ** -22 * (np.abs(b1 * m.astype(np.float64)) + np.abs((1.0 - b1) * gh)),
            'v': 2.0 ** -22 * (np.abs(b2 * v.astype(np.float64)) + np.abs((1.0 - b2) * gh * gh)),
            'p': 2.0 ** -23 * np.abs(ref['p']) + 2.0 ** -20 * np.abs(ref['u'])}
    if with_ema:
        bars['ema'] = 2.0 ** -22 * (np.abs(ref['ema']) + np.abs(ref['p']))
    else:
        assert np.array_equal(got['ema'], ema.astype(np.float64)), 'no shadow was passed'
    for k in sorted(bars):
        err = np.abs(got[k] - ref[k])
        ratio = float(np.max(np.where(bars[k] > 0, err / np.where(bars[k] > 0, bars[k], 1.0), np.where(err > 0, np.inf, 0.0))))
        print('n {} t {} clip {} {}: max |x - x64| = {:.3e}, largest error / bar = {:.3f}'.format(n, t, clip, k, float(err.max()), ratio))
    for k in sorted(bars):
        assert np.all(np.isfinite(got[k])), k
        assert np.all(np.abs(got[k] - ref[k]) <= bars[k]), k
    if clip == 'below':
        assert float(np.abs(gh - g).max()) == 0.0


@pytest.mark.parametrize('n', [1, 257, 4099, 70001])
def test_grad_sumsq(n):
    """within n 2^-52 relative of float64, identical bits on a repeated call, accumulate adds; 70001 takes several blocks"""
    import torch
    from nsynth_wavenet_amd.engine import grad_sumsq
    g = np.random.RandomState(n).standard_normal(n).astype(np.float32)
    G = torch.as_tensor(g).cuda()
    want = float((g.astype(np.float64) ** 2).sum())
    a = grad_sumsq(G)
    b = grad_sumsq(G)
    got = float(a.cpu()[0])
    print('n {}: sumsq {:.17g}, float64 {:.17g}, relative error {:.2e}'.format(n, got, want, abs(got - want) / want))
    assert torch.equal(a, b)
    assert abs(got - want) <= n * 2.0 ** -52 * want
    acc = torch.full((1,), 3.5, dtype=torch.float64, device='cuda')
    grad_sumsq(G, acc, accumulate=True)
    assert float(acc.cpu()[0]) == 3.5 + got
    grad_sumsq(G, acc)
    assert torch.equal(acc, a)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the re-pack is the fresh handle's pack
# ---------------------------------------------------------------------------------------------------------------------
VARIANTS = {'small': ({}, None), 'wide': ({'deconv_width': 256}, None), 'small-f32': ({}, 'f32')}


def _w1(w0, seed=77):
    """w0 with every scale path moved: one kernel times 8 and one times 2^-6 (pick_scale changes bucket; small values get
    subnormal lo halves), one all zero (scale 1), a random perturbation elsewhere"""
    rs = np.random.RandomState(seed)
    w1 = {}
    for k in sorted(w0):
        a = np.asarray(w0[k], np.float32)
        w1[k] = (a * (1.0 + 0.05 * rs.standard_normal(a.shape)) + 0.01 * rs.standard_normal(a.shape)).astype(np.float32)
    w1['mel_cond_3/W'] = (w1['mel_cond_3/W'] * np.float32(8)).astype(np.float32)
    w1['dilated_conv_5/W'] = (w1['dilated_conv_5/W'] * np.float32(2.0 ** -6)).astype(np.float32)
    w1['mel_cond_5/W'] = (w1['mel_cond_5/W'] * np.float32(2.0 ** -6)).astype(np.float32)
    w1['trans_conv_2/kernel'] = (w1['trans_conv_2/kernel'] * np.float32(8)).astype(np.float32)
    w1['trans_conv_1/kernel'] = (w1['trans_conv_1/kernel'] * np.float32(2.0 ** -6)).astype(np.float32)
    w1['skip_start/W'] = np.zeros_like(w1['skip_start/W'])
    return w1


def _flat(table, w):
    import torch
    name, off, shape = table[-1]
    flat = np.zeros(off + int(np.prod(shape)), np.float32)
    for name, off, shape in table:
        flat[off:off + int(np.prod(shape))] = np.asarray(w[name], np.float32).reshape(-1)
    return torch.as_tensor(flat).cuda()


def _net(cfgd, w, precision=None):
    from nsynth_wavenet_amd.engine import Engine
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    eng = Engine(cfgd, kind='teacher', precision=precision) if precision else None
    return Wavenet(cfgd, engine=eng).load_weights(w)


class _Pair(object):
    """handle A loaded from w0 and re-packed with w1, and a fresh handle B loaded from w1"""

    def __init__(self, R, tag, variants=None):
        from oracle import wavenet_np as O
        over, self.precision = (VARIANTS if variants is None else variants)[tag]
        cfgd, seed, init = D.golden_case(R, 'mol')[1]
        self.cfgd = dict(json.loads(json.dumps(cfgd)), **over)
        self.w0 = O.synth_weights(O.HP(self.cfgd), 'teacher', seed=seed, init=init)
        self.w1 = _w1(self.w0)
        self.a = _net(self.cfgd, self.w0, self.precision)
        self.b = _net(self.cfgd, self.w1, self.precision)

    def close(self):
        self.a.engine.close()
        self.b.engine.close()


@pytest.fixture(scope='module')
def R():
    return np.load(TS.GOLD)


def _outputs(net, cfgd, shape=(3, 2, 260), seeds=None):
    """everything the handle's packs feed, on fixed inputs: {name: device tensor}"""
    import torch
    eng = net.engine
    mel, x = TS._inputs(shape[1], shape[2], seeds or TS.ROW_SEEDS[shape])
    X, MEL = torch.as_tensor(x).cuda(), torch.as_tensor(mel).cuda()
    out = {'teacher_forward': eng.teacher_forward(X, MEL), 'deconv': eng.deconv(MEL)}
    rs = np.random.RandomState(31)
    Cd = int(cfgd['deconv_width'])
    for B in (3, 5):                                 # the step's GEMV form (B < 4) and its batched form
        enc = torch.as_tensor(rs.standard_normal([B, 12, Cd]).astype(np.float32)).cuda()
        forced = torch.as_tensor(rs.uniform(-0.9, 0.9, [B, 12]).astype(np.float32)).cuda()
        r = eng.ar_generate(enc, seed=5, forced_wav=forced, want_out=True)
        out['ar_generate/B%d/out_params' % B] = r['out_params']
        out['ar_generate/B%d/idx' % B] = r['idx']
        if B == 3:
            for k, v in eng.ar_cond_vars(enc).items():
                out['ar_cond_vars/' + k] = v
    res = net.loss_and_weight_grads({'wav': X, 'mel': MEL}, upsampler=True)
    out['loss'], out['log_probs'], out['d_encoding'] = res['loss'], res['log_probs'], res['d_encoding']
    out['flat_grads'], out['flat_upsampler_grads'] = res['flat_grads'], res['flat_upsampler_grads']
    for k, v in res['grads'].items():
        out['grads/' + k] = v
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize('tag', sorted(VARIANTS))
def test_repack_equals_a_fresh_handle(R, tag):
    """teacher_set_weights(w1) on a handle loaded from w0 against a fresh handle loaded from w1: identical bits of
    teacher_forward at (3, 2, 260), ar_generate (forced, want_out) on both sides of the GEMV / batched switch, ar_cond_vars,
    deconv and every tensor of loss_and_weight_grads(upsampler=True).  Then up_params=None, in the direction this handle allows
    after the first call: the stack alone is set back to w0, so the upsampler's outputs stay those of w1 while the stack follows
    w0 -- compared with a fresh handle loaded from that mixture."""
    _repack_check(_Pair(R, tag))


def _repack_check(pr, shape=(3, 2, 260), seeds=None):
    """the body of test_repack_equals_a_fresh_handle on a pair of handles, with _outputs run at `shape`"""
    import torch
    _plain = globals()['_outputs']

    def _outputs(net, cfgd):
        return _plain(net, cfgd, shape, seeds)
    try:
        ea = pr.a.engine
        before = _outputs(pr.a, pr.cfgd)
        ea.teacher_set_weights(_flat(ea.teacher_grad_table(), pr.w1), _flat(ea.deconv_grad_table(''), pr.w1))
        got, want = _outputs(pr.a, pr.cfgd), _outputs(pr.b, pr.cfgd)
        assert sorted(got) == sorted(want)
        bad = [k for k in sorted(want) if not torch.equal(got[k], want[k])]
        for k in sorted(want):
            assert bool(torch.isfinite(want[k].double()).all()), k
        assert not bad, bad
        assert not torch.equal(before['teacher_forward'], got['teacher_forward']) and not torch.equal(before['deconv'], got['deconv'])
        # the stack alone goes back to w0: a mixed model
        ea.teacher_set_weights(_flat(ea.teacher_grad_table(), pr.w0), None)
        mixed = dict(pr.w0)
        mixed.update({k: v for k, v in pr.w1.items() if k.startswith('trans_conv_')})
        nm = _net(pr.cfgd, mixed, pr.precision)
        got, want = _outputs(pr.a, pr.cfgd), _outputs(nm, pr.cfgd)
        nm.engine.close()
        bad = [k for k in sorted(want) if not torch.equal(got[k], want[k])]
        assert not bad, bad
        assert torch.equal(got['deconv'], _outputs(pr.b, pr.cfgd)['deconv'])
    finally:
        pr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. contract
# ---------------------------------------------------------------------------------------------------------------------
def test_tapes_written_before_the_repack_are_refused(R):
    import torch
    pr = _Pair(R, 'small')
    try:
        eng = pr.a.engine
        shape = (2, 2, 252)
        mel, x = TS._inputs(shape[1], shape[2], TS.ROW_SEEDS[shape])
        X, MEL = torch.as_tensor(x).cuda(), torch.as_tensor(mel).cuda()
        out, tape = eng.teacher_forward_train_tape(X, MEL)
        g = torch.ones_like(out)
        eng.teacher_backward_weights(tape, g, n_frames=shape[1])          # accepted before
        eng.teacher_set_weights(_flat(eng.teacher_grad_table(), pr.w1), None)
        with pytest.raises(ValueError, match='the tape was not written by'):
            eng.teacher_backward_weights(tape, g, n_frames=shape[1])
        with pytest.raises(ValueError, match='the tape was not written by'):
            eng.teacher_backward_input(tape, g)
        out, tape = eng.teacher_forward_train_tape(X, MEL)                # a new tape works
        eng.teacher_backward_weights(tape, g)
    finally:
        pr.close()


def test_refusals(R):
    import torch
    from nsynth_wavenet_amd import config as cfg, weights as wts
    from nsynth_wavenet_amd.engine import Engine, _ptr
    pr = _Pair(R, 'small')
    try:
        eng = pr.a.engine
        P, U = _flat(eng.teacher_grad_table(), pr.w1), _flat(eng.deconv_grad_table(''), pr.w1)
        with pytest.raises(ValueError, match='params holds'):
            eng.teacher_set_weights(P[:-1].clone(), U)
        with pytest.raises(ValueError, match='up_params holds'):
            eng.teacher_set_weights(P, torch.cat([U, U[:1]]))
        ws = torch.empty(256, dtype=torch.uint8, device='cuda')
        rc = eng.lib.wn_teacher_set_weights(eng._h, _ptr(P), P.numel(), _ptr(U), U.numel(), _ptr(ws), 16, eng._stream())
        assert rc == -22 and b'workspace' in eng.lib.wn_last_error(None)
        assert int(eng.lib.wn_teacher_set_weights_workspace_bytes(eng._h)) >= 256

        def variant(**over):
            cfgd = dict(json.loads(json.dumps(pr.cfgd)), **over)
            return cfgd, wts.synthetic_weights(cfg.load_hparams(cfgd), 'teacher', seed=3, init='unit')
        # not finalized
        e2 = Engine(pr.cfgd, kind='teacher')
        with pytest.raises(RuntimeError, match='call wn_finalize first'):
            e2.teacher_set_weights(P, U)
        e2.close()
        # handles without a parameter layout (teacher widths that are no multiple of 64 are refused by wn_create itself, so
        # no such handle exists: a ce head wider than 64 is what leaves the transposed packs out)
        for over in ({'use_mu_law': True}, {'loss_type': 'ce', 'use_mu_law': True}, {'use_weight_norm': True}):
            cfgd, w = variant(**over)
            e3 = Engine(cfgd, kind='teacher').load_weights(w)
            assert int(e3.lib.wn_teacher_set_weights_workspace_bytes(e3._h)) == 0
            with pytest.raises(ValueError, match='no parameter layout'):
                e3.teacher_set_weights(P, None)
            e3.close()
        # resize-conv upsampler: the stack alone is accepted, up_params are not
        cfgd, w = variant(use_resize_conv=True)
        e4 = Engine(cfgd, kind='teacher').load_weights(w)
        P4 = _flat(e4.teacher_grad_table(), w)
        with pytest.raises(ValueError, match='use_resize_conv'):
            e4.teacher_set_weights(P4, U)
        e4.teacher_set_weights(P4, None)
        e4.close()
        # a student handle
        st_cfg = D.golden_case(R, 'mol')[0]
        e5 = Engine(st_cfg, kind='student').load_weights(wts.synthetic_weights(cfg.load_hparams(st_cfg), 'student', seed=3, init='unit'))
        with pytest.raises(ValueError, match='student handle'):
            e5.teacher_set_weights(P, None)
        e5.close()
    finally:
        pr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. trainer
# ---------------------------------------------------------------------------------------------------------------------
TRAIN_SHAPE = (2, 3, 512)
TRAIN_LR = 1e-3
TRAIN_SCHEDULE = {0: TRAIN_LR, 2: 0.5 * TRAIN_LR}
TRAIN_LRS = [TRAIN_LR, TRAIN_LR, 0.5 * TRAIN_LR]      # what the schedule gives for steps 1, 2, 3
TRAIN_K = len(TRAIN_LRS)


def _oracle_adam(cfgd, seed, init, x, mel, lrs):
    """one step of tests/adam_oracle64.py per rate in lrs on the float64 oracle's loss and gradient: the losses before every
    step and after the last"""
    import torch
    thp, w64 = D.teacher_weights(cfgd, seed, init)
    names = sorted(w64)
    w = {k: v.clone() for k, v in w64.items()}
    m = {k: np.zeros(tuple(v.shape)) for k, v in w.items()}
    v2 = {k: np.zeros(tuple(v.shape)) for k, v in w.items()}
    losses, K = [], len(lrs)
    for t in range(1, K + 2):
        leaves = {k: w[k].clone().requires_grad_(True) for k in names}
        L = TD._oracle_loss(leaves, thp, cfgd['deconv_config'], cfgd['upsample_act'], x, mel, 'mol')
        losses.append(float(L.detach()))
        if t > K:
            break
        gs = torch.autograd.grad(L, [leaves[k] for k in names], allow_unused=True)
        for k, g in zip(names, gs):
            g = torch.zeros_like(w[k]) if g is None else g
            r = A.adam_ema_step(w[k].numpy(), g.numpy(), m[k], v2[k], None, A.lr_t(lrs[t - 1], 0.9, 0.999, t), 0.9, 0.999, 1e-8, 0.0)
            w[k], m[k], v2[k] = torch.as_tensor(r['p']), r['m'], r['v']
    return losses


def test_trainer(R):
    """TeacherTrainer on one fixed batch at (2, 3, 512).  K = 3 steps under the schedule {0: 1e-3, 2: 5e-4} (rates 1e-3, 1e-3,
    5e-4) were chosen on the float64 oracle alone (tests/distill_oracle64.py with tests/adam_oracle64.py, on the CPU; its
    losses there: 12.042, 11.615, 11.482, then 11.3 after the third step): the test repeats that run with the same rates and
    asserts that the oracle's own loss falls by at least 1e-3 over the K steps (as test_descent_through_the_public_api requires of its step)
    before it asks the engine's loss to be below its first."""
    import torch
    from oracle import wavenet_np as O
    from nsynth_wavenet_amd.train import TeacherTrainer
    cfgd, seed, init = D.golden_case(R, 'mol')[1]
    B, F, T = TRAIN_SHAPE
    mel, x = TS._inputs(F, T, TS.ROW_SEEDS[TRAIN_SHAPE])
    ora = _oracle_adam(cfgd, seed, init, x, mel, TRAIN_LRS)
    print('oracle losses', ora)
    assert ora[0] - ora[-1] >= 1e-3
    w0 = O.synth_weights(O.HP(cfgd), 'teacher', seed=seed, init=init)
    net = _net(cfgd, w0)
    X, MEL = torch.as_tensor(x).cuda(), torch.as_tensor(mel).cuda()
    batch = {'wav': X, 'mel': MEL}

    def loss_of(n):
        with torch.no_grad():
            return n.calculate_loss(n.feed_forward(batch))
    first = loss_of(net)
    ref = net.loss_and_weight_grads(batch, upsampler=True)
    norm64 = float(np.sqrt(float((ref['flat_grads'].double() ** 2).sum()) + float((ref['flat_upsampler_grads'].double() ** 2).sum())))
    tr = TeacherTrainer(net, w0, lr=TRAIN_SCHEDULE)
    losses, lr_ts = [], []
    for k in range(TRAIN_K):
        out = tr.step(batch)
        losses.append(float(out['loss']))
        lr_ts.append(tr.lr_t)
        if k == 0:
            assert torch.equal(out['loss'], first['loss']) and torch.equal(out['log_probs'], first['log_probs'])
            gn = float(out['grad_norm'])
            print('grad_norm {:.9e}, float64 norm of the engine gradients {:.9e}'.format(gn, norm64))
            assert abs(gn - norm64) <= 1e-6 * norm64
            # the shadow after step 1: w0 - (1 - 0.1) (w0 - w_1), within the EMA bar
            w_1, e_1 = tr.weights(), tr.weights(ema=True)
            for name in sorted(w0):
                a0, a1 = np.asarray(w0[name], np.float64).reshape(w_1[name].shape), w_1[name].astype(np.float64)
                want = a0 - (1.0 - 0.1) * (a0 - a1)
                assert np.all(np.abs(e_1[name] - want) <= 2.0 ** -22 * (np.abs(want) + np.abs(a1))), name
        # a fresh handle loaded from the trainer's weights scores the batch with the same bits
        fresh = _net(cfgd, tr.weights())
        a, b = loss_of(net), loss_of(fresh)
        fresh.engine.close()
        assert torch.equal(a['loss'], b['loss']) and torch.equal(a['log_probs'], b['log_probs']), k
    final = float(loss_of(net)['loss'])
    print('engine losses', losses, 'after', final)
    assert final < losses[0]
    # the schedule {0: a, 2: b}: b from the third step on, seen through lr_t
    want = [np.float32(A.lr_t(lr, 0.9, 0.999, t + 1)) for t, lr in enumerate(TRAIN_LRS)]
    assert tr.lr_history == TRAIN_LRS and [np.float32(v) for v in lr_ts] == want
    # the shadows packed into the handle: what a fresh handle loaded from weights(ema=True) computes
    tr.use_ema()
    fresh = _net(cfgd, tr.weights(ema=True))
    a, b = loss_of(net), loss_of(fresh)
    assert torch.equal(a['loss'], b['loss']) and torch.equal(a['log_probs'], b['log_probs'])
    assert torch.equal(net.engine.deconv(MEL), fresh.engine.deconv(MEL))
    fresh.engine.close()
    net.engine.close()
