"""GPU tests of the student's weight gradients: Engine.iaf_forward_train_tape / iaf_backward_weights
(csrc/wn_iaf_train.hip on the GEMM kernels of the teacher's training passes) and ParallelWavenet.loss_and_weight_grads, against
the float64 autograd oracle tests/student_grad_oracle64.py (held to StudentRef and to central differences by
tests/test_student_grad_oracle.py).

Models: S1 (width 64: the half-tile guard of the gate's reverse epilogue, a dilation cycle that wraps, ragged tiles, a shared
stack), S2 (width 128: two m-tiles, the unguarded epilogue, a layer whose taps read only the left pad, private stacks) and the
shipped parallel_wavenet.json.  Bars: values 2e-5 max(1, max |ref|) (tests/test_gpu_iaf.py's), gradients
max |g - g64| <= 1e-4 max |g64| per tensor."""
import ctypes
import os

import numpy as np
import pytest

import distill_oracle64 as D
import student_grad_oracle64 as S
from conftest import load_json

pytestmark = pytest.mark.gpu
TOL = 1e-4
VTOL = 2e-5
SEED = 11           # chosen on the CPU: the oracle has no clamp within 1e-6 of a bound and < 1e-4 near-tie mask elements
CASES = {'S1a': ('S1', (2, 25, 200)),       # one partial 256-column tile
         'S1b': ('S1', (3, 33, 264)),       # a second, ragged tile
         'S2': ('S2', (1, 64, 512)),        # the layer of dilation 512 runs
         'S3': ('S3', (1, 6, 1024))}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_distill.npz')


def _cfg(model):
    return {'S1': S.S1, 'S2': S.S2}.get(model) or load_json('parallel_wavenet.json')


def _np(t):
    return t.detach().cpu().numpy()


_ENG, _ORA = {}, {}


def _new_engine(cfgd, w):
    from nsynth_wavenet_amd.engine import Engine
    return Engine(cfgd, kind='student').load_weights(w)


def _engine(model):
    """one engine per model, shared by the tests"""
    if model not in _ENG:
        _ENG[model] = _new_engine(_cfg(model), _weights(model)[1])
    return _ENG[model]


def _weights(model, seed=SEED):
    from oracle import wavenet_np as O
    hp = O.HP(_cfg(model))
    return hp, O.synth_weights(hp, 'student', seed=seed, init='unit')


def _oracle(tag):
    """the float64 oracle of one case on dense random cotangents, computed once"""
    if tag not in _ORA:
        model, (B, F, T) = CASES[tag]
        hp, w = _weights(model)
        mel, noise, cot = S.case_inputs(B, F, T, seed=SEED + 100)
        _ORA[tag] = (hp, w, mel, noise, cot, S.StudentGrad64(w, hp).grads(mel, noise, *cot))
    return _ORA[tag]


def _check_oracle_is_clear(ref):
    """in float64, before any comparison: the ReLU masks and the clamps are not at a tie"""
    assert S.near_tie_fraction(ref['aux']) <= 1e-4
    assert S.clamps_inactive(ref['aux'])


def _compare_values(got, ref, what):
    for k in ('x', 'mean_tot', 'scale_tot'):
        r = ref[k]
        e = np.abs(_np(got[k]).astype(np.float64) - r).max()
        print('{} {:10s} max |v - v64| = {:.2e} (max |v64| {:.2e})'.format(what, k, e, np.abs(r).max()))
        assert e <= VTOL * max(1.0, np.abs(r).max()), (what, k, e)


def _compare_grads(res, ref, what, exact_zero=()):
    worst = 0.0
    for n, r in ref['grads'].items():
        g = _np(res['grads'][n]).astype(np.float64)
        assert g.shape == r.shape, n
        e = np.abs(g - r).max() / max(np.abs(r).max(), 1e-300)
        worst = max(worst, e)
        if n in exact_zero:
            assert np.all(g[r == 0] == 0), n
            continue
        assert e <= TOL, (what, n, e)
    d, rd = _np(res['d_encoding']).astype(np.float64), ref['d_encoding']
    assert d.shape == rd.shape
    ed = max(np.abs(d[s] - rd[s]).max() / np.abs(rd[s]).max() for s in range(rd.shape[0]))
    print('{}: worst gradient tensor max |g - g64| / max |g64| = {:.2e}, d_encoding {:.2e}'.format(what, worst, ed))
    assert ed <= TOL, (what, 'd_encoding', ed)
    assert np.all(d[rd == 0] == 0)                    # exactly zero outside the centre crop
    return worst, ed


@pytest.mark.parametrize('tag', sorted(CASES))
def test_values_and_gradients(tag):
    """tape forward against the oracle and against iaf_generate on the same noise; every gradient tensor and d_encoding"""
    model, (B, F, T) = CASES[tag]
    hp, w, mel, noise, cot, ref = _oracle(tag)
    _check_oracle_is_clear(ref)
    eng = _engine(model)
    assert eng.iaf_length(F) == T
    ff, tape = eng.iaf_forward_train_tape(mel, noise=noise)
    _compare_values(ff, ref['values'], tag + ' tape forward')
    gen = eng.iaf_generate(mel, noise, want=('x', 'mean_tot', 'scale_tot'))
    _compare_values(ff, {k: _np(v).astype(np.float64) for k, v in gen.items()}, tag + ' against iaf_generate')
    res = eng.iaf_backward_weights(tape, *cot)
    assert [n for n, _, _ in eng.iaf_grad_table()] == S.variable_names(hp) == list(ref['grads'])
    n_stacks = 1 if model != 'S2' else 2
    TE = F * eng.frame_shift
    assert tuple(res['d_encoding'].shape) == (n_stacks, B, TE, hp.deconv_width)
    c0 = (TE - T) // 2
    d = _np(res['d_encoding'])
    assert np.all(d[:, :, :c0] == 0) and np.all(d[:, :, c0 + T:] == 0)
    # S2: dilation 512 at T = 512 -- taps 0 and 1 of flow 1's tenth layer read only the left pad
    name = 'iaf_1/dilated_conv_10/W'
    if model == 'S2':
        assert np.all(ref['grads'][name][0, :2] == 0) and np.abs(ref['grads'][name][0, 2]).max() > 0
        assert np.all(_np(res['grads'][name])[0, :2] == 0)
        tap2 = np.abs(_np(res['grads'][name])[0, 2] - ref['grads'][name][0, 2]).max() / np.abs(ref['grads'][name]).max()
        assert tap2 <= TOL
    _compare_grads(res, ref, tag)
    assert eng.iaf_train_tape_bytes(B, F) == tape.numel()
    if tag == 'S1a':            # handed only a seed, the draw is iaf_generate's
        import torch
        drawn, _ = eng.iaf_forward_train_tape(mel, seed=7)
        gen7 = eng.iaf_generate(mel, seed=7, want=('rand_input', 'x'))
        assert torch.equal(drawn['rand_input'], gen7['rand_input'])
        _compare_values(drawn, {'x': _np(gen7['x']).astype(np.float64), 'mean_tot': _np(drawn['mean_tot']).astype(np.float64),
                                'scale_tot': _np(drawn['scale_tot']).astype(np.float64)}, tag + ' seeded draw')
    print('{}: tape {} bytes = {:.0f} per sample'.format(tag, tape.numel(), tape.numel() / float(B * T)))


def test_single_nonzero_cotangent():
    """S1: one nonzero at t = T - 1 of row 0 in each cotangent (the last valid column of a partial tile)"""
    model, (B, F, T) = CASES['S1a']
    hp, w, mel, noise, _, _ = _oracle('S1a')
    cot = [np.zeros((B, T), np.float32) for _ in range(3)]
    for i, v in enumerate((0.75, -1.5, 2.0)):
        cot[i][0, T - 1] = v
    ref = S.StudentGrad64(w, hp).grads(mel, noise, *cot)
    _check_oracle_is_clear(ref)
    eng = _engine(model)
    _, tape = eng.iaf_forward_train_tape(mel, noise=noise)
    _compare_grads(eng.iaf_backward_weights(tape, *cot), ref, 'S1a single nonzero')


def test_clamps_active():
    """S1.  (a) flow 1's out2_scale/biases so low that every scale of that flow sits on the e^-9 bound: its out2_scale
    gradients are exactly zero, the rest meets the bar.  (b) prod_k scale_k > e^7 on every element: d_scale_tot and d_x's
    share through the noise reach no variable."""
    from oracle import wavenet_np as O
    from oracle.torch_ref import EXP_7, EXP_M9
    B, F, T = CASES['S1a'][1]
    hp, w0 = _weights('S1')
    mel, noise, cot = S.case_inputs(B, F, T, seed=SEED + 100)
    # (a)
    w = dict(w0)
    w['iaf_1/out2_scale/biases'] = np.full((1,), -40.0, np.float32)
    ref = S.StudentGrad64(w, hp).grads(mel, noise, *cot)
    assert np.all(ref['aux']['softplus'][0] < EXP_M9 * (1 - 1e-6)) and np.all(ref['aux']['scales'][0] == EXP_M9)
    assert S.near_tie_fraction(ref['aux']) <= 1e-4
    eng = _new_engine(S.S1, w)
    ff, tape = eng.iaf_forward_train_tape(mel, noise=noise)
    _compare_values(ff, ref['values'], 'clamp e^-9')
    res = eng.iaf_backward_weights(tape, *cot)
    for n in ('iaf_1/out2_scale/W', 'iaf_1/out2_scale/biases'):
        assert np.all(ref['grads'][n] == 0) and np.all(_np(res['grads'][n]) == 0), n
    _compare_grads(res, ref, 'clamp e^-9', exact_zero=('iaf_1/out2_scale/W', 'iaf_1/out2_scale/biases'))
    eng.close()
    # (b)
    w = dict(w0)
    w['iaf_1/out2_scale/biases'] = np.full((1,), 12.0, np.float32)
    w['iaf_2/out2_scale/biases'] = np.full((1,), 600.0, np.float32)
    ref = S.StudentGrad64(w, hp).grads(mel, noise, *cot)
    assert np.all(ref['aux']['scale_prod'] > EXP_7 * (1 + 1e-6)) and np.all(ref['values']['scale_tot'] == EXP_7)
    assert S.near_tie_fraction(ref['aux']) <= 1e-4
    for sp in ref['aux']['softplus']:
        assert np.all(sp > EXP_M9 * (1 + 1e-6)) and np.all(sp < EXP_7 * (1 - 1e-6))
    eng = _new_engine(S.S1, w)
    ff, tape = eng.iaf_forward_train_tape(mel, noise=noise)
    _compare_values(ff, ref['values'], 'clamp e^7')
    res = eng.iaf_backward_weights(tape, *cot)
    _compare_grads(res, ref, 'clamp e^7')
    # the same bits from the cotangent of mean_tot alone: nothing of d_scale_tot or of d_x noise arrives anywhere
    only_mean = eng.iaf_backward_weights(tape, np.zeros_like(cot[0]), cot[1] + cot[0], np.zeros_like(cot[2]))
    import torch
    assert torch.equal(res['flat_grads'], only_mean['flat_grads']) and torch.equal(res['d_encoding'], only_mean['d_encoding'])
    eng.close()


def _raw(eng, mel, noise, cot, fill, B, F, T):
    """both calls through the C ABI on buffers pre-filled with `fill`: the outputs' bytes"""
    import torch
    lib, h = eng.lib, eng._h
    dev = eng.device
    buf = lambda n: torch.full((max(int(n), 256),), fill, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    mel, noise = eng._dev(mel), eng._dev(noise)
    cot = [eng._dev(c) for c in cot]
    tape, ws = buf(lib.wn_iaf_train_tape_bytes(h, B, F, T)), buf(lib.wn_iaf_train_workspace_bytes(h, B, F, T))
    out = [buf(B * T * 4) for _ in range(3)]
    st = eng._stream()
    eng._check(lib.wn_iaf_forward_train_tape(h, p(noise), p(mel), B, F, T, p(out[0]), p(out[1]), p(out[2]), p(tape),
                                             tape.numel(), p(ws), ws.numel(), st))
    n = int(lib.wn_iaf_grad_floats(h))
    grads, ws2 = buf(4 * n), buf(lib.wn_iaf_backward_weights_workspace_bytes(h, B, F, T))
    denc = buf(4 * B * F * eng.frame_shift * int(eng.hp.deconv_width) * eng.iaf_n_stacks())
    eng._check(lib.wn_iaf_backward_weights(h, p(tape), tape.numel(), p(cot[0]), p(cot[1]), p(cot[2]), B, F, T, p(grads), n,
                                           p(denc), p(ws2), ws2.numel(), st))
    torch.cuda.synchronize()
    return [t[:B * T * 4].clone() for t in out] + [grads[:4 * n].clone(), denc.clone()]


def test_prefilled_buffers_and_repeats():
    """S1 (2, 25, 200): tape, workspaces and output buffers pre-filled with 0x00, then 0xFF, then 0xFF again -- the same bits"""
    import torch
    B, F, T = CASES['S1a'][1]
    hp, w, mel, noise, cot, ref = _oracle('S1a')
    eng = _engine('S1')
    a, b, c = (_raw(eng, mel, noise, cot, fill, B, F, T) for fill in (0x00, 0xFF, 0xFF))
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(y, z)
    g = a[3].view(torch.float32)
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(a[4].view(torch.float32)).all())
    flat = np.concatenate([ref['grads'][n].ravel() for n in S.variable_names(hp)])
    assert np.abs(_np(g) - flat).max() <= TOL * np.abs(flat).max()


def _teacher_and_student():
    """S1 with the loss hparams of the golden distillation case, and that case's small MoL teacher"""
    from oracle import wavenet_np as O
    from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    R = np.load(GOLD)
    te_cfg, te_seed, te_init = D.golden_case(R, 'mol')[1]
    te = Wavenet(te_cfg).load_weights(O.synth_weights(O.HP(te_cfg), 'teacher', seed=te_seed, init=te_init))
    cfgd = dict(S.S1, num_samples=8, power_loss_factor=1.0, contrastive_loss_factor=0.3)
    _, w = _weights('S1')
    return ParallelWavenet(cfgd, teacher=te).load_weights(w), te, w


def test_public_chain():
    """ParallelWavenet.loss_and_weight_grads on S1 under the golden small teacher"""
    import torch
    B, F, T = CASES['S1a'][1]
    pw, te, w = _teacher_and_student()
    mel, noise, _ = S.case_inputs(B, F, T, seed=SEED + 100)
    rs = np.random.RandomState(3)
    inputs = {'mel': torch.as_tensor(mel).cuda(), 'mel_rand': torch.as_tensor(rs.uniform(0, 1, mel.shape).astype(np.float32)).cuda(),
              'wav': torch.as_tensor(rs.uniform(-0.5, 0.5, [B, T]).astype(np.float32)).cuda()}
    res = pw.loss_and_weight_grads(inputs, seed=5, noise=noise, upsampler=True)
    # the losses: the bits of the no-grad calculate_loss on the same forward values, noise and seeds ...
    eng = pw.engine
    ff, tape = eng.iaf_forward_train_tape(mel, noise=noise)
    with torch.no_grad():
        plain = pw.calculate_loss(dict(ff, mel=inputs['mel'], mel_rand=inputs['mel_rand'], wav=inputs['wav']), seed=5)
    assert sorted(plain) == sorted(k for k in res if k not in ('grads', 'flat_grads', 'd_encoding', 'flat_upsampler_grads'))
    for k in plain:
        assert torch.equal(plain[k], res[k]), k
    # ... and, the tape forward and the generation path being different kernels, close to the loss of feed_forward's values
    with torch.no_grad():
        gen = pw.calculate_loss(dict(pw.feed_forward(inputs, noise=noise), mel=inputs['mel'], mel_rand=inputs['mel_rand'],
                                     wav=inputs['wav']), seed=5)
    print('loss {:.9f} on the tape forward, {:.9f} on feed_forward'.format(float(res['loss']), float(gen['loss'])))
    # (the two forwards agree to 2e-5 max |ref| per element, test_values_and_gradients; the loss is a mean over B T of them)
    assert abs(float(res['loss']) - float(gen['loss'])) <= 1e-5 * max(1.0, abs(float(gen['loss'])))
    # 'grads': iaf_backward_weights applied to the .grads by hand
    leaves = {k: ff[k].detach().requires_grad_(True) for k in ('x', 'mean_tot', 'scale_tot')}
    pw.calculate_loss(dict(leaves, mel=inputs['mel'], mel_rand=inputs['mel_rand'], wav=inputs['wav']), seed=5)['loss'].backward()
    hand = eng.iaf_backward_weights(tape, leaves['x'].grad, leaves['mean_tot'].grad, leaves['scale_tot'].grad)
    assert torch.equal(hand['flat_grads'], res['flat_grads']) and torch.equal(hand['d_encoding'], res['d_encoding'])
    for n, g in hand['grads'].items():
        assert torch.equal(g, res['grads'][n]), n
    # the upsampler's variables: deconv_backward on d_encoding[0]
    up = eng.deconv_backward(inputs['mel'], res['d_encoding'][0], 'iaf_share')
    assert sorted(up['grads']) == sorted(n for n in res['grads'] if 'trans_conv' in n) and len(up['grads']) == 4
    for n, g in up['grads'].items():
        assert n.startswith('iaf_share/trans_conv_') and torch.equal(g, res['grads'][n]), n
    assert sorted(res['grads']) == sorted(w)
    assert float(res['flat_grads'].abs().max()) > 0 and bool(torch.isfinite(res['flat_grads']).all())
    without = pw.loss_and_weight_grads(inputs, seed=5, noise=noise, upsampler=False)
    assert torch.equal(without['flat_grads'], res['flat_grads']) and not any('trans_conv' in n for n in without['grads'])
    pw.engine.close()
    te.engine.close()


def test_descent_on_the_oracle():
    """A step of eps = 2^-6 along the engine's negative gradient lowers the float64 oracle's surrogate loss -- a fixed random
    linear functional of x, mean_tot, scale_tot -- by the first-order amount.  The functional's size is chosen on the oracle
    alone: the largest power of two at which the oracle's own gradient step stays within 5 % of eps |g|^2; the engine's step
    must then decrease the oracle's loss to within 10 % of the oracle's own decrease."""
    B, F, T = CASES['S1a'][1]
    hp, w, mel, noise, cot, _ = _oracle('S1a')
    ora = S.StudentGrad64(w, hp)
    eps = 2.0 ** -6
    alpha, dec64 = None, None
    for a in [2.0 ** -j for j in range(0, 24)]:
        c = [a * v for v in cot]
        g = ora.grads(mel, noise, *c)['grads']
        gg = sum(float((v ** 2).sum()) for v in g.values())
        L0 = ora.surrogate(mel, noise, c)
        dec = L0 - ora.surrogate(mel, noise, c, {n: np.asarray(w[n], np.float64) - eps * g[n] for n in g})
        if abs(dec - eps * gg) <= 0.05 * eps * gg:
            alpha, dec64 = a, dec
            break
    assert alpha is not None, 'no functional is in the linear regime at eps = 2^-6'
    c = [np.float32(alpha) * v for v in cot]
    eng = _engine('S1')
    _, tape = eng.iaf_forward_train_tape(mel, noise=noise)
    res = eng.iaf_backward_weights(tape, *c)
    L0 = ora.surrogate(mel, noise, c)
    dec = L0 - ora.surrogate(mel, noise, c, {n: np.asarray(w[n], np.float64) - eps * _np(res['grads'][n]).astype(np.float64)
                                             for n in ora.names})
    print('descent: alpha {:.3e}, oracle decrease {:.6e} with its own gradient, {:.6e} with the engine\'s'.format(alpha, dec64, dec))
    assert dec > 0 and abs(dec - dec64) <= 0.10 * dec64


def test_refusals():
    """by name: a teacher handle, a mu-law student, a weight-norm student, width 32, buffers that are no tape, a tape of
    another handle or shape, short buffers; the size queries return 0 for the refused models"""
    import torch
    from oracle import wavenet_np as O
    from nsynth_wavenet_amd import config as cfg, weights as wts
    from nsynth_wavenet_amd.engine import Engine
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    B, F, T = CASES['S1a'][1]
    mel, noise, cot = S.case_inputs(B, F, T, seed=1)

    def sizes(e):
        return [int(f(e._h, B, F, T)) for f in (e.lib.wn_iaf_train_tape_bytes, e.lib.wn_iaf_train_workspace_bytes,
                                                e.lib.wn_iaf_backward_weights_workspace_bytes)] + \
               [int(e.lib.wn_iaf_grad_floats(e._h)), int(e.lib.wn_iaf_grad_count(e._h))]
    te_cfg, te_seed, te_init = D.golden_case(np.load(GOLD), 'mol')[1]
    te = Wavenet(te_cfg).load_weights(O.synth_weights(O.HP(te_cfg), 'teacher', seed=te_seed, init=te_init))
    refused = [(te.engine, 'not a ParallelWavenet student')]
    for change, msg in ((dict(use_mu_law=True), 'mu-law student'), (dict(use_weight_norm=True), 'weight-norm student'),
                        (dict(width=32), 'multiples of 64')):
        cfgd = dict(S.S1, **change)
        refused.append((Engine(cfgd, kind='student').load_weights(wts.synthetic_weights(cfg.load_hparams(cfgd), 'student', seed=1)), msg))
    for e, msg in refused:
        assert sizes(e) == [0, 0, 0, 0, 0] and e.iaf_grad_table() == []
        with pytest.raises(ValueError, match=msg):
            e.iaf_forward_train_tape(mel, noise=np.zeros((B, e.iaf_length(F)), np.float32))
        with pytest.raises(ValueError, match=msg):
            e.iaf_backward_weights(torch.zeros(4096, dtype=torch.uint8, device='cuda'), *cot, n_frames=F)
        e.close()
    eng = _engine('S1')
    assert all(v > 0 for v in sizes(eng))
    ff, tape = eng.iaf_forward_train_tape(mel, noise=noise)
    # buffers that no tape forward wrote: a plain generation call's workspace, a copy of a tape
    eng.iaf_generate(mel, noise)
    ws = eng._ws if eng._ws.numel() >= tape.numel() else torch.zeros_like(tape)
    for not_a_tape in (ws, tape.clone()):
        with pytest.raises(ValueError, match='was not written by wn_iaf_forward_train_tape of this handle'):
            eng.iaf_backward_weights(not_a_tape, *cot, n_frames=F)
    other = _new_engine(S.S1, _weights('S1', seed=SEED + 1)[1])
    with pytest.raises(ValueError, match='was not written by wn_iaf_forward_train_tape of this handle'):
        other.iaf_backward_weights(tape, *cot, n_frames=F)
    other.close()
    with pytest.raises(ValueError, match='the tape holds B = 2, T = 200, not B = 1, T = 200'):
        eng.iaf_backward_weights(tape, *[c[:1] for c in cot], n_frames=F)
    with pytest.raises(ValueError, match='the tape holds F = 25 mel frames, not 26'):
        eng.iaf_backward_weights(tape, *cot, n_frames=F + 1)
    with pytest.raises(ValueError, match='not a multiple of the largest dilation'):
        eng.iaf_backward_weights(tape, *[c[:, :T - 1] for c in cot], n_frames=F)
    # short buffers, through the C ABI
    lib, h, st = eng.lib, eng._h, eng._stream()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    M, N = eng._dev(mel), eng._dev(noise)
    C = [eng._dev(c) for c in cot]
    out = [torch.empty((B, T), dtype=torch.float32, device='cuda') for _ in range(3)]
    tb, wb, bb, n = sizes(eng)[:4]
    tape2, ws1, ws2 = (torch.empty(k, dtype=torch.uint8, device='cuda') for k in (tb, wb, bb))
    grads = torch.empty(n, dtype=torch.float32, device='cuda')
    fwd = lambda tbytes, wbytes: lib.wn_iaf_forward_train_tape(h, p(N), p(M), B, F, T, p(out[0]), p(out[1]), p(out[2]), p(tape2),
                                                               tbytes, p(ws1), wbytes, st)
    bwd = lambda tbytes, nfl, wbytes: lib.wn_iaf_backward_weights(h, p(tape), tbytes, p(C[0]), p(C[1]), p(C[2]), B, F, T, p(grads),
                                                                  nfl, None, p(ws2), wbytes, st)
    for call, msg in ((lambda: fwd(tb - 1, wb), 'tape'), (lambda: fwd(tb, wb - 1), 'workspace'),
                      (lambda: bwd(tape.numel(), n - 1, bb), 'grads holds'), (lambda: bwd(tape.numel(), n, bb - 1), 'workspace'),
                      (lambda: bwd(tb - 1, n, bb), 'cannot hold the training tape')):
        rc = call()
        assert rc != 0 and msg in lib.wn_last_error(h).decode(), (rc, msg, lib.wn_last_error(h))
    assert bwd(tape.numel(), n, bb) == 0            # d_encoding may be NULL
    torch.cuda.synchronize()
