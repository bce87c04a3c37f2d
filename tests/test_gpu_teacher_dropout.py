"""GPU tests of dropout in the teacher's training step: wn_teacher_forward_train_tape_dropout, the masks the
reverse passes apply on its tapes (csrc/wn_teacher_dropout.hip), Engine.teacher_dropout_keep,
Wavenet.loss_and_weight_grads(dropout_seed=...) and TeacherTrainer(dropout=True).

The mask is held bit for bit to its numpy twin train.dropout_keep.  Values are held to the float64 oracle of
tests/dropout_oracle64.py (distill_oracle64.teacher_ff with the twin's masks inserted), gradients by torch autograd, at the
project's bars: out_params at TOL_FWD (2e-5 max(1, max |ref|) on the golden teachers, 5e-5 on geometry B as
tests/test_gpu_teacher_geometries.py holds it), every gradient tensor, d_encoding and d_wav at TOL = 1e-4 max |g64|, the public
chain's loss at TOL_CHAIN = 4e-5.  Every case prints what it measured before it asserts.

Near ties.  A float64 pre-ReLU value within 1e-4 of its tensor's largest magnitude of zero takes the engine's sign from the
tape (distill_oracle64.relu_masks); at most 0.1 % of a case's 2 B T skip_width pre-ReLU values may lie in that band, asserted
on the oracle before the engine is asked.  The audio rows (test_gpu_teacher_shapes._row of seeds among 1001 .. 1012, chosen per
batch position because the row index enters the hash) and the dropout seeds (among 11, 12, 13) were searched on the CPU with
the oracle and the twin alone for the fewest such values.  Found:
  golden MoL    dropout_inputs 0.5   (1, 1, 200)  rows 1003              seed 12    7 of  25 600
  golden MoL    dropout_inputs 0.5   (3, 2, 260)  rows 1007, 1005, 1010  seed 11   30 of  99 840
  golden MoL    dropout_inputs 0.3   (1, 1, 200)  rows 1005              seed 13    0 of  25 600
  golden Gauss  dropout_inputs 0.5   (1, 1, 200)  rows 1003              seed 12    7 of  25 600  (the same stack as MoL)
  golden MoL    dropout_all    0.05  (3, 2, 260)  rows 1004, 1010, 1006  seed 13   16 of  99 840
  geometry B    dropout_all    0.05  (2, 3, 512)  rows 1004, 1003        seed 13   34 of 131 072
The public chain runs the first case's inputs.

Measured on an MI355X (largest over the six cases; DESIGN.md 17 has them per case): out_params 6.0e-7, gradients and
d_encoding 3.2e-6, d_wav 1.8e-6, the chain's loss 7.2e-8; no sign came from the tape."""
import ctypes
import json

import numpy as np
import pytest

import distill_oracle64 as D
import dropout_oracle64 as DO
import teacher_nll_oracle64 as N
import test_gpu_teacher_geometries as TG
import test_gpu_teacher_shapes as TS
import test_gpu_teacher_wgrad as TW

pytestmark = pytest.mark.gpu
TOL = TS.TOL
TOL_CHAIN = TS.TOL_CHAIN
NEAR_SHARE = 1e-3
IAF_LP = 2048               # zero left pad of the l rows (csrc/wn_internal.h)

# key: (model, (B, F, T), (mode, dropout seed, rate), row seeds)
CASES = {'mol-in-0.5-small': ('mol', (1, 1, 200), ('dropout_inputs', 12, 0.5), (1003,)),
         'mol-in-0.5-ragged': ('mol', (3, 2, 260), ('dropout_inputs', 11, 0.5), (1007, 1005, 1010)),
         'mol-in-0.3-small': ('mol', (1, 1, 200), ('dropout_inputs', 13, 0.3), (1005,)),
         'gauss-in-0.5-small': ('gauss', (1, 1, 200), ('dropout_inputs', 12, 0.5), (1003,)),
         'mol-all-0.05-ragged': ('mol', (3, 2, 260), ('dropout_all', 13, 0.05), (1004, 1010, 1006)),
         'B-all-0.05': ('B', (2, 3, 512), ('dropout_all', 13, 0.05), (1004, 1003))}
MODELS = {'mol': ('mol', None, TS.TOL_FWD), 'gauss': ('gauss', None, TS.TOL_FWD), 'B': ('mol', 'B', TG.TOL_FWD)}
SMALL, RAGGED = 'mol-in-0.5-small', 'mol-in-0.5-ragged'


class _Model(object):
    def __init__(self, R, key):
        from oracle import wavenet_np as O
        from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
        self.tag, geo, self.tol_fwd = MODELS[key]
        cfgd, self.seed, self.init = D.golden_case(R, self.tag)[1]
        self.cfgd = dict(json.loads(json.dumps(cfgd)), **(TG.GEOMETRIES[geo] if geo else {}))
        # the handle's configuration carries no dropout key; the public chain and the trainer read this one from the hparams
        self.cfgd.update(dropout_inputs=True, dropout_all=False)
        self.w32 = O.synth_weights(O.HP(self.cfgd), 'teacher', seed=self.seed, init=self.init)
        self.net = Wavenet(self.cfgd).load_weights(self.w32)
        self.eng = self.net.engine


class _DOracle(object):
    """test_gpu_teacher_wgrad._WOracle on the dropped forward"""

    def __init__(self, m, mel, x, drop):
        import torch
        self.cfgd, self.mel, self.x, self.drop = m.cfgd, mel, x, drop
        self.thp, self.w = D.teacher_weights(m.cfgd, m.seed, m.init)
        self.enc = D.teacher_enc(mel, m.cfgd, m.seed, m.init)
        self.pre = {}
        with torch.no_grad():
            self.out = DO.teacher_ff(torch.as_tensor(x.astype(np.float64)), self.enc, self.w, self.thp, drop, pre=self.pre)
        self.near = TS._near(self.pre)

    def masks(self, tape):
        import torch
        B, T = self.x.shape
        masks, self.nflip = D.relu_masks(self.pre, D.tape_pre(tape, B, T, self.cfgd['skip_width']))
        self.names = sorted(k for k in self.w if TW._is_stack(k))
        self.wg = {k: self.w[k].clone().requires_grad_(True) for k in self.names}
        self.enc_g = self.enc.clone().requires_grad_(True)
        self.x64 = torch.as_tensor(self.x.astype(np.float64)).requires_grad_(True)
        w = dict(self.w)
        w.update(self.wg)
        self.out64 = DO.teacher_ff(self.x64, self.enc_g, w, self.thp, self.drop, masks=masks)
        return self

    def grads_of(self, scalar):
        """({name: d W}, d enc, d wav) of a scalar of out64 (and x64)"""
        import torch
        leaves = [self.wg[k] for k in self.names] + [self.enc_g, self.x64]
        got = torch.autograd.grad(scalar, leaves, retain_graph=True, allow_unused=True)
        got = [torch.zeros_like(l) if v is None else v for v, l in zip(got, leaves)]
        return dict(zip(self.names, got[:-2])), got[-2], got[-1]

    def vjp_all(self, g):
        return self.grads_of((self.out64 * g.detach().double().cpu()).sum())


class _DCase(object):
    def __init__(self, m, key):
        import torch
        _, shape, self.drop, seeds = CASES[key]
        self.m, self.key = m, key
        self.B, self.F, self.T = shape
        mel, x = TS._inputs(self.F, self.T, seeds)
        self.X, self.MEL = torch.as_tensor(x).cuda(), torch.as_tensor(mel).cuda()
        self.ora = _DOracle(m, mel, x, self.drop)
        self.n_pre = sum(v.numel() for v in self.ora.pre.values())
        assert self.n_pre == 2 * self.B * self.T * m.cfgd['skip_width']
        self.cap = int(NEAR_SHARE * self.n_pre)
        assert self.ora.near <= self.cap, (key, self.ora.near, self.cap)
        self.out, self.tape = m.eng.teacher_forward_train_tape(self.X, self.MEL, dropout=self.drop)
        self.ora.masks(self.tape)
        assert self.ora.nflip <= self.cap, (key, self.ora.nflip)
        self.ow = int(self.out.shape[2])

    def cotangent(self, seed):
        import torch
        rs = np.random.RandomState(seed)
        return torch.as_tensor(rs.standard_normal([self.B, self.T, self.ow]).astype(np.float32)).cuda()


@pytest.fixture(scope='module')
def R():
    return np.load(TS.GOLD)


@pytest.fixture(scope='module')
def models(R):
    made = {}

    def get(key):
        if key not in made:
            made[key] = _Model(R, key)
        return made[key]
    yield get
    for m in made.values():
        m.eng.close()


@pytest.fixture(scope='module')
def cases(models):
    made = {}

    def get(key):
        if key not in made:
            made[key] = _DCase(models(CASES[key][0]), key)
        return made[key]
    return get


def _bits(a, b):
    import torch
    return tuple(a.shape) == tuple(b.shape) and bool((a.view(torch.int32) == b.view(torch.int32)).all())


# ---------------------------------------------------------------------------------------------------------------------
# the mask
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rate', [0.5, 0.05])
@pytest.mark.parametrize('shape', [(3, 64, 260), (1, 512, 200)], ids=lambda s: 'B{}-C{}-T{}'.format(*s))
@pytest.mark.parametrize('site', [0, 1, 7])
def test_device_mask_is_the_twin(models, site, shape, rate):
    from nsynth_wavenet_amd.train import dropout_keep
    B, C, T = shape
    for seed in (12, 0xFEDCBA9876543210):
        got = models('mol').eng.teacher_dropout_keep(seed, site, B, C, T, rate)
        want = dropout_keep(seed, site, B, C, T, rate)
        assert tuple(got.shape) == (B, T, C) and str(got.dtype) == 'torch.bool'
        diff = int((got.cpu().numpy() != want).sum())
        print('site {} {} rate {} seed {:#x}: keep share {:.4f}, {} bits differ'.format(site, shape, rate, seed, want.mean(), diff))
        assert diff == 0


# ---------------------------------------------------------------------------------------------------------------------
# against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', sorted(CASES))
def test_dropped_forward_and_gradients_match_the_oracle(cases, key):
    """out_params of the dropped forward, then one reverse pass on a dense standard-normal cotangent: every gradient tensor,
    d_encoding and d_wav; the input VJP on the same tape returns d_wav's bits."""
    c = cases(key)
    eng = c.m.eng
    assert tuple(c.out.shape) == (c.B, c.T, c.ow) and TS._all_finite(c.out)
    e = TS._fwd_err(c.out, c.ora.out)
    plain = TS._fwd_err(eng.teacher_forward(c.X, c.MEL), c.ora.out)
    print('forward {}: max |out - oracle| / max(1, max |oracle|) = {:.2e} (max |oracle| {:.3f}; the undropped forward is {:.2e} '
          'away); {} near-tie pre-ReLU values of {}, {} signs from the tape'.format(key, e, float(c.ora.out.abs().max()), plain,
                                                                                  c.ora.near, c.n_pre, c.ora.nflip))
    assert e <= c.m.tol_fwd, (key, e)
    assert plain > 100 * c.m.tol_fwd, 'the case would not notice a missing mask'
    g = c.cotangent(101)
    res = eng.teacher_backward_weights(c.tape, g, want_encoding=True, want_wav=True)
    worst = TW._check_all('dropout ' + key, res, c, g)
    ref_wav = c.ora.vjp_all(g)[2]
    assert TS._all_finite(res['d_wav'])
    ew = TS._vjp_err(res['d_wav'], ref_wav)
    print('dropout {} d_wav error {:.2e} (max |oracle| {:.3e}); largest over the tensors {:.2e}'.format(
        key, ew, float(ref_wav.abs().max()), worst))
    assert ew <= TOL, (key, ew)
    assert _bits(res['d_wav'], eng.teacher_backward_input(c.tape, g)), 'the input VJP accepts a dropout tape'


def test_public_chain(cases):
    """Wavenet.loss_and_weight_grads(upsampler=True, dropout_seed=s) at (1, 1, 200): loss at TOL_CHAIN, every gradient of stack
    and head and d_encoding at TOL against the float64 gradient of the dropped loss; the upsampler's gradients are the bits of
    Engine.deconv_backward on this call's d_encoding (held to float64 by tests/test_gpu_deconv_backward.py)."""
    import torch
    c = cases(SMALL)
    m = c.m
    mode, seed, rate = c.drop
    assert m.net.dropout_inputs and mode == 'dropout_inputs' and m.net.dropout_rate == rate
    res = m.net.loss_and_weight_grads({'wav': c.X, 'mel': c.MEL}, upsampler=True, dropout_seed=seed)
    x64 = torch.as_tensor(c.ora.x.astype(np.float64))
    L_plain = float(-N.teacher_log_prob(c.ora.out, x64, m.tag, False).mean())
    e_loss = abs(float(res['loss']) - L_plain) / max(1.0, abs(L_plain))
    with torch.no_grad():
        det = m.net.calculate_loss(m.net.feed_forward({'wav': c.X, 'mel': c.MEL}))
    print('chain loss {:.7f}, oracle {:.7f}: error / max(1, |oracle|) = {:.2e}; the deterministic loss is {:.7f}'.format(
        float(res['loss']), L_plain, e_loss, float(det['loss'])))
    assert e_loss <= TOL_CHAIN, e_loss
    assert abs(float(det['loss']) - L_plain) > 100 * TOL_CHAIN, 'the case would not notice a missing mask'
    assert torch.equal(res['loss'], -res['log_probs'].mean())
    L = -N.teacher_log_prob(c.ora.out64, c.ora.x64, m.tag, False).mean()
    ref_w, ref_enc, _ = c.ora.grads_of(L)
    stack = {k: v for k, v in res['grads'].items() if TW._is_stack(k)}
    assert sorted(stack) == c.ora.names
    failed = []
    for k in c.ora.names:
        if float(ref_w[k].abs().max()) == 0:
            assert float(stack[k].abs().max()) == 0, k
            continue
        e = TW._err(stack[k], ref_w[k])
        print('chain {:24s} max |g - g64| / max |g64| = {:.2e}'.format(k, e))
        if not e <= TOL:
            failed.append((k, e))
    e = TW._err(res['d_encoding'], ref_enc)
    print('chain d_encoding max |g - g64| / max |g64| = {:.2e}'.format(e))
    assert not failed and e <= TOL, (failed, e)
    up = m.eng.deconv_backward(c.MEL, res['d_encoding'])
    assert _bits(res['flat_upsampler_grads'], up['flat_grads'])
    assert sorted(k for k in res['grads'] if not TW._is_stack(k)) == sorted(up['grads'])


# ---------------------------------------------------------------------------------------------------------------------
# exactness
# ---------------------------------------------------------------------------------------------------------------------
def _g4_rows(words, B, C, rowlen):
    """G4 rows [B][hi | lo][C / 8][rowlen][4 words] -> (hi, lo) float16 [B, rowlen, C]"""
    import torch
    h = words.view(torch.float16).reshape(B, 2, C // 8, rowlen, 4, 2)
    g, i, p = np.meshgrid(np.arange(C // 8), np.arange(4), np.arange(2), indexing='ij')
    ch = 32 * (g >> 2) + 16 * (i >> 1) + 4 * (g & 3) + 2 * (i & 1) + p              # wn_g4_channel(g, i) + p
    out = torch.empty(B, 2, rowlen, C, dtype=torch.float16, device=words.device)
    out[:, :, :, torch.as_tensor(ch.reshape(-1), device=words.device)] = h.permute(0, 1, 3, 2, 4, 5).reshape(B, 2, rowlen, C)
    return out[:, 0], out[:, 1]


def test_slot_zero_is_the_masked_raw_row(cases):
    """dropout_inputs at rate 0.5 on (3, 2, 260): slot 0 of the tape's l rows against the raw l_0 row at the end of the tape --
    both words exactly zero at dropped elements, both halves exactly doubled at kept ones, the zero left pad kept, zeros
    from column T on."""
    import torch
    from nsynth_wavenet_amd.train import dropout_keep
    c = cases(RAGGED)
    eng, (mode, seed, rate) = c.m.eng, c.drop
    W = c.m.cfgd['width']
    Tp = (c.T + 255) // 256 * 256
    RS = IAF_LP + Tp
    row = c.B * W * RS * 4
    assert row % 256 == 0
    plain_total = eng.teacher_train_tape_bytes(c.B, c.F, c.T)
    assert c.tape.numel() == plain_total + row, 'one more l row than the plain training tape'
    slot0_off = (eng.teacher_tape_bytes(c.B, c.T) + 255) // 256 * 256
    hi0, lo0 = _g4_rows(c.tape[slot0_off:slot0_off + row], c.B, W, RS)
    hir, lor = _g4_rows(c.tape[c.tape.numel() - row:], c.B, W, RS)
    keep = torch.as_tensor(dropout_keep(seed, 0, c.B, W, c.T, rate)).cuda()
    v = slice(IAF_LP, IAF_LP + c.T)
    assert float(hir[:, v].float().abs().max()) > 0
    for name, a, r in (('hi', hi0, hir), ('lo', lo0, lor)):
        assert int((a[:, :IAF_LP].view(torch.int16) != 0).sum()) == 0 and int((r[:, :IAF_LP].view(torch.int16) != 0).sum()) == 0
        assert int((a[:, IAF_LP + c.T:].view(torch.int16) != 0).sum()) == 0, 'zeros from column T on'
        assert int((a[:, v].view(torch.int16)[~keep] != 0).sum()) == 0, (name, 'a dropped word is not +0')
        assert torch.equal(a[:, v][keep], (r[:, v] * 2)[keep]), (name, 'a kept half is not doubled')
    print('slot 0: {} of {} elements kept'.format(int(keep.sum()), keep.numel()))


@pytest.mark.parametrize('mode', DO.MODES)
def test_rate_zero_is_the_plain_call(cases, mode):
    import torch
    c = cases(RAGGED)
    eng = c.m.eng
    g = c.cotangent(707)
    out0, tape0 = eng.teacher_forward_train_tape(c.X, c.MEL)
    outd, taped = eng.teacher_forward_train_tape(c.X, c.MEL, dropout=(mode, 99, 0.0))
    assert torch.equal(out0, outd)
    a = eng.teacher_backward_weights(tape0, g, want_encoding=True, want_wav=True)
    b = eng.teacher_backward_weights(taped, g, want_encoding=True, want_wav=True)
    for k in ('flat_grads', 'd_encoding', 'd_wav'):
        assert _bits(a[k], b[k]), (mode, k)


def _raw(eng, c, g, fill, drop):
    """the dropout forward and the reverse pass through the C ABI on buffers of exactly the sizes the library asks for, every
    byte pre-set to `fill`"""
    import torch
    from nsynth_wavenet_amd import _lib
    lib, h = eng.lib, eng._h
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    mode = eng.DROPOUT_MODES[drop[0]]
    with torch.cuda.device(eng.device):
        n_ws = int(lib.wn_teacher_workspace_bytes(h, c.B, c.F, c.T))
        n_tape = int(lib.wn_teacher_train_tape_dropout_bytes(h, c.B, c.F, c.T, mode))
        n_bws = int(lib.wn_teacher_backward_weights_workspace_bytes(h, c.B, c.F, c.T))
        n_g = int(lib.wn_teacher_grad_floats(h))
        assert min(n_ws, n_tape, n_bws, n_g) > 0
        ws, tape, bws = [torch.full((n,), fill, dtype=torch.uint8, device='cuda') for n in (n_ws, n_tape, n_bws)]
        out = torch.full((c.B, c.T, c.ow), float('nan'), dtype=torch.float32, device='cuda')
        flat = torch.full((n_g,), float('nan'), dtype=torch.float32, device='cuda')
        denc = torch.full((c.B, c.F * eng.frame_shift, int(eng.hp.deconv_width)), float('nan'), dtype=torch.float32, device='cuda')
        dwav = torch.full((c.B, c.T), float('nan'), dtype=torch.float32, device='cuda')
        _lib.check(lib.wn_teacher_forward_train_tape_dropout(h, ptr(c.X), ptr(c.MEL), c.B, c.F, c.T, ptr(out), ptr(tape), n_tape,
                                                             ptr(ws), n_ws, eng._stream(), mode, ctypes.c_uint64(drop[1]),
                                                             float(drop[2])), h)
        _lib.check(lib.wn_teacher_backward_weights(h, ptr(tape), n_tape, ptr(g), c.B, c.F, c.T, ptr(flat), n_g, ptr(denc),
                                                   ptr(dwav), ptr(bws), n_bws, eng._stream()), h)
        torch.cuda.synchronize()
    return {'out': out, 'flat_grads': flat, 'd_encoding': denc, 'd_wav': dwav}


@pytest.mark.parametrize('key', [RAGGED, 'mol-all-0.05-ragged'])
def test_one_seed_gives_one_result_whatever_the_buffers_held(cases, key):
    """Two calls with one seed on caller-owned buffers pre-filled with 0x00 and with 0xFF (252 pad columns of NaNs): the same
    bits as each other and as the case's own call, all finite.  Another seed gives other out_params."""
    import torch
    c = cases(key)
    eng = c.m.eng
    g = c.cotangent(101)
    ref = eng.teacher_backward_weights(c.tape, g, want_encoding=True, want_wav=True)
    ref['out'] = c.out
    r0, r1 = _raw(eng, c, g, 0x00, c.drop), _raw(eng, c, g, 0xFF, c.drop)
    for k in ('out', 'flat_grads', 'd_encoding', 'd_wav'):
        bad = int((~torch.isfinite(r0[k])).sum()), int((~torch.isfinite(r1[k])).sum())
        same = _bits(r0[k], r1[k]) and _bits(r0[k], ref[k])
        print('fills {} {}: non-finite {} / {}, same bits {}'.format(key, k, bad[0], bad[1], same))
        assert bad == (0, 0) and same, (key, k, bad, same)
    other = eng.teacher_forward_train_tape(c.X, c.MEL, dropout=(c.drop[0], c.drop[1] + 1, c.drop[2]))[0]
    assert not torch.equal(other, c.out)


# ---------------------------------------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------------------------------------
def test_trainer_steps_are_the_seeded_calls(R):
    """TeacherTrainer(dropout=True), two steps at (3, 2, 260): each step's loss is the bits of
    loss_and_weight_grads(dropout_seed=dropout_step_seed(base, k)) under the weights in force, the master and EMA buffers
    are what adam_ema_step gives by hand on that call's flat gradients, and the handle stays deterministic for feed_forward."""
    import torch
    from nsynth_wavenet_amd.engine import adam_ema_step
    from nsynth_wavenet_amd.train import TeacherTrainer, dropout_step_seed
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    m = _Model(R, 'mol')
    _, (B, F, T), _, seeds = CASES[RAGGED]
    mel, x = TS._inputs(F, T, seeds)
    batch = {'wav': torch.as_tensor(x).cuda(), 'mel': torch.as_tensor(mel).cuda()}
    base, lr, b1, b2, eps, decay = 0xABCDEF0123456789, 1e-3, 0.9, 0.999, 1e-8, 0.9999
    tr = TeacherTrainer(m.net, m.w32, lr=lr, dropout=True, dropout_seed=base)
    with pytest.raises(ValueError, match='neither dropout_inputs nor dropout_all'):
        cfgd = {k: v for k, v in m.cfgd.items() if k != 'dropout_inputs'}
        TeacherTrainer(Wavenet(cfgd, engine=m.eng), m.w32, dropout=True)
    losses = []
    for k in range(2):
        ref = m.net.loss_and_weight_grads(batch, upsampler=True, dropout_seed=dropout_step_seed(base, k))
        flats = [ref['flat_grads'], ref['flat_upsampler_grads']]
        state = [[t.clone() for t in bufs] for bufs in (tr.p, tr.m, tr.v, tr.ema)]
        out = tr.step(batch)
        assert torch.equal(out['loss'], ref['loss']) and torch.equal(out['log_probs'], ref['log_probs']), k
        losses.append(float(out['loss']))
        lr_t = float(np.float32(lr * np.sqrt(1.0 - b2 ** (k + 1)) / (1.0 - b1 ** (k + 1))))
        assert tr.lr_t == lr_t and tr.global_step == k + 1
        for i, gflat in enumerate(flats):
            p, mm, v, e = [s[i] for s in state]
            adam_ema_step(p, gflat, mm, v, e, lr_t, b1, b2, eps, min(decay, (1.0 + k) / (10.0 + k)))
            for name, mine, theirs in (('p', p, tr.p[i]), ('m', mm, tr.m[i]), ('v', v, tr.v[i]), ('ema', e, tr.ema[i])):
                assert _bits(mine, theirs), (k, i, name)
    with torch.no_grad():
        det = m.net.calculate_loss(m.net.feed_forward(batch))
        again = m.net.feed_forward(batch)['out_params']
        fresh = Wavenet(m.cfgd).load_weights(tr.weights())
        want = fresh.feed_forward(batch)['out_params']
        fresh.engine.close()
    print('dropout losses of steps 1, 2: {}; deterministic loss after them {:.6f}'.format(losses, float(det['loss'])))
    assert torch.equal(again, want), 'feed_forward after training is a fresh handle loaded from trainer.weights()'
    assert losses[0] != losses[1]
    m.eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(R, cases, models):
    import torch
    from nsynth_wavenet_amd import config as cfg, weights as wts
    from nsynth_wavenet_amd.engine import Engine
    c = cases(SMALL)
    eng = c.m.eng
    for rate in (1.0, -0.1, float('nan')):
        with pytest.raises(ValueError, match='outside'):
            eng.teacher_forward_train_tape(c.X, c.MEL, dropout=('dropout_inputs', 1, rate))
        with pytest.raises(ValueError, match='outside'):
            eng.teacher_dropout_keep(1, 0, 1, 8, 8, rate)
    for mode in (0, 3, 'dropout_none'):
        with pytest.raises(ValueError, match='unknown dropout mode'):
            eng.teacher_forward_train_tape(c.X, c.MEL, dropout=(mode, 1, 0.5))
    assert int(eng.lib.wn_teacher_train_tape_dropout_bytes(eng._h, c.B, c.F, c.T, 3)) == 0
    # a dropout tape handed to another handle
    other = _Model(R, 'mol')
    g = c.cotangent(1)
    with pytest.raises(ValueError, match='not written'):
        other.eng.teacher_backward_weights(c.tape, g, n_frames=c.F)
    with pytest.raises(ValueError, match='not written'):
        other.eng.teacher_backward_input(c.tape, g)
    other.eng.close()
    # a dropout_inputs tape cut to the plain training tape's size lacks the raw row
    cut = c.tape[:eng.teacher_train_tape_bytes(c.B, c.F, c.T)]
    with pytest.raises(ValueError, match='cannot hold'):
        eng.teacher_backward_weights(cut, g, n_frames=c.F)
    # what the plain training-tape forward refuses is refused in its words
    for over in ({'use_mu_law': True}, {'loss_type': 'ce', 'use_mu_law': True}, {'use_weight_norm': True}):
        cfgd = dict(json.loads(json.dumps(c.m.cfgd)), **over)
        e3 = Engine(cfgd, kind='teacher').load_weights(wts.synthetic_weights(cfg.load_hparams(cfgd), 'teacher', seed=3, init='unit'))
        with pytest.raises(ValueError) as plain:
            e3.teacher_forward_train_tape(c.X, c.MEL)
        with pytest.raises(ValueError) as dropped:
            e3.teacher_forward_train_tape(c.X, c.MEL, dropout=('dropout_inputs', 1, 0.5))
        assert str(dropped.value) == str(plain.value).replace('wn_teacher_forward_train_tape', 'wn_teacher_forward_train_tape_dropout'), over
        assert int(e3.lib.wn_teacher_train_tape_dropout_bytes(e3._h, c.B, c.F, c.T, 1)) == 0
        e3.close()
