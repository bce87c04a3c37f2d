"""GPU tests of the teacher's weight gradients: wn_teacher_forward_train_tape and wn_teacher_backward_weights
(csrc/wn_teacher_wgrad.hip) behind Engine.teacher_forward_train_tape / teacher_backward_weights and Wavenet.loss_and_weight_grads.
Everything is held to the float64 oracle of tests/distill_oracle64.py with requires_grad on its weight tensors (pinned by
tests/test_teacher_wgrad_oracle.py), on the small teacher of tests/golden/ref_distill.npz (width 128, skip 64, 7 layers,
largest dilation 4, frame shift 200) at shapes and per-row seeded inputs of tests/test_gpu_teacher_shapes.py, whose seeds
were searched so that at most 16 pre-ReLU values are near ties; those take the engine's sign from the tape (relu_masks),
nothing else is excluded: every element of every gradient tensor is compared.

Bar: max |g - g64| <= TOL max |g64| per tensor, TOL = 1e-4 (tests/test_gpu_distill_grad.py).  Every case prints its measured
values before it asserts.  Measured on an MI355X (largest over the tensors of a shape): 1.68e-6 at (1, 1, 200), 1.81e-6 at
(3, 2, 260), 1.57e-6 at (2, 3, 512), 3.41e-6 for the Gauss teacher."""
import ctypes

import numpy as np
import pytest

import distill_oracle64 as D
import teacher_nll_oracle64 as N
import test_gpu_teacher_shapes as TS

pytestmark = pytest.mark.gpu
TOL = TS.TOL
NEAR_MAX = TS.NEAR_MAX
SHAPES = [(1, 1, 200),      # one partial tile, enc read past its rows
          (3, 2, 260),      # c0 = 70, four valid columns in the last tile and in the second chunk, odd B
          (2, 3, 512)]      # aligned control, two chunks
FILL_SHAPES = [(1, 1, 200), (2, 2, 400)]
OFF_TILE = (3, 2, 260)
_sid = TS._sid


def _is_stack(name):
    return 'trans_conv' not in name


class _WOracle(TS._Oracle):
    """TS._Oracle whose differentiable forward also tracks the weights of the residual stack and head and the conditioning"""

    def masks(self, tape):
        import torch
        B, T = self.x.shape
        masks, self.nflip = D.relu_masks(self.pre, D.tape_pre(tape, B, T, self.cfgd['skip_width']))
        self.names = sorted(k for k in self.w if _is_stack(k))
        self.wg = {k: self.w[k].clone().requires_grad_(True) for k in self.names}
        self.enc_g = self.enc.clone().requires_grad_(True)
        self.x64 = torch.as_tensor(self.x.astype(np.float64)).requires_grad_(True)
        w = dict(self.w)
        w.update(self.wg)
        self.out64 = D.teacher_ff(self.x64, self.enc_g, w, self.thp, masks=masks)
        return self

    def vjp_all(self, g):
        """({name: d W}, d enc [B,TE,Cd], d wav) of sum(out_params * g) in float64"""
        import torch
        leaves = [self.wg[k] for k in self.names] + [self.enc_g, self.x64]
        got = torch.autograd.grad((self.out64 * g.detach().double().cpu()).sum(), leaves, retain_graph=True, allow_unused=True)
        got = [torch.zeros_like(l) if v is None else v for v, l in zip(got, leaves)]
        return dict(zip(self.names, got[:-2])), got[-2], got[-1]


class _WCase(object):
    def __init__(self, R, eng, shape, tag='mol', seeds=None, cfgd=None, near_max=None):
        """cfgd: another model than the golden one of `tag` (same seed and init); near_max: its cap on the near-tie count"""
        import torch
        self.B, self.F, self.T = shape
        (gold, seed, init) = D.golden_case(R, tag)[1]
        cfgd = gold if cfgd is None else cfgd
        near_max = NEAR_MAX if near_max is None else near_max
        mel, x = TS._inputs(self.F, self.T, seeds or TS.ROW_SEEDS[shape])
        self.X, self.MEL = torch.as_tensor(x).cuda(), torch.as_tensor(mel).cuda()
        self.ora = _WOracle(cfgd, seed, init, mel, x)
        assert self.ora.near <= near_max, (shape, self.ora.near)
        self.out, self.tape = eng.teacher_forward_train_tape(self.X, self.MEL)
        self.ora.masks(self.tape)
        assert self.ora.nflip <= near_max, (shape, self.ora.nflip)
        self.ow = int(self.out.shape[2])

    def cotangent(self, seed):
        import torch
        rs = np.random.RandomState(seed)
        return torch.as_tensor(rs.standard_normal([self.B, self.T, self.ow]).astype(np.float32)).cuda()


@pytest.fixture(scope='module')
def R():
    return np.load(TS.GOLD)


def _engine(R, tag):
    from oracle import wavenet_np as O
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    cfgd, seed, init = D.golden_case(R, tag)[1]
    return Wavenet(cfgd).load_weights(O.synth_weights(O.HP(cfgd), 'teacher', seed=seed, init=init))


@pytest.fixture(scope='module')
def eng(R):
    net = _engine(R, 'mol')
    yield net.engine
    net.engine.close()


@pytest.fixture(scope='module')
def cases(R, eng):
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = _WCase(R, eng, shape)
        return made[shape]
    return get


def _err(got, ref):
    return float((got.detach().double().cpu() - ref).abs().max()) / float(ref.abs().max())


def _check_all(label, res, c, g, want_max=True):
    """every gradient tensor and d_encoding against the oracle; returns the largest relative error"""
    import torch
    ref_w, ref_enc, ref_wav = c.ora.vjp_all(g)
    assert sorted(res['grads']) == c.ora.names, 'the engine returns exactly the variables of the stack and head'
    worst = 0.0
    for k in c.ora.names:
        got, ref = res['grads'][k], ref_w[k]
        assert tuple(got.shape) == tuple(ref.shape), (k, tuple(got.shape), tuple(ref.shape))
        assert bool(torch.isfinite(got).all()), (label, k, 'not finite')
        mx = float(ref.abs().max())
        if mx == 0:
            assert float(got.abs().max()) == 0, (label, k, 'oracle gradient is zero')
            continue
        e = _err(got, ref)
        worst = max(worst, e)
        print('{} {:24s} max |g - g64| / max |g64| = {:.2e} (max |g64| {:.3e})'.format(label, k, e, mx))
        assert e <= TOL, (label, k, e)
    if res.get('d_encoding') is not None:
        assert bool(torch.isfinite(res['d_encoding']).all()), (label, 'd_encoding not finite')
        assert tuple(res['d_encoding'].shape) == tuple(ref_enc.shape)
        e = _err(res['d_encoding'], ref_enc)
        worst = max(worst, e)
        print('{} {:24s} max |g - g64| / max |g64| = {:.2e} (max |g64| {:.3e})'.format(label, 'd_encoding', e,
                                                                                       float(ref_enc.abs().max())))
        assert e <= TOL, (label, 'd_encoding', e)
    print('{} largest relative error {:.2e}; {} near-tie pre-ReLU values, {} signs from the tape'.format(
        label, worst, c.ora.near, c.ora.nflip))
    return worst


@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_weight_gradients_match_the_oracle(cases, eng, shape):
    """Dense random cotangent: every gradient and d_encoding within the bar; out_params and d_wav are the bits of the
    existing calls; a second call gives identical bits."""
    import torch
    c = cases(shape)
    assert torch.equal(c.out, eng.teacher_forward(c.X, c.MEL)), 'out_params of the train tape forward'
    assert c.tape.numel() == eng.teacher_train_tape_bytes(c.B, c.F, c.T)
    g = c.cotangent(101)
    res = eng.teacher_backward_weights(c.tape, g, want_encoding=True, want_wav=True)
    _check_all('wgrad ' + _sid(shape), res, c, g)
    assert torch.equal(res['d_wav'], eng.teacher_backward_input(c.tape, g)), 'a training tape serves the input VJP'
    _, plain = eng.teacher_forward_tape(c.X, c.MEL)
    assert torch.equal(res['d_wav'], eng.teacher_backward_input(plain, g)), 'd_wav bits of the plain-tape input VJP'
    S = c.ora.cfgd['skip_width']                                # the plain tape's regions sit at the same offsets
    for k, v in D.tape_pre(plain, c.B, c.T, S).items():
        assert torch.equal(v, D.tape_pre(c.tape, c.B, c.T, S)[k]), k
    again = eng.teacher_backward_weights(c.tape, g, want_encoding=True, want_wav=True)
    for k in ('flat_grads', 'd_encoding', 'd_wav'):
        assert torch.equal(again[k].view(torch.int32), res[k].view(torch.int32)), (k, 'repeat differs')


def test_gauss_teacher(R):
    shape = (1, 1, 200)
    net = _engine(R, 'gauss')
    c = _WCase(R, net.engine, shape, 'gauss', (TS.GAUSS_SEED,))
    g = c.cotangent(101)
    res = net.engine.teacher_backward_weights(c.tape, g, want_encoding=True)
    _check_all('wgrad gauss ' + _sid(shape), res, c, g)
    net.engine.close()


@pytest.mark.parametrize('k', [-40, 20])
def test_gradients_scale_bit_for_bit(cases, eng, k):
    import torch
    c = cases(OFF_TILE)
    g = c.cotangent(303)
    base = eng.teacher_backward_weights(c.tape, g, want_encoding=True)
    f = 2.0 ** k
    for key in ('flat_grads', 'd_encoding'):
        assert float(base[key].abs().max()) > 0 and torch.equal(base[key] * f / f, base[key])
    sc = eng.teacher_backward_weights(c.tape, g * f, want_encoding=True)
    for key in ('flat_grads', 'd_encoding'):
        assert torch.equal(sc[key], base[key] * f), key


def _raw(eng, c, g, fill):
    """the two calls through the C ABI on buffers of exactly the sizes the library asks for, every byte pre-set to `fill`"""
    import torch
    from nsynth_wavenet_amd import _lib
    lib, h = eng.lib, eng._h
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    with torch.cuda.device(eng.device):
        n_ws = int(lib.wn_teacher_workspace_bytes(h, c.B, c.F, c.T))
        n_tape = int(lib.wn_teacher_train_tape_bytes(h, c.B, c.F, c.T))
        n_bws = int(lib.wn_teacher_backward_weights_workspace_bytes(h, c.B, c.F, c.T))
        n_g = int(lib.wn_teacher_grad_floats(h))
        assert min(n_ws, n_tape, n_bws, n_g) > 0
        ws, tape, bws = [torch.full((n,), fill, dtype=torch.uint8, device='cuda') for n in (n_ws, n_tape, n_bws)]
        out = torch.full((c.B, c.T, c.ow), float('nan'), dtype=torch.float32, device='cuda')
        flat = torch.full((n_g,), float('nan'), dtype=torch.float32, device='cuda')
        denc = torch.full((c.B, c.F * eng.frame_shift, int(eng.hp.deconv_width)), float('nan'), dtype=torch.float32, device='cuda')
        _lib.check(lib.wn_teacher_forward_train_tape(h, ptr(c.X), ptr(c.MEL), c.B, c.F, c.T, ptr(out), ptr(tape), n_tape, ptr(ws),
                                                     n_ws, eng._stream()), h)
        _lib.check(lib.wn_teacher_backward_weights(h, ptr(tape), n_tape, ptr(g), c.B, c.F, c.T, ptr(flat), n_g, ptr(denc), None,
                                                   ptr(bws), n_bws, eng._stream()), h)
        torch.cuda.synchronize()
    grads = {name: flat[off:off + int(np.prod(shape))].view(shape) for name, off, shape in eng.teacher_grad_table()}
    return out, {'grads': grads, 'flat_grads': flat, 'd_encoding': denc}


@pytest.mark.parametrize('shape', FILL_SHAPES, ids=_sid)
def test_pad_columns_do_not_leak(cases, eng, shape):
    """Buffers the test owns, pre-filled with 0x00 and with 0xFF (every fp16 and fp32 word a NaN): the same bits, finite,
    within the bar."""
    import torch
    c = cases(shape)
    g = c.cotangent(404)
    out0, r0 = _raw(eng, c, g, 0x00)
    out1, r1 = _raw(eng, c, g, 0xFF)
    assert torch.equal(out0, c.out) and torch.equal(out1, c.out)
    for k in ('flat_grads', 'd_encoding'):
        bad = int((~torch.isfinite(r0[k])).sum()), int((~torch.isfinite(r1[k])).sum())
        same = bool((r0[k].view(torch.int32) == r1[k].view(torch.int32)).all())
        print('fills {} {}: non-finite {} / {}, same bits {}'.format(_sid(shape), k, bad[0], bad[1], same))
        assert bad == (0, 0) and same, (shape, k, bad, same)
    _check_all('fills ' + _sid(shape), r0, c, g)


def test_taps_read_the_left_pad(cases, eng):
    """A cotangent only at t = 0: taps k = 0, 1 of every dilated conv multiply l_i(t - (2 - k) d) at t < (2 - k) d, the zero left
    pad, so their gradients are exactly zero.  A cotangent only at t = T - 1 of batch row 0 stays within the bar."""
    import torch
    c = cases(OFF_TILE)
    g = c.cotangent(202)
    first = torch.zeros_like(g)
    first[:, 0] = g[:, 0]
    res = eng.teacher_backward_weights(c.tape, first, want_encoding=True)
    for i in range(1, 8):
        w = res['grads']['dilated_conv_%d/W' % i]
        assert float(w[0, 0].abs().max()) == 0 and float(w[0, 1].abs().max()) == 0, i
        assert bool(torch.isfinite(w).all())
    assert float(res['grads']['dilated_conv_1/W'][0, 2].abs().max()) > 0
    _check_all('t=0 ' + _sid(OFF_TILE), res, c, first)
    last = torch.zeros_like(g)
    last[0, c.T - 1] = g[0, c.T - 1]
    res = eng.teacher_backward_weights(c.tape, last, want_encoding=True)
    _check_all('t=T-1 row 0 ' + _sid(OFF_TILE), res, c, last)
    assert float(res['d_encoding'][1:].abs().max()) == 0


CHUNK_SHAPE, CHUNK_ROWS, CHUNK_SEED = (1, 4, 768), 22, 3147


def test_chunks_longer_than_one_tile(R, eng):
    """The time chunk is a whole number of 256-column tiles fixed by B and T (about 64 slabs in all).  22 rows of T = 768 get
    chunks of 512 columns, two per row: the second chunk starts at column 512 and ends at T, so the shape crosses a chunk
    boundary once and every row contributes two slabs.  The rows are 22 copies of one row whose seed was searched like
    ROW_SEEDS (16 near ties in float64), with 22 copies of its cotangent: the weight gradients are held to 22 times the
    float64 oracle's gradient of that row at the same bar, d_encoding and d_wav of every row are the single row's bits, and
    the single row (chunks of 256) meets the oracle too."""
    import torch
    n = CHUNK_ROWS
    c = _WCase(R, eng, CHUNK_SHAPE, seeds=(CHUNK_SEED,))
    g = c.cotangent(505)
    one = eng.teacher_backward_weights(c.tape, g, want_encoding=True, want_wav=True)
    _check_all('chunk 256 ' + _sid(CHUNK_SHAPE), one, c, g)
    out, tapen = eng.teacher_forward_train_tape(c.X.repeat(n, 1), c.MEL.repeat(n, 1, 1))
    assert torch.equal(out, c.out.repeat(n, 1, 1))
    many = eng.teacher_backward_weights(tapen, g.repeat(n, 1, 1), want_encoding=True, want_wav=True)
    assert torch.equal(many['d_encoding'], one['d_encoding'].repeat(n, 1, 1))
    assert torch.equal(many['d_wav'], one['d_wav'].repeat(n, 1))
    ref_w, _, _ = c.ora.vjp_all(g)
    worst = 0.0
    for k in c.ora.names:
        ref = ref_w[k] * n
        assert bool(torch.isfinite(many['grads'][k]).all()), k
        if float(ref.abs().max()) == 0:
            assert float(many['grads'][k].abs().max()) == 0, k
            continue
        e = _err(many['grads'][k], ref)
        worst = max(worst, e)
        assert e <= TOL, (k, e)
    print('chunk 512 x 2, {} rows of T = {}: largest max |g - {} g64| / max |{} g64| = {:.2e}'.format(n, c.T, n, n, worst))


def test_refusals(R, cases, eng, student_cfg):
    import torch
    from nsynth_wavenet_amd.engine import Engine
    c = cases((1, 1, 200))
    g = c.cotangent(1)
    _, plain = eng.teacher_forward_tape(c.X, c.MEL)
    with pytest.raises(ValueError, match='plain tape'):
        eng.teacher_backward_weights(plain, g, n_frames=c.F)
    # a copy of the tape at an address no tape was ever written to: allocations start on 512-byte boundaries, this does not
    # (a plain clone may land where an earlier, freed tape of this handle was registered)
    big = torch.empty(c.tape.numel() + 512, dtype=torch.uint8, device='cuda')
    copy = big[256:256 + c.tape.numel()]
    copy.copy_(c.tape)
    assert copy.data_ptr() % 512 == 256
    with pytest.raises(ValueError, match='not written'):
        eng.teacher_backward_weights(copy, g, n_frames=c.F)
    other = _engine(R, 'mol')
    with pytest.raises(ValueError, match='not written'):
        other.engine.teacher_backward_weights(c.tape, g, n_frames=c.F)
    other.engine.close()
    with pytest.raises(ValueError, match='holds B = 3, T = 260'):          # a tape of another shape
        eng.teacher_backward_weights(cases(OFF_TILE).tape, g, n_frames=c.F)
    with pytest.raises(ValueError, match='mel frames'):
        eng.teacher_backward_weights(c.tape, g, n_frames=c.F + 1)
    lib, h = eng.lib, eng._h
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    n_g = int(lib.wn_teacher_grad_floats(h))
    n_bws = int(lib.wn_teacher_backward_weights_workspace_bytes(h, c.B, c.F, c.T))
    flat = torch.empty(n_g, dtype=torch.float32, device='cuda')
    bws = torch.empty(n_bws, dtype=torch.uint8, device='cuda')
    rc = lib.wn_teacher_backward_weights(h, ptr(c.tape), c.tape.numel(), ptr(g), c.B, c.F, c.T, ptr(flat), n_g - 1, None, None,
                                         ptr(bws), n_bws, eng._stream())
    assert rc == -12 and b'grads holds' in lib.wn_last_error(h)
    st = Engine(student_cfg)
    with pytest.raises(ValueError, match='student handle'):
        st.teacher_backward_weights(c.tape, g, n_frames=c.F)
    assert st.teacher_train_tape_bytes(1, 1, 200) == 0
    st.close()


def _oracle_loss(ora_w, thp, x, enc, tag):
    import torch
    out = D.teacher_ff(torch.as_tensor(x.astype(np.float64)), enc, ora_w, thp)
    return -N.teacher_log_prob(out, torch.as_tensor(x.astype(np.float64)), tag, False).mean()


def test_descent_through_the_public_api(R):
    """Wavenet.loss_and_weight_grads, then load_weights(w - eps g) on a fresh Wavenet lowers 'loss'.  eps is chosen on the
    float64 oracle alone (its own decrease at least 1e-3 and within 5 % of eps |g|^2); the engine's decrease must be within
    10 % of the oracle's."""
    import torch
    from oracle import wavenet_np as O
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    tag, shape = 'mol', (2, 3, 512)
    cfgd, seed, init = D.golden_case(R, tag)[1]
    B, F, T = shape
    mel, x = TS._inputs(F, T, TS.ROW_SEEDS[shape])
    w32 = O.synth_weights(O.HP(cfgd), 'teacher', seed=seed, init=init)
    thp, w64 = D.teacher_weights(cfgd, seed, init)
    enc = D.teacher_enc(mel, cfgd, seed, init)
    names = sorted(k for k in w64 if _is_stack(k))
    leaves = {k: w64[k].clone().requires_grad_(True) for k in names}
    wl = dict(w64)
    wl.update(leaves)
    L0 = _oracle_loss(wl, thp, x, enc, tag)
    g64 = dict(zip(names, torch.autograd.grad(L0, [leaves[k] for k in names], allow_unused=True)))
    g64 = {k: torch.zeros_like(w64[k]) if v is None else v for k, v in g64.items()}
    gg = float(sum((v ** 2).sum() for v in g64.values()))
    eps, dec64 = None, None
    for e in [2.0 ** -j for j in range(0, 24)]:
        stepped = dict(w64)
        stepped.update({k: w64[k] - e * g64[k] for k in names})
        with torch.no_grad():
            dec = float(L0.detach()) - float(_oracle_loss(stepped, thp, x, enc, tag))
        if dec >= 1e-3 and abs(dec - e * gg) <= 0.05 * e * gg:
            eps, dec64 = e, dec
            break
    assert eps is not None, 'no step on the oracle is both large enough and in the linear regime'
    net = Wavenet(cfgd).load_weights(w32)
    X, MEL = torch.as_tensor(x).cuda(), torch.as_tensor(mel).cuda()
    res = net.loss_and_weight_grads({'wav': X, 'mel': MEL})
    with torch.no_grad():
        plain = net.calculate_loss(net.feed_forward({'wav': X, 'mel': MEL}))
    assert torch.equal(plain['loss'], res['loss']) and torch.equal(plain['log_probs'], res['log_probs'])
    assert sorted(res['grads']) == names
    new = dict(w32)
    for k in names:
        new[k] = (w32[k].astype(np.float64) - eps * res['grads'][k].double().cpu().numpy()).astype(np.float32)
    net2 = Wavenet(cfgd).load_weights(new)
    with torch.no_grad():
        after = net2.calculate_loss(net2.feed_forward({'wav': X, 'mel': MEL}))
    dec = float(res['loss']) - float(after['loss'])
    print('descent: eps {:.3e}, |g|^2 {:.4e}, oracle loss {:.6f} decrease {:.4e}; engine loss {:.6f} decrease {:.4e}'.format(
        eps, gg, float(L0.detach()), dec64, float(res['loss']), dec))
    assert dec > 0
    assert abs(dec - dec64) <= 0.10 * dec64, (dec, dec64)
    net.engine.close()
    net2.engine.close()


def test_d_encoding_feeds_the_upsampler(cases, eng):
    """d_encoding into torch autograd over oracle.torch_ref.trans_conv1d (float64): the gradient of the deconv variables
    against the float64 gradient of the whole graph."""
    import torch
    from oracle import torch_ref as TR
    shape = (1, 1, 200)
    c = cases(shape)
    g = c.cotangent(606)
    cfgd = c.ora.cfgd
    hp = c.ora.thp
    assert hp.get('upsample_act', 'tanh') == 'leaky_relu' and not hp.get('use_resize_conv', False)
    dnames = sorted(k for k in c.ora.w if not _is_stack(k))
    dw = {k: c.ora.w[k].clone().requires_grad_(True) for k in dnames}

    def deconv():
        h = torch.as_tensor(c.ora.mel.astype(np.float64)).transpose(1, 2)
        for j, (fl, s) in enumerate(cfgd['deconv_config']):
            sc = 'trans_conv_{:d}'.format(j + 1)
            h = TR.trans_conv1d(h, dw[sc + '/kernel'], dw[sc + '/bias'], s)
        return h.transpose(1, 2)                                   # [B,TE,Cd]
    enc = deconv()
    assert float((enc.detach() - c.ora.enc).abs().max()) <= 1e-9 * float(c.ora.enc.abs().max())
    _, ref_enc, _ = c.ora.vjp_all(g)
    ref = torch.autograd.grad((enc * ref_enc).sum(), [dw[k] for k in dnames], retain_graph=True)
    res = eng.teacher_backward_weights(c.tape, g, want_encoding=True)
    got = torch.autograd.grad((enc * res['d_encoding'].double().cpu()).sum(), [dw[k] for k in dnames])
    for k, a, b in zip(dnames, got, ref):
        e = float((a - b).abs().max()) / float(b.abs().max())
        print('upsampler {:24s} max |g - g64| / max |g64| = {:.2e}'.format(k, e))
        assert e <= TOL, (k, e)

