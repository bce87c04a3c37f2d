"""GPU tests of the upsampler's reverse pass: wn_deconv_backward (csrc/wn_deconv_bwd.hip) behind
Engine.deconv_backward / deconv_grad_table and Wavenet.loss_and_weight_grads(upsampler=True).  Everything is held to the
float64 oracle of tests/deconv_grad_oracle64.py (pinned on the CPU by tests/test_deconv_grad_oracle.py) on three models: the
small teacher of tests/golden/ref_distill.npz (80 -> 64 with K = 40, S = 10; 64 -> 64 with K = 80, S = 20), a copy with
deconv_width 256 (the shipped width, four 64-channel tiles) and a copy with upsample_act tanh.

Ties of leaky-relu are handled on the oracle alone: every batch row's mel is np.random.RandomState(seed).uniform(0, 1,
[F, 80]) of the first seed from 2001 upward whose float64 hidden pre-activations have no value within 1e-4 of the row's
largest magnitude of zero (the search goes on until it finds one; every case asserts again that its rows have none), and the
dense standard-normal cotangent is zeroed where the float64 pre-activation of the last layer lies in that band (at most
0.1 % of a case, asserted).  The tanh model needs neither.  ONE case is an exception, NO_CLEAR_SEED: the 256-wide model at 27
frames has 69 120 hidden values per row and 15 to 28 of them in the band for each of the seeds 2001 .. 2010, so a clear seed
is out of reach.  That case asserts that no seed of this window is clear, takes the one with the fewest ties, and the
cotangent's component that reaches those hidden elements is projected out on the oracle (tests/deconv_grad_oracle64.py,
which asserts that their float64 cotangent is then zero), so the sign the engine takes there cannot matter.

Bar: per gradient tensor max |g - g64| <= TOL max |g64|, TOL = 1e-4 (tests/test_gpu_distill_grad.py), every element
compared; every case prints its measured value before it asserts (DESIGN.md 15 records the largest per model)."""
import ctypes
import json

import numpy as np
import pytest

import deconv_grad_oracle64 as DG
import distill_oracle64 as D
import teacher_nll_oracle64 as N
import test_gpu_teacher_shapes as TS

pytestmark = pytest.mark.gpu
TOL = TS.TOL
MODELS = {'small': {}, 'wide': {'deconv_width': 256}, 'tanh': {'upsample_act': 'tanh'}}
SHAPES = [(1, 1),       # ten hidden frames: almost every tap reads a zero pad
          (3, 2),       # odd B
          (2, 7),       # 70 hidden frames: neither a 32-frame K-step nor a 64-frame tile
          (1, 27)]      # 270 hidden frames: across 256


NO_CLEAR_SEED = ('wide', (1, 27))


def _sid(s):
    return 'B{}-F{}'.format(*s)


class _Model(object):
    def __init__(self, R, tag):
        from oracle import wavenet_np as O
        from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
        self.tag = tag
        cfgd, self.seed, self.init = D.golden_case(R, 'mol')[1]
        self.cfgd = dict(json.loads(json.dumps(cfgd)), **MODELS[tag])
        self.dc, self.act = self.cfgd['deconv_config'], self.cfgd['upsample_act']
        self.w32 = O.synth_weights(O.HP(self.cfgd), 'teacher', seed=self.seed, init=self.init)
        self.w64 = DG.weights64(self.w32, len(self.dc))
        self.net = Wavenet(self.cfgd).load_weights(self.w32)
        self.eng = self.net.engine
        self.cases = {}

    def case(self, shape, gseed=101):
        if (shape, gseed) not in self.cases:
            self.cases[(shape, gseed)] = _Case(self, shape, gseed)
        return self.cases[(shape, gseed)]


class _Case(object):
    """mel rows, a dense cotangent (masked at the last layer's near ties) and the oracle's gradients of one shape"""

    def __init__(self, m, shape, gseed):
        import torch
        self.B, self.F = shape
        self.exception = (m.tag, shape) == NO_CLEAR_SEED
        if self.exception:
            self.mel, self.seeds, window = DG.pick_rows_fewest(self.B, self.F, m.w64, m.dc)
            assert all(min(w) > 0 for w in window), ('a seed of the window is clear: the rule has an answer', window)
        else:
            self.mel, self.seeds = DG.pick_rows(self.B, self.F, m.w64, m.dc, m.act)
        TE, Cd = self.F * 200, m.cfgd['deconv_width']
        g = torch.as_tensor(np.random.RandomState(gseed).standard_normal([self.B, TE, Cd]).astype(np.float32))
        self.g, self.zeroed, self.hidden = DG.mask_last(g, self.mel, m.w64, m.dc, m.act, project=self.exception)
        assert (self.hidden > 0) == self.exception, (m.tag, shape, self.hidden)
        self.m, self.MEL, self.G = m, torch.as_tensor(self.mel).cuda(), self.g.cuda()
        self._ref = {}

    def ref(self, g=None):
        key = 'dense' if g is None else id(g)
        if key not in self._ref:
            self._ref[key] = DG.grads(self.mel, self.m.w64, self.m.dc, self.m.act, (self.g if g is None else g).double().cpu())
        return self._ref[key]


@pytest.fixture(scope='module')
def models():
    R = np.load(TS.GOLD)
    made = {}

    def get(tag):
        if tag not in made:
            made[tag] = _Model(R, tag)
        return made[tag]
    yield get
    for m in made.values():
        m.eng.close()


def _err(got, ref):
    return float((got.detach().double().cpu() - ref).abs().max()) / float(ref.abs().max())


def _check(label, grads, ref, scale=1.0):
    """every gradient tensor against scale * the oracle's; returns the largest relative error"""
    import torch
    assert sorted(grads) == sorted(ref), 'exactly the variables of the stack'
    worst = 0.0
    for k in sorted(ref):
        got, want = grads[k], ref[k] * scale
        assert tuple(got.shape) == tuple(want.shape), (k, tuple(got.shape), tuple(want.shape))
        assert bool(torch.isfinite(got).all()), (label, k, 'not finite')
        assert float(want.abs().max()) > 0
        e = _err(got, want)
        worst = max(worst, e)
        print('{} {:22s} max |g - g64| / max |g64| = {:.2e} (max |g64| {:.3e})'.format(label, k, e, float(want.abs().max())))
        assert e <= TOL, (label, k, e)
    print('{} largest relative error {:.2e}'.format(label, worst))
    return worst


@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
@pytest.mark.parametrize('tag', sorted(MODELS))
def test_gradients_match_the_oracle(models, tag, shape):
    """Dense cotangent: every gradient within the bar; the table names the TF variables in order; a second call gives
    identical bits."""
    import torch
    m = models(tag)
    c = m.case(shape)
    print('{} {}: row seeds {}, {} of {} cotangent elements zeroed at last-layer ties, {} hidden ties projected out'.format(
        tag, _sid(shape), c.seeds, c.zeroed, c.g.numel(), c.hidden))
    tab = m.eng.deconv_grad_table()
    assert [t[0] for t in tab] == DG.names(len(m.dc))
    for name, off, shp in tab:
        assert tuple(m.w32[name].shape) == shp, name
    res = m.eng.deconv_backward(c.MEL, c.G)
    assert res['flat_grads'].numel() == sum(int(np.prod(t[2])) for t in tab)
    _check('{} {}'.format(tag, _sid(shape)), res['grads'], c.ref())
    again = m.eng.deconv_backward(c.MEL, c.G)
    assert torch.equal(again['flat_grads'].view(torch.int32), res['flat_grads'].view(torch.int32)), 'repeat differs'


@pytest.mark.parametrize('k', [-40, 20])
def test_gradients_scale_bit_for_bit(models, k):
    import torch
    m = models('wide')
    c = m.case((3, 2))
    base = m.eng.deconv_backward(c.MEL, c.G)['flat_grads']
    f = 2.0 ** k
    assert float(base.abs().max()) > 0 and torch.equal(base * f / f, base)
    sc = m.eng.deconv_backward(c.MEL, c.G * f)['flat_grads']
    assert torch.equal(sc, base * f)


def _raw(m, c, fill):
    """the call through the C ABI on buffers of exactly the sizes the library asks for, every byte pre-set to `fill`"""
    import torch
    from nsynth_wavenet_amd import _lib
    eng = m.eng
    lib, h = eng.lib, eng._h
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    with torch.cuda.device(eng.device):
        n_ws = int(lib.wn_deconv_backward_workspace_bytes(h, b'', c.B, c.F))
        n_g = int(lib.wn_deconv_grad_floats(h, b''))
        assert min(n_ws, n_g) > 0
        ws = torch.full((n_ws,), fill, dtype=torch.uint8, device='cuda')
        flat = torch.full((n_g,), fill, dtype=torch.uint8, device='cuda').repeat(4).view(torch.float32)
        assert flat.numel() == n_g
        _lib.check(lib.wn_deconv_backward(h, b'', ptr(c.MEL), ptr(c.G), c.B, c.F, ptr(flat), n_g, ptr(ws), n_ws, eng._stream()), h)
        torch.cuda.synchronize()
    return flat, {name: flat[off:off + int(np.prod(shp))].view(shp) for name, off, shp in eng.deconv_grad_table()}


@pytest.mark.parametrize('tag,shape', [('small', (1, 1)), ('wide', (2, 7)), ('tanh', (3, 2))], ids=lambda v: str(v))
def test_pad_columns_do_not_leak(models, tag, shape):
    """Buffers the test owns, pre-filled with 0x00 and with 0xFF (every fp16 and fp32 word a NaN): the same bits, finite,
    within the bar."""
    import torch
    m = models(tag)
    c = m.case(shape, 404)
    f0, g0 = _raw(m, c, 0x00)
    f1, g1 = _raw(m, c, 0xFF)
    bad = int((~torch.isfinite(f0)).sum()), int((~torch.isfinite(f1)).sum())
    same = bool((f0.view(torch.int32) == f1.view(torch.int32)).all())
    print('fills {} {}: non-finite {} / {}, same bits {}'.format(tag, _sid(shape), bad[0], bad[1], same))
    assert bad == (0, 0) and same
    _check('fills {} {}'.format(tag, _sid(shape)), g0, c.ref())


SLAB_SHAPE = (1, 27)


@pytest.mark.parametrize('n', [15, 30])
def test_columns_cross_a_slab_and_phases_a_chunk(models, n):
    """Two constants of csrc/wn_deconv_bwd.hip cut reductions; the shapes are chosen against both.
    DB_SLAB cuts the reduction of a weight-gradient GEMM -- the columns (batch row x frames padded to 32) of a layer -- into
    partial sums of 4096 columns.  The last layer of F = 27 has 270 frames, 288 padded columns per row: 15 rows are 4320
    columns, so the second slab starts at frame 64 of row 14; 30 rows are 8640 columns, three slabs.
    DB_WGS = 1024 sizes the phase chunks of the data-gradient GEMM: with t = (Cin / 64) ceil(270 / 64) B = 5 B tiles it runs
    ceil(S / ceil(1024 / t)) of the S = 20 phases per workgroup.  One row: 20 chunks of one phase; 15 rows: 10 chunks of 2;
    30 rows: chunks of 3, the seventh and last a ragged one of 2 phases.
    The rows are n copies of one row with n copies of its cotangent, held to n times the oracle's gradient of that row at
    the same bar."""
    m = models('small')
    c = m.case(SLAB_SHAPE)
    many = m.eng.deconv_backward(c.MEL.repeat(n, 1, 1), c.G.repeat(n, 1, 1))
    _check('slab x{} {}'.format(n, _sid(SLAB_SHAPE)), many['grads'], c.ref(), scale=float(n))


def test_taps_read_the_left_pad(models):
    """A cotangent only at the first output sample of every row: z[0] = sum_q W[pL - S q] x[q], so of the last layer's kernel
    (K = 80, S = 20, pL = 30) only k = 30 (q = 0) and k = 10 (q = 1) multiply an input frame; k = 50 and 70 reach sample 0 through
    the zero left pad only, every other k not at all: their gradients are exactly zero.  A cotangent only at the last sample
    of row 0 stays within the bar."""
    import torch
    m = models('wide')
    c = m.case((3, 2))
    first = torch.zeros_like(c.g)
    first[:, 0] = c.g[:, 0]
    res = m.eng.deconv_backward(c.MEL, first.cuda())
    w = res['grads']['trans_conv_2/kernel']
    for k in range(w.shape[1]):
        if k in (10, 30):
            assert float(w[0, k].abs().max()) > 0, k
        else:
            assert float(w[0, k].abs().max()) == 0, k
    _check('t=0 wide B3-F2', res['grads'], c.ref(first))
    last = torch.zeros_like(c.g)
    last[0, -1] = c.g[0, -1]
    res = m.eng.deconv_backward(c.MEL, last.cuda())
    _check('t=TE-1 row 0 wide B3-F2', res['grads'], c.ref(last))


def test_public_chain_bits(models):
    """loss_and_weight_grads(upsampler=True): stack and head gradients, loss and d_encoding are the bits of the default call,
    the upsampler gradients the bits of Engine.deconv_backward(mel, d_encoding)."""
    import torch
    m = models('small')
    shape = (2, 3, 512)
    mel, x = TS._inputs(shape[1], shape[2], TS.ROW_SEEDS[shape])
    inputs = {'wav': torch.as_tensor(x).cuda(), 'mel': torch.as_tensor(mel).cuda()}
    base = m.net.loss_and_weight_grads(inputs)
    assert sorted(base) == ['d_encoding', 'flat_grads', 'grads', 'log_probs', 'loss'] and not any('trans_conv' in k for k in base['grads'])
    full = m.net.loss_and_weight_grads(inputs, upsampler=True)
    for k in ('loss', 'log_probs', 'flat_grads', 'd_encoding'):
        assert torch.equal(full[k].view(torch.int32), base[k].view(torch.int32)), k
    up = m.eng.deconv_backward(inputs['mel'], base['d_encoding'])
    assert torch.equal(full['flat_upsampler_grads'].view(torch.int32), up['flat_grads'].view(torch.int32))
    assert sorted(full['grads']) == sorted(list(base['grads']) + DG.names(2))
    for k in base['grads']:
        assert torch.equal(full['grads'][k], base['grads'][k]), k
    for k in DG.names(2):
        assert torch.equal(full['grads'][k], up['grads'][k]), k


def _oracle_loss(w, thp, dc, act, x, mel, tag):
    import torch
    enc = DG.stack_ff(mel, w, dc, act)[1]
    out = D.teacher_ff(torch.as_tensor(x.astype(np.float64)), enc, w, thp)
    return -N.teacher_log_prob(out, torch.as_tensor(x.astype(np.float64)), tag, False).mean()


@pytest.mark.parametrize('which', ['upsampler', 'all'])
def test_descent_through_the_public_api(models, which):
    """The protocol of tests/test_gpu_teacher_wgrad.py::test_descent_through_the_public_api with the upsampler in the step:
    loss_and_weight_grads(upsampler=True), then load_weights(w - eps g) on a fresh Wavenet lowers 'loss'.  eps is chosen on the
    float64 oracle alone (its own decrease at least 1e-3 and within 5 % of eps |g|^2); the engine's decrease must be within
    10 % of the oracle's.  The step is taken on the upsampler's variables only, then on every variable."""
    import torch
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    m = models('small')
    tag, shape = 'mol', (2, 3, 512)
    B, F, T = shape
    mel, x = TS._inputs(F, T, TS.ROW_SEEDS[shape])
    thp, w64 = D.teacher_weights(m.cfgd, m.seed, m.init)
    names = DG.names(2) if which == 'upsampler' else sorted(w64)
    leaves = {k: w64[k].clone().requires_grad_(True) for k in names}
    wl = dict(w64)
    wl.update(leaves)
    L0 = _oracle_loss(wl, thp, m.dc, m.act, x, mel, tag)
    g64 = dict(zip(names, torch.autograd.grad(L0, [leaves[k] for k in names], allow_unused=True)))
    g64 = {k: torch.zeros_like(w64[k]) if v is None else v for k, v in g64.items()}
    gg = float(sum((v ** 2).sum() for v in g64.values()))
    eps, dec64 = None, None
    for e in [2.0 ** -j for j in range(0, 24)]:
        stepped = dict(w64)
        stepped.update({k: w64[k] - e * g64[k] for k in names})
        with torch.no_grad():
            dec = float(L0.detach()) - float(_oracle_loss(stepped, thp, m.dc, m.act, x, mel, tag))
        if dec >= 1e-3 and abs(dec - e * gg) <= 0.05 * e * gg:
            eps, dec64 = e, dec
            break
    assert eps is not None, 'no step on the oracle is both large enough and in the linear regime'
    X, MEL = torch.as_tensor(x).cuda(), torch.as_tensor(mel).cuda()
    res = m.net.loss_and_weight_grads({'wav': X, 'mel': MEL}, upsampler=True)
    assert sorted(res['grads']) == sorted(w64)
    new = dict(m.w32)
    for k in names:
        new[k] = (m.w32[k].astype(np.float64) - eps * res['grads'][k].double().cpu().numpy()).astype(np.float32)
    net2 = Wavenet(m.cfgd).load_weights(new)
    with torch.no_grad():
        after = net2.calculate_loss(net2.feed_forward({'wav': X, 'mel': MEL}))
    dec = float(res['loss']) - float(after['loss'])
    print('descent ({}): eps {:.3e}, |g|^2 {:.4e}, oracle loss {:.6f} decrease {:.4e}; engine loss {:.6f} decrease {:.4e}'.format(
        which, eps, gg, float(L0.detach()), dec64, float(res['loss']), dec))
    net2.engine.close()
    assert dec > 0
    assert abs(dec - dec64) <= 0.10 * dec64, (dec, dec64)


@pytest.mark.parametrize('shape', [(1, 1), (3, 2)], ids=_sid)
def test_student_scope(student_cfg, shape):
    """deconv_backward on a student handle's shared stack (scope 'iaf_share', as its config defines) meets the same oracle"""
    import torch
    from nsynth_wavenet_amd.engine import Engine
    from nsynth_wavenet_amd import weights as wts, config as cfg
    cfgd = dict(student_cfg, num_iaf_layers=[3, 2])
    assert cfgd['use_share_deconv'] and cfgd['upsample_act'] == 'leaky_relu'
    w = wts.synthetic_weights(cfg.load_hparams(cfgd), seed=9, init='unit')
    dc = cfgd['deconv_config']
    w64 = DG.weights64(w, len(dc), 'iaf_share')
    B, F = shape
    mel, seeds = DG.pick_rows(B, F, w64, dc, 'leaky_relu', 'iaf_share')
    g = torch.as_tensor(np.random.RandomState(707).standard_normal([B, F * 200, cfgd['deconv_width']]).astype(np.float32))
    g, zeroed, hidden = DG.mask_last(g, mel, w64, dc, 'leaky_relu', 'iaf_share')
    assert hidden == 0
    print('student {}: row seeds {}, {} cotangent elements zeroed'.format(_sid(shape), seeds, zeroed))
    eng = Engine(cfgd).load_weights(w)
    try:
        assert [t[0] for t in eng.deconv_grad_table('iaf_share')] == DG.names(len(dc), 'iaf_share')
        res = eng.deconv_backward(mel, g, scope='iaf_share')
        _check('student ' + _sid(shape), res['grads'], DG.grads(mel, w64, dc, 'leaky_relu', g.double(), 'iaf_share'))
        with pytest.raises(ValueError, match="no deconv stack with scope ''"):
            eng.deconv_backward(mel, g, scope='')
    finally:
        eng.close()


def test_refusals(models, student_cfg):
    import torch
    from oracle import wavenet_np as O
    from nsynth_wavenet_amd.engine import Engine
    from nsynth_wavenet_amd import weights as wts, config as cfg
    m = models('small')
    c = m.case((1, 1))
    eng = m.eng
    with pytest.raises(ValueError, match="no deconv stack with scope 'iaf_7'"):
        eng.deconv_backward(c.MEL, c.G, scope='iaf_7')
    assert eng.deconv_grad_table('iaf_7') == []
    with pytest.raises(ValueError, match='d_encoding must be'):
        eng.deconv_backward(c.MEL, c.G[:, :-1])
    lib, h = eng.lib, eng._h
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    n_g = int(lib.wn_deconv_grad_floats(h, b''))
    n_ws = int(lib.wn_deconv_backward_workspace_bytes(h, b'', c.B, c.F))
    flat = torch.empty(n_g, dtype=torch.float32, device='cuda')
    ws = torch.empty(n_ws, dtype=torch.uint8, device='cuda')
    rc = lib.wn_deconv_backward(h, b'', ptr(c.MEL), ptr(c.G), c.B, c.F, ptr(flat), n_g - 1, ptr(ws), n_ws, eng._stream())
    assert rc == -22 and b'grads holds' in lib.wn_last_error(h)
    rc = lib.wn_deconv_backward(h, b'', ptr(c.MEL), ptr(c.G), c.B, c.F, ptr(flat), n_g, ptr(ws), n_ws - 1, eng._stream())
    assert rc == -22 and b'workspace' in lib.wn_last_error(h)
    rc = lib.wn_deconv_backward(h, b'', ptr(c.MEL), None, c.B, c.F, ptr(flat), n_g, ptr(ws), n_ws, eng._stream())
    assert rc == -22 and b'bad argument' in lib.wn_last_error(h)
    mel = c.mel
    g = c.g

    def refused(e, match, scope=''):
        try:
            assert e.deconv_grad_table(scope) == []
            with pytest.raises(ValueError, match=match):
                e.deconv_backward(mel, g if g.shape[2] == int(e.hp.deconv_width) else g.repeat(1, 1, 4), scope=scope)
        finally:
            e.close()
    # a handle that is not finalized: WN_ESTATE, like wn_deconv
    e = Engine(m.cfgd)
    try:
        assert e.deconv_grad_table() == []
        with pytest.raises(RuntimeError, match='wn_finalize'):
            e.deconv_backward(mel, g)
    finally:
        e.close()
    # use_resize_conv
    cfgd = dict(m.cfgd, use_resize_conv=True)
    refused(Engine(cfgd).load_weights(O.synth_weights(O.HP(cfgd), 'teacher', seed=5, init='unit')), 'use_resize_conv')
    # use_weight_norm (a student's shared stack)
    cfgd = dict(student_cfg, use_weight_norm=True, num_iaf_layers=[3, 2])
    refused(Engine(cfgd).load_weights(wts.synthetic_weights(cfg.load_hparams(cfgd), seed=9, init='unit')), 'use_weight_norm',
            'iaf_share')
    # a first layer of three taps over 80 mel channels has 15 sixteen-channel blocks, no whole number of K-steps: no split pack
    cfgd = dict(m.cfgd, deconv_config=[[30, 10], [80, 20]])
    refused(Engine(cfgd).load_weights(O.synth_weights(O.HP(cfgd), 'teacher', seed=5, init='unit')), 'no split-fp16 pack')
    # a deconv_width that is no multiple of 64 never becomes a handle: wn_create refuses the config
    with pytest.raises(ValueError, match='deconv_width'):
        Engine(dict(m.cfgd, deconv_width=96))
