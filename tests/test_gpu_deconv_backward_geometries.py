"""wn_deconv_backward (csrc/wn_deconv_bwd.hip) off the one deconv_config every other test runs it on: the nine
accepted geometries of tests/deconv_bwd_geometries.py on both handle kinds -- the 256-wide student stack (scope
'iaf_share') and the 64-wide teacher stack (scope '') -- through Engine.deconv_backward against
deconv_grad_oracle64.grads in float64, every element of every tensor, at the bar of tests/test_gpu_deconv_backward.py
(TOL = 1e-4 max |g64| per tensor, imported).  Every case prints what it measured before it asserts; DESIGN.md 25 has the
largest per tag and handle.

  1  tanh, dense cotangent, every tag and handle at (1, 1), (3, 2) and (3, F_slab): two weight-gradient slabs, the second one
     K-step; ragged data-gradient and de-interleave tiles.  tanh has no ties and a derivative that differs per element.
  2  phase chunks of the data-gradient GEMM (pchunk >= 2), ragged where the stride allows it at small size
  3  one non-zero cotangent sample: t = 0, the last sample of row 0, and t = 16 S_last (second de-interleave tile)
  4  leaky-relu under the tie rules of tests/deconv_grad_oracle64.py, unchanged
  5  relu: the reverse pass, and the forward no other test runs (Engine.deconv rows at both precisions, iaf_generate)
  6  repeated call, pre-filled workspaces and power-of-two scaling give the same bits; an fp32 handle gives the default's bits
  7  the public chain Wavenet.loss_and_weight_grads(upsampler=True) on the three-layer teacher
  8  the refused geometries, by message

The restatement of layer_dims that the shapes rest on is asserted on the CPU (tests/test_deconv_grad_oracle.py)."""
import ctypes

import numpy as np
import pytest

import deconv_bwd_geometries as BG
import deconv_grad_oracle64 as DG
import distill_oracle64 as D
import teacher_nll_oracle64 as N
import test_gpu_deconv_backward as TD
import test_gpu_deconv_geometries as TF
import test_gpu_teacher_geometries as TGEO
import test_gpu_teacher_shapes as TS
import test_gpu_teacher_wgrad as TW

pytestmark = pytest.mark.gpu
TOL = TD.TOL
KINDS = ('teacher', 'student')


def _sid(s):
    return 'B{}-F{}'.format(*s)


class _Handle(object):
    """one engine handle of (kind, tag, activation) and its float64 weights"""

    def __init__(self, kind, tag, act, precision=None, **extra):
        from nsynth_wavenet_amd.engine import Engine
        self.kind, self.tag, self.act = kind, tag, act
        self.cfgd = BG.cfg_of(kind, tag, upsample_act=act, **extra)
        self.dc, self.width = self.cfgd['deconv_config'], int(self.cfgd['deconv_width'])
        self.scope = BG.scope_of(kind) if self.cfgd.get('use_share_deconv', True) or kind == 'teacher' else 'iaf_1'
        self.w32 = BG.weights(kind, self.cfgd)
        self.w64 = DG.weights64(self.w32, len(self.dc), self.scope)
        self.eng = Engine(self.cfgd, precision=precision).load_weights(self.w32)
        self.cases = {}

    def case(self, shape, gseed=101):
        if (shape, gseed) not in self.cases:
            self.cases[(shape, gseed)] = _Case(self, shape, gseed)
        return self.cases[(shape, gseed)]

    def backward(self, mel, g):
        return self.eng.deconv_backward(mel, g, scope=self.scope)


class _Case(object):
    """mel rows by the oracle's rule, a dense standard-normal cotangent masked at the last layer's near ties (tanh: none)"""

    def __init__(self, h, shape, gseed):
        import torch
        self.h, (self.B, self.F) = h, shape
        self.mel, self.seeds = DG.pick_rows(self.B, self.F, h.w64, h.dc, h.act, h.scope)
        g = torch.as_tensor(np.random.RandomState(gseed).standard_normal([self.B, self.F * BG.hop(h.tag), h.width]).astype(np.float32))
        self.g, self.zeroed, hidden = DG.mask_last(g, self.mel, h.w64, h.dc, h.act, h.scope)
        assert hidden == 0
        self.MEL = torch.as_tensor(self.mel).cuda()

    def ref(self, g=None):
        """not kept: the large shapes are used once"""
        return DG.grads(self.mel, self.h.w64, self.h.dc, self.h.act, (self.g if g is None else g).double(), self.h.scope)


@pytest.fixture(scope='module')
def handles():
    made = {}

    def get(kind, tag, act='tanh'):
        if (kind, tag, act) not in made:
            made[kind, tag, act] = _Handle(kind, tag, act)
        return made[kind, tag, act]
    yield get
    for h in made.values():
        h.eng.close()


def _run(h, shape, label):
    c = h.case(shape)
    print('{}: row seeds {}, {} of {} cotangent elements zeroed at last-layer ties'.format(label, c.seeds, c.zeroed, c.g.numel()))
    tab = h.eng.deconv_grad_table(h.scope)
    assert [t[0] for t in tab] == DG.names(len(h.dc), h.scope)
    res = h.backward(c.MEL, c.g.cuda())
    assert res['flat_grads'].numel() == sum(int(np.prod(t[2])) for t in tab)
    return TD._check(label, res['grads'], c.ref())


# ---- 1. tanh, dense cotangent ----
TANH = [(kind, tag, s) for tag in BG.TAGS for kind in KINDS for s in BG.tanh_shapes(tag)]


@pytest.mark.parametrize('kind,tag,shape', TANH, ids=['{}-{}-{}'.format(k, t, _sid(s)) for k, t, s in TANH])
def test_tanh_gradients_match_the_oracle(handles, kind, tag, shape):
    h = handles(kind, tag)
    d = BG.layer_dims(h.dc, h.width, *shape)
    print('DECONV-BWD-GEO 1 {} {} {}: last layer L {} Lp {} nslab {} R {}'.format(kind, tag, _sid(shape), d[-1]['L'], d[-1]['Lp'],
                                                                                 d[-1]['nslab'], d[-1]['R']))
    _run(h, shape, 'DECONV-BWD-GEO 1 {} {} {}'.format(kind, tag, _sid(shape)))
    del h.cases[(shape, 101)]


def test_tanh_private_stacks_and_width_128(handles):
    """a student with one stack per flow (use_share_deconv off, scope 'iaf_1') on taps6, and a teacher of deconv_width 128
    on three: its hidden layers have C / 64 x cinp / 64 = 2 x 2 weight-gradient tiles, between the 1 x 1 of width 64 and the
    4 x 4 of width 256"""
    hs = [_Handle('student', 'taps6', 'tanh', use_share_deconv=False), _Handle('teacher', 'three', 'tanh', deconv_width=128)]
    try:
        assert hs[0].scope == 'iaf_1' and hs[0].eng.iaf_stack_scopes() == ['iaf_1']
        for h in hs:
            for shape in [(1, 1), (3, 2)]:
                _run(h, shape, 'DECONV-BWD-GEO 1 {} {} width {} scope {!r} {}'.format(h.kind, h.tag, h.width, h.scope, _sid(shape)))
    finally:
        for h in hs:
            h.eng.close()


# ---- 2. phase chunks ----
@pytest.mark.parametrize('tag,shape,layer,chunks', BG.PCHUNK_SHAPES,
                         ids=['{}-{}-layer{}'.format(t, _sid(s), l % len(BG.ACCEPTED[t]) + 1) for t, s, l, _ in BG.PCHUNK_SHAPES])
def test_phases_share_a_workgroup(handles, tag, shape, layer, chunks):
    """The data-gradient GEMM runs pchunk >= 2 phases per workgroup and db_dxsum_kernel adds npc chunks, the last one ragged
    on hop256 (16 = 5 x 3 + 1), taps6 (8 = 3 + 3 + 2) and taps8 (20 = 6 x 3 + 2).  'three' has two shapes: (3, 225) for its
    last layer (L = 8 F) and (3, 897) for its middle layer (L = 2 F), where the last layer runs all four phases in one
    workgroup."""
    h = handles('student', tag)
    d = BG.layer_dims(h.dc, h.width, *shape)[layer]
    assert (d['pchunk'], d['npc']) == chunks
    _run(h, shape, 'DECONV-BWD-GEO 2 {} {} layer {} pchunk {} npc {}'.format(tag, _sid(shape), layer % len(h.dc) + 1, *chunks))
    del h.cases[(shape, 101)]


# ---- 3. one non-zero cotangent sample ----
@pytest.mark.parametrize('tag', BG.TAGS)
@pytest.mark.parametrize('kind', KINDS)
def test_single_samples_reach_the_edge_taps(handles, kind, tag):
    """Only t = 0, only the last sample of row 0, only t = 16 S_last (the first sample of the second de-interleave tile): the
    edge taps and the tile seam with nothing to average them away.  (1, 2), except that 'three' (TE = 64 = 16 S_last) and
    'single' (two frames) have no second tile there: their third cotangent is at the smallest F that has one, 3 and 17."""
    import torch
    h = handles(kind, tag)
    S = h.dc[-1][1]
    for name, F, t in (('t=0', 2, 0), ('t=TE-1', 2, 2 * BG.hop(tag) - 1), ('t=16S', BG.f_second_tile(tag), S * BG.DB_FT)):
        c = h.case((1, F), 303)
        one = torch.zeros_like(c.g)
        assert 0 <= t < one.shape[1]
        one[0, t] = c.g[0, t]
        res = h.backward(c.MEL, one.cuda())
        TD._check('DECONV-BWD-GEO 3 {} {} B1-F{} {}'.format(kind, tag, F, name), res['grads'], c.ref(one))


# ---- 4. leaky-relu ----
LEAKY = BG.leaky_cases()


@pytest.mark.parametrize('kind,tag,shape', LEAKY, ids=['{}-{}-{}'.format(k, t, _sid(s)) for k, t, s in LEAKY])
def test_leaky_relu_gradients_match_the_oracle(handles, kind, tag, shape):
    """The shipped activation, and the sign taken from y in the G4 words: first clear seeds from 2001, at most 0.1 % of the
    cotangent zeroed, no hidden tie (asserted by pick_rows / mask_last).  The one case left out, the 64-wide s6 at (1, 1), is
    held to still miss the rule by tests/test_deconv_grad_oracle.py on the CPU."""
    _run(handles(kind, tag, 'leaky_relu'), shape, 'DECONV-BWD-GEO 4 {} {} {}'.format(kind, tag, _sid(shape)))


# ---- 5. relu ----
RELU = [(kind, tag, s) for tag in BG.RELU_TAGS for kind in KINDS for s in BG.RELU_SHAPES]


@pytest.mark.parametrize('kind,tag,shape', RELU, ids=['{}-{}-{}'.format(k, t, _sid(s)) for k, t, s in RELU])
def test_relu_gradients_match_the_oracle(handles, kind, tag, shape):
    _run(handles(kind, tag, 'relu'), shape, 'DECONV-BWD-GEO 5 {} {} {}'.format(kind, tag, _sid(shape)))


@pytest.mark.parametrize('tag', BG.RELU_TAGS)
def test_relu_forward(handles, tag):
    """deconv_act's relu branch: Engine.deconv rows with split-fp16 and fp32 GEMMs, and the G4 words through iaf_generate on
    the student handle, against oracle.wavenet_np in float64 at the bars of tests/test_gpu_deconv_geometries.py."""
    from oracle import wavenet_np as O
    from nsynth_wavenet_amd.engine import Engine
    h = handles('student', tag, 'relu')
    hp = O.HP(h.cfgd)
    f32 = Engine(h.cfgd, precision='f32').load_weights(h.w32)
    try:
        rs = np.random.RandomState(41)
        for B, F in ((1, 1), (3, 2), (2, BG.f_a(tag))):
            mel = rs.uniform(0, 1, [B, F, BG.N_MEL]).astype(np.float32)
            ref = O.deconv_stack(mel, h.w32, hp, h.scope, np.float64)
            assert float(ref.min()) == 0.0 and float((ref == 0).mean()) > 0.05, 'relu'
            scale = max(1.0, np.abs(ref).max())
            err = {}
            for p, e in (('f16x3', h.eng), ('f32', f32)):
                got = TF._np(e.deconv(mel))
                assert got.shape == ref.shape and np.isfinite(got).all()
                err[p] = float(np.abs(got - ref).max())
                print('DECONV-BWD-GEO 5 forward {} {} B={} F={}: {:.2e} of the range'.format(tag, p, B, F, err[p] / scale))
            for p in err:
                assert err[p] <= TF.BAR * scale, (tag, p, B, F, err[p])
            assert err['f16x3'] <= 2 * err['f32'] + 1e-7 * scale, (tag, B, F, err)
        for B, F in ((2, BG.f_crop(tag)),):
            mel, noise, T = BG.student_inputs(tag, B, F)
            assert T == O.iaf_length(F, hp) > 0
            ref = O.iaf_feed_forward(mel, noise, h.w32, hp, np.float64)
            for p, e in (('f16x3', h.eng), ('f32', f32)):
                out = e.iaf_generate(mel, noise, want=TF.OUTS)
                for k in TF.OUTS:
                    r = TF._rel(TF._np(out[k]), ref[k])
                    print('DECONV-BWD-GEO 5 iaf_generate {} {} B={} F={} {}: {:.2e} of the range'.format(tag, p, B, F, k, r))
                    assert r <= TF.BAR, (tag, p, B, F, k, r)
    finally:
        f32.close()


# ---- 6. properties ----
def _raw(h, c, g, fill):
    """the call through the C ABI on buffers of exactly the sizes the library asks for, every byte pre-set to `fill`"""
    import torch
    from nsynth_wavenet_amd import _lib
    eng, sc = h.eng, h.scope.encode()
    lib, hd = eng.lib, eng._h
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    with torch.cuda.device(eng.device):
        n_ws = int(lib.wn_deconv_backward_workspace_bytes(hd, sc, c.B, c.F))
        n_g = int(lib.wn_deconv_grad_floats(hd, sc))
        assert min(n_ws, n_g) > 0
        ws = torch.full((n_ws,), fill, dtype=torch.uint8, device='cuda')
        flat = torch.full((n_g,), fill, dtype=torch.uint8, device='cuda').repeat(4).view(torch.float32)
        assert flat.numel() == n_g
        _lib.check(lib.wn_deconv_backward(hd, sc, ptr(c.MEL), ptr(g), c.B, c.F, ptr(flat), n_g, ptr(ws), n_ws, eng._stream()), hd)
        torch.cuda.synchronize()
    return flat


@pytest.mark.parametrize('tag', BG.TAGS)
def test_bits_repeat_ignore_the_workspace_and_scale(handles, tag):
    """(3, 2) on the student handle: a repeated call, workspaces pre-filled with 0x00 and 0xFF (every fp16 and fp32 word a
    NaN) and a cotangent scaled by 2^-40 and 2^20 give the same bits (scaled)."""
    import torch
    h = handles('student', tag)
    c = h.case((3, 2), 404)
    G = c.g.cuda()
    base = h.backward(c.MEL, G)['flat_grads']
    TD._check('DECONV-BWD-GEO 6 {}'.format(tag), h.backward(c.MEL, G)['grads'], c.ref())
    bits = lambda t: t.view(torch.int32)
    assert torch.equal(bits(h.backward(c.MEL, G)['flat_grads']), bits(base)), 'repeat differs'
    f0, f1 = _raw(h, c, G, 0x00), _raw(h, c, G, 0xFF)
    bad = int((~torch.isfinite(f0)).sum()), int((~torch.isfinite(f1)).sum())
    print('DECONV-BWD-GEO 6 {}: non-finite {} / {}'.format(tag, *bad))
    assert bad == (0, 0) and torch.equal(bits(f0), bits(f1)) and torch.equal(bits(f0), bits(base))
    for k in (-40, 20):
        f = 2.0 ** k
        assert float(base.abs().max()) > 0 and torch.equal(base * f / f, base)
        assert torch.equal(bits(h.backward(c.MEL, G * f)['flat_grads']), bits(base * f)), k


def test_an_fp32_handle_gives_the_default_handles_bits(handles):
    """the call reruns the forward in split-fp16 whatever the handle's precision"""
    import torch
    h = handles('student', 'taps6')
    c = h.case((3, 2), 404)
    f32 = _Handle('student', 'taps6', 'tanh', precision='f32')
    try:
        a, b = h.backward(c.MEL, c.g.cuda())['flat_grads'], f32.backward(c.MEL, c.g.cuda())['flat_grads']
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    finally:
        f32.eng.close()


# ---- 7. the public chain ----
CHAIN_SHAPE = (2, 16, 512)


def test_public_chain_on_three_layers():
    """Wavenet.loss_and_weight_grads(batch, upsampler=True) on teacher_cfg('three') (leaky-relu, the shipped activation) at
    (2, 16): T = 512 = the whole encoding.  The body and bars of test_gpu_teacher_geometries.test_public_chain: mel rows are
    pick_rows' clear seeds, the last layer's near ties take the engine's sign (at most 0.1 % of them), the stack's pre-ReLU
    near ties the tape's; x rows are the two seeds of 1001 .. 1012 with the fewest near values."""
    import torch
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    B, F, T = CHAIN_SHAPE
    cfgd = BG.teacher_cfg('three')
    dc, act = cfgd['deconv_config'], cfgd['upsample_act']
    assert act == 'leaky_relu' and len(dc) == 3 and F * BG.hop('three') == T
    thp, w64 = D.teacher_weights(cfgd, BG.SEED, BG.INIT)
    w32 = BG.weights('teacher', cfgd)
    mel, mseeds = DG.pick_rows(B, F, DG.weights64(w32, len(dc)), dc, act)
    count = {s: TS._Oracle(cfgd, BG.SEED, BG.INIT, mel[:1], TS._inputs(F, T, (s,))[1]).near for s in range(1001, 1013)}
    xseeds = tuple(sorted(count, key=lambda s: (count[s], s))[:B])
    x = TS._inputs(F, T, xseeds)[1]
    ora = TS._Oracle(cfgd, BG.SEED, BG.INIT, mel, x)
    n_pre = sum(v.numel() for v in ora.pre.values())
    cap = TGEO._near_cap(cfgd, CHAIN_SHAPE)
    assert ora.near <= cap, (ora.near, n_pre)
    pre, enc64 = DG.stack_ff(mel, w64, dc, act)
    assert float((enc64 - ora.enc).abs().max()) <= 1e-9 * float(ora.enc.abs().max())
    assert sum(int(DG.near(z).sum()) for z in pre[:-1]) == 0, 'a hidden pre-activation is a near tie'
    near_last = DG.near(pre[-1])
    n_last = int(near_last.sum())
    assert n_last <= DG.MAX_ZEROED * near_last.numel(), (n_last, near_last.numel())
    net = Wavenet(cfgd).load_weights(w32)
    eng = net.engine
    try:
        X, MEL = torch.as_tensor(x).cuda(), torch.as_tensor(mel).cuda()
        res = net.loss_and_weight_grads({'wav': X, 'mel': MEL}, upsampler=True)
        L_plain = float(TD._oracle_loss(w64, thp, dc, act, x, mel, 'mol'))
        e_loss = abs(float(res['loss']) - L_plain) / max(1.0, abs(L_plain))
        print('DECONV-BWD-GEO 7 loss {:.7f}, oracle {:.7f}: error / max(1, |oracle|) = {:.2e}'.format(float(res['loss']), L_plain, e_loss))
        _, tape = eng.teacher_forward_tape(X, MEL)
        masks, nflip = D.relu_masks(ora.pre, D.tape_pre(tape, B, T, cfgd['skip_width']))
        assert nflip <= cap, nflip
        pos_dev = (eng.deconv(MEL).double().cpu() > 0).transpose(1, 2)
        pos = torch.where(near_last, pos_dev, pre[-1] > 0)
        nflip_up = int((pos != (pre[-1] > 0)).sum())
        assert nflip_up <= n_last
        slope = torch.where(pos, 1.0, 0.4).double()
        print('DECONV-BWD-GEO 7: {} near-tie pre-ReLU values of {} ({} signs from the tape, x seeds {}); mel seeds {}, {} of {} '
              'last-layer pre-activations near ties ({} signs from the engine)'.format(ora.near, n_pre, nflip, xseeds, mseeds, n_last,
                                                                                      near_last.numel(), nflip_up))
        names = sorted(w64)
        leaves = {k: w64[k].clone().requires_grad_(True) for k in names}
        x64 = torch.as_tensor(x.astype(np.float64))
        out64 = D.teacher_ff(x64, TGEO._stack_grad_graph(mel, leaves, dc, slope), leaves, thp, masks=masks)
        L = -N.teacher_log_prob(out64, x64, 'mol', False).mean()
        assert abs(float(L.detach()) - L_plain) <= 1e-9 * abs(L_plain), 'the masks change no value'
        ref = dict(zip(names, torch.autograd.grad(L, [leaves[k] for k in names], allow_unused=True)))
        assert sorted(res['grads']) == names and set(DG.names(3)) <= set(names)
        last = 'res_%d/' % cfgd['num_layers']
        worst, failed = {'stack': 0.0, 'upsampler': 0.0}, []
        for k in names:
            got = res['grads'][k]
            assert tuple(got.shape) == tuple(w64[k].shape) and TS._all_finite(got), k
            if ref[k] is None or float(ref[k].abs().max()) == 0:
                assert k.startswith(last) and float(got.abs().max()) == 0, k
                continue
            e = TW._err(got, ref[k])
            part = 'stack' if TW._is_stack(k) else 'upsampler'
            worst[part] = max(worst[part], e)
            print('DECONV-BWD-GEO 7 {:24s} max |g - g64| / max |g64| = {:.2e} (max |g64| {:.3e})'.format(k, e, float(ref[k].abs().max())))
            if e > TOL:
                failed.append((k, e))
        print('DECONV-BWD-GEO 7 largest relative error: stack and head {:.2e}, upsampler {:.2e}'.format(worst['stack'], worst['upsampler']))
        assert e_loss <= TGEO.TOL_CHAIN, e_loss
        assert not failed, failed
    finally:
        eng.close()


# ---- 8. refusals ----
@pytest.mark.parametrize('tag', sorted(BG.REFUSED))
@pytest.mark.parametrize('kind', KINDS)
def test_refused_geometries_are_refused_by_name(kind, tag):
    """the queries return 0 and the table is empty; deconv_backward names the reason; the re-pack takes no up_params
     and changes nothing"""
    import torch
    from nsynth_wavenet_amd.engine import Engine
    dc, resize, why = BG.REFUSED[tag]
    cfgd = BG.cfg_of(kind, tag)
    scope, sc = BG.scope_of(kind), BG.scope_of(kind).encode()
    w = BG.weights(kind, cfgd)
    eng = Engine(cfgd).load_weights(w)
    try:
        lib, hd = eng.lib, eng._h
        assert int(lib.wn_deconv_grad_count(hd, sc)) == 0 and int(lib.wn_deconv_grad_floats(hd, sc)) == 0
        assert int(lib.wn_deconv_backward_workspace_bytes(hd, sc, 1, 1)) == 0
        assert eng.deconv_grad_table(scope) == [] and eng.deconv_grad_floats(scope) == 0
        mel = np.random.RandomState(3).uniform(0, 1, [1, 1, BG.N_MEL]).astype(np.float32)
        g = np.ones([1, BG.hop(tag), int(cfgd['deconv_width'])], np.float32)
        with pytest.raises(ValueError, match=why):
            eng.deconv_backward(mel, g, scope=scope)
        before = eng.deconv(mel).clone()
        up = torch.zeros(16, dtype=torch.float32, device='cuda')
        msg = 'use_resize_conv' if resize else 'no parameter layout'
        if kind == 'teacher':
            P = torch.zeros(max(eng.teacher_grad_floats(), 1), dtype=torch.float32, device='cuda')
            with pytest.raises(ValueError, match=msg):
                eng.teacher_set_weights(P, up)
        else:
            P = torch.zeros(max(eng.iaf_grad_floats(), 1), dtype=torch.float32, device='cuda')
            with pytest.raises(ValueError, match=msg):
                eng.iaf_set_weights(P, {scope: up})
        assert torch.equal(eng.deconv(mel), before)
    finally:
        eng.close()
