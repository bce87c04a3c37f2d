"""wn_deconv_backward_input (csrc/wn_deconv_bwd.hip) behind Engine.deconv_backward_input: d mel of a deconv stack
against input_grad_oracle64.stack_d_mel in float64, every element, at the project's bar max |g - g64| <= TOL max |g64|
(TOL of tests/test_gpu_distill_grad.py, imported).  Every accepted geometry of tests/deconv_bwd_geometries.py on both handle
kinds -- the 256-wide student stack (scope 'iaf_share') and the 64-wide teacher stack (scope '').  Every case prints what it
measured before it asserts; DESIGN.md 26 has the largest per part.

  1  tanh, dense cotangent: (1, 1), (3, 2), (2, 7), and for 'base' and 'three' (2, 67) -- the first layer's frame axis is F
     itself, so 67 frames cross the 64-frame tile of db_dgrad_kernel with a ragged second tile
  2  phase chunks of the FIRST layer's data-gradient GEMM: two phases per workgroup (every shape of 1 runs one per chunk)
  3  leaky-relu and relu under the tie rules of tests/deconv_grad_oracle64.py (pick_rows seeds, mask_last on the cotangent);
     tests/test_input_grad_oracle.py asserts on the CPU that the chosen seeds stay inside them
  4  the padding rows n_mel .. cinp - 1 never leak: a guard word behind d_mel and a NaN pre-fill, through the C ABI
  5  a cotangent scaled by 2^k scales d_mel bit for bit; two calls give the same bits; a cotangent that is zero in batch row
     0 gives exactly zero there; deconv_backward returns the bits it returned before the new call ran
  6  refusals by message, in the words of wn_deconv_backward
"""
import ctypes

import numpy as np
import pytest

import deconv_bwd_geometries as BG
import input_grad_cases as C
from test_gpu_distill_grad import TOL

pytestmark = pytest.mark.gpu


def _sid(s):
    return 'B{}-F{}'.format(*s)


class _Handle(object):
    def __init__(self, kind, tag, act):
        from nsynth_wavenet_amd.engine import Engine
        self.kind, self.tag, self.act = kind, tag, act
        self.cfgd = BG.cfg_of(kind, tag, upsample_act=act)
        self.scope = BG.scope_of(kind)
        self.w32 = BG.weights(kind, self.cfgd)
        self.eng = Engine(self.cfgd).load_weights(self.w32)

    def case(self, shape, gseed=101):
        return C.DeconvCase(self.kind, self.tag, self.act, shape, gseed, w32=self.w32)

    def d_mel(self, mel, g):
        return self.eng.deconv_backward_input(mel, g, scope=self.scope)


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


def _check(label, got, ref):
    import torch
    assert tuple(got.shape) == tuple(ref.shape) and bool(torch.isfinite(got).all()), label
    scale = float(ref.abs().max())
    assert scale > 0
    e = float((got.double().cpu() - ref).abs().max()) / scale
    print('{} d_mel max |g - g64| / max |g64| = {:.2e} (max |g64| {:.3e})'.format(label, e, scale))
    assert e <= TOL, (label, e)
    return e


def _run(h, shape, label):
    c = h.case(shape)
    seeds = c.seeds if len(c.seeds) <= 8 else '{} .. {}'.format(c.seeds[0], c.seeds[-1])
    print('{}: row seeds {}, {} of {} cotangent elements zeroed at last-layer ties'.format(label, seeds, c.zeroed, c.g.numel()))
    return _check(label, h.d_mel(c.mel, c.g), c.ref())


# ---- 1 ----
TANH = C.tanh_cases()


@pytest.mark.parametrize('kind,tag,shape', TANH, ids=['{}-{}-{}'.format(k, t, _sid(s)) for k, t, s in TANH])
def test_tanh_d_mel_matches_the_oracle(handles, kind, tag, shape):
    _run(handles(kind, tag), shape, 'DECONV-IN 1 {} {} {}'.format(kind, tag, _sid(shape)))


# ---- 2 ----
@pytest.mark.parametrize('tag', BG.TAGS)
def test_first_layer_phases_share_a_workgroup(handles, tag):
    h = handles('student', tag)
    shape = C.chunk_shape(tag)
    pchunk, npc = C.first_layer_chunks(tag, BG.WIDTH['student'], *shape)
    assert pchunk == 2
    _run(h, shape, 'DECONV-IN 2 {} {} first layer pchunk {} npc {}'.format(tag, _sid(shape), pchunk, npc))


# ---- 3 ----
@pytest.mark.parametrize('kind,tag,shape', C.LEAKY, ids=['{}-{}-{}'.format(k, t, _sid(s)) for k, t, s in C.LEAKY])
def test_leaky_relu_d_mel_matches_the_oracle(handles, kind, tag, shape):
    _run(handles(kind, tag, 'leaky_relu'), shape, 'DECONV-IN 3 leaky {} {} {}'.format(kind, tag, _sid(shape)))


@pytest.mark.parametrize('kind,tag,shape', C.RELU, ids=['{}-{}-{}'.format(k, t, _sid(s)) for k, t, s in C.RELU])
def test_relu_d_mel_matches_the_oracle(handles, kind, tag, shape):
    _run(handles(kind, tag, 'relu'), shape, 'DECONV-IN 3 relu {} {} {}'.format(kind, tag, _sid(shape)))


# ---- 4 ----
GUARD = 0x5A


def _raw(h, mel, g, fill, n_ws=None):
    """the call through the C ABI: the workspace of exactly the size the library asks for pre-set to `fill`, d_mel pre-filled
    with NaN and followed by 64 guard bytes -> (d_mel, guard bytes)"""
    import torch
    from nsynth_wavenet_amd import _lib
    eng, sc = h.eng, h.scope.encode()
    lib, hd = eng.lib, eng._h
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    B, F = int(mel.shape[0]), int(mel.shape[1])
    with torch.cuda.device(eng.device):
        n = int(lib.wn_deconv_backward_input_workspace_bytes(hd, sc, B, F)) if n_ws is None else n_ws
        assert n > 0
        ws = torch.full((n,), fill, dtype=torch.uint8, device='cuda')
        n_out = B * F * BG.N_MEL
        buf = torch.full((4 * n_out + 64,), GUARD, dtype=torch.uint8, device='cuda')
        out = buf[:4 * n_out].view(torch.float32)
        out.fill_(float('nan'))
        _lib.check(lib.wn_deconv_backward_input(hd, sc, ptr(mel), ptr(g), B, F, ptr(out), ptr(ws), n, eng._stream()), hd)
        torch.cuda.synchronize()
    return out.view(B, F, BG.N_MEL), buf[4 * n_out:]


@pytest.mark.parametrize('tag', BG.TAGS)
@pytest.mark.parametrize('kind', C.KINDS)
def test_padding_rows_never_leak(handles, kind, tag):
    """n_mel = 80 < cinp = 128: the GEMM's second m-tile holds 48 padding rows, which the last kernel drops.  Every element
    of d_mel is written (no NaN of the pre-fill is left), nothing behind it is (the guard keeps its bytes), and a workspace
    of NaN words gives the bits of a zeroed one -- the bits of the Engine's call."""
    import torch
    h = handles(kind, tag)
    c = h.case((3, 2), 404)
    MEL, G = torch.as_tensor(c.mel).cuda(), c.g.cuda()
    base = h.d_mel(MEL, G)
    bits = lambda t: t.contiguous().view(torch.int32)
    for fill in (0x00, 0xFF):
        out, guard = _raw(h, MEL, G, fill)
        assert int(torch.isnan(out).sum()) == 0, (fill, 'an element of d_mel was not written')
        assert bool((guard == GUARD).all()), (fill, 'a store behind d_mel')
        assert torch.equal(bits(out), bits(base)), fill


# ---- 5 ----
@pytest.mark.parametrize('tag', BG.TAGS)
def test_bits_scale_repeat_rows_and_leave_deconv_backward_alone(handles, tag):
    import torch
    h = handles('student', tag)
    c = h.case((3, 2), 404)
    MEL, G = torch.as_tensor(c.mel).cuda(), c.g.cuda()
    bits = lambda t: t.contiguous().view(torch.int32)
    before = h.eng.deconv_backward(MEL, G, scope=h.scope)['flat_grads'].clone()
    base = h.d_mel(MEL, G)
    _check('DECONV-IN 5 {}'.format(tag), base, c.ref())
    assert torch.equal(bits(h.d_mel(MEL, G)), bits(base)), 'repeat differs'
    for k in (-40, 20):
        f = 2.0 ** k
        assert torch.equal(base * f / f, base)
        assert torch.equal(bits(h.d_mel(MEL, G * f)), bits(base * f)), k
    G0 = G.clone()
    G0[0] = 0
    row0 = h.d_mel(MEL, G0)
    assert int((bits(row0[0]) & 0x7fffffff != 0).sum()) == 0, 'row 0 has a zero cotangent'
    after = h.eng.deconv_backward(MEL, G, scope=h.scope)['flat_grads']
    assert torch.equal(bits(after), bits(before)), 'deconv_backward changed'


# ---- 6 ----
@pytest.mark.parametrize('tag', sorted(BG.REFUSED))
@pytest.mark.parametrize('kind', C.KINDS)
def test_refused_geometries_are_refused_by_name(kind, tag):
    from nsynth_wavenet_amd.engine import Engine
    dc, resize, why = BG.REFUSED[tag]
    cfgd = BG.cfg_of(kind, tag)
    scope = BG.scope_of(kind)
    eng = Engine(cfgd).load_weights(BG.weights(kind, cfgd))
    try:
        assert int(eng.lib.wn_deconv_backward_input_workspace_bytes(eng._h, scope.encode(), 1, 1)) == 0
        mel = np.random.RandomState(3).uniform(0, 1, [1, 1, BG.N_MEL]).astype(np.float32)
        g = np.ones([1, BG.hop(tag), int(cfgd['deconv_width'])], np.float32)
        with pytest.raises(ValueError, match='wn_deconv_backward_input: .*' + why):
            eng.deconv_backward_input(mel, g, scope=scope)
    finally:
        eng.close()


def test_refusals(handles):
    """an unknown scope, a handle that is not finalized, a workspace one byte short, null arguments; the size query returns
    0 for what the work call refuses"""
    import torch
    from nsynth_wavenet_amd.engine import Engine
    h = handles('student', 'base')
    c = h.case((3, 2), 404)
    MEL, G = torch.as_tensor(c.mel).cuda(), c.g.cuda()
    eng, lib, hd = h.eng, h.eng.lib, h.eng._h
    with pytest.raises(ValueError, match="wn_deconv_backward_input: no deconv stack with scope 'iaf_7'"):
        eng.deconv_backward_input(MEL, G, scope='iaf_7')
    with pytest.raises(ValueError, match="no deconv stack with scope ''"):
        eng.deconv_backward_input(MEL, G, scope='')
    assert int(lib.wn_deconv_backward_input_workspace_bytes(hd, b'iaf_7', 3, 2)) == 0
    assert int(lib.wn_deconv_backward_input_workspace_bytes(hd, b'iaf_share', 0, 2)) == 0
    assert int(lib.wn_deconv_backward_input_workspace_bytes(hd, b'iaf_share', 3, 0)) == 0
    with pytest.raises(ValueError, match='d_encoding must be'):
        eng.deconv_backward_input(MEL, G[:, :-1], scope=h.scope)
    n = int(lib.wn_deconv_backward_input_workspace_bytes(hd, b'iaf_share', 3, 2))
    assert n > 0
    with pytest.raises(ValueError, match='wn_deconv_backward_input: workspace {} < {} bytes'.format(n - 1, n)):
        _raw(h, MEL, G, 0, n_ws=n - 1)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    ws = torch.empty(n, dtype=torch.uint8, device='cuda')
    out = torch.empty_like(MEL)
    for args in ((None, ptr(G), ptr(out)), (ptr(MEL), None, ptr(out)), (ptr(MEL), ptr(G), None)):
        rc = lib.wn_deconv_backward_input(hd, b'iaf_share', args[0], args[1], 3, 2, args[2], ptr(ws), n, eng._stream())
        assert rc != 0 and 'wn_deconv_backward_input: bad argument' in lib.wn_last_error(hd).decode()
    fresh = Engine(h.cfgd, kind='student')                  # created, no weights: not finalized
    try:
        assert int(fresh.lib.wn_deconv_backward_input_workspace_bytes(fresh._h, b'iaf_share', 3, 2)) == 0
        with pytest.raises(RuntimeError, match='wn_deconv_backward_input: call wn_finalize first'):
            fresh.deconv_backward_input(MEL, G, scope=h.scope)
    finally:
        fresh.close()
