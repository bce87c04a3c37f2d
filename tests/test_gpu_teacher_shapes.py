"""GPU tests of the full-sequence teacher off its 256-column tile ("Pad columns"): the forward, the tape and the
input VJP wn_teacher_backward_input (csrc/wn_teacher_bwd.hip) at lengths T that are no multiple of TG_TN = 256, where every
workspace row carries pad columns [T, Tp) that the GEMM kernel computes without a guard and the anti-causal taps of the reverse
pass read.  Everything is held to the float64 oracle of tests/distill_oracle64.py on the small teacher of
tests/golden/ref_distill.npz (width 128, skip 64, gate 128, 7 layers, largest dilation 4, frame shift 200), at the bars the
project already applies to this teacher: 2e-5 max(1, max |ref|) for out_params, TOL = 1e-4 of max |g| for the input VJP
(tests/test_gpu_distill_grad.py) and TOL_CHAIN = 4e-5 for the public chain (tests/test_gpu_teacher_nll_grad.py).

Inputs.  The ReLU derivative is discontinuous, so where a float64 pre-ReLU value lies within 1e-4 of its tensor's maximum from
zero the oracle takes the engine's sign from the tape (distill_oracle64.relu_masks), as the existing gradient tests do, and at
most 16 such signs may differ.  That cap holds here before the engine is asked: every batch row is drawn from a seed of its
own (ROW_SEEDS, GAUSS_SEED), chosen by a search over the float64 oracle alone on the CPU, so that at every shape the oracle
has at most 16 pre-ReLU values in that band at all (found: 4, 12, 8, 8 and 15 for the five shapes in the order of SHAPES,
4 for the Gauss head) -- each case asserts it again on the values it computes."""
import os

import numpy as np
import pytest

import distill_oracle64 as D
import teacher_nll_oracle64 as N

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_distill.npz')
TOL_FWD = 2e-5          # out_params: max-abs error / max(1, max |ref|)       (tests/test_gpu_teacher.py)
TOL = 1e-4              # input VJP: max-abs error / max |g|                  (tests/test_gpu_distill_grad.py)
TOL_CHAIN = 4e-5        # calculate_loss(feed_forward(.)).backward() -> x.grad (tests/test_gpu_teacher_nll_grad.py)
NEAR_MAX = 16           # pre-ReLU values of the oracle within 1e-4 max of zero, and so ReLU derivatives taken from the tape

# (B, F, T): Tp = ceil(T / 256) 256 columns per row, TE = 200 F conditioning columns, c0 = (TE - T) / 2 its centre crop.
# Every T is a multiple of the largest dilation (4) as the table of the pad situations gives it.
SHAPES = [(1, 1, 200),      # one partial tile; T == TE, c0 = 0: the gate reads enc past the end of its rows
          (2, 2, 400),      # T == TE; a full tile and a partial one; the batch stride sits next to the pad
          (3, 2, 260),      # c0 = 70; 4 valid columns in the last tile; odd B
          (2, 2, 252),      # 4 columns short of a full tile
          (2, 3, 512)]      # control: tile-aligned
OFF_TILE = (3, 2, 260)
EDGE_SHAPES = [(2, 2, 252), (2, 2, 400)]
FILL_SHAPES = [(1, 1, 200), (2, 2, 400)]
ROW_SEEDS = {(1, 1, 200): (1001,), (2, 2, 400): (1117, 1253), (3, 2, 260): (1270, 1398, 1185), (2, 2, 252): (1099, 1002),
             (2, 3, 512): (11243, 1196)}
GAUSS_SEED = 1001


def _sid(s):
    return 'B{}-F{}-T{}'.format(*s)


def _row(F, T, seed):
    """one batch row: mel [F,80] in [0, 1), audio [T] = a sine of random phase plus noise, clipped"""
    rs = np.random.RandomState(seed)
    mel = rs.uniform(0, 1, [F, 80]).astype(np.float32)
    ph = rs.uniform(0, 2 * np.pi)
    x = np.clip(0.5 * np.sin(0.05 * np.arange(T) + ph) + 0.1 * rs.standard_normal(T), -0.95, 0.95).astype(np.float32)
    return mel, x


def _inputs(F, T, seeds):
    rows = [_row(F, T, s) for s in seeds]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def _near(pre):
    """pre-ReLU values within relu_masks' band (1e-4 of the tensor's largest magnitude) of zero"""
    return sum(int((v.abs() < 1e-4 * float(v.abs().max())).sum()) for v in pre.values())


class _Oracle(object):
    """float64 side of one case, computed once: out_params with the plain ReLU, the pre-ReLU tensors and their near-tie count;
    after masks(tape) the differentiable forward whose VJPs the tests share"""

    def __init__(self, cfgd, seed, init, mel, x):
        import torch
        self.cfgd, self.mel, self.x = cfgd, mel, x
        self.thp, self.w = D.teacher_weights(cfgd, seed, init)
        self.enc = D.teacher_enc(mel, cfgd, seed, init)             # [B,TE,Cd]; teacher_ff crops it to the centre T columns
        self.pre = {}
        with torch.no_grad():
            self.out = D.teacher_ff(torch.as_tensor(x.astype(np.float64)), self.enc, self.w, self.thp, pre=self.pre)
        self.near = _near(self.pre)

    def masks(self, tape):
        import torch
        B, T = self.x.shape
        masks, self.nflip = D.relu_masks(self.pre, D.tape_pre(tape, B, T, self.cfgd['skip_width']))
        self.x64 = torch.as_tensor(self.x.astype(np.float64)).requires_grad_(True)
        self.out64 = D.teacher_ff(self.x64, self.enc, self.w, self.thp, masks=masks)
        return self

    def vjp(self, g):
        import torch
        return torch.autograd.grad((self.out64 * g.detach().double().cpu()).sum(), self.x64, retain_graph=True)[0]


class _Case(object):
    """one shape on the MoL teacher: device inputs, the engine's forward + tape, the oracle with the tape's near-tie signs"""

    def __init__(self, R, eng, shape):
        import torch
        self.B, self.F, self.T = shape
        (cfgd, seed, init) = D.golden_case(R, 'mol')[1]
        mel, x = _inputs(self.F, self.T, ROW_SEEDS[shape])
        self.X, self.MEL = torch.as_tensor(x).cuda(), torch.as_tensor(mel).cuda()
        self.ora = _Oracle(cfgd, seed, init, mel, x)
        assert self.ora.near <= NEAR_MAX, (shape, self.ora.near)
        self.out, self.tape = eng.teacher_forward_tape(self.X, self.MEL)
        self.ora.masks(self.tape)
        assert self.ora.nflip <= NEAR_MAX, (shape, self.ora.nflip)
        self.ow = int(self.out.shape[2])

    def cotangent(self, seed):
        import torch
        rs = np.random.RandomState(seed)
        return torch.as_tensor(rs.standard_normal([self.B, self.T, self.ow]).astype(np.float32)).cuda()


@pytest.fixture(scope='module')
def R():
    return np.load(GOLD)


@pytest.fixture(scope='module')
def eng(R):
    from oracle import wavenet_np as O
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    cfgd, seed, init = D.golden_case(R, 'mol')[1]
    net = Wavenet(cfgd).load_weights(O.synth_weights(O.HP(cfgd), 'teacher', seed=seed, init=init))
    yield net.engine
    net.engine.close()


@pytest.fixture(scope='module')
def cases(R, eng):
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = _Case(R, eng, shape)
        return made[shape]
    return get


def _fwd_err(got, ref):
    """max |got - ref| / max(1, max |ref|)"""
    return float((got.detach().double().cpu() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def _vjp_err(got, ref):
    """max |got - ref| / max |ref|"""
    return float((got.detach().double().cpu() - ref).abs().max()) / float(ref.abs().max())


def _all_finite(t):
    import torch
    return bool(torch.isfinite(t).all())


@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_forward_off_the_tile(cases, eng, shape):
    """out_params against the float64 oracle on the centre-cropped conditioning; the tape forward writes the same bits."""
    import torch
    c = cases(shape)
    out = eng.teacher_forward(c.X, c.MEL)
    assert tuple(out.shape) == (c.B, c.T, c.ow) and _all_finite(out)
    e = _fwd_err(out, c.ora.out)
    print('forward {}: max |out - oracle| / max(1, max |oracle|) = {:.2e} (max |oracle| {:.3f})'.format(
        _sid(shape), e, float(c.ora.out.abs().max())))
    assert e <= TOL_FWD, (shape, e)
    out_t, tape = eng.teacher_forward_tape(c.X, c.MEL)
    assert torch.equal(out_t, out) and torch.equal(c.out, out)
    assert tape.numel() == eng.teacher_tape_bytes(c.B, c.T)


@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_input_vjp_matches_oracle(cases, eng, shape):
    """teacher_backward_input on a dense random cotangent against torch.autograd.grad of the float64 oracle."""
    c = cases(shape)
    g = c.cotangent(101)
    d_wav = eng.teacher_backward_input(c.tape, g)
    assert tuple(d_wav.shape) == (c.B, c.T)
    ref = c.ora.vjp(g)
    finite = _all_finite(d_wav)
    e = _vjp_err(d_wav, ref) if finite else float('nan')
    print('input VJP {}: max |d_wav - oracle| / max |oracle| = {:.2e} (max |oracle| {:.3e}; {} near-tie pre-ReLU values, {} signs '
          'from the tape)'.format(_sid(shape), e, float(ref.abs().max()), c.ora.near, c.ora.nflip))
    assert finite, (shape, 'd_wav is not finite')
    assert e <= TOL, (shape, e)


def _edge_cotangent(c, kind):
    import torch
    g = c.cotangent(202)
    keep = torch.zeros_like(g)
    if kind == 'last_column':             # the anti-causal taps read only pad and right-pad columns beyond it
        keep[:, c.T - 1] = 1
    elif kind == 'first_column':
        keep[:, 0] = 1
    elif kind == 'row0':
        keep[0] = 1
    return g * keep                       # 'zero': all of it


@pytest.mark.parametrize('kind', ['last_column', 'first_column', 'row0', 'zero'])
@pytest.mark.parametrize('shape', EDGE_SHAPES, ids=_sid)
def test_cotangents_at_the_edges(cases, eng, shape, kind):
    """Cotangents that are non-zero only at t = T - 1, only at t = 0 (out_params(0) sees no audio -- the input is shifted right
    -- so the gradient is exactly zero), only in batch row 0, and nowhere (the m == 0 branch of wn_scale_kernel)."""
    c = cases(shape)
    g = _edge_cotangent(c, kind)
    d_wav = eng.teacher_backward_input(c.tape, g)
    assert _all_finite(d_wav), (shape, kind)
    ref = c.ora.vjp(g)
    mx = float(ref.abs().max())
    if kind == 'row0':
        assert float(d_wav[1:].abs().max()) == 0 and float(ref[1:].abs().max()) == 0
    if kind in ('zero', 'first_column'):
        assert mx == 0
    else:
        assert mx > 0
    if mx == 0:
        assert float(d_wav.abs().max()) == 0, (shape, kind)
        return
    e = _vjp_err(d_wav, ref)
    print('edge {} {}: max |d_wav - oracle| / max |oracle| = {:.2e} (max |oracle| {:.3e})'.format(_sid(shape), kind, e, mx))
    assert e <= TOL, (shape, kind, e)


@pytest.mark.parametrize('k', [-40, 20])
def test_vjp_is_linear_in_the_engines_own_arithmetic(cases, eng, k):
    """The operand scale is a power of two found on the device from the valid cotangent alone, so scaling the cotangent by
    2^k scales d_wav by 2^k bit for bit; a scale that saw pad contents or a stale word would not."""
    import torch
    c = cases(OFF_TILE)
    g = c.cotangent(303)
    base = eng.teacher_backward_input(c.tape, g)
    assert _all_finite(base) and float(base.abs().max()) > 0
    f = 2.0 ** k
    assert torch.equal(g * f / f, g) and torch.equal(base * f / f, base)       # exact in float32: no under- or overflow
    assert torch.equal(eng.teacher_backward_input(c.tape, g * f), base * f)


def _raw_pair(eng, c, g, fill):
    """wn_teacher_forward_tape + wn_teacher_backward_input through the C ABI on buffers of exactly the sizes the library asks
    for, every byte of workspace, tape and backward workspace set to `fill` before the calls"""
    import ctypes
    import torch
    from nsynth_wavenet_amd import _lib
    lib, h = eng.lib, eng._h
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    with torch.cuda.device(eng.device):
        n_ws = int(lib.wn_teacher_workspace_bytes(h, c.B, c.F, c.T))
        n_tape = int(lib.wn_teacher_tape_bytes(h, c.B, c.T))
        n_bws = int(lib.wn_teacher_backward_workspace_bytes(h, c.B, c.T))
        assert min(n_ws, n_tape, n_bws) > 0
        ws, tape, bws = [torch.full((n,), fill, dtype=torch.uint8, device='cuda') for n in (n_ws, n_tape, n_bws)]
        out = torch.full((c.B, c.T, c.ow), float('nan'), dtype=torch.float32, device='cuda')
        d_wav = torch.full((c.B, c.T), float('nan'), dtype=torch.float32, device='cuda')
        _lib.check(lib.wn_teacher_forward_tape(h, ptr(c.X), ptr(c.MEL), c.B, c.F, c.T, ptr(out), ptr(tape), n_tape, ptr(ws), n_ws,
                                               eng._stream()), h)
        _lib.check(lib.wn_teacher_backward_input(h, ptr(tape), n_tape, ptr(g), c.B, c.T, ptr(d_wav), ptr(bws), n_bws,
                                                 eng._stream()), h)
        torch.cuda.synchronize()
    return out, d_wav


@pytest.mark.parametrize('shape', FILL_SHAPES, ids=_sid)
def test_results_do_not_depend_on_what_the_buffers_held(cases, eng, shape):
    """The same pair of calls on buffers pre-filled with 0x00 bytes and with 0xFF bytes (every fp16 and fp32 word a NaN):
    out_params and d_wav are the same bits, finite, and within the bars of the forward and the VJP."""
    import torch
    c = cases(shape)
    g = c.cotangent(404)
    out0, dw0 = _raw_pair(eng, c, g, 0x00)
    out1, dw1 = _raw_pair(eng, c, g, 0xFF)
    bad = {k: int((~torch.isfinite(t)).sum()) for k, t in (('out 0x00', out0), ('out 0xFF', out1), ('d_wav 0x00', dw0),
                                                             ('d_wav 0xFF', dw1))}
    same = (torch.equal(out0, out1), bool((dw0.view(torch.int32) == dw1.view(torch.int32)).all()))
    print('fills {}: non-finite elements {}; out_params same bits {}, d_wav same bits {}'.format(_sid(shape), bad, *same))
    assert not any(bad.values()), (shape, bad)
    assert all(same), (shape, same)
    ref = c.ora.vjp(g)
    e_out, e_wav = _fwd_err(out0, c.ora.out), _vjp_err(dw0, ref)
    print('fills {}: out_params error {:.2e}, d_wav error {:.2e}'.format(_sid(shape), e_out, e_wav))
    assert torch.equal(out0, c.out)
    assert e_out <= TOL_FWD and e_wav <= TOL, (shape, e_out, e_wav)


@pytest.mark.parametrize('tag', ['mol', 'gauss'])
def test_public_chain_off_the_tile(R, tag):
    """Wavenet.calculate_loss(feed_forward({'wav': x, 'mel': mel}))['loss'].backward() at (B, F, T) = (1, 1, 200), as
    test_loss_backpropagates_to_the_audio_through_both_paths runs it at T = 256: x.grad sums the engine's input VJP and the
    gradient through the target."""
    import torch
    from oracle import wavenet_np as O
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    cfgd, seed, init = D.golden_case(R, tag)[1]
    B, F, T = 1, 1, 200
    mel, x = _inputs(F, T, ROW_SEEDS[(B, F, T)] if tag == 'mol' else (GAUSS_SEED,))
    ora = _Oracle(cfgd, seed, init, mel, x)
    assert ora.near <= NEAR_MAX, (tag, ora.near)
    net = Wavenet(cfgd).load_weights(O.synth_weights(O.HP(cfgd), 'teacher', seed=seed, init=init))
    xg = torch.as_tensor(x).cuda().requires_grad_(True)
    melg = torch.as_tensor(mel).cuda()
    ff = net.feed_forward({'wav': xg, 'mel': melg})
    assert ff['out_params'].grad_fn is not None
    res = net.calculate_loss(ff)
    res['loss'].backward()
    with torch.no_grad():
        plain = net.calculate_loss(net.feed_forward({'wav': xg, 'mel': melg}))
    assert torch.equal(plain['loss'], res['loss'].detach()) and torch.equal(plain['log_probs'], res['log_probs'].detach())
    _, tape = net.engine.teacher_forward_tape(xg.detach(), melg)
    ora.masks(tape)
    assert ora.nflip <= NEAR_MAX
    L = -N.teacher_log_prob(ora.out64, ora.x64, tag, False).mean()
    L.backward()
    ref = ora.x64.grad
    _, _, target_part = N.grads(ora.out64.detach().numpy(), x, np.full([B, T], -1.0 / (B * T)), tag, False)
    assert float(target_part.abs().max()) > 0 and float((ref - target_part).abs().max()) > 0           # both paths carry gradient
    assert _all_finite(xg.grad)
    e = _vjp_err(xg.grad, ref)
    print('chain {} T=200: loss {:.6f} (oracle {:.6f}), x.grad error / max |g| = {:.2e}; max |g| {:.3e}, target path {:.3e}, {} '
          'ReLU derivatives from the tape'.format(tag, float(res['loss'].detach()), float(L.detach()), e, float(ref.abs().max()),
                                                  float(target_part.abs().max()), ora.nflip))
    assert e <= TOL_CHAIN, (tag, e)
    net.engine.close()
