"""GPU tests of the eight distillation kernels of csrc/wn_distill.hip called directly, off the shapes the rest of the suite runs
("Ragged shapes"): dx_mol_kernel / dx_mol_grad_kernel, dx_gauss_kernel / dx_gauss_grad_kernel, pw_kernel /
pw_grad_kernel / pw_ola_kernel and dx_reduce_kernel, on synthetic out_params -- no teacher forward, no ReLU ties -- against the
float64 oracle of tests/distill_oracle64.py with the bin mass in its product form (stable=True, pinned to the reference's
difference form by tests/test_distill_grad_oracle.py).  Every output tensor is compared whole, d_out_params as three tensors
(logits, means, log-scales), each against its own largest magnitude.

Inputs come from the seeded generators below, rounded to float32 before either side sees them.  The regimes of the mixture
kernels: `interior` (every draw inside the thresholds, mean_tot near a component mean) with FLOOR_ROWS extra batch rows whose
components are all below the 1e-12 floor (their oracle gradients of mean_tot and of the mixture parameters are exactly zero, so
a kernel that fails to zero a gradient below the floor shows as a d mean of order inv_s in the interior max-norm); `tails`
(every draw below min_thres or above max_thres, about half each); `clamp` (log-scales U(-9, -5), a fifth exactly -7.0).
Before the GPU is asked anything each case asserts on the float64 side alone: no draw within 1e-5 of a threshold (the
float32 x = rl scale + mean is off by at most 3 * 2^-24 (|rl scale| + |mean|) < 1e-6), no component that carries a mixture
weight above 1e-6 -- the dominant one included -- with a mass within 1 % of the floor (the kernel's float32 mass is off by about
1e-6), and the occupancy the regime claims.  The seeds (MOL_SEEDS) were checked on the CPU: these counts are zero at every
(shape, regime), and no element is left out of any comparison.

Bars (the project's own): forward rows 2e-5 max(1, |ref|) per sample, forward sums 1e-5 relative (tests/test_gpu_distill.py),
gradients max |g - g64| <= TOL max |g64| per tensor with TOL = 1e-4 (tests/test_gpu_distill_grad.py), power loss
1e-5 max(1, |ref|).  Every case prints its measured errors before it asserts.

Which case fails for which line of the kernels, and for no other reason:
  draw loop `s >= S` / `nq`            mol (3, 77, 5, 10): the last block of four holds one draw; (2, 130, 21, 17): block 5 holds one
  draw loop `q += DX_WAVES`            mol (2, 130, 21, 17): wave 0 takes blocks 0 and 4, wave 1 blocks 1 and 5 (S = 21 > 16)
  `live` guards                        mol T = 77, 130 and 1 (13, 2 and 1 live lanes in the last workgroup); gauss 231 and 260
                                       rows; the NaN guards of test_nothing_is_written_outside_the_outputs
  the MM = 32 instantiation            mol (2, 130, 21, 17) and (1, 1, 1, 32); mol_mix = 33 is refused
  log-scale clamp conditional          regime `clamp` (exact 0.0 below -7, the oracle's non-zero value at exactly -7), gauss
  floor conditional                    the floor rows of regime `interior` (d mean, d log-scale, d mean_tot exactly 0)
  the two tail branches                regime `tails`
  `f0 + fr < NF`                       power L = 801 and 1000 (5 frames: the second workgroup holds one), 1337 (7 frames); the
                                       gradient workspace of exactly the asked size between NaN guards (L = 801, 1337)
  `flo` / `fhi` of the overlap-add     power L = 1000 and 1337 (j >= 800: flo >= 1, frames of two workgroups are summed)
  blockIdx / row strides               row independence at every shape; the centre-trimmed views of the power loss

The value-only lines of that table were also tried once as changes of the kernel source (a library built aside): `>=` to `>` at
the clamp failed the four clamp cases and the three gauss cases; the floor test dropped failed the four interior cases (and
(2, 130, 21, 17) clamp, where components below the floor carry weight); the upper tail dropped failed the three tails cases with
draws in both tails (the single draw of (1, 1, 1, 32) lies in the lower one); `q += 2 DX_WAVES` and the MM = 10 kernel for M = 17
failed only cases of (2, 130, 21, 17); the gradient kernel without `s >= S` failed every mol case but the aligned control
(1, 64, 4, 10); `flo = 0` failed power L = 1000, 1337, the trimmed views and the zero-frame case and passed L <= 801.  The `live`
guards and the `f0 + fr < NF` store guard were not changed: without them a kernel stores out of bounds; they are held by the NaN
guards around outputs and workspaces of exactly the asked size.

Measured on an MI355X, largest over all shapes and regimes (DESIGN.md 12 has the table):
  dx_mol_kernel        H_bl 1.3e-6 (bar 2e-5, (3, 77, 5, 10) clamp), sums 1.2e-7 (bar 1e-5)
  dx_mol_grad_kernel   logits 2.4e-6, means 9.5e-6, log-scales 8.2e-6, d mean_tot 9.5e-6, d scale_tot 6.9e-6 (bar 1e-4; the four
                       largest at (1, 64, 4, 10) clamp, where inv_s reaches e^7); tails <= 6.0e-7, interior <= 6.2e-6
  dx_gauss_kernel      kl_bl 9.1e-7, sums 1.4e-7;  dx_gauss_grad_kernel 6.0e-7 (d scale_tot)
  pw_kernel            3.1e-7 (L = 799);  pw_grad_kernel + pw_ola_kernel 1.9e-6 (L = 200), 1.8e-6 on the trimmed views
  composed calculate_loss at (3, 2, 260), S = 5: value 6.2e-8, x 2.4e-6, mean_tot 9.7e-7, scale_tot 1.5e-7
No guard word changed, and no comparison failed: the kernels needed no fix."""
import ctypes

import numpy as np
import pytest

import distill_oracle64 as D
import test_gpu_teacher_nll_grad as NG
import test_gpu_teacher_shapes as TS

pytestmark = pytest.mark.gpu
TOL = 1e-4                  # gradients: max-abs error / max |g64| per tensor   (tests/test_gpu_distill_grad.py)
TOL_ROW = 2e-5              # forward rows: error / max(1, |ref|) per sample
TOL_SUM = 1e-5              # forward sums, relative                           (tests/test_gpu_distill.py)
TOL_PW = 1e-5               # power loss: error / max(1, |ref|)
Q = D.Q
MIN_THRES, MAX_THRES = 0.5 / (Q / 2.) - 1.0, (Q - 1 - 0.5) / (Q / 2.) - 1.0
FLOOR = 1e-12
FLOOR_ROWS = 2              # batch rows appended to an `interior` call whose components all lie below the floor
FAC = (0.37, -0.11)         # d loss / d sums: two unequal values of opposite sign
GUARD = 256                 # float32 words of guard on both sides of every carved output

# (B, T, S, M)
MOL_SHAPES = [(3, 77, 5, 10),       # two workgroups per row, 13 live lanes in the last; odd B; S % 4 = 1; waves 2, 3 idle
              (2, 130, 21, 17),     # 2 live lanes in the third workgroup; MM = 32; a second block of draws per wave
              (1, 64, 4, 10),       # aligned control
              (1, 1, 1, 32)]        # one lane, one draw, DX_MAX_MIX components
REGIMES = ['interior', 'tails', 'clamp']
# checked on the CPU (mol_report: zero draws near a threshold, zero weighted components near the floor); a case that fails
# these conditions gets another seed here, never a mask
MOL_SEEDS = {(s, r): 1 for s in MOL_SHAPES for r in REGIMES}
MOL_SEEDS[((1, 1, 1, 32), 'clamp')] = 3          # the one draw's own component sits at exactly -7
GAUSS_SHAPES = [(3, 77), (2, 130), (1, 256)]        # 231 rows: one partial workgroup; 260: 4 rows in the second; aligned
PW_LENGTHS = [200, 799, 801, 1000, 1337]
COMPOSED = (3, 2, 260)
COMPOSED_S = 5
COMPOSED_SEED = 0
# mel_rand rows, searched like TS.ROW_SEEDS: at most 16 pre-ReLU values of the float64 teacher near a tie under mel_rand too
COMPOSED_MEL_RAND_SEEDS = (2005, 2015, 2023)


def _mid(s):
    return 'B{}-T{}-S{}-M{}'.format(*s)


# ---- inputs (host, float32) and what the float64 side says about them ----
def _logistic(rs, shape):
    u = rs.uniform(1e-5, 1 - 1e-5, shape)
    return np.log(u) - np.log(1 - u)


def _mol_rows(rs, regime, B, T, S, M):
    lg = rs.standard_normal([B, T, M])
    rl = _logistic(rs, [B, S, T])
    k = rs.randint(0, M, [B, T, 1])
    pick = lambda a: np.take_along_axis(a, k, -1)[..., 0]
    if regime == 'floor':
        # every component far from x: means in [-0.8, -0.3], x in [0.35, 0.75], inv_s >= e^6: masses below e^-260
        mu, ls = rs.uniform(-0.8, -0.3, [B, T, M]), rs.uniform(-8, -6, [B, T, M])
        mean, scale = rs.uniform(0.4, 0.7, [B, T]), np.exp(rs.uniform(-7, -5.5, [B, T]))
    elif regime == 'interior':
        mu, ls = rs.uniform(-0.8, 0.8, [B, T, M]), rs.uniform(-6.5, -2, [B, T, M])
        mean = np.clip(pick(mu) + 0.5 * np.exp(pick(ls)) * rs.standard_normal([B, T]), -0.9, 0.9)
        scale = np.minimum(np.exp(rs.uniform(-7, -3, [B, T])), (0.98 - np.abs(mean)) / 12)      # |rl| < 11.6: |x| < 0.98
    elif regime == 'tails':
        mu, ls = rs.uniform(-0.8, 0.8, [B, T, M]), rs.uniform(-6.5, -2, [B, T, M])
        mean = rs.uniform(1.02, 1.2, [B, T]) * np.where(rs.uniform(size=[B, T]) < 0.5, -1.0, 1.0)
        scale = np.exp(rs.uniform(-8, -6.5, [B, T]))                                             # |rl scale| < 0.018
    elif regime == 'clamp':
        mu, ls = rs.uniform(-0.8, 0.8, [B, T, M]), rs.uniform(-9, -5, [B, T, M])
        ls = np.where(rs.uniform(size=[B, T, M]) < 0.2, -7.0, ls)
        sk = np.exp(np.maximum(pick(ls), -7.0))
        mean = pick(mu) + 0.5 * sk * rs.standard_normal([B, T])
        scale = sk * np.exp(rs.uniform(-2.5, 0.3, [B, T]))              # x within 16 scales of the picked component
    else:
        raise ValueError(regime)
    return {'te': np.concatenate([lg, mu, ls], -1), 'mean': mean, 'scale': scale, 'rl': rl}


def mol_inputs(shape, regime, seed=None):
    """float32 inputs of one (shape, regime): te [B',T,3M], mean / scale [B',T], rl [B',S,T]; B' = B + FLOOR_ROWS for
    `interior` (the floor rows last), else B"""
    B, T, S, M = shape
    rs = np.random.RandomState(MOL_SEEDS[(shape, regime)] if seed is None else seed)
    d = _mol_rows(rs, regime, B, T, S, M)
    if regime == 'interior':
        f = _mol_rows(rs, 'floor', FLOOR_ROWS, T, S, M)
        d = {k: np.concatenate([d[k], f[k]], 0) for k in d}
    return {k: v.astype(np.float32) for k, v in d.items()}


def mol_report(inp):
    """counts on the float64 side: draws per branch, draws within 1e-5 of a threshold, components near the floor that carry
    weight, draws whose components all lie below the floor, log-scales below and at -7"""
    te, mean, scale, rl = (np.asarray(inp[k], np.float64) for k in ('te', 'mean', 'scale', 'rl'))
    M = te.shape[-1] // 3
    lg, mu, ls = te[..., :M], te[..., M:2 * M], te[..., 2 * M:]
    x = rl * scale[:, None] + mean[:, None]                                # [B,S,T]
    lower, upper = x < MIN_THRES, x > MAX_THRES
    inside = ~(lower | upper)
    inv = np.exp(-np.maximum(ls, -7.0))[:, None]                           # [B,1,T,M]
    c = x[..., None] - mu[:, None]
    a, b = inv * (c + 1.0 / Q), inv * (c - 1.0 / Q)
    sig = lambda v: np.exp(-np.logaddexp(0.0, -v))
    mass = sig(a) * sig(-b) * (-np.expm1(-(2.0 / Q) * inv))
    with np.errstate(divide='ignore'):
        score = (lg - np.logaddexp.reduce(lg, -1, keepdims=True))[:, None] + np.log(np.maximum(mass, FLOOR))
    w = np.exp(score - np.logaddexp.reduce(score, -1, keepdims=True))
    dom = np.take_along_axis(mass, np.argmax(score, -1)[..., None], -1)[..., 0]
    band = np.abs(mass / FLOOR - 1.0) < 0.01
    return {'draws': int(x.size), 'lower': int(lower.sum()), 'upper': int(upper.sum()),
            'near_threshold': int(((np.abs(x - MIN_THRES) < 1e-5) | (np.abs(x - MAX_THRES) < 1e-5)).sum()),
            'near_floor_dominant': int((inside & (np.abs(dom / FLOOR - 1.0) < 0.01)).sum()),
            'near_floor_weighted': int((inside[..., None] & band & (w > 1e-6)).sum()),
            'all_below_floor': int((inside & (mass < FLOOR).all(-1)).sum()),
            'ls_below_-7': int((ls < -7.0).sum()), 'ls_at_-7': int((ls == -7.0).sum()),
            'smallest_weighted_mass': float(np.where(inside[..., None] & (w > 1e-6), mass, 1.0).min())}


def assert_mol_regime(shape, regime, inp, rep):
    """the regime is what it claims, and nothing sits where a float32 evaluation may take another branch than float64"""
    B, T, S, M = shape
    assert rep['near_threshold'] == 0 and rep['near_floor_dominant'] == 0 and rep['near_floor_weighted'] == 0, rep
    n = B * S * T
    if regime == 'interior':
        assert rep['draws'] == n + FLOOR_ROWS * S * T and rep['lower'] == 0 and rep['upper'] == 0, rep
        fl = mol_report({k: v[B:] for k, v in inp.items()})
        assert fl['all_below_floor'] == fl['draws'] == FLOOR_ROWS * S * T, fl
        assert mol_report({k: v[:B] for k, v in inp.items()})['all_below_floor'] < n, rep
    elif regime == 'tails':
        assert rep['lower'] + rep['upper'] == n, rep
        if n >= 100:
            assert min(rep['lower'], rep['upper']) >= 0.4 * n, rep
    else:
        assert rep['lower'] == 0 and rep['upper'] == 0, rep
        assert rep['ls_at_-7'] >= 1 and rep['ls_below_-7'] >= 1, rep
        if B * T * M >= 100:
            assert rep['ls_at_-7'] >= 0.15 * B * T * M and rep['ls_below_-7'] >= 0.3 * B * T * M, rep


def mol_oracle(inp, fac=FAC):
    """float64: H_bl, the two sums, and the gradients of fac[0] sum H_bl + fac[1] sum log scale_tot"""
    import torch
    te, mean, scale = (torch.as_tensor(inp[k].astype(np.float64)).requires_grad_(True) for k in ('te', 'mean', 'scale'))
    rl = torch.as_tensor(inp['rl'].astype(np.float64))
    hb = D.kl_logistic(te, mean, scale, rl, stable=True)['H_bl']
    s0, s1 = hb.sum(), torch.log(scale).sum()
    (fac[0] * s0 + fac[1] * s1).backward()
    return {'H_bl': hb.detach(), 'sums': (float(s0.detach()), float(s1.detach())), 'd_te': te.grad, 'd_mean': mean.grad, 'd_scale': scale.grad}


def gauss_inputs(shape, seed=5):
    """te [B,T,2] (mean, log-scale U(-9, -3), a tenth exactly -7), the student's mean within two teacher scales, its scale
    within e^+-1 of the teacher's"""
    B, T = shape
    rs = np.random.RandomState(seed + 7 * T)
    mp, lsp = rs.uniform(-0.8, 0.8, [B, T]), rs.uniform(-9, -3, [B, T])
    lsp = np.where(rs.uniform(size=[B, T]) < 0.1, -7.0, lsp)
    sp = np.exp(np.maximum(lsp, -7.0))
    mq = mp + 2.0 * sp * rs.standard_normal([B, T])
    sq = sp * np.exp(rs.uniform(-1, 1, [B, T]))
    return {'te': np.stack([mp, lsp], -1).astype(np.float32), 'mean': mq.astype(np.float32), 'scale': sq.astype(np.float32)}


def gauss_oracle(inp, fac=FAC):
    import torch
    te, mean, scale = (torch.as_tensor(inp[k].astype(np.float64)).requires_grad_(True) for k in ('te', 'mean', 'scale'))
    kl = D.kl_gauss(te, mean, scale)['kl_bl']
    reg = (torch.clamp(te[..., 1], min=-7.0) - torch.log(scale)) ** 2
    s0, s1 = kl.sum(), reg.sum()
    (fac[0] * s0 + fac[1] * s1).backward()
    return {'kl_bl': kl.detach(), 'sums': (float(s0.detach()), float(s1.detach())), 'd_te': te.grad, 'd_mean': mean.grad, 'd_scale': scale.grad}


def pw_inputs(B, L, seed=3):
    rs = np.random.RandomState(seed + L)
    t = np.arange(L)
    pred = np.stack([0.3 * np.sin(0.05 * (b + 1) * t + rs.uniform(0, 6)) + 0.1 * rs.standard_normal(L) for b in range(B)])
    orig = np.stack([0.3 * np.sin(0.045 * (b + 1) * t + rs.uniform(0, 6)) + 0.1 * rs.standard_normal(L) for b in range(B)])
    return pred.astype(np.float32), orig.astype(np.float32)


def pw_oracle(pred, orig):
    """D.power_loss in float64 and its gradient with respect to pred (trims included)"""
    import torch
    p = torch.as_tensor(pred.astype(np.float64)).requires_grad_(True)
    loss = D.power_loss(p, torch.as_tensor(orig.astype(np.float64)))
    loss.backward()
    assert bool(torch.isfinite(p.grad).all())
    return float(loss.detach()), p.grad


def composed_inputs(seed=COMPOSED_SEED):
    """mel / x of TS.ROW_SEEDS at (3, 2, 260), mel_rand of COMPOSED_MEL_RAND_SEEDS, wav of 267 samples (an odd
    trim), mean_tot near x, scale_tot e^U(-7, -4.5), draws [B, S, T] for the KL and the contrastive term"""
    B, F, T = COMPOSED
    mel, x = TS._inputs(F, T, TS.ROW_SEEDS[COMPOSED])
    rs = np.random.RandomState(seed)
    mean = (x + 0.01 * rs.standard_normal([B, T])).astype(np.float32)
    scale = np.exp(rs.uniform(-7, -4.5, [B, T])).astype(np.float32)
    wav = np.clip(0.4 * np.sin(0.04 * np.arange(T + 7) + 1.0) + 0.1 * rs.standard_normal([B, T + 7]), -0.95, 0.95)
    rl = [_logistic(rs, [B, COMPOSED_S, T]).astype(np.float32) for _ in range(2)]
    return {'mel': mel, 'mel_rand': TS._inputs(F, T, COMPOSED_MEL_RAND_SEEDS)[0], 'x': x, 'mean': mean, 'scale': scale,
            'wav': wav.astype(np.float32), 'rl': rl}


# ---- device side ----
@pytest.fixture(scope='module')
def R():
    return np.load(TS.GOLD)


@pytest.fixture(scope='module')
def engines(R):
    """teacher handles without weights (the loss kernels read none): mol_mix 10, 17 and 32, and a Gauss head"""
    from nsynth_wavenet_amd.engine import Engine
    made = {}

    def get(key):
        if key not in made:
            made[key] = Engine(NG._small_cfg(R, 'gauss') if key == 'gauss' else NG._small_cfg(R, 'mol', mol_mix=key))
        return made[key]
    yield get
    for e in made.values():
        e.close()


def _cuda(inp):
    import torch
    return {k: torch.as_tensor(v).cuda() for k, v in inp.items()}


def _fac():
    import torch
    return torch.tensor(FAC, dtype=torch.float64).cuda()


def _cmp_grad(label, name, got, ref):
    """max |g - g64| / max |g64| against TOL; exact zero where the oracle's tensor is identically zero"""
    import torch
    got = got.detach().double().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (label, name, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), (label, name, 'not finite')
    mx = float(ref.abs().max())
    if mx == 0:
        print('{} {:12s} oracle identically zero; engine max |g| = {:.1e}'.format(label, name, float(got.abs().max())))
        assert float(got.abs().max()) == 0, (label, name, 'oracle gradient is zero')
        return 0.0
    e = float((got - ref).abs().max()) / mx
    print('{} {:12s} max |g - g64| / max |g64| = {:.2e} (bar {:.0e}; max |g64| {:.3e})'.format(label, name, e, TOL, mx))
    assert e <= TOL, (label, name, e)
    return e


def _cmp_rows(label, name, got, ref):
    got = got.detach().double().cpu()
    assert tuple(got.shape) == tuple(ref.shape)
    e = float(((got - ref).abs() / ref.abs().clamp(min=1.0)).max())
    print('{} {:12s} max |v - v64| / max(1, |v64|) = {:.2e} (bar {:.0e}; max |v64| {:.3e})'.format(
        label, name, e, TOL_ROW, float(ref.abs().max())))
    assert e <= TOL_ROW, (label, name, e)
    return e


def _cmp_sums(label, got, ref):
    got = [float(v) for v in got.cpu()]
    es = [abs(g - r) / max(abs(r), 1e-300) for g, r in zip(got, ref)]
    print('{} sums         relative error {:.2e}, {:.2e} (bar {:.0e}; {:.6e}, {:.6e})'.format(label, es[0], es[1], TOL_SUM,
                                                                                               ref[0], ref[1]))
    assert max(es) <= TOL_SUM, (label, got, ref)
    return max(es)


def _mol_calls(eng, d, S, **kw):
    f = eng.distill_mol_xent(d['te'], d['mean'], d['scale'], S, **kw)
    g = eng.distill_mol_xent_grad(d['te'], d['mean'], d['scale'], S, _fac(), **kw)
    return f, g


# ---- 2a ----
@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('shape', MOL_SHAPES, ids=_mid)
def test_mol_xent_and_gradient_match_the_oracle(engines, shape, regime):
    import torch
    B, T, S, M = shape
    inp = mol_inputs(shape, regime)
    rep = mol_report(inp)
    label = 'mol {} {}'.format(_mid(shape), regime)
    print('{} occupancy: {}'.format(label, rep))
    assert_mol_regime(shape, regime, inp, rep)
    ref = mol_oracle(inp)
    ls = torch.as_tensor(inp['te'][..., 2 * M:])
    ref_ls = ref['d_te'][..., 2 * M:]
    below, tie = ls < -7.0, ls == -7.0
    moved = ref_ls[tie].abs() > 1e-3 * float(ref_ls.abs().max())
    assert float(ref_ls[below].abs().sum()) == 0, 'the oracle passes nothing below the clamp'
    if regime == 'clamp':                # tf.maximum passes the gradient at the tie: the oracle's is non-zero there
        assert int(moved.sum()) >= 1, 'no log-scale at exactly -7 carries a gradient'
    d = _cuda(inp)
    f, (d_te, d_mean, d_scale) = _mol_calls(engines(M), d, S, noise=d['rl'])
    _cmp_rows(label, 'H_bl', f['H_bl'], ref['H_bl'])
    _cmp_sums(label, f['sums'], ref['sums'])
    _cmp_grad(label, 'd logits', d_te[..., :M], ref['d_te'][..., :M])
    _cmp_grad(label, 'd means', d_te[..., M:2 * M], ref['d_te'][..., M:2 * M])
    _cmp_grad(label, 'd log-scales', d_te[..., 2 * M:], ref_ls)
    _cmp_grad(label, 'd mean_tot', d_mean, ref['d_mean'])
    _cmp_grad(label, 'd scale_tot', d_scale, ref['d_scale'])
    got_ls = d_te[..., 2 * M:].cpu()
    assert float(got_ls[below].abs().sum()) == 0, 'exactly zero below the clamp'
    if regime == 'clamp':
        assert bool((got_ls[tie][moved] != 0).all()), 'the gradient passes at log_scale == -7'
        e = float((got_ls[tie].double() - ref_ls[tie]).abs().max()) / float(ref_ls.abs().max())
        print('{} at the tie: {} elements, {} with |g64| > 1e-3 max, error / max |g64| = {:.2e}'.format(
            label, int(tie.sum()), int(moved.sum()), e))
        assert e <= TOL
    if regime == 'interior':
        # the floor rows: exact zeros wherever the oracle's are
        for name, got, want in (('d means', d_te[B:, :, M:2 * M], ref['d_te'][B:, :, M:2 * M]),
                                ('d log-scales', d_te[B:, :, 2 * M:], ref['d_te'][B:, :, 2 * M:]),
                                ('d mean_tot', d_mean[B:], ref['d_mean'][B:])):
            assert float(want.abs().max()) == 0, (name, 'the oracle is zero below the floor')
            assert float(got.abs().max()) == 0, (label, name, 'not zero below the floor')


# ---- 2b ----
@pytest.mark.parametrize('shape', GAUSS_SHAPES, ids=lambda s: 'B{}-T{}'.format(*s))
def test_gauss_kl_and_gradient_match_the_oracle(engines, shape):
    import torch
    inp = gauss_inputs(shape)
    ls = torch.as_tensor(inp['te'][..., 1])
    below, tie = ls < -7.0, ls == -7.0
    label = 'gauss B{}-T{}'.format(*shape)
    print('{} occupancy: {} rows, log-scales below -7: {}, at -7: {}'.format(label, ls.numel(), int(below.sum()), int(tie.sum())))
    assert int(below.sum()) >= 0.2 * ls.numel() and int(tie.sum()) >= 0.05 * ls.numel()
    ref = gauss_oracle(inp)
    ref_ls = ref['d_te'][..., 1]
    moved = ref_ls[tie].abs() > 1e-3 * float(ref_ls.abs().max())
    assert float(ref_ls[below].abs().sum()) == 0 and int(moved.sum()) >= 1
    d = _cuda(inp)
    eng = engines('gauss')
    f = eng.distill_gauss_kl(d['te'], d['mean'], d['scale'])
    d_te, d_mean, d_scale = eng.distill_gauss_kl_grad(d['te'], d['mean'], d['scale'], _fac())
    _cmp_rows(label, 'kl_bl', f['kl_bl'], ref['kl_bl'])
    _cmp_sums(label, f['sums'], ref['sums'])
    _cmp_grad(label, 'd mean', d_te[..., 0], ref['d_te'][..., 0])
    _cmp_grad(label, 'd log-scale', d_te[..., 1], ref_ls)
    _cmp_grad(label, 'd mean_tot', d_mean, ref['d_mean'])
    _cmp_grad(label, 'd scale_tot', d_scale, ref['d_scale'])
    got_ls = d_te[..., 1].cpu()
    assert float(got_ls[below].abs().sum()) == 0, 'exactly zero below the clamp'
    assert bool((got_ls[tie][moved] != 0).all()), 'the gradient passes at log_scale == -7'
    e = float((got_ls[tie].double() - ref_ls[tie]).abs().max()) / float(ref_ls.abs().max())
    print('{} at the tie: {} elements, {} with |g64| > 1e-3 max, error / max |g64| = {:.2e}'.format(
        label, int(tie.sum()), int(moved.sum()), e))
    assert e <= TOL


# ---- 2c ----
def _pw_check(label, pred, orig, zero=None):
    """the differentiable power loss and the no-grad one on (pred, orig) against the oracle; returns the device gradient"""
    import torch
    from nsynth_wavenet_amd import distill_autograd as dag
    from nsynth_wavenet_amd.engine import power_loss
    val, g64 = pw_oracle(pred, orig)
    P = torch.as_tensor(pred).cuda().requires_grad_(True)
    O = torch.as_tensor(orig).cuda()
    loss = dag.power_loss(P, O)
    loss.backward()
    with torch.no_grad():
        plain = power_loss(P.detach(), O)
    assert torch.equal(plain, loss.detach()), 'the no-grad path gives the same bits'
    e = abs(float(loss.detach()) - val) / max(1.0, abs(val))
    print('{} loss {:.8e} (oracle {:.8e}): error / max(1, |ref|) = {:.2e} (bar {:.0e})'.format(label, float(loss.detach()), val, e,
                                                                                               TOL_PW))
    assert e <= TOL_PW, (label, float(loss.detach()), val)
    _cmp_grad(label, 'd pred', P.grad, g64)
    return P.grad.cpu(), g64


@pytest.mark.parametrize('L', PW_LENGTHS)
def test_power_loss_and_gradient_match_the_oracle(L):
    pred, orig = pw_inputs(2, L)
    _pw_check('power L={}'.format(L), pred, orig)


@pytest.mark.parametrize('longer', ['pred', 'orig'])
def test_power_loss_on_centre_trimmed_views(longer):
    """one side 7 samples longer: the library sees a view that starts 3 samples in with a row stride of L + 7"""
    L = 1000
    pred, orig = pw_inputs(2, L + 7, seed=11)
    if longer == 'pred':
        orig = np.ascontiguousarray(orig[:, :L])
    else:
        pred = np.ascontiguousarray(pred[:, :L])
    g, g64 = _pw_check('power trimmed ({} longer)'.format(longer), pred, orig)
    if longer == 'pred':
        assert float(g64[:, :3].abs().max()) == 0 and float(g64[:, L + 3:].abs().max()) == 0
        assert float(g[:, :3].abs().max()) == 0 and float(g[:, L + 3:].abs().max()) == 0, 'no gradient to the trimmed samples'


def test_power_loss_gradient_is_zero_where_every_frame_is_zero():
    """pred = 0 on [0, 1000) of L = 1337: frames 0 and 1 are all zero, and samples below 400 lie in no other frame, so their
    gradient is exactly 0 (|z|' = 0 at 0); frame 2 onwards is live and every sample meets the bar."""
    pred, orig = pw_inputs(2, 1337, seed=12)
    pred[:, :1000] = 0.0
    g, g64 = _pw_check('power zero frames', pred, orig)
    assert float(g64[:, :400].abs().max()) == 0 and float(g64[:, 400:600].abs().max()) > 0
    assert float(g[:, :400].abs().max()) == 0


def test_power_loss_of_equal_signals_is_zero():
    import torch
    from nsynth_wavenet_amd import distill_autograd as dag
    pred, _ = pw_inputs(2, 1337, seed=13)
    val, g64 = pw_oracle(pred, pred.copy())
    assert val == 0 and float(g64.abs().max()) == 0
    P = torch.as_tensor(pred).cuda().requires_grad_(True)
    loss = dag.power_loss(P, torch.as_tensor(pred.copy()).cuda())
    loss.backward()
    assert float(loss.detach()) == 0 and float(P.grad.abs().max()) == 0


# ---- 2d ----
def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _same(a, b):
    import torch
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize('shape', MOL_SHAPES, ids=_mid)
def test_mol_calls_repeat_and_rows_are_independent(engines, shape):
    """two calls give the same bits, and the rows of a [B', T] call are the bits of the B' one-row calls"""
    B, T, S, M = shape
    d = _cuda(mol_inputs(shape, 'interior'))
    eng = engines(M)
    f, g = _mol_calls(eng, d, S, noise=d['rl'])
    f2, g2 = _mol_calls(eng, d, S, noise=d['rl'])
    assert _same(f['H_bl'], f2['H_bl']) and _same(f['sums'], f2['sums'])
    for a, b in zip(g, g2):
        assert _same(a, b)
    for b in range(B + FLOOR_ROWS):
        row = {k: v[b:b + 1].contiguous() for k, v in d.items()}
        fr, gr = _mol_calls(eng, row, S, noise=row['rl'])
        assert _same(fr['H_bl'], f['H_bl'][b:b + 1]), (shape, b, 'H_bl')
        for name, a, full in zip(('d_out_params', 'd_mean_tot', 'd_scale_tot'), gr, g):
            assert _same(a, full[b:b + 1]), (shape, b, name)


@pytest.mark.parametrize('shape', GAUSS_SHAPES, ids=lambda s: 'B{}-T{}'.format(*s))
def test_gauss_calls_repeat_and_rows_are_independent(engines, shape):
    d = _cuda(gauss_inputs(shape))
    eng = engines('gauss')
    run = lambda v: (eng.distill_gauss_kl(v['te'], v['mean'], v['scale'])['kl_bl'],) + \
        tuple(eng.distill_gauss_kl_grad(v['te'], v['mean'], v['scale'], _fac()))
    full = run(d)
    for a, b in zip(full, run(d)):
        assert _same(a, b)
    for b in range(shape[0]):
        for a, f in zip(run({k: v[b:b + 1].contiguous() for k, v in d.items()}), full):
            assert _same(a, f[b:b + 1]), (shape, b)


@pytest.mark.parametrize('shape', MOL_SHAPES[:2], ids=_mid)
def test_device_draws_fed_back_give_the_same_bits(engines, shape):
    import torch
    B, T, S, M = shape
    d = _cuda(mol_inputs(shape, 'interior'))
    eng = engines(M)
    f, g = _mol_calls(eng, d, S, seed=7)
    nz = eng.distill_mol_xent(d['te'], d['mean'], d['scale'], S, seed=7, want_noise=True)
    assert tuple(nz['noise'].shape) == (B + FLOOR_ROWS, S, T) and bool(torch.isfinite(nz['noise']).all())
    assert float(nz['noise'].abs().max()) < 11.6 and float(nz['noise'].std()) > 1.0
    assert _same(nz['H_bl'], f['H_bl'])
    f2, g2 = _mol_calls(eng, d, S, noise=nz['noise'])
    assert _same(f2['H_bl'], f['H_bl']) and torch.equal(f2['sums'], f['sums'])
    for a, b in zip(g, g2):
        assert _same(a, b)
    other = eng.distill_mol_xent(d['te'], d['mean'], d['scale'], S, seed=8, want_noise=True)['noise']
    assert not torch.equal(other, nz['noise'])


class _Arena(object):
    """outputs carved out of one device buffer whose every 32-bit word is 0xFFFFFFFF (a NaN as float32 and, in pairs, as
    float64), with at least GUARD words of it on both sides of each"""

    def __init__(self, **words):
        import torch
        self.off, n = {}, GUARD
        for k, w in words.items():
            self.off[k] = (n, w)
            n += (w + 63) // 64 * 64 + GUARD
        self.buf = torch.full((n,), -1, dtype=torch.int32, device='cuda')

    def view(self, k, dtype):
        o, w = self.off[k]
        return self.buf[o:o + w].view(dtype)

    def ptr(self, k):
        return ctypes.c_void_p(self.view(k, self.buf.dtype).data_ptr())

    def guards_touched(self):
        import torch
        keep = torch.ones_like(self.buf, dtype=torch.bool)
        for o, w in self.off.values():
            keep[o:o + w] = False
        return int((self.buf[keep] != -1).sum())


def test_nothing_is_written_outside_the_outputs(engines):
    """The C ABI on outputs carved out of NaN-filled buffers of the test's own: afterwards every output element is finite and
    is what the Python API returns, every guard word still holds its fill, and so does the slack of the workspace.  Every buffer
    has exactly the size the library asks for."""
    import torch
    from nsynth_wavenet_amd import _lib
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    f32, f64 = torch.float32, torch.float64
    fac = _fac()
    for shape in MOL_SHAPES[:2]:
        B, T, S, M = shape
        d = _cuda(mol_inputs(shape, 'interior'))
        Bp = B + FLOOR_ROWS
        eng = engines(M)
        lib, h = eng.lib, eng._h
        want_f, want_g = _mol_calls(eng, d, S, seed=7)
        n_ws = int(lib.wn_distill_workspace_bytes(h, Bp, T))
        assert n_ws > 0 and n_ws % 4 == 0
        a = _Arena(h_bl=Bp * T, noise=Bp * S * T, sums=4, ws=n_ws // 4, d_te=Bp * T * 3 * M, d_mean=Bp * T, d_scale=Bp * T)
        with torch.cuda.device(eng.device):
            _lib.check(lib.wn_distill_mol_xent(h, ptr(d['te']), 3 * M, ptr(d['mean']), ptr(d['scale']), Bp, T, S, None,
                                               ctypes.c_uint64(7), a.ptr('h_bl'), a.ptr('noise') if S == 5 else None,
                                               a.ptr('sums'), a.ptr('ws'), n_ws, eng._stream()), h)
            _lib.check(lib.wn_distill_mol_xent_grad(h, ptr(d['te']), 3 * M, ptr(d['mean']), ptr(d['scale']), Bp, T, S, None,
                                                    ctypes.c_uint64(7), ptr(fac), a.ptr('d_te'), a.ptr('d_mean'),
                                                    a.ptr('d_scale'), eng._stream()), h)
            torch.cuda.synchronize()
        touched = a.guards_touched()
        outs = {'h_bl': want_f['H_bl'], 'd_te': want_g[0], 'd_mean': want_g[1], 'd_scale': want_g[2]}
        if S == 5:
            outs['noise'] = eng.distill_mol_xent(d['te'], d['mean'], d['scale'], S, seed=7, want_noise=True)['noise']
        else:
            assert bool((a.view('noise', torch.int32) == -1).all()), 'noise_out not asked for, not written'
        print('guards mol {}: {} guard words changed'.format(_mid(shape), touched))
        assert touched == 0
        for k, want in outs.items():
            got = a.view(k, f32)
            assert bool(torch.isfinite(got).all()), (shape, k)
            assert _same(got, want.reshape(-1)), (shape, k)
        assert bool(torch.isfinite(a.view('sums', f64)).all()) and torch.equal(a.view('sums', f64), want_f['sums'])
        nblk = Bp * ((T + 63) // 64)
        ws = a.view('ws', torch.int32)
        assert bool(torch.isfinite(ws[:4 * nblk].view(f64)).all()) and bool((ws[4 * nblk:] == -1).all())
    for shape in GAUSS_SHAPES[:2]:
        B, T = shape
        d = _cuda(gauss_inputs(shape))
        eng = engines('gauss')
        lib, h = eng.lib, eng._h
        want_f = eng.distill_gauss_kl(d['te'], d['mean'], d['scale'])
        want_g = eng.distill_gauss_kl_grad(d['te'], d['mean'], d['scale'], fac)
        n_ws = int(lib.wn_distill_workspace_bytes(h, B, T))
        a = _Arena(kl_bl=B * T, sums=4, ws=n_ws // 4, d_te=B * T * 2, d_mean=B * T, d_scale=B * T)
        with torch.cuda.device(eng.device):
            _lib.check(lib.wn_distill_gauss_kl(h, ptr(d['te']), 2, ptr(d['mean']), ptr(d['scale']), B, T, a.ptr('kl_bl'),
                                               a.ptr('sums'), a.ptr('ws'), n_ws, eng._stream()), h)
            _lib.check(lib.wn_distill_gauss_kl_grad(h, ptr(d['te']), 2, ptr(d['mean']), ptr(d['scale']), B, T, ptr(fac),
                                                    a.ptr('d_te'), a.ptr('d_mean'), a.ptr('d_scale'), eng._stream()), h)
            torch.cuda.synchronize()
        print('guards gauss B{}-T{}: {} guard words changed'.format(B, T, a.guards_touched()))
        assert a.guards_touched() == 0
        for k, want in (('kl_bl', want_f['kl_bl']), ('d_te', want_g[0]), ('d_mean', want_g[1]), ('d_scale', want_g[2])):
            got = a.view(k, f32)
            assert bool(torch.isfinite(got).all()) and _same(got, want.reshape(-1)), (shape, k)
        assert torch.equal(a.view('sums', f64), want_f['sums'])
    from nsynth_wavenet_amd.engine import power_loss_grad, power_loss_sums
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for L in (801, 1337):
        B = 2
        pred, orig = (torch.as_tensor(v).cuda() for v in pw_inputs(B, L))
        want_s, want_g = power_loss_sums(pred, orig), power_loss_grad(pred, orig, fac)
        n_ws, n_gws = int(lib.wn_power_loss_workspace_bytes(B, L)), int(lib.wn_power_loss_grad_workspace_bytes(B, L))
        nf = (L + 199) // 200
        assert n_gws == (B * nf * 800 * 4 + 255) // 256 * 256
        a = _Arena(out2=4, ws=n_ws // 4, gws=n_gws // 4, d_pred=B * L)
        _lib.check(lib.wn_power_loss(ptr(pred), L, ptr(orig), L, B, L, a.ptr('out2'), a.ptr('ws'), n_ws, stream))
        _lib.check(lib.wn_power_loss_grad(ptr(pred), L, ptr(orig), L, B, L, ptr(fac), a.ptr('d_pred'), L, a.ptr('gws'), n_gws,
                                          stream))
        torch.cuda.synchronize()
        print('guards power L={}: {} guard words changed'.format(L, a.guards_touched()))
        assert a.guards_touched() == 0
        assert torch.equal(a.view('out2', f64), want_s)
        got = a.view('d_pred', f32)
        assert bool(torch.isfinite(got).all()) and _same(got, want_g.reshape(-1))
        gws = a.view('gws', torch.int32)
        assert bool(torch.isfinite(gws[:B * nf * 800].view(f32)).all()), 'every frame of the gradient workspace is written'
        assert bool((gws[B * nf * 800:] == -1).all())


def test_more_than_32_components_are_refused(R, engines):
    import torch
    from nsynth_wavenet_amd.engine import Engine
    eng = Engine(NG._small_cfg(R, 'mol', mol_mix=33))
    te = torch.zeros(1, 4, 99, device='cuda')
    mean, scale = torch.zeros(1, 4, device='cuda'), torch.ones(1, 4, device='cuda')
    for fn in (lambda: eng.distill_mol_xent(te, mean, scale, 4), lambda: eng.distill_mol_xent_grad(te, mean, scale, 4, _fac())):
        with pytest.raises(ValueError, match=r'33 mixture components \(1\.\.32 supported\)'):
            fn()
    eng.close()
    assert engines(32).hp.mol_mix == 32          # accepted, and run above


# ---- 2e ----
def test_composed_calculate_loss_off_the_golden_shape(R):
    """ParallelWavenet.calculate_loss(...)['loss'].backward() for the mol student and the small golden teacher at
    (B, F, T) = (3, 2, 260), S = 5, wav of 267 samples: the autograd glue (the fac values, the trim, the contrastive term's sign)
    at a ragged shape, at the bars of tests/test_gpu_distill_grad.py."""
    import torch
    from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet
    B, F, T = COMPOSED
    S = COMPOSED_S
    hp, (cfgd, seed, init), _, _ = D.golden_case(R, 'mol')
    hp = dict(hp, num_samples=S)
    assert hp['power_loss_factor'] > 0 and hp['contrastive_loss_factor'] > 0
    inp = composed_inputs()
    teacher = NG._wavenet(cfgd)
    assert (seed, init) == (1234, 'unit')
    eng = teacher.engine
    pw = ParallelWavenet(hp, teacher=teacher)
    dev = {k: torch.as_tensor(inp[k]).cuda() for k in ('mel', 'mel_rand', 'x', 'mean', 'scale', 'wav')}
    rl = [torch.as_tensor(v).cuda() for v in inp['rl']]
    # the oracle's teacher under mel and under mel_rand, ReLU derivatives near a tie taken from the engine's tapes
    ora, masks = {}, {}
    for key in ('mel', 'mel_rand'):
        o = ora[key] = TS._Oracle(cfgd, seed, init, inp[key], inp['x'])
        assert o.near <= TS.NEAR_MAX, (key, o.near)
        _, tape = eng.teacher_forward_tape(dev['x'], dev[key])
        masks[key], nflip = D.relu_masks(o.pre, D.tape_pre(tape, B, T, cfgd['skip_width']))
        assert nflip <= TS.NEAR_MAX, (key, nflip)
        rep = mol_report({'te': o.out.numpy(), 'mean': inp['mean'], 'scale': inp['scale'], 'rl': inp['rl'][key == 'mel_rand']})
        print('composed {}: {} near-tie pre-ReLU values, {} signs from the tape; {}'.format(key, o.near, nflip, rep))
        assert rep['near_threshold'] == 0 and rep['near_floor_dominant'] == 0 and rep['near_floor_weighted'] == 0, rep
    v = {k: torch.as_tensor(inp[k].astype(np.float64)).requires_grad_(True) for k in ('x', 'mean', 'scale')}
    te = lambda key: D.teacher_ff(v['x'], ora[key].enc, ora[key].w, ora[key].thp, masks=masks[key])
    ff64 = {'x': v['x'], 'mean_tot': v['mean'], 'scale_tot': v['scale'], 'wav': torch.as_tensor(inp['wav'].astype(np.float64))}
    ref = D.calculate_loss(hp, te('mel'), te('mel_rand'), ff64, rl[0].double().cpu(), rl[1].double().cpu(), stable=True)
    ref['loss'].backward()
    g = {k: dev[k].clone().requires_grad_(True) for k in ('x', 'mean', 'scale')}
    ff = {'x': g['x'], 'mean_tot': g['mean'], 'scale_tot': g['scale'], 'mel': dev['mel'], 'mel_rand': dev['mel_rand'],
          'wav': dev['wav']}
    losses = pw.calculate_loss(ff, noise=rl[0], cl_noise=rl[1])
    assert {'kl_loss', 'power_loss', 'contrastive_loss', 'loss'} <= set(losses)
    losses['loss'].backward()
    val = float(ref['loss'].detach())
    e = abs(float(losses['loss'].detach()) - val) / max(1.0, abs(val))
    print('composed loss {:.8e} (oracle {:.8e}): error / max(1, |ref|) = {:.2e} (bar 1e-05)'.format(
        float(losses['loss'].detach()), val, e))
    for k in ('kl_loss', 'power_loss', 'contrastive_loss'):
        print('composed {} {:.8e} (oracle {:.8e})'.format(k, float(losses[k].detach()), float(ref[k].detach())))
        assert abs(float(losses[k].detach()) - float(ref[k].detach())) <= 1e-5 * max(1.0, abs(float(ref[k].detach())))
    assert e <= 1e-5
    for k in ('x', 'mean', 'scale'):
        _cmp_grad('composed', 'd ' + k, g[k].grad, v[k].grad)
    pw.engine.close()
    eng.close()
