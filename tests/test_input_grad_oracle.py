"""CPU pin of the float64 oracles the input-gradient tests compare with (tests/input_grad_oracle64.py), and of
the conditions their cases rest on (tests/input_grad_cases.py):

  1  d mel of a deconv stack (deconv_grad_oracle64.stack_ff with mel as the leaf) against float64 central differences
  2  d noise of the student (StudentGrad64.forward restated with the noise in the graph): the restatement's values are the
     method's, its d_encoding is grads()', its d noise agrees with central differences
  3  d noise is causal: a cotangent on sample t0 alone gives exactly 0 for t > t0
  4  the composed gradient (mel and noise through stacks and flows) against central differences
  5  the shapes hit their seams -- the 64-frame tile of the first layer's data-gradient GEMM, its phase chunks -- and the
     chosen seeds keep every case inside the tie rules (at most MAX_ZEROED of a cotangent zeroed, no hidden near tie)
"""
import numpy as np
import pytest
import torch

import deconv_bwd_geometries as BG
import deconv_grad_oracle64 as DG
import input_grad_cases as C
import input_grad_oracle64 as IG
import student_grad_oracle64 as S

H = 1e-6                 # central-difference step
FD_TOL = 1e-6            # |fd - g| <= FD_TOL max |g|: the bar of tests/test_deconv_grad_oracle.py's sibling checks


def _fd_entries(value, x, got, n, seed, what):
    """central differences of value(x) at n random entries of the float64 array x against got"""
    rs = np.random.RandomState(seed)
    scale = np.abs(got).max()
    assert scale > 0
    for idx in sorted(set(int(i) for i in rs.randint(0, x.size, n))):
        vals = []
        for sgn in (1.0, -1.0):
            xp = x.copy()
            xp.reshape(-1)[idx] += sgn * H
            vals.append(value(xp))
        fd = (vals[0] - vals[1]) / (2 * H)
        err = abs(fd - got.reshape(-1)[idx])
        print('{} entry {}: fd {:.9e} autograd {:.9e}'.format(what, idx, fd, got.reshape(-1)[idx]))
        assert err <= FD_TOL * scale, (what, idx, fd, got.reshape(-1)[idx])


# ---- 1 ----
@pytest.mark.parametrize('act', ['leaky_relu', 'tanh', 'relu'])
@pytest.mark.parametrize('tag', ['base', 'three', 'single'])
def test_d_mel_matches_central_differences(tag, act):
    cfgd = BG.teacher_cfg(tag, upsample_act=act)
    dc = cfgd['deconv_config']
    w64 = DG.weights64(BG.weights('teacher', cfgd), len(dc))
    rs = np.random.RandomState(5)
    mel = rs.uniform(0, 1, [2, 3, BG.N_MEL])
    g = rs.standard_normal([2, 3 * BG.hop(tag), 64])
    got = IG.stack_d_mel(mel, w64, dc, act, g).numpy()
    assert got.shape == mel.shape
    _fd_entries(lambda m: IG.stack_value(m, w64, dc, act, g), mel, got, 6, 9, 'd mel {} {}'.format(tag, act))


# ---- 2, 3 ----
@pytest.fixture(scope='module')
def s1():
    hp, w = C.iaf_weights('S1')
    mel, noise, cot = S.case_inputs(2, 4, 32, seed=C.IAF_SEED + 100)
    return S.StudentGrad64(w, hp), mel, noise.astype(np.float64), cot


def test_restated_forward_is_the_oracles(s1):
    ora, mel, noise, cot = s1
    encs = ora.encodings(mel)
    with torch.no_grad():
        a = IG.student_forward(ora, torch.as_tensor(noise), encs)
        b, _ = ora.forward(noise, encs)
    for k in ('x', 'mean_tot', 'scale_tot'):
        assert torch.equal(a[k], b[k]), k
    ref = ora.grads(mel, noise, *cot)
    got = IG.student_input_grads(ora, mel, noise, cot)
    assert np.array_equal(got['d_encoding'], ref['d_encoding'])


def test_d_noise_matches_central_differences(s1):
    ora, mel, noise, cot = s1
    got = IG.student_input_grads(ora, mel, noise, cot)['d_noise']
    assert got.shape == noise.shape
    _fd_entries(lambda z: IG.student_value(ora, mel, z, cot), noise, got, 8, 3, 'd noise S1')


def test_d_noise_is_causal(s1):
    """x[t], mean_tot[t] and scale_tot[t] read the noise at t and before (the start conv sees shift_right(x)): a cotangent on
    sample t0 alone leaves d noise exactly 0 behind t0 -- and reaches t0 itself through x = noise scale_tot + mean_tot"""
    ora, mel, noise, _ = s1
    for t0 in (0, 13, 31):
        cot = [np.zeros_like(noise) for _ in range(3)]
        for i, v in enumerate((0.75, -1.5, 2.0)):
            cot[i][:, t0] = v
        d = IG.student_input_grads(ora, mel, noise, cot)['d_noise']
        assert np.all(d[:, t0 + 1:] == 0), t0
        assert np.all(d[:, t0] != 0) and (t0 == 0 or np.abs(d[:, :t0]).max() > 0), t0


# ---- 4 ----
def test_composed_gradient_matches_central_differences():
    hp, w = C.iaf_weights('S2')              # private stacks: every flow's own encoding reaches mel
    ora = S.StudentGrad64(w, hp)
    rs = np.random.RandomState(8)
    mel = rs.uniform(0, 1, [1, 64, 80])
    _, noise, cot = S.case_inputs(1, 64, 512, seed=4)
    noise = noise.astype(np.float64)
    got = IG.feed_forward_grads(ora, mel, noise, cot)
    _fd_entries(lambda m: IG.feed_forward_grads(ora, m, noise, cot)['value'], mel, got['d_mel'], 3, 1, 'composed d mel')
    _fd_entries(lambda z: IG.feed_forward_grads(ora, mel, z, cot)['value'], noise, got['d_noise'], 3, 2, 'composed d noise')
    # with every sign given as its own, the graph with `pos` is the same function
    pre = IG.stacks_pre(ora, mel)
    same = IG.feed_forward_grads(ora, mel, noise, cot, pos={p: z[-1] > 0 for p, z in pre.items()})
    # (z * slope and leaky_relu(z) round differently: to float64 rounding, not to the bit)
    assert np.abs(same['d_mel'] - got['d_mel']).max() <= 1e-12 * np.abs(got['d_mel']).max()
    assert np.abs(same['d_noise'] - got['d_noise']).max() <= 1e-12 * np.abs(got['d_noise']).max()
    # and the student's half alone is student_input_grads
    assert np.array_equal(IG.student_input_grads(ora, mel, noise, cot)['d_noise'], got['d_noise'])


# ---- 5 ----
def test_shapes_hit_their_seams():
    for tag in C.TILE_TAGS:
        for kind in C.KINDS:
            d = BG.layer_dims(BG.ACCEPTED[tag], BG.WIDTH[kind], *C.TILE_SHAPE)[0]
            assert d['L'] == 67 and d['cinp'] == 128 and d['cin'] == 80, d       # two 64-frame tiles, the second 3 frames
    for tag in BG.TAGS:
        S0 = BG.ACCEPTED[tag][0][1]
        for kind in C.KINDS:
            for shape in C.SHAPES:
                assert C.first_layer_chunks(tag, BG.WIDTH[kind], *shape) == (1, S0)      # one phase per chunk: npc = S > 1
        B, F = C.chunk_shape(tag)
        pchunk, npc = C.first_layer_chunks(tag, BG.WIDTH['student'], B, F)
        print('first-layer chunk shape {}: B = {}, S = {}, pchunk {}, npc {}'.format(tag, B, S0, pchunk, npc))
        assert F == 1 and pchunk == 2 and npc == (S0 + 1) // 2
        assert C.first_layer_chunks(tag, BG.WIDTH['student'], B - 1, F)[0] == 1
        assert npc > 1 or tag == 'three'         # 'three' has S = 2 in its first layer: two phases are one chunk


TIES = [('leaky_relu',) + c for c in C.LEAKY] + [('relu',) + c for c in C.RELU]


@pytest.mark.parametrize('act,kind,tag,shape', TIES, ids=['{}-{}-{}-B{}-F{}'.format(a, k, t, *s) for a, k, t, s in TIES])
def test_tie_rules_hold_for_the_chosen_seeds(act, kind, tag, shape):
    """DeconvCase asserts them (pick_rows: no hidden near tie; mask_last: at most MAX_ZEROED of the cotangent zeroed)"""
    c = C.DeconvCase(kind, tag, act, shape)
    print('{} {} {} {}: seeds {}, {} of {} zeroed'.format(act, kind, tag, shape, c.seeds, c.zeroed, c.g.numel()))
    assert c.zeroed <= DG.MAX_ZEROED * c.g.numel()


@pytest.mark.parametrize('tag', sorted(C.FF_CASES))
def test_composed_cases_are_clear(tag):
    hp, w, ora, mel, seeds, noise, cot = C.ff_inputs(tag)
    assert seeds[0] == C.FF_CASES[tag][2], 'FF_CASES names the first clear seed'
    pre = IG.stacks_pre(ora, mel)
    for p, zs in pre.items():
        assert sum(int(DG.near(z).sum()) for z in zs[:-1]) == 0, p
        n = int(DG.near(zs[-1]).sum())
        print('{} {}: mel seeds {}, {} of {} last-layer pre-activations near ties'.format(tag, p, seeds, n, zs[-1].numel()))
        assert n <= DG.MAX_ZEROED * zs[-1].numel()
    ref = ora.grads(mel, noise, *cot)
    assert S.near_tie_fraction(ref['aux']) <= 1e-4 and S.clamps_inactive(ref['aux'])
