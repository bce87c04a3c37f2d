"""CPU side of the upsampler geometry sweep (tests/test_gpu_deconv_geometries.py).

1. The table of tests/deconv_geometries.py states what wn_pack_deconv derives from each deconv_config (taps, pL, phase groups,
   frame-axis table): held against the pack's formulas restated in deconv_geometries.pack_facts.

2. The float64 oracle the GPU tests compare with (oracle/wavenet_np.py: trans_conv1d, resize_conv1d) is a restatement of the
   closed form the kernels were derived from, so it is pinned here, on exactly these geometries, against an independent
   implementation: torch.nn.functional.conv_transpose1d cropped to [pL, pL + S L), and nearest-neighbour repeat_interleave +
   SAME-padded conv1d, in float64, to 1e-12 max |ref|.

3. Sensitivity of the consumer tests.  Tests B (student) and C (teacher) see the upsampler's split-fp16 G4 output only through
   a consumer, at the bar 2e-5 max(1, max |ref|).  For the weights those tests use (deconv_geometries.student_weights /
   teacher_weights) the oracle itself must move by at least SENS_COLUMN = 20 bars when ONE time column of the conditioning
   (all channels at one t) is zeroed -- at the first and the last column the consumer reads and on both sides of the last
   layer's L_in = 256 (DC_QW) and 640 (PG_FRAMES) seams -- and by at least SENS_ELEMENT = 4 bars when ONE element of magnitude
   >= 0.1 is zeroed.  A tile, phase, column or word the kernel drops, misplaces or leaves stale then fails B / C by a wide
   margin.
   THE LIMIT: a one-element error of relative size 2^-11 (a lost lo half of a split-fp16 word) moves the consumer's output by
   about 2^-11 x the single-element figure, far below the bar: B and C do NOT hold the GEMM arithmetic to rounding level.
   Test A (fp32 rows against the float64 oracle, every element) does that; B and C hold the split-output epilogues against
   missing, misplaced or stale words.
"""
import numpy as np
import pytest
import torch

import deconv_geometries as G
from oracle import wavenet_np as O

BAR = 2e-5                # tests B and C: max-abs error / max(1, max |ref|)
SENS_COLUMN = 20.0        # a zeroed conditioning column moves the oracle by at least this many bars
SENS_ELEMENT = 4.0        # ... and one zeroed element of |enc| >= 0.1 by this many


@pytest.mark.parametrize('tag', G.TAGS)
def test_table_states_what_the_pack_derives(tag):
    g = G.GEOMETRIES[tag]
    layers, pg, rg, fa = G.pack_facts(g['deconv_config'], bool(g.get('resize')))
    assert (layers, pg, rg, fa) == (g['layers'], g['pg'], g['pg_rg'], g['fa'])
    assert G.hop(tag) == g['hop']
    assert len(g['kernels']['rows']) == len(g['kernels']['g4']) == len(g['kernels']['f32']) == len(g['deconv_config'])
    assert len(g['kernels']['no_pg']) == len(g['kernels'].get('no_pg_rows', g['kernels']['rows'])) == len(g['deconv_config'])
    assert set(g['kernels']) <= {'rows', 'g4', 'f32', 'no_pg', 'no_pg_rows'}
    for column in G.TEACHER_KERNELS.get(tag, {}).values():
        assert len(column) == len(g['deconv_config'])
    assert set(G.TEACHER_KERNELS) == set(G.TEACHER_TAGS)


def test_frame_counts_and_narrow_row_groups():
    assert (G.f_a('hop256'), G.f_b('hop256')) == (17, 41)
    assert (G.f_a('three'), G.f_b('three')) == (33, 81)
    assert (G.f_a('one'), G.f_b('one')) == (257, None)
    # 64 channels (test C): row groups that are / are not a multiple of 8 take deconv_pg_kernel's two block mappings
    rg64 = {t: G.pack_facts(G.GEOMETRIES[t]['deconv_config'], width=64)[2] for t in ('hop256', 's12', 'three')}
    assert rg64 == {'hop256': 8, 's12': 6, 'three': 2}
    for tag in G.TAGS:
        for B, F in G.student_shapes(tag):
            assert F * G.hop(tag) // 512 > 0
        B, F = G.student_shapes(tag)[-1]
        assert (F * G.hop(tag) - F * G.hop(tag) // 512 * 512) // 2 > 0
        assert G.f_b_seen(tag) == (69 if tag == 's6' else G.f_b(tag))


@pytest.mark.parametrize('tag', G.TAGS)
def test_oracle_layers_match_torch(tag):
    g = G.GEOMETRIES[tag]
    rs = np.random.RandomState(5)
    for F in (1, 2, 7):
        L, cin = F, G.N_MEL
        for K, S in g['deconv_config']:
            x = rs.standard_normal([2, L, cin])
            b = rs.standard_normal([256])
            xt = torch.from_numpy(x).permute(0, 2, 1)
            if g.get('resize'):
                W = rs.standard_normal([1, K, cin, 256])                            # HWIO
                got = O.resize_conv1d(x, W, b, S, None)
                pl = (K - 1) // 2
                up = torch.nn.functional.pad(torch.repeat_interleave(xt, S, dim=2), (pl, K - 1 - pl))
                ref = torch.nn.functional.conv1d(up, torch.from_numpy(W[0]).permute(2, 1, 0), torch.from_numpy(b))
            else:
                W = rs.standard_normal([1, K, 256, cin])                            # [1, K, cout, cin]
                got = O.trans_conv1d(x, W, b, S, None)
                pL = (K - S) // 2
                full = torch.nn.functional.conv_transpose1d(xt, torch.from_numpy(W[0]).permute(2, 1, 0), torch.from_numpy(b),
                                                            stride=S)
                ref = full[:, :, pL:pL + S * L]
            ref = ref.permute(0, 2, 1).numpy()
            assert got.dtype == np.float64 and got.shape == ref.shape == (2, S * L, 256)
            assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (tag, F, K, S)
            L, cin = S * L, 256


def _patched(enc, t=None, ch=None):
    e = enc.copy()
    if t is not None:
        e[:, t, slice(None) if ch is None else ch] = 0.0
    return e


def _moves(base, out, keys):
    """largest movement over the outputs, in bars of each output"""
    return max(np.abs(out[k] - base[k]).max() / (BAR * max(1.0, np.abs(base[k]).max())) for k in keys)


def _element_channels(enc, t):
    """eight channels, evenly spaced among those with |enc[0, t, c]| >= 0.1, the smallest such magnitude among them"""
    big = np.flatnonzero(np.abs(enc[0, t]) >= 0.1)
    assert len(big) >= 8
    pick = list(big[np.linspace(0, len(big) - 1, 7).astype(int)])
    return pick + [int(big[np.argmin(np.abs(enc[0, t, big]))])]


@pytest.mark.parametrize('tag', G.TAGS)
def test_student_outputs_see_a_dropped_column_and_a_dropped_element(tag, monkeypatch):
    cfgd, w = G.student_weights(tag)
    hp = O.HP(cfgd)
    F = G.f_b_seen(tag) or G.f_a(tag)
    mel, noise, T = G.student_inputs(tag, 1, F)
    enc = O.deconv_stack(mel, w, hp, 'iaf_share', np.float64)
    c0 = (enc.shape[1] - T) // 2
    cur = {}
    monkeypatch.setattr(O, 'deconv_stack', lambda *a, **k: cur['enc'])

    def run(e):
        cur['enc'] = e
        return O.iaf_feed_forward(mel, noise, w, hp, np.float64)
    base = run(enc)
    keys = ('x', 'mean_tot', 'scale_tot')
    cols = G.seam_columns(tag, F, c0, T)
    assert {'first', 'last', '256-', '256+'} <= set(cols) and (G.f_b(tag) is None or {'640-', '640+'} <= set(cols))
    for name, t in cols.items():
        m = _moves(base, run(_patched(enc, t)), ('x',))
        print('{} student F={} column {} (t={}): x moves {:.0f} bars'.format(tag, F, name, t, m))
        assert m >= SENS_COLUMN, (tag, name, t, m)
    t = c0 + T // 2
    worst = min((_moves(base, run(_patched(enc, t, c)), keys), c) for c in _element_channels(enc, t))
    print('{} student F={} one element at t={}: least movement {:.1f} bars (channel {}, |enc| {:.3f})'.format(
        tag, F, t, worst[0], worst[1], abs(enc[0, t, worst[1]])))
    assert worst[0] >= SENS_ELEMENT, (tag, worst)


@pytest.mark.parametrize('tag', G.TEACHER_TAGS)
def test_teacher_outputs_see_a_dropped_column(tag):
    cfgd, w = G.teacher_weights(tag)
    hp = O.HP(cfgd)
    F = G.f_a(tag)
    mel, wav = G.teacher_inputs(tag, 1, F)
    enc = O.deconv_stack(mel, w, hp, '', np.float64)
    x = O.encode_signal(wav, hp, np.float64)
    base = {'out': O.teacher_feed_forward(x, enc, w, hp, np.float64)}
    cols = G.seam_columns(tag, F, 0, enc.shape[1])
    assert {'first', 'last', '256-', '256+'} <= set(cols)
    for name, t in cols.items():
        m = _moves(base, {'out': O.teacher_feed_forward(x, _patched(enc, t), w, hp, np.float64)}, ('out',))
        print('{} teacher F={} column {} (t={}): out_params move {:.0f} bars'.format(tag, F, name, t, m))
        assert m >= SENS_COLUMN, (tag, name, t, m)
