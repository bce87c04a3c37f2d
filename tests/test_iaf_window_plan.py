"""Windowed IAF generation on the host: the geometry config.iaf_window_geometry derives (reach of the flows,
frame span of the upsampler, period of the centre crop) against the float64 oracle, the constraints of
config.iaf_plan_windows, and a plan executed row by row in float64 against the whole utterance."""
import numpy as np
import pytest

from conftest import load_json
from iaf_window_oracle import SMALL, feed_forward_cropped, run_plan
from nsynth_wavenet_amd import config as C
from oracle import wavenet_np as O

# md = 16 with frame_shift 8: period 2, odd frame counts have a centre crop of 4 columns
SMALL5 = dict(SMALL, num_stages=5)
RESIZE = dict(SMALL, use_resize_conv=True, deconv_config=[[5, 2], [7, 4]])


def _student(cfgd, seed=11):
    hp = O.HP(cfgd)
    return hp, O.synth_weights(hp, 'student', seed=seed, init='unit')


def _inputs(hp, B, F, seed):
    rs = np.random.RandomState(seed)
    mel = rs.uniform(0, 1, [B, F, 80])
    T = O.iaf_length(F, hp)
    return mel, O.logistic_from_uniform(rs.uniform(1e-5, 1 - 1e-5, [B, T]), np.float64), T


KEYS = ('x', 'mean_tot', 'scale_tot')


def test_reach_is_sufficient_and_tight():
    """Noise reach + 1 samples before t leaves x, mean_tot and scale_tot at t bit-identical, noise at distance reach changes
    x at t.  (Seed 11 of the 'unit' weights: no ReLU of the two heads masks the path at the samples probed; a seed that
    did would need replacing, the property is the network's, not the seed's.)"""
    for cfgd in (SMALL, SMALL5):
        hp, w = _student(cfgd)
        g = C.iaf_window_geometry(hp)
        fl = hp.filter_length
        assert g.reach == sum(fl + (fl - 1) * sum(2 ** (i % hp.num_stages) for i in range(n)) for n in hp.num_iaf_layers)
        mel, noise, T = _inputs(hp, 1, 40, 3)
        ref = O.iaf_feed_forward(mel, noise, w, hp, np.float64)
        changed = 0
        for t in (g.reach + 1, g.reach + 30, T - 1):
            far, near = noise.copy(), noise.copy()
            far[0, t - g.reach - 1] += 1.0
            near[0, t - g.reach] += 1.0
            a = O.iaf_feed_forward(mel, far, w, hp, np.float64)
            b = O.iaf_feed_forward(mel, near, w, hp, np.float64)
            for k in KEYS:
                assert a[k][0, t] == ref[k][0, t], (k, t)
                assert np.array_equal(a[k][0, :t - g.reach - 1], ref[k][0, :t - g.reach - 1])     # causal as well
            changed += b['x'][0, t] != ref['x'][0, t]
        assert changed == 3


@pytest.mark.parametrize('cfgd', [SMALL, RESIZE, dict(load_json('parallel_wavenet.json'), deconv_width=8, width=8,
                                                         num_iaf_layers=[1])],
                         ids=['trans_conv', 'resize_conv', 'shipped_stack'])
def test_frame_span_is_sufficient_and_tight(cfgd):
    """Through the deconv stack a frame frames_before + 1 to the left (frames_after + 1 to the right) of the frame that
    holds an upsampled column leaves that column bit-identical; the last counted frame on either side changes a column of
    the frame."""
    hp, w = _student(cfgd)
    g = C.iaf_window_geometry(hp)
    fs = C.frame_shift(hp)
    F, f = 24, 11
    assert f - g.frames_before - 1 >= 0 and f + g.frames_after + 1 < F
    mel = np.random.RandomState(5).uniform(0, 1, [1, F, 80])
    ref = O.deconv_stack(mel, w, hp, 'iaf_share', np.float64)[0, f * fs:(f + 1) * fs]

    def cols(frame):
        m = mel.copy()
        m[0, frame] += 1.0
        return O.deconv_stack(m, w, hp, 'iaf_share', np.float64)[0, f * fs:(f + 1) * fs]
    assert np.array_equal(cols(f - g.frames_before - 1), ref) and np.array_equal(cols(f + g.frames_after + 1), ref)
    assert not np.array_equal(cols(f - g.frames_before), ref) and not np.array_equal(cols(f + g.frames_after), ref)


def test_mel_frames_beyond_the_span_leave_a_sample_alone():
    """End to end: sample t reads the conditioning of samples t - reach .. t, so a mel frame one beyond frames_before of the
    first of those columns, or one beyond frames_after of the last, leaves x, mean_tot and scale_tot at t bit-identical;
    the last counted frame on the right changes x at some t of its frame."""
    hp, w = _student(SMALL5)
    g = C.iaf_window_geometry(hp)
    fs = C.frame_shift(hp)
    F = 41
    mel, noise, T = _inputs(hp, 1, F, 4)
    c0 = (F * fs - T) // 2
    assert c0 == 4
    ref = O.iaf_feed_forward(mel, noise, w, hp, np.float64)
    t = 200
    lo = (t - g.reach + c0) // fs - g.frames_before - 1
    hi = (t + c0) // fs + g.frames_after + 1
    assert lo >= 0 and hi < F
    for frame in (lo, hi):
        m = mel.copy()
        m[0, frame] += 1.0
        a = O.iaf_feed_forward(m, noise, w, hp, np.float64)
        for k in KEYS:
            assert a[k][0, t] == ref[k][0, t], (k, frame)
    m = mel.copy()
    m[0, hi - 1] += 1.0
    a = O.iaf_feed_forward(m, noise, w, hp, np.float64)
    f = (t + c0) // fs
    assert np.any(a['x'][0, f * fs - c0:(f + 1) * fs - c0] != ref['x'][0, f * fs - c0:(f + 1) * fs - c0])


def test_shipped_figures():
    for name in ('parallel_wavenet.json', 'parallel_wavenet_gauss.json'):
        g = C.iaf_window_geometry(C.load_hparams(load_json(name)))
        assert g.reach == 3 * 2049 + 6141 == 12288 and g.period == 64
        assert g.frames_before <= 3 and g.frames_after <= 3       # the prefix test of test_gpu_iaf.py drops 3 frames


def _check_plan(hp, F, wf, crop):
    g = C.iaf_window_geometry(hp)
    fs = C.frame_shift(hp)
    md = 2 ** (hp.num_stages - 1)
    Fw, rows = C.iaf_plan_windows(hp, F, wf, crop)
    T = C.iaf_length(hp, F)
    assert T == (F * fs // md) * md
    Tw = C.iaf_length(hp, Fw)
    c0w = (Fw * fs - Tw) // 2
    c0g = (F * fs - T) // 2 if crop == 'centre' else 0
    assert Fw % g.period == (F % g.period if crop == 'centre' else 0) or (len(rows) == 1 and Fw == F)
    if F <= Fw:
        assert rows == [(0, 0, 0, T, 0)]
    pos = 0
    for i, (f0, to, kf, kt, ot) in enumerate(rows):
        first, last = i == 0, i == len(rows) - 1
        assert 0 <= f0 and f0 + Fw <= F
        assert to % 4 == 0 and to == f0 * fs + c0w - c0g
        assert 0 <= kf <= kt <= Tw
        assert ot == pos == to + kf                                 # the kept ranges tile [0, T) in order, once
        pos += kt - kf
        if first:
            assert f0 == 0 and to == 0 and kf == 0                   # the utterance's own start
        else:
            assert kf >= g.reach
            # ... and the conditioning of every sample a kept sample reads is the utterance's own on the left
            assert (kf - g.reach + c0w) // fs - g.frames_before >= 0
        if last:
            assert f0 + Fw == F and to + kt == T                     # ends at frame F, exactly at the last sample
        else:
            assert (kt - 1 + c0w) // fs + g.frames_after <= Fw - 1
    assert pos == T
    return Fw, rows


def test_planner_constraints():
    hp = C.load_hparams(load_json('parallel_wavenet.json'))
    n = 0
    for crop in ('centre', 'left'):
        for wf in (128, 192, 384, 1000):
            for F in list(range(390, 390 + 64)) + [129, 200, 1000, 1537, 10240, 48000]:
                if crop == 'left' and F < 256 and F % 64:
                    continue                                          # too short for a left-aligned plan: refused below
                Fw, rows = _check_plan(hp, F, wf, crop)
                n += len(rows) > 1
    assert n > 300
    with pytest.raises(ValueError):
        C.iaf_plan_windows(hp, 100, 384, 'left')                      # 100 frames: no window = 0 (mod 64) fits
    with pytest.raises(ValueError):
        C.iaf_plan_windows(hp, 100, 384, 'middle')
    # a small student with period 2 and one with period 1; windows too small for the geometry grow to the smallest that fits
    for cfgd in (SMALL, SMALL5, RESIZE):
        hs = O.HP(cfgd)
        for crop in ('centre', 'left'):
            for wf in (4, 24, 40, 64):
                for F in (20, 37, 61, 100, 101, 333):
                    if crop == 'left' and F < 40 and F % 2:
                        continue
                    _check_plan(hs, F, wf, crop)


def test_grid_rows_do_not_depend_on_the_frame_count():
    """What lets a stream run a window before the utterance ends: all rows but the tail are those of any longer plan."""
    hp = C.load_hparams(load_json('parallel_wavenet.json'))
    Fw, long_rows = C.iaf_plan_windows(hp, 5000, 192, 'left')
    for F in (400, 401, 463, 464, 1000, 4999):
        Fw2, rows = C.iaf_plan_windows(hp, F, 192, 'left')
        assert Fw2 == Fw == 192 and rows[:-1] == long_rows[:len(rows) - 1]
        assert all(f0 + Fw < F for f0, *_ in rows[:-1])


@pytest.mark.parametrize('crop', ['centre', 'left'])
def test_plan_against_float64(crop):
    """The plan executed row by row with the float64 oracle reproduces the whole utterance on every sample to 1e-12."""
    worst = 0.0
    for cfgd, F, wf in ((SMALL5, 61, 24), (SMALL5, 100, 40), (SMALL5, 101, 41), (SMALL, 77, 30), (RESIZE, 61, 24)):
        hp, w = _student(cfgd)
        mel, noise, T = _inputs(hp, 2, F, 9)
        Fw, rows = C.iaf_plan_windows(hp, F, wf, crop)
        assert len(rows) > 2
        c0 = (F * C.frame_shift(hp) - T) // 2
        ref = O.iaf_feed_forward(mel, noise, w, hp, np.float64)
        mine = feed_forward_cropped(mel, noise, w, hp, c0)
        for k in KEYS:
            assert np.array_equal(mine[k], ref[k])                    # the helper is the oracle at the centre crop
        if crop == 'left':
            ref = feed_forward_cropped(mel, noise, w, hp, 0)
        got, writers = run_plan(mel, noise, w, hp, Fw, rows)
        assert np.all(writers == 1)
        for k in KEYS:
            err = float(np.abs(got[k] - ref[k]).max())
            worst = max(worst, err)
            assert err <= 1e-12, (cfgd is SMALL5, F, wf, k, err)
    print('plan against float64, crop {}: largest error {:.3e}'.format(crop, worst))
