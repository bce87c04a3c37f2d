"""Windowed IAF generation on the GPU: Engine.iaf_generate_long / iaf_stream and the C call
wn_iaf_generate_windows against the one-shot call and the float64 oracle, on the synthetic weights of test_gpu_iaf.py."""
import ctypes
import threading

import numpy as np
import pytest

from conftest import load_json
from iaf_window_oracle import SMALL, feed_forward_cropped

pytestmark = pytest.mark.gpu
ALL = ('wav', 'idx', 'x', 'mean_tot', 'scale_tot', 'rand_input')
KEYS = ('x', 'mean_tot', 'scale_tot')
# width 64 / deconv width 256 keep the MFMA kernels; seven stages: reach 2 (3 + 2 * 127) = 514, period 64 / gcd(200, 64) = 8
REDUCED = {'num_stages': 7, 'num_iaf_layers': [7, 7]}


def _engine(cfgd, weights, precision=None):
    from nsynth_wavenet_amd.engine import Engine
    return Engine(cfgd, precision=precision).load_weights(weights)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return _np(t).view(np.int32) if t.dtype.is_floating_point else _np(t)


@pytest.fixture(scope='module')
def shipped():
    from oracle import wavenet_np as O
    cfgd = load_json('parallel_wavenet.json')
    hp = O.HP(cfgd)
    w = O.synth_weights(hp, 'student', seed=1234, init='tf')
    eng = _engine(cfgd, w, 'f16x3-hoisted')
    yield cfgd, hp, w, eng
    eng.close()


@pytest.mark.parametrize('precision', [None, 'f32'])
def test_single_row_plan_is_the_one_shot_bit_for_bit(precision):
    """b = r, t_origin = 0, everything kept: the window kernels reproduce the one-shot's noise and outputs as bit patterns,
    with device noise and with injected noise, odd centre crop (F = 11: 76 columns) and none (F = 64)."""
    from oracle import wavenet_np as O
    from nsynth_wavenet_amd import config as C
    cfgd = load_json('parallel_wavenet.json')
    hp = O.HP(cfgd)
    eng = _engine(cfgd, O.synth_weights(hp, 'student', seed=1234, init='tf'), precision)
    rs = np.random.RandomState(2)
    for B, F in ((2, 11), (1, 64), (3, 23)):
        mel = rs.uniform(0, 1, [B, F, 80]).astype(np.float32)
        T = O.iaf_length(F, hp)
        assert C.iaf_plan_windows(eng.hp, F)[1] == [(0, 0, 0, T, 0)]
        noise = O.logistic_from_uniform(rs.uniform(1e-5, 1 - 1e-5, [B, T]))
        for nz in (None, noise):
            a = eng.iaf_generate(mel, nz, seed=77, want=ALL)
            b = eng.iaf_generate_long(mel, nz, seed=77, want=ALL, rows_per_call=2)
            for k in ALL:
                assert a[k].shape == b[k].shape == (B, T) and a[k].dtype == b[k].dtype
                assert np.array_equal(_bits(a[k]), _bits(b[k])), (precision, F, nz is None, k)
    eng.close()


@pytest.mark.parametrize('groups', [True, False])
def test_shipped_model_against_the_one_shot(shipped, groups):
    """Multi-window plans of the shipped model against one-shot calls on the same seed: the device noise bit for bit
    (absolute Philox positions), x / mean_tot / scale_tot to 1e-5 max(1, max|ref|) -- the bar test_full_size_properties_config2
    sets for the same samples computed by calls of different length -- and idx = clip_quant of the window path's own x."""
    from nsynth_wavenet_amd import config as C
    cfgd, hp, w, eng = shipped
    eng.set_layer_groups(groups)
    try:
        worst, worst_seam = 0.0, 0.0
        for F in (320, 330):
            mel = np.random.RandomState(F).uniform(0, 1, [3, F, 80]).astype(np.float32)
            ref = {k: _np(v) for k, v in eng.iaf_generate(mel, seed=9, want=ALL).items()}
            assert (F * 200 - ref['x'].shape[1]) // 2 == (0 if F == 320 else 232)
            for wf in (128, 192):
                Fw, plan = C.iaf_plan_windows(eng.hp, F, wf)
                assert len(plan) >= 3
                seam = np.zeros(ref['x'].shape[1], bool)
                for (f0, to, kf, kt, ot) in plan[1:]:
                    seam[ot:ot + 512] = True
                for rpc in (1, 8):
                    out = eng.iaf_generate_long(mel, seed=9, want=ALL, window_frames=wf, rows_per_call=rpc)
                    assert np.array_equal(_bits(out['rand_input']), ref['rand_input'].view(np.int32)), (F, wf, rpc)
                    for k in KEYS:
                        err = np.abs(_np(out[k]) - ref[k])
                        bar = 1e-5 * max(1.0, float(np.abs(ref[k]).max()))
                        worst, worst_seam = max(worst, float(err.max() / bar)), max(worst_seam, float(err[:, seam].max() / bar))
                        assert err.max() <= bar, (F, wf, rpc, k, float(err.max()), bar)
                    wav, idx = eng.clip_quant(out['x'])
                    assert np.array_equal(_np(idx), _np(out['idx'])) and np.array_equal(_bits(wav), _bits(out['wav']))
        print('windows vs one-shot, groups={}: largest error {:.3f} of the bar, over the first 512 kept samples of each '
              'window {:.3f} of the bar'.format(groups, worst, worst_seam))
    finally:
        eng.set_layer_groups(None)


OFF_SPEC = {
    'reduced_mfma': (dict(REDUCED), 60, 24),
    'private_stacks_gauss': (dict(REDUCED, use_share_deconv=False, loss_type='gauss', num_iaf_layers=[7, 7, 7, 7]), 61, 32),
    'generic': (dict(SMALL, num_stages=5, deconv_width=64), 101, 41),
    'resize_conv': (dict(REDUCED, use_resize_conv=True, upsample_act='tanh'), 60, 24),
}


@pytest.mark.parametrize('name', sorted(OFF_SPEC))
def test_off_spec_students_against_the_float64_oracle(name):
    """Students off the shipped geometry, both crops, every sample against O.iaf_feed_forward of the WHOLE utterance in
    float64 at the one-shot's own bar (test_ragged_and_edge_shapes): 2e-5 max(1, max|ref|)."""
    from oracle import wavenet_np as O
    from nsynth_wavenet_amd import config as C
    patch, F, wf = OFF_SPEC[name]
    cfgd = dict(load_json('parallel_wavenet.json'), **patch)
    hp = O.HP(cfgd)
    w = O.synth_weights(hp, 'student', seed=21, init='unit')
    eng = _engine(cfgd, w)
    assert eng.iaf_window_geometry() == tuple(vars(C.iaf_window_geometry(eng.hp))[k]
                                              for k in ('reach', 'frames_before', 'frames_after', 'period'))
    rs = np.random.RandomState(8)
    B = 1                                                      # (the float64 upsampler is what this test's time goes to)
    mel = rs.uniform(0, 1, [B, F, 80]).astype(np.float32)
    T = O.iaf_length(F, hp)
    noise = rs.standard_normal([B, T]).astype(np.float32) if cfgd['loss_type'] == 'gauss' else \
        O.logistic_from_uniform(rs.uniform(1e-5, 1 - 1e-5, [B, T]))
    refs = {'centre': O.iaf_feed_forward(mel, noise, w, hp, np.float64)}
    refs['left'] = feed_forward_cropped(mel, noise, w, hp, 0)
    for crop in ('centre', 'left'):
        Fw, plan = C.iaf_plan_windows(eng.hp, F, wf, crop)
        assert len(plan) >= 3, (name, crop, Fw, plan)
        out = eng.iaf_generate_long(mel, noise, want=KEYS, window_frames=wf, rows_per_call=3, crop=crop)
        for k in KEYS:
            err = float(np.abs(_np(out[k]) - refs[crop][k]).max())
            bar = 2e-5 * max(1.0, float(np.abs(refs[crop][k]).max()))
            print('{} crop={} {}: error {:.3e} (bar {:.3e}), {} rows of {} frames'.format(name, crop, k, err, bar, len(plan), Fw))
            assert err <= bar, (name, crop, k, err, bar)
    eng.close()


@pytest.fixture(scope='module')
def reduced():
    from oracle import wavenet_np as O
    cfgd = dict(load_json('parallel_wavenet.json'), **REDUCED)
    eng = _engine(cfgd, O.synth_weights(O.HP(cfgd), 'student', seed=21, init='unit'))
    yield eng
    eng.close()


def _stream_all(eng, mel, cuts, seed, wf):
    import torch
    st = eng.iaf_stream(batch=int(mel.shape[0]), seed=seed, window_frames=wf, want=ALL)
    parts, at = [], 0
    for n in cuts:
        parts.append(st.push(mel[:, at:at + n]))
        at += n
    assert at == mel.shape[1]
    parts.append(st.finish())
    return {k: torch.cat([p[k] for p in parts], 1) for k in ALL}


def test_stream_equals_the_long_call_however_the_frames_are_cut(reduced):
    import torch
    eng = reduced
    F, wf, B = 131, 24, 2
    mel = torch.as_tensor(np.random.RandomState(4).uniform(0, 1, [B, F, 80]).astype(np.float32)).to(eng.device)
    ref = eng.iaf_generate_long(mel, seed=5, want=ALL, window_frames=wf, crop='left')
    assert ref['x'].shape == (B, eng.iaf_length(F)) and bool(torch.isfinite(ref['x']).all())
    for cuts in ((1, 7, 64, 3, F - 75), (F,), (1,) * F):
        got = _stream_all(eng, mel, cuts, 5, wf)
        for k in ALL:
            assert got[k].shape == ref[k].shape and np.array_equal(_bits(got[k]), _bits(ref[k])), (cuts[:5], k)
    # F a multiple of the period: the left-aligned crop is the one-shot's centred crop -- the same noise bit for bit, and x
    # within twice the 2e-5 bar each of the two holds against the float64 oracle
    F = 128
    one = eng.iaf_generate(mel[:, :F], seed=5, want=ALL)
    got = _stream_all(eng, mel[:, :F], (50, 50, 28), 5, wf)
    assert np.array_equal(_bits(got['rand_input']), _bits(one['rand_input']))
    assert float((got['x'] - one['x']).abs().max()) <= 4e-5 * max(1.0, float(one['x'].abs().max()))


def test_two_streams_on_forks_from_two_threads(reduced):
    import torch
    eng = reduced
    F, wf = 100, 24
    mels = [torch.as_tensor(np.random.RandomState(s).uniform(0, 1, [1, F, 80]).astype(np.float32)).to(eng.device)
            for s in (1, 2)]
    serial = [_stream_all(eng, m, (30, 30, 40), 3 + i, wf) for i, m in enumerate(mels)]
    torch.cuda.synchronize()
    got, errs = [None, None], []

    def work(i):
        try:
            fork = eng.fork()
            with torch.cuda.stream(torch.cuda.Stream(eng.device)):
                got[i] = _stream_all(fork, mels[i], (30, 30, 40), 3 + i, wf)
                torch.cuda.current_stream().synchronize()
            fork.close()
        except Exception as e:                                     # surfaced below, in the main thread
            errs.append(e)
    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for i in range(2):
        for k in ALL:
            assert np.array_equal(_bits(got[i][k]), _bits(serial[i][k])), (i, k)


def test_beyond_the_one_shot_limit(shipped):
    """F = 10 240 frames = 2 048 000 samples: the one-shot refuses, the long call returns finite audio on the 2^-15 grid, and
    a 20 000-sample section in the middle matches a one-shot on the mel slice around it (context included, the long call's
    own noise injected) at the bar of test_shipped_model_against_the_one_shot."""
    import torch
    cfgd, hp, w, eng = shipped
    F = 10240
    mel = torch.as_tensor(np.random.RandomState(31).uniform(0, 1, [1, F, 80]).astype(np.float32)).to(eng.device)
    assert eng.iaf_needs_windows(F)
    with pytest.raises(ValueError, match='2,000,000'):
        eng.iaf_generate(mel)
    out = eng.iaf_generate_long(mel, seed=1, want=ALL)
    assert out['wav'].shape == (1, F * 200)
    wav = out['wav'].double()
    assert bool(torch.isfinite(out['x']).all()) and bool((wav * 32768 == torch.round(wav * 32768)).all())
    assert float(wav.min()) >= -1 and float(wav.max()) <= 1 - 2.0 ** -15
    # the section holds the seam at sample 1 030 288 (window 16 of the default plan); the slice is 256 frames long, a multiple
    # of the period like the utterance, so both crops are 0 and slice sample t is sample 200 fa + t
    fa, Fs, s0 = 5030, 256, 1020000
    assert fa * 200 + 12288 + 2 * 200 <= s0 and s0 + 20000 + 2 * 200 <= (fa + Fs) * 200
    one = eng.iaf_generate(mel[:, fa:fa + Fs], out['rand_input'][:, fa * 200:(fa + Fs) * 200], want=KEYS)
    for k in KEYS:
        a, b = out[k][:, s0:s0 + 20000], one[k][:, s0 - fa * 200:s0 - fa * 200 + 20000]
        bar = 1e-5 * max(1.0, float(b.abs().max()))
        err = float((a - b).abs().max())
        print('beyond the limit, {}: section error {:.3e} (bar {:.3e})'.format(k, err, bar))
        assert err <= bar, (k, err, bar)


def test_refusals_by_name_and_geometry_twin(shipped):
    import torch
    from nsynth_wavenet_amd import _lib, config as C
    cfgd, hp, w, eng = shipped
    assert eng.iaf_window_geometry() == (12288, 2, 2, 64)
    g = C.iaf_window_geometry(eng.hp)
    assert eng.iaf_window_geometry() == (g.reach, g.frames_before, g.frames_after, g.period)
    Fw, Tw = 11, 2048
    mel = torch.zeros((2, Fw, 80), device=eng.device)
    out = eng._window_outputs(2, 3000, ('x',))
    ok = [(0, 0, 0, Tw, 0), (1, 0, 0, Tw, 0)]
    eng.iaf_generate_windows(mel, ok, out)
    for bad, name in (((0, 2, 0, Tw, 0), 't_origin'), ((0, -4, 0, Tw, 0), 't_origin'),
                      ((0, 0, 0, Tw + 1, 0), 'kept range'), ((0, 0, -1, Tw, 0), 'kept range'), ((0, 0, 9, 8, 0), 'kept range'),
                      ((0, 0, 0, Tw, 3000 - Tw + 1), 'T_out'), ((2, 0, 0, Tw, 0), 'B_out'), ((-1, 0, 0, Tw, 0), 'B_out'),
                      ((1, 0, 100, 200, Tw - 50), 'overlapping')):
        with pytest.raises(ValueError, match=name):
            eng.iaf_generate_windows(mel, [bad, ok[1]], out)
    with pytest.raises(ValueError, match='unknown form'):
        eng.iaf_generate_windows(mel, ok, out, form=7)
    with pytest.raises(ValueError, match='shorter than one max-dilation block'):
        eng.iaf_generate_windows(mel[:, :2].contiguous(), ok, out)
    # the 2,000,000-sample limit is the window's: refused before the workspace is looked at
    table = (_lib.WindowRow * 1)(_lib.WindowRow(0, 0, 0, 512, 0))
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=eng.device)
    big = torch.zeros((1, 10001, 80), device=eng.device)
    rc = eng.lib.wn_iaf_generate_windows(eng._h, -1, 1, ctypes.c_void_p(big.data_ptr()), 1, 10001, table, None, 2, 3000, 0,
                                         ctypes.c_void_p(out['wav'].data_ptr()), None, None, None, None, None,
                                         ctypes.c_void_p(ws.data_ptr()), ws.numel(), None)
    assert rc == -22 and b'2,000,000' in eng.lib.wn_last_error(eng._h)
    from nsynth_wavenet_amd.engine import Engine
    teacher = Engine(load_json('wavenet_mol.json'))
    assert teacher.lib.wn_iaf_window_geometry(teacher._h, None, None, None, None) == -22
    teacher.close()
