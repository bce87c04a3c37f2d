"""deconv_front_kernel (csrc/wn_deconv.hip): the first upsampler layer of the shipped geometry -- deconv_config
[[40, 10], [80, 20]], 80 mels, 256 channels -- as ONE launch (fp32 mel in, G4 words out) wherever the stack ends in
deconv_pg_kernel, in place of mel_to_split_kernel + deconv_mfma_h_kernel<false> + deconv_interleave_g4_kernel<10>.

Its G4 words have no public view.  They are seen through the two consumers that make wn_run_deconv write G4 words:
  student  iaf_generate(want=('x',)) of parallel_wavenet.json with one flow of ten layers.  The student generates
           F * 200 // 512 * 512 samples, so it sees nothing at F = 1 and 2;
  teacher  teacher_forward of a 64-channel wavenet_mol.json with deconv_width 256 (the tiny teacher of
           tests/deconv_geometries.py, widened): every one of the F * 200 columns, from F = 1 on.
Engine.deconv writes fp32 rows, which keeps the three launches: it is held to the same oracle on the same inputs, so that
both routes through the first layer are pinned on every shape here.

Everything is compared with the float64 oracle (oracle/wavenet_np.py) at the bar of tests/test_gpu_deconv_geometries.py,
max |got - ref| <= 2e-5 max(1, max |ref|); tests/test_deconv_geometry_oracle.py shows for these consumers that a missing,
displaced or stale column is tens of bars, not rounding.  Shapes: F = 1 .. 4 (fewer frames than taps: every tap meets the
zero pad), 16, 17, 33 (one full block of 16 frames, one frame past it, two blocks and one), B = 3 with a different mel per
utterance, mels that are zero but for a first and a last frame of 8.0, a short call behind a long one on the same engine
(stale margins), two geometries that must keep the three launches, and the fp16 range guard of the layer's epilogue.
"""
import numpy as np
import pytest

import deconv_geometries as G

pytestmark = pytest.mark.gpu
BAR = 2e-5                  # tests/test_gpu_deconv_geometries.py: max-abs error / max(1, max |ref|)
DC = [[40, 10], [80, 20]]
HOP = 200
FRAMES = (1, 2, 3, 4, 16, 17, 33)


def _np(t):
    return t.detach().cpu().numpy()


def _rel(got, ref):
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))


def _engine(cfgd, w, precision=None):
    from nsynth_wavenet_amd.engine import Engine
    return Engine(cfgd, precision=precision).load_weights(w)


def _student_cfg():
    cfgd = dict(G.load_json('parallel_wavenet.json'), num_iaf_layers=[10])
    assert cfgd['deconv_config'] == DC and cfgd['deconv_width'] == 256
    return cfgd


def _teacher_cfg():
    return dict(G.load_json('wavenet_mol.json'), deconv_config=DC, width=64, double_gate_width=True, skip_width=64,
                deconv_width=256, num_layers=3, num_stages=2)


class Models(object):
    def __init__(self):
        from oracle import wavenet_np as O
        self.O = O
        self.s_cfg, self.t_cfg = _student_cfg(), _teacher_cfg()
        self.s_hp, self.t_hp = O.HP(self.s_cfg), O.HP(self.t_cfg)
        self.s_w = O.synth_weights(self.s_hp, 'student', seed=G.STUDENT_SEED, init=G.STUDENT_INIT)
        self.t_w = O.synth_weights(self.t_hp, 'teacher', seed=G.TEACHER_SEED, init=G.TEACHER_INIT)
        self.student = _engine(self.s_cfg, self.s_w, 'f16x3')
        self.teacher = _engine(self.t_cfg, self.t_w)
        self.fallbacks = 0

    def close(self):
        self.student.close()
        self.teacher.close()

    def inputs(self, B, F, seed=0):
        rs = np.random.RandomState(100 * seed + 17 * B + F)
        T = self.O.iaf_length(F, self.s_hp)
        mel = rs.uniform(0, 1, [B, F, G.N_MEL]).astype(np.float32)
        noise = self.O.logistic_from_uniform(rs.uniform(1e-5, 1 - 1e-5, [B, T]))
        wav = rs.uniform(-1, 1, [B, F * HOP]).astype(np.float32)
        return mel, noise, wav

    def check(self, mel, noise, wav, label):
        """rows, student and teacher on one set of inputs against the float64 oracle; returns the three device results"""
        O = self.O
        B, F = mel.shape[:2]
        # the two consumers take the front launch, Engine.deconv the three launches (no kernel runs for these questions)
        assert self.student.deconv_forms(B, F, split_out=True) == self.teacher.deconv_forms(B, F, split_out=True) == ['front', 'pg']
        assert self.student.deconv_forms(B, F) == ['h<false> g4<10>', 'hs<4> il']
        rows64 = O.deconv_stack(mel, self.s_w, self.s_hp, 'iaf_share', np.float64)
        rows = _np(self.student.deconv(mel))
        assert rows.shape == rows64.shape == (B, F * HOP, 256)
        r = _rel(rows, rows64)
        print('DECONV-FRONT {} B={} F={} rows: {:.2e} of the range'.format(label, B, F, r))
        assert np.isfinite(rows).all() and r <= BAR, (label, B, F, r)
        x = None
        if noise.shape[1] > 0:
            ref = O.iaf_feed_forward(mel, noise, self.s_w, self.s_hp, np.float64)
            x = _np(self.student.iaf_generate(mel, noise, want=('x',))['x'])
            r = _rel(x, ref['x'])
            print('DECONV-FRONT {} B={} F={} student x: {:.2e} of the range'.format(label, B, F, r))
            assert np.isfinite(x).all() and r <= BAR, (label, B, F, r)
            assert self.student.range_fallbacks == self.fallbacks      # (only the range-guard test raises the count)
        enc64 = O.deconv_stack(mel, self.t_w, self.t_hp, '', np.float64)
        tref = O.teacher_feed_forward(O.encode_signal(wav, self.t_hp, np.float64), enc64, self.t_w, self.t_hp, np.float64)
        out = _np(self.teacher.teacher_forward(wav, mel))
        assert out.shape == tref.shape
        r = _rel(out, tref)
        print('DECONV-FRONT {} B={} F={} teacher: {:.2e} of the range'.format(label, B, F, r))
        assert np.isfinite(out).all() and r <= BAR, (label, B, F, r)
        return rows, x, out


@pytest.fixture(scope='module')
def models():
    m = Models()
    yield m
    m.close()


@pytest.mark.parametrize('F', FRAMES)
def test_frames_around_the_taps_and_the_frame_block(F, models):
    """F < 4: every tap of every output frame reads the zero pad somewhere; 16 / 17 / 33: the seam of the 16-frame block."""
    mel, noise, wav = models.inputs(1, F)
    assert (noise.shape[1] > 0) == (F >= 3)
    models.check(mel, noise, wav, 'frames')


def test_batch_stride_of_the_mel_reads_and_the_g4_rows(models):
    """B = 3 at F = 17, a different mel per utterance: every utterance against the oracle, and the same bits as its own
    single-utterance call (B = 1)."""
    mel, noise, wav = models.inputs(3, 17)
    assert not np.array_equal(mel[0], mel[1]) and not np.array_equal(mel[1], mel[2])
    rows, x, out = models.check(mel, noise, wav, 'batch')
    for b in range(3):
        r1, x1, o1 = models.check(mel[b:b + 1], noise[b:b + 1], wav[b:b + 1], 'batch, row {}'.format(b))
        assert np.array_equal(rows[b], r1[0]) and np.array_equal(x[b], x1[0]) and np.array_equal(out[b], o1[0]), b


@pytest.mark.parametrize('F', (4, 17))
def test_a_first_and_a_last_frame_of_8_and_zeros_between(F, models):
    """A wrong tap offset or phase shows as a displaced peak: the oracle's peaks are where the first and the last frame
    reach, and nowhere else is there anything but the bias."""
    mel, noise, wav = models.inputs(2, F, seed=1)
    mel[:] = 0
    mel[0, 0], mel[0, -1] = 8.0, 8.0
    mel[1, 0, ::2], mel[1, -1, 1::2] = 8.0, 8.0
    models.check(mel, noise, wav, 'peaks')


def test_a_short_call_behind_a_long_one_finds_no_stale_margin(models):
    """F = 33, then F = 3 on the same engines: the second call's row stride is shorter and its zero margins lie where the
    first call left data.  Bit for bit what fresh engines give."""
    long_in, short_in = models.inputs(1, 33, seed=2), models.inputs(1, 3, seed=2)
    models.check(*long_in, 'stale, long')
    mel, noise, wav = short_in
    rows, x, out = models.check(mel, noise, wav, 'stale, short')
    fresh_s = _engine(models.s_cfg, models.s_w, 'f16x3')
    fresh_t = _engine(models.t_cfg, models.t_w)
    try:
        assert np.array_equal(x, _np(fresh_s.iaf_generate(mel, noise, want=('x',))['x']))
        assert np.array_equal(rows, _np(fresh_s.deconv(mel)))
        assert np.array_equal(out, _np(fresh_t.teacher_forward(wav, mel)))
    finally:
        fresh_s.close()
        fresh_t.close()


def test_what_the_forms_query_refuses(models):
    """wn_deconv_forms: WN_ENOENT for an unknown scope and WN_ESTATE before wn_finalize, as wn_deconv; WN_EINVAL for a null
    or short buffer, a shape below 1 and a precision wn_config.precision does not take."""
    import ctypes
    from nsynth_wavenet_amd.engine import Engine
    eng = models.student
    assert eng.deconv_forms(1, 3, split_out=True) == ['front', 'pg']
    with pytest.raises(KeyError):
        eng.deconv_forms(1, 3, scope='iaf_9')
    with pytest.raises(ValueError):
        eng.deconv_forms(0, 3)
    buf = ctypes.create_string_buffer(64)
    call = eng.lib.wn_deconv_forms
    assert call(eng._h, b'iaf_share', 1, 3, 1, -1, buf, len(buf)) == 0 and buf.value == b'front, pg'
    assert call(eng._h, b'iaf_share', 1, 3, 1, -1, buf, len(b'front, pg')) == -22        # no room for the terminator
    assert call(eng._h, b'iaf_share', 1, 3, 1, -1, None, 64) == -22
    assert call(eng._h, b'iaf_share', 1, 3, 1, 2, buf, len(buf)) == -22
    raw = Engine(models.s_cfg, precision='f16x3')
    try:
        with pytest.raises(RuntimeError):
            raw.deconv_forms(1, 3)
    finally:
        raw.close()


@pytest.mark.parametrize('tag', ('taps6', 'oddtap'))
def test_geometries_that_keep_the_three_launches(tag):
    """taps6: the first entry of tests/deconv_geometries.py with a layer of taps != 4 (its last layer has six, so no
    deconv_pg_kernel behind the first layer); oddtap: the first whose FIRST layer has (three).  Engine.deconv_forms says
    which kernels run; the result is held as well."""
    from oracle import wavenet_np as O
    cfgd, w = G.student_weights(tag)
    hp = O.HP(cfgd)
    eng = _engine(cfgd, w, 'f16x3')
    try:
        B, F = 2, G.f_crop(tag)
        forms = eng.deconv_forms(B, F, split_out=True)
        assert forms == G.GEOMETRIES[tag]['kernels']['g4'] and 'front' not in forms, (tag, forms)
        mel, noise, T = G.student_inputs(tag, B, F)
        ref = O.iaf_feed_forward(mel, noise, w, hp, np.float64)
        x = _np(eng.iaf_generate(mel, noise, want=('x',))['x'])
        r = _rel(x, ref['x'])
        print('DECONV-FRONT {} B={} F={} student x: {:.2e} of the range'.format(tag, B, F, r))
        assert np.isfinite(x).all() and r <= BAR and eng.range_fallbacks == 0, (tag, r)
    finally:
        eng.close()


def test_the_range_guard_of_the_epilogue_sends_the_call_to_the_fp32_form(models):
    """A mel inside the fp16 range whose layer-1 pre-activation is outside it: frame 3 is switched on where the weights of
    one output element (channel 5, sample 10 * 3 + 0) are positive in each of the four taps' frames, then scaled so that this
    pre-activation is 1.5 x 65504.  The split of the layer's OUTPUT must raise the flag; the call falls back to the fp32 form
    and returns what an fp32 engine returns."""
    O = models.O
    F, co, f, p = 8, 5, 3, 0
    W = O.get_kernel(models.s_w, 'iaf_share/trans_conv_1', 'kernel', models.s_hp.get('use_weight_norm', False), deconv=True,
                     dtype=np.float64)                                                   # [1, K, cout, cin]
    b1 = np.asarray(models.s_w['iaf_share/trans_conv_1/bias'], np.float64)
    mel = np.zeros([1, F, G.N_MEL], np.float64)
    r, d = (p + 15) % 10, (p + 15) // 10
    for j in range(4):
        mel[0, f + d - j] = (W[0, 10 * j + r, co] > 0)
    pre = O.trans_conv1d(mel, W, b1, 10, None)
    peak = np.abs(pre).max()
    assert peak == abs(pre[0, 10 * f + p, co]) and peak > 2.0, peak
    mel = (mel * (1.5 * 65504 / peak)).astype(np.float32)
    pre = O.trans_conv1d(mel.astype(np.float64), W, b1, 10, None)
    assert np.abs(mel).max() < 0.8 * 65504 < 1.2 * 65504 < np.abs(pre).max()
    T = O.iaf_length(F, models.s_hp)
    noise = O.logistic_from_uniform(np.random.RandomState(5).uniform(1e-5, 1 - 1e-5, [1, T]))
    eng = models.student
    before = eng.range_fallbacks
    x = _np(eng.iaf_generate(mel, noise, want=('x',), check_range=True)['x'])
    assert eng.range_fallbacks == before + 1
    models.fallbacks = before + 1
    assert np.isfinite(x).all()
    f32 = _engine(models.s_cfg, models.s_w, 'f32')
    try:
        x32 = _np(f32.iaf_generate(mel, noise, want=('x',))['x'])
    finally:
        f32.close()
    r = _rel(x, x32)
    print('DECONV-FRONT range guard: fallback against the fp32 engine {:.2e} of the range'.format(r))
    assert r <= BAR, r
    # ... and an in-range call afterwards is served by the split form again, within the bar
    mel2, noise2, wav2 = models.inputs(1, F, seed=3)
    models.check(mel2, noise2, wav2, 'after the fallback')
    assert eng.range_fallbacks == before + 1
