"""Upsampler forward (csrc/wn_deconv.hip and the frame-axis GEMM of csrc/wn_iaf_f.hip) off the two deconv_configs the rest
of the suite runs: the ten geometries of tests/deconv_geometries.py (its table names the kernels every row runs, and tests B
and C hold every cell of it against Engine.deconv_forms, the plan the runner launches from), each at shapes
(B, F) that put almost every tap on a zero pad (1, 1), have an odd batch (3, 2), cross one DC_QW = 256 workgroup of q columns
on the last layer (2, F_a) and one PG_FRAMES = 640 tile (1, F_b).

  A  Engine.deconv -- fp32 rows -- against the float64 oracle, every element, split-fp16 and fp32 GEMMs, tf-init and unit
     weights:  max |got - ref| <= 2e-5 max(1, max |ref|)  (the bar of tests/test_gpu_iaf.py for this comparison), the split-fp16
     error within 2 x the fp32 error + 1e-7 of the range (test_split_fp16_is_as_accurate_as_fp32's rule), two calls the same
     bits, a row of a batch the same bits as the single-row call.  This is what holds the GEMM arithmetic to rounding level.
  B  the split-fp16 G4 output of the last layer has no public view, so it is seen through the MFMA student (one flow of ten
     layers): x, mean_tot and scale_tot of a split-fp16 handle, of one created under WN_DC_NO_PG=1 (phase-major GEMM +
     interleave in place of deconv_pg_kernel and of the frame-axis GEMM) and of an fp32 handle, each within 2e-5 of the float64
     oracle, the first two within 4e-6 of each other (the cross-form bar of test_phase_group_upsampler_matches_the_phase_major_form).
  C  the same at 64 channels through a tiny teacher (row-group counts 8, 6 and 2: both block mappings of deconv_pg_kernel).
  D  deconv_configs outside what wn_create accepts are refused, not served.

B and C see a missing, misplaced or stale column or word, not a rounding-level error: tests/test_deconv_geometry_oracle.py
proves, for the very weights used here, that one zeroed conditioning column moves the oracle's outputs by >= 20 bars and one
zeroed element of magnitude >= 0.1 by >= 4 bars, and states the limit.

Measured on an MI355X (largest over geometries, shapes and weights, as a fraction of the range; per geometry in DESIGN.md
18.2): A 1.5e-6 with split-fp16 and 2.1e-6 with fp32 GEMMs; B 7.1e-7 (split-fp16, both upsampler forms) and 1.7e-6 (fp32)
against the oracle, and exactly 0 between the two upsampler forms, which add the same products in the same order; C 5.8e-7.
Would-fail checks on scratch builds: a phase-group pack with pg_d off by one fails B and C on every geometry
that has the pack; the hs kernel taking halo column 0 for every tap fails A on taps6 and three; the code before the fix of
DESIGN.md 18.5 fails B on oddtap and the 256-channel fp32 teacher.
"""
import numpy as np
import pytest

import deconv_geometries as G

pytestmark = pytest.mark.gpu
BAR = 2e-5                  # against the float64 oracle: max-abs error / max(1, max |ref|)
BAR_FORMS = 4e-6            # phase-group upsampler against the phase-major one, same arithmetic in another order
OUTS = ('x', 'mean_tot', 'scale_tot')


def _np(t):
    return t.detach().cpu().numpy()


def _rel(got, ref):
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))


def _engine(cfgd, w, precision=None):
    from nsynth_wavenet_amd.engine import Engine
    return Engine(cfgd, precision=precision).load_weights(w)


@pytest.fixture(scope='module')
def students():
    """the student handles of deconv_geometries.student_weights, one per (tag, precision), shared by tests A and B"""
    made = {}

    def get(tag, precision):
        if (tag, precision) not in made:
            cfgd, w = G.student_weights(tag)
            made[tag, precision] = _engine(cfgd, w, precision)
        return made[tag, precision]
    yield get
    for e in made.values():
        e.close()


def _assert_forms(e, B, F, rows, g4, who):
    """what the engine's upsampler launches for fp32 rows and (g4 not None) for G4 words, against the table; no launch"""
    assert e.deconv_forms(B, F) == rows, (who, B, F, 'rows')
    if g4 is not None:
        assert e.deconv_forms(B, F, split_out=True) == g4, (who, B, F, 'G4')


def _rows_case(tag, engs, w, hp, label):
    """test A on one set of weights: engs = {'f16x3': ..., 'f32': ...}"""
    from oracle import wavenet_np as O
    rs = np.random.RandomState(len(tag) + 31)
    for B, F in G.rows_shapes(tag):
        mel = rs.uniform(0, 1, [B, F, G.N_MEL]).astype(np.float32)
        ref = O.deconv_stack(mel, w, hp, 'iaf_share', np.float64)
        scale = max(1.0, np.abs(ref).max())
        err = {}
        for p, e in engs.items():
            got = _np(e.deconv(mel))
            assert got.shape == ref.shape == (B, F * G.hop(tag), 256)
            err[p] = float(np.abs(got - ref).max())
            print('DECONV-GEO A {} {} {} B={} F={}: max|got - ref| = {:.3e} = {:.2e} of the range'.format(
                tag, label, p, B, F, err[p], err[p] / scale))
            assert np.isfinite(got).all(), (tag, label, p, B, F)
            assert np.array_equal(got, _np(e.deconv(mel))), (tag, label, p, B, F)              # deterministic
            if B > 1:
                for b in range(B):
                    assert np.array_equal(got[b], _np(e.deconv(mel[b:b + 1]))[0]), (tag, label, p, B, F, b)
        for p in engs:
            assert err[p] <= BAR * scale, (tag, label, p, B, F, err[p])
        assert err['f16x3'] <= 2 * err['f32'] + 1e-7 * scale, (tag, label, B, F, err)


@pytest.mark.parametrize('tag', G.TAGS)
def test_rows_match_the_float64_oracle(tag, students):
    """Test A."""
    from oracle import wavenet_np as O
    cfgd, w = G.student_weights(tag)
    hp = O.HP(cfgd)
    _rows_case(tag, {p: students(tag, p) for p in ('f16x3', 'f32')}, w, hp, G.STUDENT_INIT)
    w_tf = O.synth_weights(hp, 'student', seed=777, init='tf')
    engs = {p: _engine(cfgd, w_tf, p) for p in ('f16x3', 'f32')}
    try:
        _rows_case(tag, engs, w_tf, hp, 'tf')
    finally:
        for e in engs.values():
            e.close()


@pytest.mark.parametrize('tag', G.TAGS)
def test_g4_words_through_the_student(tag, students, monkeypatch):
    """Test B."""
    from oracle import wavenet_np as O
    cfgd, w = G.student_weights(tag)
    hp = O.HP(cfgd)
    monkeypatch.delenv('WN_DC_NO_PG', raising=False)
    engs = {'f16x3': students(tag, 'f16x3'), 'f32': students(tag, 'f32')}
    monkeypatch.setenv('WN_DC_NO_PG', '1')
    engs['f16x3, phase-major'] = _engine(cfgd, w, 'f16x3')
    monkeypatch.delenv('WN_DC_NO_PG', raising=False)
    try:
        # the kernels column of the table is what these handles launch.  An fp32 student never asks for G4 words; a
        # split-fp16 one runs the fp32 column in the one call that re-runs a range-guard fallback
        k = G.GEOMETRIES[tag]['kernels']
        B, F = G.student_shapes(tag)[0]
        _assert_forms(engs['f16x3'], B, F, k['rows'], k['g4'], (tag, 'f16x3'))
        _assert_forms(engs['f16x3, phase-major'], B, F, k.get('no_pg_rows', k['rows']), k['no_pg'], (tag, 'WN_DC_NO_PG'))
        _assert_forms(engs['f32'], B, F, k['f32'], None, (tag, 'f32'))
        assert engs['f16x3'].deconv_forms(B, F, precision='f32') == k['f32'], tag
        if k['g4'][0] == 'front':
            # past the 32-bit store offsets of deconv_front_kernel the first layer is three launches again
            Fp = G.f_past_front(tag)
            assert engs['f16x3'].deconv_forms(1, Fp - 1, split_out=True) == k['g4'], tag
            assert engs['f16x3'].deconv_forms(1, Fp, split_out=True) == k['rows'][:1] + k['g4'][1:], tag
        for B, F in G.student_shapes(tag):
            mel, noise, T = G.student_inputs(tag, B, F)
            assert T == O.iaf_length(F, hp) > 0
            ref = O.iaf_feed_forward(mel, noise, w, hp, np.float64)
            out = {}
            for p, e in engs.items():
                # the default form is what runs: layer groups on hoisted conditioning (split-fp16), hoisted conditioning (fp32)
                assert e.iaf_cond_hoisted(B, F), (tag, p, B, F)
                assert bool(e.iaf_layer_groups(B, F)) == (p != 'f32'), (tag, p, B, F)
                out[p] = {k: _np(v) for k, v in e.iaf_generate(mel, noise, want=OUTS).items()}
                again = e.iaf_generate(mel, noise, want=OUTS)
                for k in OUTS:
                    r = _rel(out[p][k], ref[k])
                    print('DECONV-GEO B {} {} B={} F={} {}: {:.2e} of the range'.format(tag, p, B, F, k, r))
                    assert np.isfinite(out[p][k]).all(), (tag, p, B, F, k)
                    assert np.array_equal(out[p][k], _np(again[k])), (tag, p, B, F, k)
                assert e.range_fallbacks == 0, (tag, p, B, F)
            for k in OUTS:
                r = _rel(out['f16x3'][k], out['f16x3, phase-major'][k])
                print('DECONV-GEO B {} forms B={} F={} {}: {:.2e} of the range'.format(tag, B, F, k, r))
            for p in engs:
                for k in OUTS:
                    assert _rel(out[p][k], ref[k]) <= BAR, (tag, p, B, F, k)
            for k in OUTS:
                assert _rel(out['f16x3'][k], out['f16x3, phase-major'][k]) <= BAR_FORMS, (tag, B, F, k)
    finally:
        engs['f16x3, phase-major'].close()


def _teacher_case(tag, cfgd, w, precisions, shapes, label, kernels):
    from oracle import wavenet_np as O
    hp = O.HP(cfgd)
    engs = {p: _engine(cfgd, w, p) for p in precisions}
    try:
        for p, e in engs.items():
            pre = 'f32_' if p == 'f32' else ''
            _assert_forms(e, *shapes[-1], kernels[pre + 'rows'], kernels[pre + 'g4'], (tag, label, p))
        for B, F in shapes:
            mel, wav = G.teacher_inputs(tag, B, F)
            enc64 = O.deconv_stack(mel, w, hp, '', np.float64)
            ref = O.teacher_feed_forward(O.encode_signal(wav, hp, np.float64), enc64, w, hp, np.float64)
            for p, e in engs.items():
                out = _np(e.teacher_forward(wav, mel))
                assert out.shape == ref.shape
                r = _rel(out, ref)
                print('DECONV-GEO C {} {} {} B={} F={}: {:.2e} of the range'.format(tag, label, p or 'f16x3', B, F, r))
                assert np.isfinite(out).all(), (tag, p, B, F)
                assert np.array_equal(out, _np(e.teacher_forward(wav, mel))), (tag, p, B, F)
                assert r <= BAR, (tag, label, p, B, F, r)
    finally:
        for e in engs.values():
            e.close()


@pytest.mark.parametrize('tag', G.TEACHER_TAGS)
def test_g4_words_of_64_channels_through_the_teacher(tag):
    """Test C."""
    cfgd, w = G.teacher_weights(tag)
    _teacher_case(tag, cfgd, w, (None, 'f32'), ((2, 3), (1, G.f_a(tag))), '64 channels', G.TEACHER_KERNELS[tag])


def test_fp32_upsampler_of_256_channels_hands_a_teacher_g4_words():
    """A teacher handle created with precision='f32' runs its upsampler on the fp32 GEMMs and still has to hand the layer
    kernels G4 words.  At 256 channels the last layer is the frame-axis GEMM, which wove its output into fp32 rows whatever
    the consumer asked for (found by this sweep); the suite's fp32 teachers were all 64 channels wide."""
    from oracle import wavenet_np as O
    cfgd = dict(G.teacher_cfg('hop256'), deconv_width=256)
    w = O.synth_weights(O.HP(cfgd), 'teacher', seed=G.TEACHER_SEED, init=G.TEACHER_INIT)
    _teacher_case('hop256', cfgd, w, ('f32', None), ((2, 3),), '256 channels', G.TEACHER_256_KERNELS)


REFUSED = [('filter not a multiple of the stride', [[40, 12], [80, 20]]),
           ('filter - stride odd', [[40, 10], [30, 15]]),
           ('filter - stride odd in the first layer', [[10, 5], [80, 20]]),
           ('nine taps', [[40, 10], [180, 20]]),
           ('stride 33', [[40, 10], [99, 33]]),
           ('five layers', [[4, 2]] * 5)]


@pytest.mark.parametrize('why,dc', REFUSED, ids=[r[0].replace(' ', '-') for r in REFUSED])
def test_refusals_stay_refusals(why, dc):
    """Test D."""
    from nsynth_wavenet_amd.engine import Engine
    for precision in ('f16x3', 'f32'):
        with pytest.raises(ValueError):
            Engine(dict(G.load_json('parallel_wavenet.json'), deconv_config=dc, num_iaf_layers=[10]), precision=precision)
    with pytest.raises(ValueError):
        Engine(dict(G.load_json('wavenet_mol.json'), deconv_config=dc))


def test_a_mis_shaped_mel_is_refused(students):
    eng = students('oddtap', 'f16x3')
    mel, noise, T = G.student_inputs('oddtap', 1, G.f_crop('oddtap'))
    with pytest.raises(ValueError):
        eng.iaf_generate(mel[:, :, :79], noise, want=('x',))
    with pytest.raises(ValueError):
        eng.iaf_generate(mel[0], noise, want=('x',))


def test_three_taps_on_both_layers_is_served_not_refused():
    """[[30, 10], [60, 20]] has filter - stride even on both layers (20, 40) and three taps on each: wn_create accepts it
    (no split-fp16 pack on the first layer, so the fp32 GEMMs, as in 'oddtap'), and then it has to be right."""
    from oracle import wavenet_np as O
    cfgd = dict(G.load_json('parallel_wavenet.json'), deconv_config=[[30, 10], [60, 20]], num_iaf_layers=[10])
    hp = O.HP(cfgd)
    w = O.synth_weights(hp, 'student', seed=G.STUDENT_SEED, init='unit')
    eng = _engine(cfgd, w, 'f16x3')
    mel = np.random.RandomState(3).uniform(0, 1, [2, 3, G.N_MEL]).astype(np.float32)
    ref = O.deconv_stack(mel, w, hp, 'iaf_share', np.float64)
    r = _rel(_np(eng.deconv(mel)), ref)
    print('DECONV-GEO D [[30,10],[60,20]] rows: {:.2e} of the range'.format(r))
    assert r <= BAR
    eng.close()
