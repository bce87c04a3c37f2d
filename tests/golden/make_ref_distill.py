"""Distillation-loss vectors produced by the REFERENCE'S OWN ParallelWavenet.calculate_loss and its parts
(wavenet/parallel_wavenet.py:361-512), executed in the build container over the numpy evaluator of the TensorFlow primitives
(tests/golden/tf_standin.py, imported through make_ref_float.import_reference(); read its header for what that does and
does not pin).

Run in the build container only (needs the reference tree; nothing of it travels -- only the .npz below):
    python tests/golden/make_ref_distill.py
Writes tests/golden/ref_distill.npz.

Two student / teacher pairs of the reduced-width goldens, weights from oracle.wavenet_np.synth_weights:
  mol    iaf_logistic_unit student, ar_mol teacher
  gauss  iaf_gauss_perflow student, ar_gauss teacher
The teachers take the students' upsampler shape (deconv_config [[40, 10], [80, 20]], 200 samples per frame): teacher and
student read the same mel in kl_loss_logistic / kl_loss_gauss, and the reference asserts that the teacher's conditioning
covers the student's audio (wavenet.py:79).  Hyper-parameters: the reference's own parallel_wavenet*.json overlaid with the
case's settings (num_samples replaced by S = 8 to keep the file small).

What is recorded, float64 throughout (tf.float32 mapped to float64), inputs float32-valued so that the device sees the
same numbers:
  student   x, mean_tot, scale_tot, log_scale_tot of the student's forward (oracle.wavenet_np.iaf_feed_forward in float64 on
            the injected noise, rounded to float32) -- fed to the reference's graph through placeholders
  full      ParallelWavenet(hparams, teacher).calculate_loss as written: its dict, the teacher's out_params for mel and
            mel_rand, the per-sample H_Ps_Pt_bl (mol: the reduce_mean input of H_Ps_Pt, found in the graph)
  parts     kl_loss_logistic / kl_loss_gauss as written, with the teacher's feed_forward answered by a placeholder that
            carries the float32-rounded out_params (so that a device kernel given those out_params is compared with the
            reference's arithmetic on the same numbers), per-sample H_Ps_Pt_bl / kl_loss_bl; power_loss as written for
            the three trim cases (pred longer, orig longer, equal)
  randoms   the uniforms of the two random nodes of the logistic loss ([B*S, T]: kl_loss_logistic's, then
            contrastive_loss's), float32-valued, NOT stored: `uniforms()` below regenerates them from U_SEED (numpy's
            legacy RandomState stream is fixed), and so do the tests
The teacher's float64 out_params are not stored either: tests/test_distill_golden.py recomputes them with the float64 oracle
(oracle.wavenet_np.teacher_feed_forward); only their float32 rounding, the input of the device kernels, is.  B = 2, T = 512.
tf.contrib.signal.stft is not in the stand-in; it is attached below as a restatement of TensorFlow's documented semantics
(frame with pad_end, periodic Hann window, rfft of fft_length) -- like every float kernel of the stand-in it restates
TensorFlow's kernel, it does not pin it.
"""
import json
import os
import sys
import tempfile
from argparse import Namespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_ref_float as MRF  # noqa: E402
import tf_standin as tf  # noqa: E402
from oracle import wavenet_np as O  # noqa: E402
from nsynth_wavenet_amd import weights as wts, config as cfgmod  # noqa: E402

OUT = os.path.join(HERE, 'ref_distill.npz')
S = 8
B = 2
FRAMES = 3                      # T = 512 samples: the shortest length the students' 512-sample dilation cycle allows
U_SEED = 2025
STUDENT_DECONV = [[40, 10], [80, 20]]


def uniforms(B, S, T, seed=U_SEED):
    """the [B*S, T] uniforms of the logistic loss's two random nodes (kl_loss_logistic's, then contrastive_loss's),
    float32-valued; regenerated from the seed by the tests instead of stored (the file stays small)"""
    u = np.random.RandomState(seed).uniform(1e-5, 1 - 1e-5, [2, B * S, T]).astype(np.float32).astype(np.float64)
    return u[0], u[1]


def _stft(signals, frame_length, frame_step, fft_length=None, window_fn=None, pad_end=False, name=None):
    """tf.contrib.signal.stft: frames of frame_length every frame_step (pad_end: ceil(L / step) frames, zeros appended),
    periodic Hann window (the default window_fn), rfft of fft_length (each frame zero-padded at its end)."""
    assert window_fn is None
    nfft = int(fft_length) if fft_length is not None else int(frame_length)

    def f(a):
        L = a.shape[-1]
        nf = -(-L // frame_step) if pad_end else 1 + (L - frame_length) // frame_step
        pad = max(0, (nf - 1) * frame_step + frame_length - L)
        a = np.pad(a, [(0, 0)] * (a.ndim - 1) + [(0, pad)])
        idx = np.arange(nf)[:, None] * frame_step + np.arange(frame_length)[None, :]
        n = np.arange(frame_length)
        w = (0.5 - 0.5 * np.cos(2.0 * np.pi * n / frame_length)).astype(a.dtype)
        return np.fft.rfft(a[..., idx] * w, n=nfft, axis=-1)
    return tf._op(f, signals)


class _StubTeacher(object):
    """What kl_loss_logistic / kl_loss_gauss ask of their teacher: feed_forward(...)['out_params'] -- answered by a
    placeholder, so that the parts are evaluated on given (float32-rounded) teacher parameters."""

    def __init__(self, real, out_ph):
        self.__dict__.update(vars(real))          # the attributes ParallelWavenet.__init__ checks
        self.out_ph = out_ph

    def feed_forward(self, inputs, init=False):
        return {'out_params': self.out_ph}


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def pair_case(R, tag, st_tag, te_tag, out, tmp):
    gs, gt = np.load(os.path.join(HERE, st_tag + '.npz')), np.load(os.path.join(HERE, te_tag + '.npz'))
    st_cfg = json.loads(str(gs['cfg_json']))
    te_cfg = json.loads(str(gt['cfg_json']))
    te_cfg['deconv_config'] = STUDENT_DECONV
    hp_s, hp_t = O.HP(st_cfg), O.HP(te_cfg)
    w_s = O.synth_weights(hp_s, 'student', seed=int(gs['seed']), init=str(gs['init']))
    w_t = O.synth_weights(hp_t, 'teacher', seed=int(gt['seed']), init=str(gt['init']))
    ckpt_t = wts.save_checkpoint(os.path.join(tmp, tag + '_te.npz'), w_t, cfgmod.load_hparams(te_cfg))
    F = FRAMES
    T = O.iaf_length(F, hp_s)
    rs = np.random.RandomState(2024)
    mel = rs.uniform(0, 1, [B, F, 80]).astype(np.float32)
    mel_rand = rs.uniform(0, 1, [B, F, 80]).astype(np.float32)
    gauss = st_cfg['loss_type'] == 'gauss'
    noise = rs.standard_normal([B, T]) if gauss else O.logistic_from_uniform(rs.uniform(1e-5, 1 - 1e-5, [B, T]), np.float64)
    ff = O.iaf_feed_forward(mel, f32(noise), w_s, hp_s, np.float64)
    x, mean_tot, scale_tot = f32(ff['x']), f32(ff['mean_tot']), f32(ff['scale_tot'])
    log_scale_tot = f32(ff['log_scale_tot'])
    # real audio of three lengths (the trim cases of power_loss, parallel_wavenet.py:464-468)
    wavs = {'eq': T, 'long': T + 301, 'short': T - 250}
    wav = {k: f32(np.clip(0.3 * rs.standard_normal([B, n]), -1, 1)) for k, n in wavs.items()}
    u_kl, u_cl = uniforms(B, S, T)
    st_hp = MRF.reference_hparams(st_cfg, 'student')
    st_hp.num_samples = S
    te_hp = Namespace(**dict(vars(MRF.reference_hparams(te_cfg, 'teacher')), use_as_teacher=True))
    ema = R.fastgen.get_ema_shadow_dict
    tf.set_float(np.float64)
    feeds_np = {'mel': mel, 'mel_rand': mel_rand, 'x': x, 'mean_tot': mean_tot, 'scale_tot': scale_tot,
                'log_scale_tot': log_scale_tot}

    def placeholders():
        ph = {k: tf.placeholder(tf.float32, list(v.shape)) for k, v in feeds_np.items()}
        return ph, {ph[k]: feeds_np[k] for k in ph}

    # -- full: calculate_loss as written, the teacher's own forward inside
    tf.set_random_source(MRF.TableSource({0: lambda step: u_kl, 1: lambda step: u_cl}))
    with tf.Graph().as_default(), tf.Session() as sess:
        teacher = R.wavenet.Wavenet(te_hp)
        pw = R.parallel_wavenet.ParallelWavenet(st_hp, teacher)
        ph, feed = placeholders()
        wav_ph = tf.placeholder(tf.float32, [B, T + 301])
        fd = dict(ph)
        fd['wav'] = wav_ph
        feed[wav_ph] = wav['long']
        loss = pw.calculate_loss(fd)
        te_out = teacher.feed_forward({'wav_scaled': ph['x'], 'mel': ph['mel']})['out_params']
        te_out_rand = teacher.feed_forward({'wav_scaled': ph['x'], 'mel': ph['mel_rand']})['out_params']
        tf.train.Saver(ema(tf.trainable_variables())).restore(sess, ckpt_t)
        fetch = dict(loss)
        fetch['te_out'], fetch['te_out_rand'] = te_out, te_out_rand
        if not gauss:
            bl = loss['H_Ps_Pt'].inputs[0]
            assert bl.get_shape().as_list() == [B, T]
            fetch['H_bl'] = bl
        vals = sess.run(fetch, feed_dict=feed)
    for k, v in vals.items():
        if not k.startswith('te_out'):         # the teacher's float64 output is recomputed by the tests (oracle)
            out['{}/full_{}'.format(tag, k)] = np.asarray(v, np.float64)
    print(tag, 'calculate_loss', {k: float(v) for k, v in vals.items() if np.ndim(v) == 0})

    # -- parts on the float32-rounded teacher parameters
    te32 = f32(vals['te_out'])
    tf.set_random_source(MRF.TableSource({0: lambda step: u_kl}))
    with tf.Graph().as_default(), tf.Session() as sess:
        te_ph = tf.placeholder(tf.float32, list(te32.shape))
        teacher = R.wavenet.Wavenet(te_hp)
        pw = R.parallel_wavenet.ParallelWavenet(st_hp, _StubTeacher(teacher, te_ph))
        ph, feed = placeholders()
        feed[te_ph] = te32
        fetch = {}
        if gauss:
            kl = pw.kl_loss_gauss(ph)['kl_loss']
            # kl_loss = reduce_mean(kl_loss_bl) + 4 * reg  (parallel_wavenet.py:426-427)
            mean_node = kl.inputs[0]
            assert mean_node.inputs[0].get_shape().as_list() == [B, T]
            fetch.update(kl_loss=kl, kl_bl=mean_node.inputs[0])
        else:
            d = pw.kl_loss_logistic(ph, S)
            fetch.update(d)
            fetch['H_bl'] = d['H_Ps_Pt'].inputs[0]
        wph = {k: tf.placeholder(tf.float32, list(v.shape)) for k, v in wav.items()}
        for k in wav:
            fetch['power_loss_' + k] = pw.power_loss({'x': ph['x'], 'wav': wph[k]})['power_loss']
            feed[wph[k]] = wav[k]
        vals = sess.run(fetch, feed_dict=feed)
    for k, v in vals.items():
        out['{}/parts_{}'.format(tag, k)] = np.asarray(v, np.float64)
    print(tag, 'parts', {k: float(v) for k, v in vals.items() if np.ndim(v) == 0})

    for k, v in feeds_np.items():
        out['{}/in_{}'.format(tag, k)] = v.astype(np.float32)
    for k, v in wav.items():
        out['{}/in_wav_{}'.format(tag, k)] = v.astype(np.float32)
    out[tag + '/in_te_out_f32'] = te32.astype(np.float32)
    if not gauss:
        out[tag + '/u_seed'] = np.array(U_SEED)
    out[tag + '/st_cfg_json'] = np.array(json.dumps(vars(st_hp)))
    out[tag + '/te_cfg_json'] = np.array(json.dumps(te_cfg))
    out[tag + '/st_seed'] = np.array(int(gs['seed']))
    out[tag + '/st_init'] = np.array(str(gs['init']))
    out[tag + '/te_seed'] = np.array(int(gt['seed']))
    out[tag + '/te_init'] = np.array(str(gt['init']))


def main():
    R = MRF.import_reference()
    tf.contrib.signal.stft = _stft
    out = {'S': np.array(S)}
    with tempfile.TemporaryDirectory() as tmp:
        pair_case(R, 'mol', 'iaf_logistic_unit', 'ar_mol', out, tmp)
        pair_case(R, 'gauss', 'iaf_gauss_perflow', 'ar_gauss', out, tmp)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
