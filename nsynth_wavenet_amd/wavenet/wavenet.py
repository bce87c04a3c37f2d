"""Host-side mirror of the reference's `Wavenet.deconv_stack` and `Fastgen`
(wavenet/wavenet.py:94-155,318-514) for the generation path."""
import numpy as np
import torch

from .. import config as cfg
from ..engine import Engine


def _wants_grad(x):
    """a torch tensor that autograd would track now"""
    return isinstance(x, torch.Tensor) and x.requires_grad and torch.is_grad_enabled()


class _TeacherBase(object):
    def __init__(self, hparams, device=None, engine=None):
        self.hparams = cfg.load_hparams(hparams)
        hp = self.hparams
        self.use_mu_law = hp.use_mu_law
        self.loss_type = hp.loss_type
        self.use_weight_norm = getattr(hp, 'use_weight_norm', False)
        self.double_gate_width = getattr(hp, 'double_gate_width', True)
        self.dropout_inputs = getattr(hp, 'dropout_inputs', False)
        self.dropout_all = getattr(hp, 'dropout_all', False)
        assert not (self.dropout_inputs and self.dropout_all)
        self.quant_chann = cfg.quant_chann(hp)
        self.out_width = cfg.teacher_out_width(hp)
        self.engine = engine if engine is not None else Engine(hp, kind='teacher', device=device)

    def load_weights(self, weights):
        self.engine.load_weights(weights)
        return self

    def restore(self, checkpoint_path):
        self.engine.load_checkpoint(checkpoint_path)
        return self


class Wavenet(_TeacherBase):
    """The teacher's inference graphs: the upsampler and the full-sequence forward."""

    def deconv_stack(self, mel_inputs, init=False):
        return {'encoding': self.engine.deconv(mel_inputs['mel'])}

    def encode_signal(self, inputs):
        """wavenet.py:157-178 on the host (numpy): 'wav' [B,T] -> 'wav_scaled' (the network input), 'real_targets', 'cate_targets'.
        feed_forward / calculate_loss take the raw 'wav' and derive these on the device; this is the reference's function for
        callers that want the targets themselves."""
        from ..auxilaries import utils
        x = np.asarray(inputs['wav'], np.float32)
        q = self.quant_chann
        if self.use_mu_law:
            xq = utils.mu_law_numpy(x, mu=np.float32(255))          # float32 arithmetic, like the TF twin (utils.py:72-87)
            scaled = (xq / np.float32(q / 2.)).astype(np.float32)
            return {'wav_scaled': scaled, 'real_targets': scaled, 'cate_targets': xq.astype(np.int32) + q // 2}
        return {'wav_scaled': x, 'real_targets': x, 'cate_targets': np.floor(x * np.float32(q / 2)).astype(np.int32) + q // 2}

    def feed_forward(self, inputs, init=False):
        """wavenet.py:180-291 with 'wav' [B,T] raw audio and 'mel' [B,F,80]: the reference derives
        'wav_scaled' from 'wav' (wavenet.py:157-178); here the device does.  Returns 'out_params'
        [B,T,out_width] (and 'encoding' on request through deconv_stack: it is not materialised
        in the reference layout by this call)."""
        if init:
            raise ValueError('data-dependent initialisation is a training-time feature')
        # 'wav' is passed through so that the reference's own call sequence (train_wavenet.py:104-108, tests/test_wavenet.py:38-42:
        # ff_dict = feed_forward(inputs); ff_dict.update(encode_signal(inputs)); calculate_loss(ff_dict)) runs unchanged
        # A 'wav' that requires grad (a student's sample scored by the frozen teacher) takes the tape forward, whose backward is
        # the engine's input VJP: the same out_params bits, and the engine's own refusals (mu-law teachers,
        # widths that are no multiple of 64).  'wav' goes on undetached: calculate_loss adds the gradient through the target.
        wav = inputs['wav']
        if _wants_grad(wav):
            from .. import distill_autograd as dag
            wav = wav.to(device=self.engine.device, dtype=torch.float32)
            return {'out_params': dag.TeacherForward.apply(wav, inputs['mel'], self.engine), 'wav': wav}
        return {'out_params': self.engine.teacher_forward(wav, inputs['mel']), 'wav': wav}

    def calculate_loss(self, ff_dict):
        """wavenet.py:293-316 for scoring audio under the teacher.  ff_dict holds 'out_params' (feed_forward) and the audio: the
        raw 'wav' (feed_forward passes it through; the device derives the targets of encode_signal from it), or -- the reference's
        own keys -- encode_signal's 'real_targets' / 'cate_targets' alone: without mu-law the real target IS the audio; with it
        the class index is handed back as the centre of its bin, inv_mu_law(i), which the device's mu_law maps to the same index
        and the same real target i / 128 (the codec round trip of SURVEY K7, tests/test_ref_codec.py).
        Returns {'loss': -mean log-likelihood, 'log_probs': [B,T]}.  The mixture-of-logistics score is the float64-accurate
        value of the bin mass, not the float32 difference of two sigmoids TensorFlow evaluates (include/wnhip.h).
        With grad mode on and an 'out_params' or audio tensor that requires grad, the result is differentiable (the same values):
        to out_params, and to the audio through the target -- zero for mu-law and ce teachers, whose targets are quantised."""
        if 'wav' in ff_dict:
            wav = ff_dict['wav']
        elif self.use_mu_law and 'cate_targets' in ff_dict:
            from ..auxilaries import utils
            cate = ff_dict['cate_targets']
            cate = cate.cpu().numpy() if hasattr(cate, 'cpu') else np.asarray(cate)
            wav = utils.inv_mu_law_numpy(cate.astype(np.int32) - self.quant_chann // 2).astype(np.float32)
        elif not self.use_mu_law and 'real_targets' in ff_dict:
            wav = ff_dict['real_targets']
        else:
            raise KeyError("calculate_loss needs 'wav', or encode_signal's 'real_targets' / 'cate_targets', beside 'out_params'")
        out_params = ff_dict['out_params']
        if _wants_grad(out_params) or _wants_grad(wav):
            # the same kernel on the same values (the same bits), with wn_teacher_log_prob_grad as its backward
            from .. import distill_autograd as dag
            dev = self.engine.device
            lp = dag.TeacherLogProb.apply(torch.as_tensor(out_params).to(device=dev, dtype=torch.float32),
                                          torch.as_tensor(wav).to(device=dev, dtype=torch.float32), self.engine)
        else:
            lp = self.engine.teacher_log_prob(out_params, wav)
        return {'loss': -lp.mean(), 'log_probs': lp}

    @property
    def dropout_rate(self):
        """wavenet.py:132-135"""
        return getattr(self.hparams, 'dropout_rate', 0.5 if self.dropout_inputs else 0.05)

    def loss_and_weight_grads(self, inputs, upsampler=False, dropout_seed=None):
        """The loss train_wavenet.py minimises and its gradient: 'wav' [B,T] raw audio and 'mel' [B,F,80] ->
        {'loss': -mean log p (the bits of the no-grad calculate_loss(feed_forward(.))), 'log_probs': [B,T],
         'grads': {tf variable name: d loss / d variable, in the TF shape} for every loaded variable of the residual stack and
         output head, 'flat_grads': the same values as one float32 vector (Engine.teacher_grad_table gives the offsets),
         'd_encoding': d loss / d encoding [B, F frame_shift, deconv_width], the cotangent the upsampler's variables need}.
        One training-tape forward and one reverse pass on the device.  MoL and Gauss teachers without mu-law
        and without weight norm.
        dropout_seed=None: the deterministic forward feed_forward evaluates, whatever the hparams say about dropout.
        dropout_seed=s (an integer, 64 bits are used): the training graph of train_wavenet.py -- the hparams' `dropout_inputs`
        (conv_dropout on l and skip_dropout on s after skip_start, default rate 0.5) or `dropout_all` (conv_dropout and every
        res_dropout_i, default rate 0.05) at rate `dropout_rate`, with the masks train.dropout_keep(s, site, ...) gives
        (DESIGN.md 17).  'loss', 'log_probs' and every gradient are those of the dropped forward.  ValueError when the hparams
        ask for neither.
        upsampler=True: 'grads' also holds trans_conv_j/kernel and trans_conv_j/bias, from one Engine.deconv_backward on this
        call's own d_encoding, and 'flat_upsampler_grads' is that call's flat vector
        (Engine.deconv_grad_table gives the offsets).  Everything else is the bits of the default call."""
        dropout = None
        if dropout_seed is not None:
            if not (self.dropout_inputs or self.dropout_all):
                raise ValueError('loss_and_weight_grads: dropout_seed given, but the hparams set neither dropout_inputs nor '
                                 'dropout_all')
            dropout = ('dropout_inputs' if self.dropout_inputs else 'dropout_all', int(dropout_seed), float(self.dropout_rate))
        eng = self.engine
        wav = eng._dev(inputs['wav'])
        out, tape = eng.teacher_forward_train_tape(wav, inputs['mel'], dropout=dropout)
        lp = eng.teacher_log_prob(out, wav)
        d_lp = torch.full_like(lp, -1.0 / lp.numel())
        d_out, _ = eng.teacher_log_prob_grad(out, wav, d_lp, want_wav=False)
        res = eng.teacher_backward_weights(tape, d_out, want_encoding=True)
        ret = {'loss': -lp.mean(), 'log_probs': lp, 'grads': res['grads'], 'flat_grads': res['flat_grads'],
               'd_encoding': res['d_encoding']}
        if upsampler:
            up = eng.deconv_backward(inputs['mel'], res['d_encoding'])
            ret['grads'] = dict(res['grads'])
            ret['grads'].update(up['grads'])
            ret['flat_upsampler_grads'] = up['flat_grads']
        return ret


class Fastgen(_TeacherBase):
    """Incremental teacher: `sample({'wav': [B,1], 'encoding': [B,Cd]})` is one step.
    The two FIFO queues per causal layer are a device-resident ring state created by
    `init()` (the reference's sess.run(init_ops))."""

    def __init__(self, hparams, batch_size=2, device=None, engine=None):
        super(Fastgen, self).__init__(hparams, device, engine)
        self.batch_size = batch_size
        self.state = None

    def init(self):
        self.state = self.engine.ar_new_state(self.batch_size)
        return self

    def cond_vars(self, inputs):
        """wavenet.py:353-377: {'mel_cond_1' .. 'mel_cond_<num_layers>', 'mel_cond_out1'} of inputs['encoding']
        [B, T, deconv_width], each [B, T, gate_width] ([B, T, skip_width] for the last) -- one bulk evaluation on the device."""
        return self.engine.ar_cond_vars(inputs['encoding'])

    def sample(self, inputs, rnd=None, seed=0, want_out=False):
        if self.state is None:
            self.init()
        wav = inputs['wav']
        res = self.engine.ar_step(self.state, wav, inputs['encoding'], rnd=rnd, seed=seed, want_out=want_out)
        if want_out:
            s, out = res
            return {'sample': s.reshape(self.batch_size, 1), 'out_params': out}
        return {'sample': res.reshape(self.batch_size, 1)}
